"""The GroupNorm passes and the consumers a GroupNorm is folded into (bdm_amd/csrc/dense_ops.hip), ELEMENTWISE against float64.

(a) bdm_group_norm            gn_onepass_kernel / gn_stats_vec + gn_apply_vec / gn_stats + gn_apply, chosen by shape, stride, alignment
(b) bdm_group_norm_stats      the slice partials of the two-pass kernels
(c) bdm_max_over_neighbors(_gn)   maximum over the neighbour axis, plain and over Swish(GroupNorm(x)) (max_u_gn_kernel, lpr lanes per row)
(d) bdm_se_gate, bdm_se_gate_gn(_pf)   row means of Swish(GroupNorm(x)), the rows' affine forms, the SE gate
(e) bdm_devoxelize_gn_gate_add(_pf), bdm_devoxelize_gn_se_add, bdm_devoxelize_gate_add   trilinear gather, global-memory and LDS forms

One case table per operation; every row names the route it is meant to reach.
* CPU half (no GPU): the launch path's own choosers (bdm_group_norm_route, bdm_max_over_neighbors_gn_lanes, bdm_devoxelize_gn_route)
  return that route for every row; only addresses and strides are looked at, so the rows are laid out on torch's meta device.
* GPU half: every row against the same operation in float64 PyTorch on the CPU, element by element.

Inputs: x[:, ch] = randn (0.5 + ch % 5) + k ((ch % 7) - 3) with k in 0.1, 1.3, 5.3 (a group's |mean| / std: roughly 0.3, 4, 16 over a few
channels, 0.6, 8, 32 at most where a group is a single channel), gamma and beta independent randn per channel, fixed seeds: a wrong
channel or group index changes the result by whole units, not by roundings.
Larger offsets are kept OUT of the tables: the two-pass kernels finalise E[x^2] - mean^2 from single-pass fp32 sums, whose conditioning
limit an fp32 emulation of gn_stats_vec_kernel reaches at |mean| / std = 64 (11 units of the bound below where plain fp32 PyTorch keeps
1.1); up to 16 the emulation stays within 1.3 - 3.8 units and plain fp32 PyTorch within 0.9 - 3.5.

Tolerances (none measured on the kernel), u = 2^-24:
* per output element mag = the magnitude of the terms that go into it, computed in float64:
      normalised value (and its Swish: |swish'| <= 1.1)   (|x| + |mean|) rstd |gamma| + |beta|   (|x| = |x| + |residual| with a residual)
      maximum over neighbours                             the largest mag of the row
      row mean                                            the mean of the row's mag
      devoxelisation                                      sum_i w_i mag_i |gate| + mag_add
      affine forms (coef)                                 |gamma| rstd   and   |beta| + |mean gamma| rstd
      SE gate (after the sigmoid)                         1 + sum |w2| |hidden|   (no entry point returns the hidden vector: its error
                                                          is inside the gate's figure, which is held to this bound all the same)
  the figure is max |got - ref64| / (u mag); the yardstick is the same operation in plain fp32 PyTorch on the CPU (TF.group_norm,
  x sigmoid(x), max, mean, the eight trilinear weights written out) against the same float64 reference; the kernel may be at most
  4 x max(yardstick, 1): 4 for another summation order, another libm and the hardware rcp / exp2, the floor of one unit (one rounding
  of the result's own magnitude) so that a lucky yardstick on a tiny case decides nothing.  The whole-tensor rel-L2 is reported next to
  the 3e-6 the older tests assert.
* slice partials (b): |sum err| <= (4 iters + 3) u sum |v|, |sum of squares err| <= (4 iters + 4) u sum v^2, iters = the length of one
  thread's chain, ceil(ceil((cg L / 4) / S) / 256) float4 steps (scalar route, fp64 accumulation: the same with cg L elements).
* bit-exact (torch.equal): a repeated launch, in place against out=, the LDS against the global-memory devoxelisation, the plain
  maximum against x.max(-1).

The row (2, 24, 8196, 8) was meant to put 3 channels per group on the vector route, but its chunks hold 3 x 8196 = 24588 floats and the
launch path keeps them in one pass: it stays in the table under the route it really takes, and (2, 24, 24580, 8) reaches the vector
kernels with 3 channels per group.

Views that cannot be expressed and are therefore not run: bdm_group_norm_stats takes (batch stride) only -- its rows are dense and it
has neither out nor residual -- so of the scalar rows of (a) it runs the odd lengths and the misaligned base, not the column slice and
not the out= / residual row.  The folded devoxelisations allocate their output themselves: no strided output there.
"""
import ctypes
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from helpers import current_test, parity

U = 2.0 ** -24
DEV = torch.device("cuda")
EPS = 1e-5
OFFSETS = (0.1, 1.3, 5.3)
SENT = -777.0
ONE_PASS, VECTOR, SCALAR = 0, 1, 2


def cdiv(a, b):
    return (a + b - 1) // b


# ---- case tables --------------------------------------------------------------------------------------------------------------------
# (a) view: None (contiguous), "cols" (x and out are the column slice [:, :, 4:4+L] of a (B, C, L+8) buffer), "lead1" (x and out start one
# float into a flat buffer), "outres" (out = such a column slice, residual = the slice [:, :, 8:8+L] of a (B, C, L+44) buffer; in place: x
# itself is the column slice)
GN = namedtuple("GN", "id b c l groups route view")
GN_CASES = [
    GN("one_1float4", 2, 8, 4, 8, ONE_PASS, None),                 # one float4 per chunk
    GN("one_cg3", 3, 24, 12, 8, ONE_PASS, None),                   # 3 channels per group, L / 4 = 3
    GN("one_5groups", 2, 40, 100, 5, ONE_PASS, None),
    GN("one_1group_oddL4", 1, 6, 2052, 1, ONE_PASS, None),
    GN("one_edge65536", 2, 128, 4096, 8, ONE_PASS, None),          # exactly 65536 floats per chunk
    GN("one_c512", 2, 512, 16, 8, ONE_PASS, None),
    GN("vec_edge65540", 1, 8, 65540, 8, VECTOR, None),             # four floats past the edge; 5 slices
    GN("vec_32768", 2, 64, 32768, 8, VECTOR, None),
    GN("one_cg3_l8196", 2, 24, 8196, 8, ONE_PASS, None),           # 3 x 8196 = 24588 floats per chunk: still one pass (see the docstring)
    GN("vec_cg3", 2, 24, 24580, 8, VECTOR, None),                  # 3 channels per group on the vector route: 73740 floats, 5 slices
    GN("vec_slicecap", 1, 64, 131076, 8, VECTOR, None),            # 65 slices wanted, capped at 64; apply grid capped
    GN("sc_l33", 2, 24, 33, 8, SCALAR, None),
    GN("sc_l4099", 1, 16, 4099, 2, SCALAR, None),                  # 3 slices
    GN("sc_colslice", 2, 32, 512, 8, SCALAR, "cols"),
    GN("sc_misaligned", 2, 16, 256, 8, SCALAR, "lead1"),
    GN("sc_out_res_slices", 2, 16, 256, 8, SCALAR, "outres"),
]
GN_LAYOUT = {  # view -> ((x, residual) in place, (x, residual, out) with out=)
    None: (("dense", "dense"), ("dense", "dense", "dense")),
    "cols": (("cols", "dense"), ("cols", "dense", "cols")),
    "lead1": (("lead1", "dense"), ("lead1", "dense", "lead1")),
    "outres": (("cols", "cols44"), ("dense", "cols44", "cols")),
}
STATS_CASES = [c for c in GN_CASES if c.route != ONE_PASS and c.view in (None, "lead1")]

# (c) lpr = the lanes per row max_u_gn_kernel is meant to run with; view: None, "lead1" (misaligned base), "out" (strided output)
MX = namedtuple("MX", "id b c m u groups lpr view")
MX_U = (4, 8, 16, 32, 64, 128, 256)
MX_CASES = [MX(f"m{m}_u{u}", 2, 16, m, u, 8, u // 4, None) for m in (1, 65, 100) for u in MX_U] + [
    MX("u12_not_pow2", 2, 16, 65, 12, 8, 1, None),
    MX("u5", 2, 16, 65, 5, 8, 1, None),
    MX("u1", 2, 16, 65, 1, 8, 1, None),
    MX("u260", 2, 16, 65, 260, 8, 1, None),
    MX("u32_misaligned", 2, 16, 65, 32, 8, 1, "lead1"),
    MX("channel_loop", 2, 264, 70, 8, 8, 2, None),                  # 33 channels per group, c > 256: the channel grid-stride loop
    MX("strided_out", 2, 16, 65, 16, 8, 4, "out"),
]
MX_SLICES = (1, 3, 64, 65, 130)
PLAIN_U = MX_U + (12, 5, 1, 260)

# (d) (C, hidden, l, groups, misaligned)
SE = namedtuple("SE", "id c hidden l groups lead")
SE_CASES = [
    SE("c8_l1", 8, 1, 1, 2, 0),
    SE("c24_l513", 24, 3, 513, 8, 0),
    SE("c64_l4096", 64, 8, 4096, 8, 0),
    SE("c264_l512", 264, 33, 512, 8, 0),
    SE("c512_l516", 512, 64, 516, 8, 0),
    SE("c64_l515_misaligned", 64, 8, 515, 8, 1),                    # the scalar row loop of row_mean_gn_kernel
]
SE_B, SE_SLICES, SE_PF_SLICES, SE_PF_GROUPS, SE_PF_POINTS = 3, (1, 5, 64), (1, 33), 4, 37

# (e) route: the kernel bdm_devoxelize_gn_gate_add(_pf) launches with BDM_STAGING = staging (None: unset)
DV = namedtuple("DV", "id b c r n staging route")
DV_CASES = [
    DV("r8_early_return", 3, 5, 8, 300, None, 0),                   # 15 units: not a multiple of 8
    DV("r8_c72", 2, 72, 8, 257, None, 0),                           # more than 64 channel slots
    DV("r16_lds", 2, 24, 16, 600, None, 1),                         # LDS by default, two channels per workgroup
    DV("r16_c3_t1024", 2, 3, 16, 2100, None, 1),                    # odd channel tail, 1024 threads
    DV("r8_forced_lds", 1, 24, 8, 100, "1", 1),                     # 16 channels per workgroup and a tail of 8
    DV("r32_forced_lds", 1, 4, 32, 300, "1", 1),                    # one channel per workgroup, 128 KB of LDS
]


def ids(cases):
    return [c.id for c in cases]


# ---- layouts and route queries (CPU and GPU halves) ----------------------------------------------------------------------------------
def placed(shape, kind, dev):
    """(buffer, view): a buffer full of SENT and the (B, C, L) view of it that `kind` names."""
    B, C, L = shape
    if kind == "dense":
        buf = torch.full(shape, SENT, device=dev)
        return buf, buf
    if kind == "cols":
        buf = torch.full((B, C, L + 8), SENT, device=dev)
        return buf, buf[:, :, 4:4 + L]
    if kind == "cols44":
        buf = torch.full((B, C, L + 44), SENT, device=dev)
        return buf, buf[:, :, 8:8 + L]
    assert kind == "lead1"
    buf = torch.full((1 + B * C * L,), SENT, device=dev)
    return buf, buf[1:].view(B, C, L)


def addr(t):
    """The address the launch path would see: the real one on the GPU, elsewhere a 4096-aligned base plus the view's offset."""
    if t is None:
        return None
    return t.data_ptr() if t.is_cuda else 4096 + 4 * t.storage_offset()


def gn_route(x, res, out, groups):
    from bdm_amd import _lib, ops
    _, _, C, l, bs_x, ld_x = ops._bcl(x)
    _, _, _, _, bs_y, ld_y = ops._bcl(out)
    bs_r, ld_r = ops._bcl(res)[4:] if res is not None else (0, 0)
    return _lib.lib().bdm_group_norm_route(C, l, groups, addr(x), bs_x, ld_x, addr(res), bs_r, ld_r, addr(out), bs_y, ld_y)


def gn_tensors(case, dev, inplace, with_res):
    """(x buffer, x, residual, out buffer, out) of a row's in-place or out= launch, laid out as GN_LAYOUT says (values: SENT)."""
    shape = (case.b, case.c, case.l)
    kinds = GN_LAYOUT[case.view][0 if inplace else 1]
    xbuf, x = placed(shape, kinds[0], dev)
    res = placed(shape, kinds[1], dev)[1] if with_res else None
    obuf, out = (xbuf, x) if inplace else placed(shape, kinds[2], dev)
    return xbuf, x, res, obuf, out


def stats_slices(case):
    return min(64, max(1, cdiv((case.c // case.groups) * case.l, 16384)))


def mx_lanes(u, a):
    from bdm_amd import _lib
    return _lib.lib().bdm_max_over_neighbors_gn_lanes(u, a)


def dv_route(case, with_se, a=4096):
    from bdm_amd import _lib
    return _lib.lib().bdm_devoxelize_gn_route(case.b, case.c, case.r, a, int(with_se))


# ---- CPU half ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GN_CASES, ids=ids(GN_CASES))
def test_group_norm_row_reaches_its_route(case):
    for inplace in (True, False):
        for with_res in (False, True):
            _, x, res, _, out = gn_tensors(case, "meta", inplace, with_res)
            assert gn_route(x, res, out, case.groups) == case.route, (inplace, with_res)
    cg = case.c // case.groups
    assert (case.route == ONE_PASS) == (case.view is None and case.l % 4 == 0 and cg * case.l <= 65536)


def test_group_norm_table_covers_the_edges():
    by = {c.id: c for c in GN_CASES}
    assert by["one_edge65536"].c // 8 * by["one_edge65536"].l == 65536 and by["vec_edge65540"].c // 8 * by["vec_edge65540"].l == 65540
    assert stats_slices(by["vec_edge65540"]) == 5
    cap = by["vec_slicecap"]
    assert cdiv(cap.c // cap.groups * cap.l, 16384) == 65 and stats_slices(cap) == 64 and cap.c // cap.groups * cap.l // 4 > 64 * 1024
    assert stats_slices(by["sc_l4099"]) == 3
    assert {c.route for c in GN_CASES} == {ONE_PASS, VECTOR, SCALAR}
    for route in (ONE_PASS, VECTOR, SCALAR):   # channels per group: a power of two and not
        cgs = {c.c // c.groups for c in GN_CASES if c.route == route}
        assert any(cg & (cg - 1) for cg in cgs) and any(cg & (cg - 1) == 0 for cg in cgs), route
    assert 4 * cap.b * cap.c * cap.l <= 34 * 2 ** 20   # the largest tensor of the file


@pytest.mark.parametrize("case", STATS_CASES, ids=ids(STATS_CASES))
def test_stats_row_reaches_its_route(case):
    _, x = placed((case.b, case.c, case.l), "lead1" if case.view else "dense", "meta")
    assert gn_route(x, None, x, case.groups) == case.route
    assert {c.route for c in STATS_CASES} == {VECTOR, SCALAR}


@pytest.mark.parametrize("case", MX_CASES, ids=ids(MX_CASES))
def test_max_row_reaches_its_lanes(case):
    assert mx_lanes(case.u, 4096 + (4 if case.view == "lead1" else 0)) == case.lpr
    assert case.c % case.groups == 0


def test_max_table_covers_every_lane_count_and_fall_back():
    for m in (1, 65, 100):
        assert {c.lpr for c in MX_CASES if c.m == m and c.view is None and c.u in MX_U} == {1, 2, 4, 8, 16, 32, 64}
    fall_backs = {c.id: c for c in MX_CASES if c.lpr == 1 and c.u != 4}
    assert any(c.u % 4 == 0 and (c.u // 4) & (c.u // 4 - 1) and c.u <= 256 for c in fall_backs.values())   # u / 4 not a power of two
    assert sum(c.u % 4 != 0 for c in fall_backs.values()) >= 2 and any(c.u > 256 and c.u % 4 == 0 for c in fall_backs.values())
    assert any(c.view == "lead1" and mx_lanes(c.u, 4096) > 1 for c in fall_backs.values())                 # only the base is off
    assert any(c.c > 256 and (c.c // c.groups) & (c.c // c.groups - 1) for c in MX_CASES)
    assert max(MX_SLICES) > 128 and 64 in MX_SLICES and 65 in MX_SLICES and 1 in MX_SLICES


@pytest.mark.parametrize("case", DV_CASES, ids=ids(DV_CASES))
def test_devoxelisation_row_reaches_its_route(case, monkeypatch):
    monkeypatch.delenv("BDM_STAGING", raising=False)
    if case.staging is not None:
        assert dv_route(case, False) == 0, "the row is meant to need BDM_STAGING for the LDS form"
        monkeypatch.setenv("BDM_STAGING", case.staging)
    assert dv_route(case, False) == case.route
    assert dv_route(case, True) == 0                       # the SE layers in the kernel: global form only
    assert dv_route(case, False, 4096 + 4) == 0            # a grid off 16 bytes never takes the float4 fill
    monkeypatch.setenv("BDM_STAGING", "0")
    assert dv_route(case, False) == 0
    monkeypatch.setenv("BDM_STAGING", "1")
    assert dv_route(case, False) == 1                      # every row fits LDS: both forms can be compared


def test_devoxelisation_table_covers_the_edges():
    by = {c.id: c for c in DV_CASES}
    assert (by["r8_early_return"].b * by["r8_early_return"].c) % 8 != 0 and by["r8_c72"].c > 64
    cpw = {c.id: max(1, min(c.c, 8192 // c.r ** 3)) for c in DV_CASES}
    assert cpw["r16_lds"] == 2 and cpw["r16_c3_t1024"] == 2 and by["r16_c3_t1024"].c % 2 == 1 and by["r16_c3_t1024"].n >= 2048
    assert cpw["r8_forced_lds"] == 16 and by["r8_forced_lds"].c % 16 == 8
    assert cpw["r32_forced_lds"] == 1 and 4 * by["r32_forced_lds"].r ** 3 == 128 * 1024


# ---- GPU half: data, references, figures ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(hip):
    from bdm_amd import ops as o
    return o


def channel_data(shape, k, seed):
    """x[:, ch] = randn (0.5 + ch % 5) + k ((ch % 7) - 3), float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(shape[1], dtype=torch.float32).view(1, -1, *([1] * (len(shape) - 2)))
    return torch.randn(*shape, generator=g) * (0.5 + ch % 5) + k * (ch % 7 - 3)


def affine(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(c, generator=g), torch.randn(c, generator=g)


def gn_module(groups, gamma, beta):
    gn = torch.nn.GroupNorm(groups, gamma.numel(), eps=EPS)
    gn.weight.data.copy_(gamma)
    gn.bias.data.copy_(beta)
    return gn.to(DEV)


def group_stats64(v, groups):
    """(mean, rstd) per (shape, group) of v (B, C, L) float64, each (B, groups, 1)."""
    vg = v.reshape(v.shape[0], groups, -1)
    return vg.mean(-1, keepdim=True), 1.0 / torch.sqrt(vg.var(-1, unbiased=False, keepdim=True) + EPS)


def gn64(v, absv, groups, gamma, beta):
    """GroupNorm of v (B, C, L) in float64 and the bound term mag = (|x| + |mean|) rstd |gamma| + |beta| per element."""
    B, C, L = v.shape
    mean, rstd = group_stats64(v, groups)
    ga, be = gamma.double()[None, :, None], beta.double()[None, :, None]
    h = ((v.reshape(B, groups, -1) - mean) * rstd).view(B, C, L) * ga + be
    mag = ((absv.reshape(B, groups, -1) + mean.abs()) * rstd).view(B, C, L) * ga.abs() + be.abs()
    return h, mag


def swish(t):
    return t * torch.sigmoid(t)


def group_totals(v, groups):
    """(sum, sum of squares) per (shape, group) of v (B, C, L) float64: (B, groups, 2)."""
    vg = v.reshape(v.shape[0], groups, -1)
    return torch.stack([vg.sum(-1), (vg * vg).sum(-1)], -1)


def uneven_partials(tot, S, seed):
    """tot (B, G, 2) float64 cut into S slices of very different sizes that add up to it: (B, G, S, 2) as a producer leaves them."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(S, generator=g, dtype=torch.float64) + 0.05
    w[::3] *= 7.0
    w /= w.sum()
    p = tot[:, :, None, :] * w[None, None, :, None]
    p[:, :, -1, :] = tot - p[:, :, :-1, :].sum(2)
    return p.contiguous()


class Figures:
    """The figures of one test: reported through helpers.parity as they are measured, asserted together at the end."""

    def __init__(self):
        self.bad = []

    def check(self, name, got, ref, unit, plain, what):
        """max |got - ref| / unit (unit = u mag, float64) against 4 x max(the same figure of plain fp32 PyTorch, 1)."""
        g = got.detach().double().cpu().reshape(ref.shape)
        unit = unit.expand_as(ref).clamp_min(1e-300)
        fig = float(((g - ref).abs() / unit).max())
        yard = float(((plain.double().reshape(ref.shape) - ref).abs() / unit).max())
        bound = 4.0 * max(yard, 1.0)
        parity(f"{current_test()} {name} [u mag]", fig, bound, note=f"{what}; fp32 PyTorch {yard:.3g}")
        parity(f"{current_test()} {name} rel-L2", float((g - ref).norm() / ref.norm().clamp_min(1e-300)), 3e-6, note=what)
        print(f"{name:12s} {what:60s} kernel {fig:8.3f}  fp32 PyTorch {yard:8.3f}  bound {bound:8.3f}")
        if not fig <= bound:
            self.bad.append(f"{name}, {what}: {fig:.3g} units of u mag, plain fp32 PyTorch {yard:.3g}, allowed {bound:.3g}")

    def fraction(self, name, frac, what):
        parity(f"{current_test()} {name}", frac, 1.0, note=what)
        print(f"{name:12s} {what:60s} {frac:8.4f} of the bound")
        if not frac <= 1.0:
            self.bad.append(f"{name}, {what}: {frac:.3g} x its bound")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def twice(launch):
    """Run a launch twice (fresh outputs each time) and assert bit-equal results; returns the first."""
    first, second = launch(), launch()
    for a, c in zip(first, second):
        assert torch.equal(a, c), "two launches of the same case differ"
    return first


def untouched_outside(buf, view):
    """Does every element of `buf` outside `view` still hold SENT?"""
    probe = buf.clone()
    probe.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    return bool((probe == SENT).all())


# ---- (a) bdm_group_norm -------------------------------------------------------------------------------------------------------------
GN_RUNS = [(c, k) for c in GN_CASES for k in OFFSETS]


@pytest.mark.gpu
@pytest.mark.parametrize("case,k", GN_RUNS, ids=[f"{c.id}-k{k}" for c, k in GN_RUNS])
def test_group_norm_against_float64(ops, case, k):
    seed = 100 * GN_CASES.index(case) + 7
    shape = (case.b, case.c, case.l)
    x0, r0 = channel_data(shape, k, seed), 0.5 * channel_data(shape, -0.5 * k, seed + 1)
    gamma, beta = affine(case.c, seed + 2)
    xd, rd, gd, bd = x0.to(DEV), r0.to(DEV), gamma.to(DEV), beta.to(DEV)
    fig = Figures()
    for with_res in (False, True):
        v32 = x0 + r0 if with_res else x0
        h, mag = gn64(x0.double() + r0.double() if with_res else x0.double(), x0.abs().double() + (r0.abs().double() if with_res else 0),
                      case.groups, gamma, beta)
        plain = TF.group_norm(v32, case.groups, gamma, beta, EPS)
        for act in (False, True):
            def launch(inplace):
                xbuf, x, res, obuf, out = gn_tensors(case, DEV, inplace, with_res)
                x.copy_(xd)
                if res is not None:
                    res.copy_(rd)
                assert gn_route(x, res, out, case.groups) == case.route
                assert case.view != "lead1" or (x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4)
                y = ops.group_norm_(x, gd, bd, groups=case.groups, eps=EPS, swish=act, residual=res, out=None if inplace else out)
                assert y.data_ptr() == out.data_ptr()
                assert inplace or torch.equal(x, xd), "out= launch changed its input"
                assert res is None or torch.equal(res, rd), "the residual was changed"
                return obuf, out
            obuf, y_out = twice(lambda: launch(False))
            ibuf, y_in = twice(lambda: launch(True))
            assert untouched_outside(obuf, y_out) and untouched_outside(ibuf, y_in), "a byte outside the view was written"
            assert torch.equal(y_in, y_out), "in place and out= differ on the same route"
            what = f"{'residual + ' if with_res else ''}GroupNorm({case.groups}){' + Swish' if act else ''}"
            fig.check("group_norm", y_out, swish(h) if act else h, U * mag, swish(plain) if act else plain, what)
    fig.done()


@pytest.mark.gpu
def test_group_norm_of_an_empty_batch_returns(ops):
    gamma, beta = affine(8, 1)
    x = torch.empty(0, 8, 16, device=DEV)
    assert ops.group_norm_(x, gamma.to(DEV), beta.to(DEV), groups=4) is x
    out = torch.empty(0, 8, 16, device=DEV)
    assert ops.group_norm_(x, gamma.to(DEV), beta.to(DEV), groups=4, swish=True, out=out) is out
    torch.cuda.synchronize()


# ---- (b) bdm_group_norm_stats -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STATS_CASES, ids=ids(STATS_CASES))
def test_group_norm_stats_against_float64(ops, case):
    from bdm_amd import _lib
    B, C, L, G = case.b, case.c, case.l, case.groups
    cg, S = C // G, stats_slices(case)
    steps = cg * L // 4 if case.route == VECTOR else cg * L   # float4 steps of the vector kernel, elements of the scalar one
    iters = cdiv(cdiv(steps, S), 256)
    fig = Figures()
    for k in OFFSETS:
        x0 = channel_data((B, C, L), k, 100 * GN_CASES.index(case) + 11)
        _, x = placed((B, C, L), "lead1" if case.view else "dense", DEV)
        x.copy_(x0)
        assert gn_route(x, None, x, G) == case.route

        def launch():
            ws = torch.full((B * G * 64 * 2,), float("nan"), dtype=torch.float64, device=DEV)
            n = ctypes.c_int(-1)
            _lib.check(_lib.lib().bdm_group_norm_stats(B, C, L, G, _lib.ptr(x), C * L, _lib.ptr(ws), ctypes.byref(n), _lib.stream()), "stats")
            assert n.value == S
            return ws[:B * G * S * 2], torch.isnan(ws[B * G * S * 2:])
        written, rest_is_nan = twice(launch)
        p = written.view(B, G, S, 2).cpu()
        assert bool(torch.isfinite(p).all()) and bool(rest_is_nan.all()), "slices written: not exactly the first S"
        v = x0.double().view(B, G, -1)
        got = p.sum(2)
        fs = float(((got[..., 0] - v.sum(-1)).abs() / ((4 * iters + 3) * U * v.abs().sum(-1))).max())
        fq = float(((got[..., 1] - (v * v).sum(-1)).abs() / ((4 * iters + 4) * U * (v * v).sum(-1))).max())
        fig.fraction("sum", fs, f"k = {k}, {S} slices, chains of {iters}")
        fig.fraction("sum of squares", fq, f"k = {k}, {S} slices, chains of {iters}")
    fig.done()


# ---- (c) maximum over the neighbours --------------------------------------------------------------------------------------------------
def on_device(t, lead):
    """A copy of t on the GPU, `lead` floats into its buffer."""
    flat = torch.empty(lead + t.numel(), device=DEV)
    view = flat[lead:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * lead
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("case", MX_CASES, ids=ids(MX_CASES))
def test_max_over_neighbors_gn_against_float64(ops, case):
    B, C, M, Uu, G = case.b, case.c, case.m, case.u, case.groups
    seed = 100 * MX_CASES.index(case) + 13
    gamma, beta = affine(C, seed + 2)
    gn = gn_module(G, gamma, beta)
    fig = Figures()
    for k in OFFSETS:
        x0 = channel_data((B, C, M, Uu), k, seed)
        flat = x0.view(B, C, M * Uu)
        h, mag = gn64(flat.double(), flat.abs().double(), G, gamma, beta)
        ref = swish(h).view(B, C, M, Uu).max(-1).values
        rowmag = mag.view(B, C, M, Uu).max(-1).values
        plain = swish(TF.group_norm(flat, G, gamma, beta, EPS)).view(B, C, M, Uu).max(-1).values
        tot = group_totals(flat.double(), G)
        xd = on_device(x0, 1 if case.view == "lead1" else 0)
        assert mx_lanes(Uu, xd.data_ptr()) == case.lpr
        for S in MX_SLICES:
            p = uneven_partials(tot, S, seed + S).to(DEV)

            def launch():
                if case.view != "out":
                    y = ops.max_over_neighbors(xd, fold=((p, S, G), gn))
                    return y, y
                buf = torch.full((B, C + 3, M + 5), SENT, device=DEV)
                y = buf[:, 2:2 + C, 1:1 + M]
                assert ops.max_over_neighbors(xd, out=y, fold=((p, S, G), gn)).data_ptr() == y.data_ptr()
                return buf, y
            buf, y = twice(launch)
            assert case.view != "out" or untouched_outside(buf, y), "a byte outside the output view was written"
            fig.check("max_gn", y, ref, U * rowmag, plain, f"k = {k}, {S} slices, {case.lpr} lanes per row")
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize("u", PLAIN_U)
def test_plain_max_over_neighbors_is_exact(ops, u):
    x0 = channel_data((2, 16, 65, u), 1.3, 900 + u)
    xd = on_device(x0, 0)
    (y,) = twice(lambda: (ops.max_over_neighbors(xd),))
    assert torch.equal(y, xd.max(-1).values) and torch.equal(y.cpu(), x0.max(-1).values)
    buf = torch.full((2, 19, 70), SENT, device=DEV)
    view = buf[:, 2:18, 1:66]
    ops.max_over_neighbors(xd, out=view)
    assert torch.equal(view, y) and untouched_outside(buf, view)


@pytest.mark.gpu
def test_plain_max_over_neighbors_on_a_misaligned_base(ops):
    """u % 4 == 0 one float into a buffer: the scalar loop (the float4 loop needs 16-byte aligned rows)."""
    for u in (32, 4, 260):
        x0 = channel_data((2, 16, 65, u), 1.3, 950 + u)
        xd = on_device(x0, 1)
        (y,) = twice(lambda: (ops.max_over_neighbors(xd),))
        assert torch.equal(y.cpu(), x0.max(-1).values), u


# ---- (d) SE row means, affine forms, gates -------------------------------------------------------------------------------------------
def se_weights(c, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(hidden, c, generator=g) / c ** 0.5, torch.randn(c, hidden, generator=g) / hidden ** 0.5


def se_gate64(mean, w1, w2):
    """(gate, its bound term 1 + sum |w2| |hidden|) in the precision of `mean`."""
    hid = torch.relu(mean @ w1.to(mean.dtype).T)
    return torch.sigmoid(hid @ w2.to(mean.dtype).T), 1.0 + hid.abs() @ w2.to(mean.dtype).abs().T


def coef_ref(v, groups, gamma, beta):
    """Affine forms (gamma rstd, beta - mean gamma rstd) per (shape, channel) in the precision of v (B, C, L), and their bound terms."""
    B, C = v.shape[:2]
    vg = v.reshape(B, groups, -1)
    mean = vg.mean(-1, keepdim=True).expand(B, groups, C // groups).reshape(B, C)
    rstd = (1.0 / torch.sqrt(vg.var(-1, unbiased=False, keepdim=True) + EPS)).expand(B, groups, C // groups).reshape(B, C)
    ga, be = gamma.to(v.dtype)[None], beta.to(v.dtype)[None]
    a = ga * rstd
    return torch.stack([a, be - mean * a], -1), torch.stack([a.abs(), be.abs() + (mean * a).abs()], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SE_CASES, ids=ids(SE_CASES))
def test_se_means_and_gates_against_float64(ops, case):
    B, C, hidden, l, G = SE_B, case.c, case.hidden, case.l, case.groups
    seed = 100 * SE_CASES.index(case) + 17
    gamma, beta = affine(C, seed + 2)
    pgamma, pbeta = affine(C, seed + 3)
    gn, pgn = gn_module(G, gamma, beta), gn_module(SE_PF_GROUPS, pgamma, pbeta)
    w1, w2 = se_weights(C, hidden, seed + 4)
    w1d, w2d = w1.to(DEV), w2.to(DEV)
    fig = Figures()
    for k in OFFSETS:
        x0, p0 = channel_data((B, C, l), k, seed), channel_data((B, C, SE_PF_POINTS), k, seed + 5)
        xd = on_device(x0, case.lead)
        # plain SE gate of x itself, both forms
        mean64 = x0.double().mean(-1)
        gate64, gmag = se_gate64(mean64, w1, w2)
        gate32, _ = se_gate64(x0.mean(-1), w1, w2)
        (g2,) = twice(lambda: (ops.se_gate(xd, w1d, w2d),))
        (g1,) = twice(lambda: (ops.se_gate(xd, w1d, w2d, fused=True),))
        assert torch.equal(g1, g2), "one-launch and two-launch SE gates differ"
        fig.check("se_gate", g2, gate64, U * gmag, gate32, f"k = {k}")
        # folded forms
        h, mag = gn64(x0.double(), x0.abs().double(), G, gamma, beta)
        mean64, mmag = swish(h).mean(-1), mag.mean(-1)
        mean32 = swish(TF.group_norm(x0, G, gamma, beta, EPS)).mean(-1)
        gate64, gmag = se_gate64(mean64, w1, w2)
        gate32, _ = se_gate64(mean32, w1, w2)
        coef64, cmag = coef_ref(x0.double(), G, gamma, beta)
        coef32, _ = coef_ref(x0, G, gamma, beta)
        pcoef64, pmag = coef_ref(p0.double(), SE_PF_GROUPS, pgamma, pbeta)
        pcoef32, _ = coef_ref(p0, SE_PF_GROUPS, pgamma, pbeta)
        tot, ptot = group_totals(x0.double(), G), group_totals(p0.double(), SE_PF_GROUPS)
        for S in SE_SLICES:
            stats = (uneven_partials(tot, S, seed + S).to(DEV), S)
            gate, coef = twice(lambda: ops.se_gate_gn(xd, stats, gn, w1d, w2d))
            mean, coef_m = twice(lambda: ops.se_means_gn(xd, stats, gn))
            assert torch.equal(coef, coef_m)
            what = f"k = {k}, {S} slices"
            fig.check("mean", mean, mean64, U * mmag, mean32, what)
            fig.check("coef", coef, coef64, U * cmag, coef32, what)
            fig.check("gate", gate, gate64, U * gmag, gate32, what)
            for PS in SE_PF_SLICES:
                pf = ((uneven_partials(ptot, PS, seed + 50 + PS).to(DEV), PS, SE_PF_GROUPS), pgn)
                gate_p, coef_p, pcoef = twice(lambda: ops.se_gate_gn(xd, stats, gn, w1d, w2d, pf=pf, n_points=SE_PF_POINTS))
                mean_p, coef_pm, pcoef_m = twice(lambda: ops.se_means_gn(xd, stats, gn, pf=pf, n_points=SE_PF_POINTS))
                assert torch.equal(gate_p, gate) and torch.equal(coef_p, coef) and torch.equal(coef_pm, coef), "pf changes the grid's results"
                assert torch.equal(mean_p, mean) and torch.equal(pcoef_m, pcoef)
                fig.check("pf_coef", pcoef, pcoef64, U * pmag, pcoef32, f"{what}, point branch {PS} slices")
    fig.done()


# ---- (e) devoxelisation -------------------------------------------------------------------------------------------------------------
def devox_coords(B, n, r, seed):
    """(B, 3, n) float32 in [0, r - 1]; one point in eight sits on exact integers on one, two or all three axes (0 and r - 1 among them)."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(B, 3, n, generator=g) * (r - 1)).clamp_(0.0, float(r - 1))
    lattice = torch.randint(0, r, (B, 3, n), generator=g).float()
    edge = (r - 1) * torch.randint(0, 2, (B, 3, n), generator=g).float()
    lattice[:, :, 0::16] = edge[:, :, 0::16]   # every other lattice point: on the grid's faces, edges or corners
    for j in range(0, n, 8):
        axes = [(0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)][(j // 8) % 7]
        for a in axes:
            c[:, a, j] = lattice[:, a, j]
    assert float(c.min()) >= 0.0 and float(c.max()) <= r - 1
    return c


def corners(coords, r):
    """The eight (cell index (B, n), weight (B, n)) pairs of every point, in the precision of coords; weight-0 corners stay in the grid."""
    lo = coords.floor()
    f1 = coords - lo
    f0 = 1.0 - f1
    lo = lo.long()
    hi = (lo + 1).clamp_max(r - 1)
    out = []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                ix, iy, iz = (hi if dx else lo)[:, 0], (hi if dy else lo)[:, 1], (hi if dz else lo)[:, 2]
                w = (f1 if dx else f0)[:, 0] * (f1 if dy else f0)[:, 1] * (f1 if dz else f0)[:, 2]
                out.append(((ix * r + iy) * r + iz, w))
    return out


def gather(vals, cs):
    """sum_i w_i vals[..., cell_i]: vals (B, C, r^3) -> (B, C, n)"""
    B, C = vals.shape[:2]
    return sum(w[:, None, :] * vals.gather(2, idx[:, None, :].expand(B, C, -1)) for idx, w in cs)


def devox_expected(dt, coords, r, grid, ab, gate, add, add_ab):
    """(result, bound term) of trilinear(swish(a grid + b) gate) + add' in dtype dt; ab None: the unfolded form trilinear(grid gate) + add."""
    cs = corners(coords.to(dt), r)
    g = grid.to(dt)
    s = gate.to(dt)[:, :, None] if gate is not None else torch.ones((), dtype=dt)
    if ab is not None:
        a, b = ab.to(dt)[:, :, 0:1], ab.to(dt)[:, :, 1:2]
        vals, vmag = swish(g * a + b) * s, ((g * a).abs() + b.abs()) * s.abs()
    else:
        vals, vmag = g * s, (g * s).abs()
    out, mag = gather(vals, cs), gather(vmag, cs)
    if add is not None:
        ad = add.to(dt)
        if add_ab is not None:
            pa, pb = add_ab.to(dt)[:, :, 0:1], add_ab.to(dt)[:, :, 1:2]
            out, mag = out + swish(ad * pa + pb), mag + (ad * pa).abs() + pb.abs()
        else:
            out, mag = out + ad, mag + ad.abs()
    return out, mag


@pytest.mark.gpu
@pytest.mark.parametrize("case", DV_CASES, ids=ids(DV_CASES))
def test_devoxelisation_against_float64(ops, case, monkeypatch):
    B, C, r, n = case.b, case.c, case.r, case.n
    seed = 100 * DV_CASES.index(case) + 19
    hidden = max(1, C // 8)
    g = torch.Generator().manual_seed(seed)
    coords = devox_coords(B, n, r, seed + 1)
    ab = torch.stack([0.4 * torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)], -1)
    add_ab = torch.stack([0.4 * torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)], -1)
    gate = 0.05 + 0.9 * torch.rand(B, C, generator=g)
    se_mean = torch.randn(B, C, generator=g)
    w1, w2 = se_weights(C, hidden, seed + 4)
    cd, abd, aabd, gated, meand, w1d, w2d = (t.to(DEV) for t in (coords, ab, add_ab, gate, se_mean, w1, w2))
    fig = Figures()

    def both_routes(launch):
        """The launch under the row's own BDM_STAGING (its route asserted), and bit-equal on the other route."""
        res = {}
        for staging in ("0", "1"):
            monkeypatch.setenv("BDM_STAGING", staging)
            assert dv_route(case, False, gridd.data_ptr()) == int(staging)
            (res[int(staging)],) = twice(lambda: (launch(),))
        assert torch.equal(res[0], res[1]), "LDS and global-memory devoxelisation differ"
        monkeypatch.delenv("BDM_STAGING")
        if case.staging is not None:
            monkeypatch.setenv("BDM_STAGING", case.staging)
        assert dv_route(case, False, gridd.data_ptr()) == case.route
        (own,) = twice(lambda: (launch(),))
        assert torch.equal(own, res[case.route])
        monkeypatch.delenv("BDM_STAGING", raising=False)
        return own

    for k in OFFSETS:
        grid, add = channel_data((B, C, r ** 3), k, seed + 2), channel_data((B, C, n), k, seed + 3)
        gridd, addd = grid.to(DEV), add.to(DEV)
        wide = torch.full((B, C + 5, n), SENT, device=DEV)
        adds = wide[:, 3:3 + C]
        adds.copy_(addd)
        assert adds.stride(0) != C * n
        variants = [("no gate, no add", None, None, None, None), ("gate + add", gated, addd, None, add),
                    ("gate + add as a channel slice", gated, adds, None, add), ("gate + Swish(GroupNorm(add))", gated, addd, aabd, add),
                    ("no gate, Swish(GroupNorm(add)) as a channel slice", None, adds, aabd, add)]
        for what, gt, ad, aab, ad_cpu in variants:
            got = both_routes(lambda: ops.devoxelize_gn_gate_add(cd, gridd, abd, r, gate=gt, add=ad, add_coef=aab))
            args = (coords, r, grid, ab, gate if gt is not None else None, ad_cpu, add_ab if aab is not None else None)
            ref, mag = devox_expected(torch.float64, *args)
            fig.check("devox_gn", got, ref, U * mag, devox_expected(torch.float32, *args)[0], f"k = {k}, {what}")
        # the SE layers evaluated in the kernel from the channel means (global-memory form only)
        s64, _ = se_gate64(se_mean.double(), w1, w2)
        s32, _ = se_gate64(se_mean, w1, w2)
        for what, ad, ad_cpu in (("SE + add", addd, add), ("SE + add as a channel slice", adds, add), ("SE, no add", None, None)):
            assert dv_route(case, True, gridd.data_ptr()) == 0
            (got,) = twice(lambda: (ops.devoxelize_gn_se_add(cd, gridd, abd, r, meand, w1d, w2d, add=ad),))
            ref, mag = devox_expected(torch.float64, coords, r, grid, ab, s64, ad_cpu, None)
            fig.check("devox_se", got, ref, U * mag, devox_expected(torch.float32, coords, r, grid, ab, s32, ad_cpu, None)[0], f"k = {k}, {what}")
        # the unfolded form
        for what, gt, ad, ad_cpu in (("gate + add", gated, addd, add), ("gate + add as a channel slice", gated, adds, add), ("plain", None, None, None)):
            (got,) = twice(lambda: (ops.devoxelize_gate_add(cd, gridd, r, gate=gt, add=ad),))
            args = (coords, r, grid, None, gate if gt is not None else None, ad_cpu, None)
            ref, mag = devox_expected(torch.float64, *args)
            fig.check("devox_plain", got, ref, U * mag, devox_expected(torch.float32, *args)[0], f"k = {k}, unfolded, {what}")
        assert untouched_outside(wide, adds) and torch.equal(adds, addd), "the addend was changed"
    fig.done()
