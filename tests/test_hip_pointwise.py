"""Every tile and epilogue of the 1x1-convolution GEMM (pw_gemm_kernel / pw_skinny_kernel, bdm_amd/csrc/dense_ops.hip) against float64.

The kernel picks its variant from (b, m, k, n): tiles of 32 MI rows x 128 NI columns with K chunk BK, or the skinny K-split kernel
with NB column blocks.  ONE case table below names, per row, the variant it is meant to reach.

* CPU half (no GPU): `bdm_pointwise_conv_variant` (the launch path's own chooser) returns that variant for every row; a sweep of
  the chooser over a grid of shapes returns no variant the table does not cover; the table holds the C2 step's own layer shapes.
* GPU half: every row against the same operation in float64 PyTorch on the CPU, ELEMENTWISE.

Tolerances (derived, none measured on the kernel):
* linear part: any summation order of K fp32 terms obeys
      |got - ref| <= (K + 4) 2^-24 1.01 (|W| |x| + |bias| + |batch_bias| + |residual|)      per output element
  (LeakyReLU scales by at most 1 and adds one rounding: inside the + 4).  Reported as the worst element's fraction of that bound
  (must be <= 1), next to the whole-tensor rel-L2 < 2e-6 the older tests assert.
* exact GELU and the folded Swish(GroupNorm(x)) operand go through erff / expf, whose accuracy is not derivable here: the yardstick
  is the same operation in plain fp32 PyTorch on the CPU, its worst elementwise distance from float64 in units of the bound above;
  the kernel may be at most 4x that far (another summation order, another libm).
* GroupNorm slice partials: one slice sums at most 32 x 128 = 4096 fp32 values before it goes to fp64, so per slice
      |sum err| <= 4096 2^-24 sum |v|,   |sum of squares err| <= 4097 2^-24 sum v^2       (v = the values the kernel WROTE)
* amax, the two-source form, a repeated launch and the tile-independence of a shape's results are bit-exact (torch.equal).
"""
import ctypes
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from helpers import current_test, parity

U = 2.0 ** -24
DEV = torch.device("cuda")


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# variant: (MI, NI, BK) of pw_gemm_kernel, or "skinny1" / "skinny2" (pw_skinny_kernel<NB>).
# halves: which GPU halves the row runs in -- "plain" (a), "two" (b), "fold" (c), "stats" (d; needs a power-of-two >= 4 channels per
# group that divides m).  Every row runs in every half it names; determinism (f) is asserted on every launch of every half.
# c2: the module of the C2 benchmark step (B = 16, N = 4096) whose 1x1 convolution has exactly this shape (test_c2_* derives them).
Case = namedtuple("Case", "id b m k n variant halves c2")
ALL = ("plain", "two", "fold", "stats")
CASES = [
    # (2, 2, 16): 64 x 256 tile
    Case("t22_mtail_n4133", 16, 100, 35, 4133, (2, 2, 16), ALL, None),         # M tail 36/64, 33 column blocks, n % 4 != 0, K % 16 != 0
    Case("t22_mtail_n4100", 16, 72, 200, 4100, (2, 2, 16), ALL, None),         # n % 4 == 0 (vector loads + the two other scalar triggers)
    Case("t22_k8", 16, 96, 8, 4000, (2, 2, 16), ALL, None),                    # K < BK; 32 rows per group: 3 row blocks over 64-row tiles
    Case("c2_classifier_hidden", 16, 128, 64, 4096, (2, 2, 16), ("plain", "stats"), "classifier.0.layers.0"),
    Case("c2_fp3_mlp1", 16, 128, 128, 4096, (2, 2, 16), ("two", "fold"), "fp_layers.3.0.mlp.layers.3"),
    Case("c2_sa1_attention_qkv", 16, 192, 64, 4096, (2, 2, 16), ("stats",), "sa_layers.1.0.voxel_layers attention q,k,v"),
    # (1, 2, 16): 32 x 256 tile (m <= 32 at large batch)
    Case("t12_n8200", 16, 24, 35, 8200, (1, 2, 16), ALL, None),                # M tail, 65 column blocks, n % 4 == 0
    Case("t12_n8195", 16, 32, 390, 8195, (1, 2, 16), ALL, None),               # n % 4 != 0, K % 16 != 0
    Case("t12_k8", 16, 28, 8, 8200, (1, 2, 16), ALL, None),                    # K < BK
    # (2, 1, 64): 64 x 128 tile, 64-deep K chunk
    Case("t21d_mtail_n4100", 16, 40, 200, 4100, (2, 1, 64), ALL, None),        # M tail, N tail, K % 64 != 0, n % 4 == 0
    Case("t21d_n4099", 16, 48, 131, 4099, (2, 1, 64), ALL, None),              # n % 4 != 0, K % 64 = 3
    Case("c2_fp3_mlp2", 16, 64, 128, 4096, (2, 1, 64), ("plain", "fold", "stats"), "fp_layers.3.0.mlp.layers.6"),
    # (2, 1, 16)
    Case("t21_mtail_n4100", 16, 40, 35, 4100, (2, 1, 16), ALL, None),
    Case("t21_k8_n4099", 16, 60, 8, 4099, (2, 1, 16), ALL, None),              # K < BK, n % 4 != 0
    Case("c2_fp3_pvconv_point", 16, 64, 64, 4096, (2, 1, 16), ("plain", "two", "stats"), "fp_layers.3.1.point_features.layers.0"),
    # (1, 1, 16)
    Case("t11_n301", 3, 24, 35, 301, (1, 1, 16), ALL, None),
    Case("t11_mtail_n300", 2, 40, 67, 300, (1, 1, 16), ALL, None),
    Case("t11_k8_rt2", 2, 128, 8, 260, (1, 1, 16), ALL, None),                 # K < BK; 64 rows per group
    Case("c2_sa0_pvconv_point", 16, 32, 32, 4096, (1, 1, 16), ("plain", "stats"), "sa_layers.0.1.point_features.layers.0"),
    # (1, 1, 64)
    Case("t11d_n1100", 1, 100, 200, 1100, (1, 1, 64), ALL, None),
    Case("t11d_n515", 2, 36, 323, 515, (1, 1, 64), ALL, None),
    Case("c2_sa3_mlp1", 16, 256, 256, 512, (1, 1, 64), ("fold", "stats"), "sa_layers.3.mlps.0.layers.3"),
    Case("c2_classifier_out", 16, 3, 128, 4096, (1, 1, 64), ("plain", "two", "fold"), "classifier.2"),
    # skinny kernel, one 32-column block
    Case("ts1_n7", 2, 40, 131, 7, "skinny1", ALL, None),
    Case("ts1_k1024", 2, 100, 1024, 20, "skinny1", ALL, None),
    Case("c2_global_attention_qkv", 16, 1536, 512, 16, "skinny1", ALL, "global_att q,k,v"),
    # skinny kernel, two 32-column blocks
    Case("ts2_n33", 2, 72, 136, 33, "skinny2", ALL, None),
    Case("ts2_k1000", 2, 100, 1000, 50, "skinny2", ALL, None),
    Case("c2_fp0_mlp1", 16, 256, 256, 64, "skinny2", ("fold", "stats"), "fp_layers.0.mlp.layers.3"),
]
CASE_IDS = [c.id for c in CASES]
WIDE = [(2, 2, 16), (1, 2, 16), (2, 1, 64), (2, 1, 16)]
# every variant the chooser can return today (pw_wide_bk() == 16 keeps the BK = 32 branches of pw_dispatch unreachable)
VARIANTS = [(1, 1, 16), (1, 1, 64), (1, 2, 16), (2, 1, 16), (2, 1, 64), (2, 2, 16), "skinny1", "skinny2"]
# (m, k, n, variant alone, variant as one of 16): the same shape under a small and under a wide tile (half e)
INDEPENDENCE = [(256, 384, 4096, (1, 1, 64), (2, 2, 16)), (128, 64, 32768, (2, 1, 16), (2, 2, 16))]


def chosen_variant(b, m, k, n):
    """What the launch path picks for this shape (host query: no GPU needed)."""
    from bdm_amd import _lib
    mi, ni, bk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nb = _lib.lib().bdm_pointwise_conv_variant(b, m, k, n, ctypes.byref(mi), ctypes.byref(ni), ctypes.byref(bk))
    return f"skinny{nb}" if nb else (mi.value, ni.value, bk.value)


def stat_widths(m):
    """Channels per group to ask statistics for: the widest below 32, 32, and the narrowest above 32 that divide m."""
    below = [cg for cg in (16, 8, 4) if m % cg == 0][:1]
    return below + [cg for cg in (32,) if m % cg == 0] + [cg for cg in (64, 128) if m % cg == 0][:1]


def fold_groups(k):
    """Two GroupNorm group counts (8 and fewer) that divide k."""
    return [g for g in (8, 5, 7, 4, 3, 2, 1) if k % g == 0][:2]


def split_points(k, chunk):
    """k1 of the two-source form: on a K-chunk boundary (when K spans more than one chunk) and off it."""
    on = [chunk * max(1, (k // 2) // chunk)] if k > chunk else []
    off = [k1 for k1 in {(k // 2) | 1, k - 1, 1} if 1 <= k1 < k and k1 % chunk]
    return on + sorted(off)[-2:]


# ---- CPU half -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_reaches_its_variant(case):
    assert chosen_variant(case.b, case.m, case.k, case.n) == case.variant
    assert set(case.halves) <= set(ALL) and case.halves
    if "stats" in case.halves:
        assert stat_widths(case.m), "no power-of-two group width divides m"
    if "fold" in case.halves:
        assert case.k <= 1024 and fold_groups(case.k)


def test_chooser_sweep_returns_only_covered_variants():
    """The variants the chooser CAN return (a few thousand shapes) are all in the table, and each of them has a row with a folded
    operand as well as plain ones.  Fails the day a retune makes another kernel instance reachable (the BK = 32 branches of
    pw_dispatch, say) without a row here."""
    seen = set()
    for b in (1, 2, 3, 8, 16, 32):
        for m in (3, 8, 24, 32, 33, 40, 64, 65, 100, 128, 192, 256, 512, 1536):
            for k in (8, 16, 35, 64, 127, 128, 200, 390, 512, 1024):
                for n in (1, 7, 16, 32, 33, 64, 65, 128, 129, 300, 512, 1100, 2048, 4096, 4133, 8192, 8200, 32768, 131072, 524288):
                    seen.add(chosen_variant(b, m, k, n))
    assert seen == set(VARIANTS), sorted(map(str, seen))
    for half in ALL:
        covered = {c.variant for c in CASES if half in c.halves}
        assert seen <= covered, f"no '{half}' row for {sorted(map(str, seen - covered))}"


def test_table_covers_the_edges_of_every_wide_tile():
    """Per 256-column / 64-row variant: an M tail inside the tile, an N tail (for NI = 2 an odd number of 128-column blocks), K not
    a multiple of BK, K below BK (where the chooser allows it: BK = 64 needs k >= 128), n % 4 != 0 and == 0 (the latter carry the
    misaligned-base and odd-row-stride launches), and statistics over fewer than 32, 32 and (m permitting) more than 32 rows."""
    for v in WIDE:
        mi, ni, bk = v
        rows = [c for c in CASES if c.variant == v]
        assert any(c.m % (32 * mi) for c in rows), v
        assert any(c.n % (128 * ni) and (ni == 1 or cdiv(c.n, 128) % 2 == 1) for c in rows), v
        assert any(c.k % bk for c in rows), v
        assert bk == 64 or any(c.k < bk for c in rows), v
        for half in ("plain", "two", "fold"):
            assert any(c.n % 4 for c in rows if half in c.halves) and any(c.n % 4 == 0 for c in rows if half in c.halves), (v, half)
        widths = {cg for c in rows if "stats" in c.halves for cg in stat_widths(c.m)}
        assert min(widths) < 32 and 32 in widths and (mi == 1 or max(widths) > 32), (v, widths)
        # amax_rows 32 / 64 / 128 against the tile's rows, with m not a multiple of amax_rows
        assert any(c.m % 64 and c.m % 128 for c in rows if "stats" in c.halves), v
    for v in VARIANTS:
        assert any(fold_groups(c.k)[0] == 8 for c in CASES if c.variant == v and "fold" in c.halves), v
        assert any(fold_groups(c.k)[-1] < 8 for c in CASES if c.variant == v and "fold" in c.halves), v


def c2_step_layers():
    """(b, m, k, n) of 1x1 convolutions of the C2 step (B = 16 shapes, N = 4096 points), read off the denoiser's own modules."""
    from bdm_amd.modules import Attention, PVConv
    from bdm_amd.pvcnn import PVCNN2Base
    B, N = 16, 4096
    net = PVCNN2Base(num_classes=3, embed_dim=64)
    points = [N] + [sa[1][0] for sa in net.sa_blocks]     # points per level: the centers of each set abstraction

    def conv(mod, n):
        return (B, mod.weight.shape[0], mod.weight[0].numel(), n)

    def qkv(att, n):
        c = att.q.weight.shape[0]
        return (B, 3 * c, c, n)

    pv0 = [m for m in net.sa_layers[0] if isinstance(m, PVConv)][1]
    pv1 = net.sa_layers[1][0]
    att1 = [m for m in pv1.voxel_layers if isinstance(m, Attention)][0]
    fp3_pv = [m for m in net.fp_layers[3] if isinstance(m, PVConv)][0]
    return {
        "sa_layers.0.1.point_features.layers.0": conv(pv0.point_features.layers[0], points[0]),
        "sa_layers.1.0.voxel_layers attention q,k,v": qkv(att1, pv1.resolution ** 3),
        "sa_layers.3.mlps.0.layers.3": conv(net.sa_layers[3].mlps[0].layers[3], points[4] * net.sa_blocks[3][1][2]),
        "global_att q,k,v": qkv(net.global_att, points[4]),
        "fp_layers.0.mlp.layers.3": conv(net.fp_layers[0][0].mlp.layers[3], points[3]),
        "fp_layers.3.0.mlp.layers.3": conv(net.fp_layers[3][0].mlp.layers[3], N),
        "fp_layers.3.0.mlp.layers.6": conv(net.fp_layers[3][0].mlp.layers[6], N),
        "fp_layers.3.1.point_features.layers.0": conv(fp3_pv.point_features.layers[0], N),
        "classifier.0.layers.0": conv(net.classifier[0].layers[0], N),
        "classifier.2": conv(net.classifier[-1], N),
    }


def test_c2_step_layers_are_in_the_table_verbatim():
    layers = c2_step_layers()
    rows = {c.c2: (c.b, c.m, c.k, c.n) for c in CASES if c.c2}
    assert rows == layers
    # the step uses every variant but the 32 x 256 tile (m <= 32 rows at B = 16 never has 512 such tiles): one row each
    assert {c.variant for c in CASES if c.c2} == set(VARIANTS) - {(1, 2, 16)}


@pytest.mark.parametrize("m,k,n,alone,batched", INDEPENDENCE)
def test_independence_shapes_change_tile_with_the_batch(m, k, n, alone, batched):
    assert chosen_variant(1, m, k, n) == alone and chosen_variant(16, m, k, n) == batched


# ---- GPU half -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(hip):
    from bdm_amd import ops as o
    return o


_cache = {}


def case_data(case):
    """Inputs of a row (float32, CPU) and the float64 linear part W x with its bound term |W| |x|; one row is kept at a time."""
    if _cache.get("id") != case.id:
        _cache.clear()
        g = torch.Generator().manual_seed(1000 + CASE_IDS.index(case.id))
        b, m, k, n = case.b, case.m, case.k, case.n
        x = torch.randn(b, k, n, generator=g) * (0.5 + torch.rand(1, k, 1, generator=g)) + 0.3 * torch.randn(1, k, 1, generator=g)
        d = dict(id=case.id, x=x, w=torch.randn(m, k, generator=g) / k ** 0.5, bias=torch.randn(m, generator=g),
                 bb=torch.randn(b, m, generator=g), res=torch.randn(b, m, n, generator=g))
        d["lin"] = torch.matmul(d["w"].double(), x.double())
        d["mag"] = torch.matmul(d["w"].double().abs(), x.double().abs())
        _cache.update(d)
    return _cache


def linear_bound(k, *magnitudes):
    return (k + 4) * U * 1.01 * sum(magnitudes)


def worst_fraction(got, ref, bound):
    """max over the elements of |got - ref| / bound, in float64 on the device of `got` (ref, bound: float64 from the CPU)."""
    return float(((got.double() - ref.to(got.device)).abs() / bound.to(got.device).clamp_min(1e-300)).max())


def check_linear(got, ref, bound, what):
    # (one parity name per test and kind: the session summary keeps the worst launch of each)
    frac = parity(current_test() + " elementwise", worst_fraction(got, ref, bound), 1.0, note=what)
    r = ref.to(got.device)
    l2 = parity(current_test() + " rel-L2", float((got.double() - r).norm() / r.norm()), 2e-6, note=what)
    assert frac <= 1.0, f"{what}: an element is {frac:.3g} x its bound (K + 4) 2^-24 1.01 (|W||x| + ...)"
    assert l2 < 2e-6, f"{what}: rel-L2 {l2:.3e}"


def check_yardstick(got, plain32, ref, bound, what):
    """got within 4x the distance plain fp32 PyTorch (CPU) keeps from float64, both in units of the elementwise bound."""
    yard = float(((plain32.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    frac = parity(current_test() + " vs 4 x fp32 PyTorch", worst_fraction(got, ref, bound), 4 * yard,
                  note=f"{what}; fp32 PyTorch on the CPU: {yard:.3g} of the elementwise bound")
    assert frac <= 4 * yard, f"{what}: worst element {frac:.3g} of its bound, plain fp32 PyTorch {yard:.3g}"


def twice(launch):
    """Run a launch twice (fresh outputs each time) and assert bit-equal results (f); returns the first."""
    first, second = launch(), launch()
    for a, c in zip(first, second):
        assert torch.equal(a, c), "two launches of the same case differ"
    return first


def embedded(t, channels_before, channels_after, columns_after=0, lead=0):
    """A copy of (B, C, L) `t` on the device as a view into a larger buffer: extra channels around it (batch stride > C * ld), extra
    columns after each row (row stride L + columns_after) and `lead` floats before the first element."""
    B, C, L = t.shape
    flat = torch.zeros(lead + B * (C + channels_before + channels_after) * (L + columns_after), device=DEV)
    big = flat[lead:].view(B, C + channels_before + channels_after, L + columns_after)
    view = big[:, channels_before:channels_before + C, :L]
    view.copy_(t)
    return view


def half_plain(ops, case):
    d = case_data(case)
    b, m, k, n = case.b, case.m, case.k, case.n
    x, w, bias, bb, res = (d[key].to(DEV) for key in ("x", "w", "bias", "bb", "res"))
    lin, mag = d["lin"], d["mag"]
    bias64, bb64 = d["bias"].double()[None, :, None], d["bb"].double()[:, :, None]
    ref0, bound0 = lin + bias64, linear_bound(k, mag, bias64.abs())
    (y0,) = twice(lambda: (ops.pointwise_conv(x, w, bias),))
    check_linear(y0, ref0, bound0, "bias")
    # the operand as a view: channel slice with a larger batch stride; then, one at a time, the two other triggers of the scalar-load
    # path (n % 4 != 0 is the row's own): base one float into its buffer, row stride not a multiple of 4 -- same values, same bits
    pad = 3 if n % 4 != 1 else 2
    views = (("batch stride", embedded(d["x"], 2, 3)), ("base + 4 bytes", embedded(d["x"], 0, 0, lead=1)),
             ("odd row stride", embedded(d["x"], 4, 1, columns_after=pad)))
    assert views[0][1].stride(0) > k * n and views[1][1].data_ptr() % 16 == 4 and views[2][1].stride(1) % 4 != 0
    for what, view in views:
        (yv,) = twice(lambda: (ops.pointwise_conv(view, w, bias),))
        check_linear(yv, ref0, bound0, what)
        assert torch.equal(yv, y0), what
    # every epilogue term, written into a channel slice of a larger buffer
    full64 = ref0 + bb64
    ref2 = TF.leaky_relu(full64, 0.1) + d["res"].double()
    bound2 = linear_bound(k, mag, bias64.abs(), bb64.abs(), d["res"].double().abs())

    def into_slice():
        buf = torch.zeros(b, m + 5, n, device=DEV)
        ops.pointwise_conv(x, w, bias, out=buf[:, 3:3 + m], batch_bias=bb, act=2, slope=0.1, residual=res)
        return (buf,)
    (buf,) = twice(into_slice)
    check_linear(buf[:, 3:3 + m], ref2, bound2, "bias + batch_bias + LeakyReLU + residual")
    assert float(buf[:, :3].abs().max()) == 0.0 and float(buf[:, 3 + m:].abs().max()) == 0.0
    # exact GELU
    ref3 = TF.gelu(full64) + d["res"].double()
    plain = TF.gelu(TF.conv1d(d["x"], d["w"][:, :, None], d["bias"]) + d["bb"][:, :, None]) + d["res"]
    (y3,) = twice(lambda: (ops.pointwise_conv(x, w, bias, batch_bias=bb, act=3, residual=res),))
    check_yardstick(y3, plain, ref3, bound2, "GELU")


def half_two(ops, case):
    d = case_data(case)
    k = case.k
    x, w, bias = d["x"].to(DEV), d["w"].to(DEV), d["bias"].to(DEV)
    bias64 = d["bias"].double()[None, :, None]
    ref0, bound0 = d["lin"] + bias64, linear_bound(k, d["mag"], bias64.abs())
    whole = ops.pointwise_conv(x, w, bias)
    chunk = 8 if isinstance(case.variant, str) else case.variant[2]   # (skinny: a wave's K range is cut in 8-deep blocks)
    k1s = split_points(k, chunk)
    assert any(k1 % chunk for k1 in k1s) and (k <= chunk or any(k1 % chunk == 0 for k1 in k1s))
    for k1 in k1s:
        x1 = d["x"][:, :k1].contiguous().to(DEV)
        x2 = embedded(d["x"][:, k1:], 2, 1)   # strided view
        (y,) = twice(lambda: (ops.pointwise_conv_gn(x1, w, bias, x2=x2),))
        assert torch.equal(y, whole), f"k1 = {k1}: reading cat([x, x2]) in place differs from the concatenated copy"
    check_linear(y, ref0, bound0, f"two sources, k1 = {k1}")


def group_norm_swish64(x, groups, gamma, beta, eps):
    B, K, n = x.shape
    xg = x.double().view(B, groups, -1)
    mean, var = xg.mean(-1, keepdim=True), xg.var(-1, unbiased=False, keepdim=True)
    h = ((xg - mean) / torch.sqrt(var + eps)).view(B, K, n) * gamma.double()[None, :, None] + beta.double()[None, :, None]
    return h * torch.sigmoid(h)


def producer_partials(x, groups):
    """(sum, sum of squares) of x per (shape, group) in slices of 128 columns, float64: what the producing convolution leaves."""
    B, K, n = x.shape
    S = cdiv(n, 128)
    xp = torch.zeros(B, K, S * 128, dtype=torch.float64)
    xp[:, :, :n] = x.double()
    t = xp.view(B, groups, K // groups, S, 128)
    return torch.stack([t.sum(dim=(2, 4)), (t * t).sum(dim=(2, 4))], -1).contiguous(), S


def half_fold(ops, case):
    d = case_data(case)
    k = case.k
    x, w, bias = d["x"].to(DEV), d["w"].to(DEV), d["bias"].to(DEV)
    bias64 = d["bias"].double()[None, :, None]
    g = torch.Generator().manual_seed(7)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.3 * torch.randn(k, generator=g)
    for groups in fold_groups(k):
        gn = torch.nn.GroupNorm(groups, k, eps=1e-5)
        gn.weight.data.copy_(gamma)
        gn.bias.data.copy_(beta)
        h64 = group_norm_swish64(d["x"], groups, gamma, beta, gn.eps)
        ref = torch.matmul(d["w"].double(), h64) + bias64
        bound = linear_bound(k, torch.matmul(d["w"].double().abs(), h64.abs()), bias64.abs())
        with torch.no_grad():
            plain = TF.conv1d(TF.silu(gn(d["x"])), d["w"][:, :, None], d["bias"])
        partial, S = producer_partials(d["x"], groups)
        gn = gn.to(DEV)
        stats = (partial.to(DEV), S, groups)
        (y,) = twice(lambda: (ops.pointwise_conv_gn(x, w, bias, fold_in=(stats, gn)),))
        check_yardstick(y, plain, ref, bound, f"Swish(GroupNorm({groups})) operand")


def slice_sums(y, cg):
    """Per (shape, group, slice) sum, sum of squares and sum of magnitudes of y (B, M, n) float64 over the canonical regions: the 32-row
    blocks of a group (the whole group below 32 rows) x the 128-column blocks, slice = column block * row blocks + row block."""
    B, M, n = y.shape
    G, rb, rt, ncb = M // cg, min(cg, 32), max(cg // 32, 1), cdiv(n, 128)
    yp = torch.zeros(B, M, ncb * 128, dtype=torch.float64, device=y.device)
    yp[:, :, :n] = y
    t = yp.view(B, G, rt, rb, ncb, 128)

    def red(v):
        return v.sum(dim=(3, 5)).permute(0, 1, 3, 2).reshape(B, G, ncb * rt)
    return red(t), red(t * t), red(t.abs())


def check_slices(y, stats, cg, case, what):
    from bdm_amd import _lib
    partial, slices, groups = stats
    B, M, n = y.shape
    assert groups == M // cg and slices == _lib.lib().bdm_pointwise_conv_gn_slices(case.b, M, case.k, n, groups)
    assert slices == cdiv(n, 128) * max(cg // 32, 1)
    s, q, a = slice_sums(y.double(), cg)
    p = partial.view(B, groups, slices, 2)
    fs = float(((p[..., 0] - s).abs() / (4096 * U * a).clamp_min(1e-300)).max())
    fq = float(((p[..., 1] - q).abs() / (4097 * U * q).clamp_min(1e-300)).max())
    parity(current_test() + " slice sums", fs, 1.0, note=f"{what}, {cg} rows per group")
    parity(current_test() + " slice sums of squares", fq, 1.0, note=f"{what}, {cg} rows per group")
    assert fs <= 1.0 and fq <= 1.0, f"{what}, {cg} rows per group: a slice is {fs:.3g} / {fq:.3g} x its bound"


def check_amax(y, am, rows, what):
    B, M, n = y.shape
    slots = cdiv(M, rows)
    ya = torch.zeros(B, slots * rows, n, device=y.device)
    ya[:, :M] = y.abs()
    assert torch.equal(am.view(B, slots), ya.view(B, slots, rows * n).amax(-1)), f"{what}: amax, {rows} rows per slot"


def half_stats(ops, case):
    d = case_data(case)
    b, m, k, n = case.b, case.m, case.k, case.n
    x, w, bias, bb, res = (d[key].to(DEV) for key in ("x", "w", "bias", "bb", "res"))
    bias64, bb64, add64 = d["bias"].double()[None, :, None], d["bb"].double()[:, :, None], d["res"].double()
    ref0, bound0 = d["lin"] + bias64, linear_bound(k, d["mag"], bias64.abs())
    widths = stat_widths(m)
    for cg in widths:
        def launch():
            yy, s = ops.pointwise_conv_gn(x, w, bias, out_groups=m // cg)
            return yy, s[0]
        y, st = twice(launch)
        check_linear(y, ref0, bound0, f"statistics, {cg} rows per group")
        check_slices(y, (st, st.numel() // (2 * b * (m // cg)), m // cg), cg, case, "plain")
    cg = widths[0]
    # per-shape bias inside the statistics and amax (bdm_pointwise_conv_gn_bb); amax_rows below / at / above the tile's rows
    ref_bb, bound_bb = ref0 + bb64, linear_bound(k, d["mag"], bias64.abs(), bb64.abs())
    for rows in (32, 64, 128):
        def launch():
            am = torch.zeros(b * cdiv(m, rows), device=DEV)
            yy, s = ops.pointwise_conv_gn(x, w, bias, out_groups=m // cg, amax=am, amax_rows=rows, batch_bias=bb)
            return yy, s[0], am
        y, st, am = twice(launch)
        check_amax(y, am, rows, "batch_bias")
    check_linear(y, ref_bb, bound_bb, "batch_bias")
    check_slices(y, (st, st.numel() // (2 * b * (m // cg)), m // cg), cg, case, "batch_bias")
    # amax alone (the attention projections' form)
    rows = 64

    def launch():
        am = torch.zeros(b * cdiv(m, rows), device=DEV)
        return ops.pointwise_conv_gn(x, w, bias, amax=am, amax_rows=rows), am
    y, am = twice(launch)
    check_amax(y, am, rows, "amax alone")
    if isinstance(case.variant, str):
        return   # the per-element addend is not offered on the skinny shapes (the entry point refuses them)
    # per-element addend inside the statistics and amax (bdm_pointwise_conv_gn_add), alone and with the per-shape bias
    cg = widths[-1]
    for with_bb in (False, True):
        def launch():
            am = torch.zeros(b * cdiv(m, 32), device=DEV)
            yy, s = ops.pointwise_conv_gn(x, w, bias, out_groups=m // cg, amax=am, amax_rows=32, add=res, batch_bias=bb if with_bb else None)
            return yy, s[0], am
        y, st, am = twice(launch)
        what = "add + batch_bias" if with_bb else "add"
        check_linear(y, ref0 + add64 + (bb64 if with_bb else 0), linear_bound(k, d["mag"], bias64.abs(), add64.abs(), bb64.abs() if with_bb else 0), what)
        check_slices(y, (st, st.numel() // (2 * b * (m // cg)), m // cg), cg, case, what)
        check_amax(y, am, 32, what)


HALVES = {"plain": half_plain, "two": half_two, "fold": half_fold, "stats": half_stats}
GPU_RUNS = [(c, h) for c in CASES for h in ALL if h in c.halves]


@pytest.mark.gpu
@pytest.mark.parametrize("case,half", GPU_RUNS, ids=[f"{c.id}-{h}" for c, h in GPU_RUNS])
def test_pointwise_against_float64(ops, case, half):
    assert chosen_variant(case.b, case.m, case.k, case.n) == case.variant
    HALVES[half](ops, case)


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n,alone,batched", INDEPENDENCE)
def test_results_do_not_depend_on_the_tile(ops, m, k, n, alone, batched):
    """(e) A shape launched alone (small tile) and as shape r of 16 different ones (wide tile): the same output bits, the same
    statistics slices, the same amax -- the canonical decomposition dense_ops.hip promises ("a shape must not see its batch-mates"),
    for the plain operand, the folded one, and every epilogue term."""
    assert chosen_variant(1, m, k, n) == alone and chosen_variant(16, m, k, n) == batched
    g = torch.Generator().manual_seed(m + k)
    B, r = 16, 11
    x = (torch.randn(B, k, n, generator=g) * 0.7 + 0.2).to(DEV)
    w, bias = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV), torch.randn(m, generator=g).to(DEV)
    bb = torch.randn(B, m, generator=g).to(DEV)
    gn = torch.nn.GroupNorm(8, k, eps=1e-5)
    gn.weight.data.copy_(1 + 0.3 * torch.randn(k, generator=g))
    gn.bias.data.copy_(0.3 * torch.randn(k, generator=g))
    gn = gn.to(DEV)
    S = cdiv(n, 128)
    xs = torch.zeros(B, k, S * 128, dtype=torch.float64, device=DEV)
    xs[:, :, :n] = x.double()
    t = xs.view(B, 8, k // 8, S, 128)
    in_partial = torch.stack([t.sum(dim=(2, 4)), (t * t).sum(dim=(2, 4))], -1).contiguous()
    del xs, t
    one = slice(r, r + 1)
    for cg in (16, 32, 64):
        for fold in (False, True):
            def launch(sel, nb):
                am = torch.zeros(nb * cdiv(m, 64), device=DEV)
                fi = ((in_partial[sel].contiguous(), S, 8), gn) if fold else None
                y, st = ops.pointwise_conv_gn(x[sel], w, bias, fold_in=fi, out_groups=m // cg, amax=am, amax_rows=64, batch_bias=bb[sel])
                return y, st[0].view(nb, m // cg, st[1], 2), am.view(nb, -1)
            ya, pa, aa = twice(lambda: launch(one, 1))
            yb, pb, ab = twice(lambda: launch(slice(None), B))
            what = f"{cg} rows per group, {'folded' if fold else 'plain'} operand"
            assert torch.equal(ya[0], yb[r]), f"output depends on the tile ({what})"
            assert torch.equal(aa[0], ab[r]), f"amax depends on the tile ({what})"
            assert torch.equal(pa[0], pb[r]), f"statistics slices depend on the tile ({what})"
    res = torch.randn(1, m, n, generator=g).to(DEV)
    for act in (0, 2, 3):
        ya = ops.pointwise_conv(x[one], w, bias, batch_bias=bb[one], act=act, slope=0.1, residual=res)
        xr = x.clone()
        yb = ops.pointwise_conv(xr, w, bias, batch_bias=bb, act=act, slope=0.1, residual=res.expand(B, -1, -1).contiguous())
        assert torch.equal(ya[0], yb[r]), f"output depends on the tile (act = {act})"
