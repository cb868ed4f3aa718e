"""Every tile of the dense fp16x3 3x3x3 convolution (conv3d_h2q_kernel, bdm_amd/csrc/conv3d_h2.hip), its GroupNorm-statistics
epilogue, its weight packer and its operand producer against float64.

The launcher picks one of eight kernel instances <MT, NT, R, TX, TY, NW> from (b, cout, r).  ONE case table below names, per row, the
instance it is meant to reach.

* CPU half (no GPU): `bdm_conv3d_h2_variant` (the launch path's own chooser) returns that instance for every row; a sweep of the
  chooser returns no instance the table lacks; the table holds the C2 step's own layers; and the elementwise bound below is checked
  against a plain torch restatement of the kernel's arithmetic (`emulate`): the restatement stays inside it, the same restatement
  with one of the three partial products dropped, or with one tap reading the neighbouring voxel, falls outside it.
* GPU half: every row through ops.to_h2 -> ops.conv3d_h2 / ops.conv3d_h2_gn against TF.conv3d in float64 on the CPU.

The elementwise bound (derived; nothing in it is measured on the kernel).  Notation: u = 2^-24; a = w 2^e[co] and b = x s are the
operands after their exact power-of-two scaling; K = 27 * 8 * ceil(cin / 8) products per output element (pads included).

1. Operand representation.  hi = RN16(a) has an 11-bit significand: for a in [2^e, 2^(e+1)) |a - hi| <= 2^(e-11) <= 2^-11 |a|.  The
   remainder is a multiple of fp32's ulp 2^(e-23), so it is an integer of at most 2^12 such units; fp16 holds integers up to 2^11
   exactly and only the EVEN ones from there to 2^12, so lo = RN16(a - hi) can be off by one unit:
       |a - (hi + lo)| <= 2^(e-23) <= 2^-23 |a| = 2 u |a|
   -- hi (11 bits) + the sign of lo + lo (11 bits) hold 23 of fp32's 24 bits; the "2^-24 |x|" in the header of conv3d_h2.hip is
   the typical case, not the worst one.  Below fp16's normal range (|lo| < 2^-14, spacing 2^-24) the error is absolute, <= 2^-25 in
   scaled units.  Both cases are covered by padding the magnitudes the bound is taken over:
       |x|~ = |x| + 2^-2 / s                     (2^-25 / s = 2 u * 2^-2 / s)
       |w|~ = |w| + 2^-11 max |w[co]|            (2^-25 2^-e[co] <= 2^-34 max |w[co]|, as max |w[co]| 2^e[co] >= 2^9)
   so that |a - (hi + lo)| <= 2 u |a|~ for every operand, and a product of two represented operands is within
   2 u (2 + 2 u) |a|~ |b|~ of a b.
2. The dropped lo.lo term: |lo| <= 2^-11 (1 + 2^-11) |a|~, so |a_lo b_lo| <= 2^-22 (1 + 2^-10) |a|~ |b|~ = 4.004 u |a|~ |b|~ (the
   header's "2^-24 |a b|" is again the typical size).
3. Each of the three remaining partial products is exact in fp32 (11 x 11 bits); their sum over the K products, 3K fp32 terms added
   in any order with one rounding per addition, is within (3K - 1) u / (1 - 3K u) of the sum of their magnitudes,
   <= (1 + 2^-10 + 2^-22) sum |a|~ |b|~.  Unscaling is exact; adding the bias is one more rounding.
Together, per output element, with |W|~ (*) |x|~ a second float64 convolution of the padded magnitudes:
       |got - ref| <= c(K) u (|W|~ (*) |x|~ + |bias|),        c(K) = 1.01 (3K + 10)
(4.000001 + 4.004 + 1 < 10; the factor 1.01 covers 1 / (1 - 3K u) and the (1 + 2^-10) for cin <= 264.)

That constant is far looser than what tells a good kernel from a broken one: c(K) grows like 3K, while the error of a correct kernel
stays near 1 u (|W|~ (*) |x|~) at every K (3K roundings of random sign), and a kernel without its lo.hi products is off by about
2^-12 sqrt(K) |w| |x| per element -- inside c(K) u K |w| |x| from cin = 16 on.  So the bound in force is the tighter of c(K) and a
constant taken from the restatement: over every row and input family of EMULATION_ROWS (cin from 1 to 256; corner voxels of
cin = 1 sum only 8 products) the restatement's worst element is at 3.83 u (|W|~ (*) |x|~ + |bias|) (family "outlier", cin = 1; per
family, worst row: normal 2.89, wide 2.84, tiny 3.08, outlier 3.83; at cin = 256: 1.28, 0.81, 0.96, 1.23).  EMU_WORST = 3.9 is
asserted by test_emulation_stays_inside_the_bound, and the kernel may be 4 x that far (another summation order inside the matrix
instruction, thousands of times as many elements):
       c = min(c(K), 4 EMU_WORST) = min(1.01 (3K + 10), 15.6)
The mutants of test_broken_emulation_falls_outside_the_bound are at 196 u (hi.lo dropped, "outlier", cin = 256) to 4900 u (a dropped
product) and 5e5 u to 3e7 u (a shifted tap): at least 12 x outside.

GroupNorm slice partials: a canonical unit sums 64 UB fp32 values per 4-channel block before going to fp64 (a lane: 4 channels of
one voxel; butterfly over the 16 voxels of a block; the unit's UB blocks in ascending order) -- UB = r^2 / 16 at 8^3 and 16^3 (an
x-plane), 32 at 32^3 (a 2 x 8 x 32 tile): n32 = 256 / 1024 / 2048 values.  Per slice and group, against the values the kernel WROTE:
       |sum err| <= n32 u sum |v|,        |sum of squares err| <= (n32 + 1) u sum v^2

Exact rows, repeated launches, tile independence (outputs AND slice partials), packer scales: bit-exact (torch.equal).
"""
import ctypes
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from helpers import current_test, parity

U = 2.0 ** -24
EMU_WORST = 3.9          # worst element of the CPU restatement, in units of u (|W|~ (*) |x|~ + |bias|): see the module docstring
C_TIGHT = 4 * EMU_WORST
DEV = torch.device("cuda")


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# variant: <MT, NT, R, TX, TY, NW> of conv3d_h2q_kernel.
# halves: "exact" (a: integer data, torch.equal), the input families of (b) -- "normal" also carries the GroupNorm partials (c).
# Every launch of every half is repeated once (f).
# c2: the first PVConv of the C2 benchmark step (B = 16, N = 4096) whose second convolution has exactly this shape and takes the
# dense kernel (test_c2_* derives them).
Case = namedtuple("Case", "id b cin cout r variant halves c2")
FAMILIES = ("normal", "wide", "tiny", "outlier")
ALL = ("exact",) + FAMILIES
BIG = ("exact", "normal")      # rows whose float64 references are expensive: one family
V32_BIG, V32_SMALL = (4, 4, 32, 2, 8, 8), (2, 4, 32, 2, 8, 8)
V16_SMALL, V16_BIG, V16_NARROW = (2, 2, 16, 1, 16, 8), (4, 4, 16, 2, 16, 8), (2, 4, 16, 2, 16, 8)
V8_TINY, V8_SMALL, V8_FULL = (2, 1, 8, 1, 8, 4), (2, 2, 8, 2, 8, 4), (2, 2, 8, 4, 8, 8)
CASES = [
    # 32^3, 64 channels x 512 voxels per workgroup
    Case("r32big_c8_m40", 4, 8, 40, 32, V32_BIG, ALL, None),                  # one chunk; M tail 40 / 64
    Case("r32big_c35_m100", 2, 35, 100, 32, V32_BIG, BIG, None),              # cin % 8 = 3; two channel tiles, M tail 36 / 64
    # 32^3, 32 channels x 512 voxels
    Case("r32small_c7_m8", 1, 7, 8, 32, V32_SMALL, ALL, None),                # cout < 16, one chunk of 7
    Case("r32small_c35_m40", 2, 35, 40, 32, V32_SMALL, ALL, None),            # cout > 32 in the small tiling: M tail 8 / 32
    # 16^3, 32 channels x 256 voxels (few workgroups)
    Case("r16small_c35_m40", 3, 35, 40, 16, V16_SMALL, ALL, None),
    Case("r16small_c256_m100", 2, 256, 100, 16, V16_SMALL, BIG, None),        # 32 chunks; M tail 4 / 32
    Case("c2_sa1_pvconv", 16, 64, 64, 16, V16_SMALL, BIG, "sa_layers.1.0"),
    # 16^3, 64 channels x 512 voxels
    Case("r16big_c8_m40", 32, 8, 40, 16, V16_BIG, ALL, None),                 # one chunk; M tail 40 / 64
    Case("r16big_c7_m136", 11, 7, 136, 16, V16_BIG, ALL, None),               # three channel tiles, M tail 8 / 64
    Case("c2_fp2_pvconv", 16, 128, 128, 16, V16_BIG, BIG, "fp_layers.2.1"),
    # 16^3, 32 channels x 512 voxels (cout <= 32)
    Case("r16narrow_c7_m8", 2, 7, 8, 16, V16_NARROW, ALL, None),              # cout < 16
    Case("r16narrow_c64_m24", 3, 64, 24, 16, V16_NARROW, ALL, None),          # M tail 24 / 32
    Case("r16narrow_c256_m32", 1, 256, 32, 16, V16_NARROW, BIG, None),        # 32 chunks
    # 8^3, 32 channels x 64 voxels
    Case("r8tiny_c7_m8", 2, 7, 8, 8, V8_TINY, ALL, None),                     # cout < 16
    Case("r8tiny_c259_m100", 3, 259, 100, 8, V8_TINY, ALL, None),             # 33 chunks, the last one of 3; M tail 4 / 32
    # 8^3, 32 channels x 128 voxels
    Case("r8small_c35_m100", 16, 35, 100, 8, V8_SMALL, ALL, None),
    Case("r8small_c8_m72", 22, 8, 72, 8, V8_SMALL, ALL, None),                # M tail 8 / 32
    Case("r8small_c7_m8", 64, 7, 8, 8, V8_SMALL, ALL, None),                  # cout < 16
    Case("c2_sa2_pvconv", 16, 128, 128, 8, V8_SMALL, BIG, "sa_layers.2.0"),
    # 8^3, 32 channels x 256 voxels
    Case("r8full_c7_m100", 32, 7, 100, 8, V8_FULL, ALL, None),
    Case("r8full_c40_m136", 26, 40, 136, 8, V8_FULL, ALL, None),              # M tail 8 / 32
    Case("r8full_c1_m8", 128, 1, 8, 8, V8_FULL, ALL, None),                   # cin = 1, cout < 16
    Case("c2_fp0_pvconv", 16, 256, 256, 8, V8_FULL, BIG, "fp_layers.0.1"),
]
CASE_IDS = [c.id for c in CASES]
VARIANTS = [V32_BIG, V32_SMALL, V16_SMALL, V16_BIG, V16_NARROW, V8_TINY, V8_SMALL, V8_FULL]
# (cin, cout, r, b_small, b_big): the same shapes under two different instances (half d) -- every adjacent pair of tilings
INDEPENDENCE = [
    (35, 128, 8, 1, 16, V8_TINY, V8_SMALL),
    (35, 128, 8, 16, 32, V8_SMALL, V8_FULL),
    (40, 128, 16, 1, 16, V16_SMALL, V16_BIG),
    (35, 64, 32, 1, 4, V32_SMALL, V32_BIG),
]
# small rows of the CPU restatement: (b, cin, cout, r)
EMULATION_ROWS = [(2, 1, 8, 8), (2, 7, 8, 8), (1, 8, 12, 8), (1, 35, 16, 8), (1, 64, 8, 8), (1, 256, 8, 8)]


def chosen_variant(b, cin, cout, r):
    """What the launch path picks for this shape (host query: no GPU needed)."""
    from bdm_amd import _lib
    v = [ctypes.c_int() for _ in range(5)]
    rc = _lib.lib().bdm_conv3d_h2_variant(b, cin, cout, r, *[ctypes.byref(t) for t in v])
    assert rc == 0, rc
    mt, nt, tx, ty, nw = (t.value for t in v)
    return (mt, nt, r, tx, ty, nw)


def channel_tile(variant):
    return 16 * variant[0]


def stat_groups(cout, variant):
    """GroupNorm group counts to ask statistics for: 8 where the kernel takes it, and another count -- channels per group a power
    of two >= 4 that divides the channel tile (the contract of bdm_conv3d_3x3x3_h2_gn)."""
    ok = [g for g in range(1, cout + 1) if cout % g == 0 and (cout // g) >= 4 and (cout // g) & (cout // g - 1) == 0
          and channel_tile(variant) % (cout // g) == 0]
    first = [8] if 8 in ok else ok[:1]
    return first + [g for g in reversed(ok) if g not in first][:1]     # ... and the narrowest groups


def c_bound(cin):
    k = 27 * 8 * cdiv(cin, 8)
    return min(1.01 * (3 * k + 10), C_TIGHT)


# ---- inputs, float64 reference, bound ------------------------------------------------------------------------------------------------
def pow2_below(v):
    return 2.0 ** math.floor(math.log2(v))


def family_inputs(family, b, cin, cout, r, seed):
    """-> x (b, cin, r^3), w (cout, cin, 3, 3, 3), bias (cout), activation scale (a power of two), all float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, r ** 3, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    scale = None
    if family == "wide":      # per-channel weight scales from 1e-4 to 1e4, activations with a 1e-3 .. 30 spread
        w = w * (10.0 ** torch.linspace(-4, 4, cout)).view(-1, 1, 1, 1, 1)
        x = x * (10.0 ** torch.linspace(-3, 1.5, cin)).view(1, -1, 1)
    elif family == "tiny":    # everything far below fp16's normal range before scaling
        x, w = x * 1e-6, w * 1e-5
    elif family == "outlier":  # one element in 500 at 30 x the bulk, and a scale that leaves the bulk at ~0.5: its lo is ~2^-13,
        hit = torch.rand(x.shape, generator=g) < 2e-3   # at the edge of fp16's subnormal range (2^-14)
        x = torch.where(hit, 30 * x.sign(), x)
        scale = 0.5
    bias = torch.randn(cout, generator=g) * float(w.abs().mean() * x.abs().mean()) * 10
    if scale is None:         # what ops.to_h2 picks without a GroupNorm
        scale = pow2_below(32768.0 / max(float(x.abs().max()), 1e-30))
    return x, w, bias, scale


def reference(x, w, bias, scale, r):
    """float64 convolution and the magnitude term |W|~ (*) |x|~ + |bias| of the bound, both (b, cout, r^3)."""
    b, cin = x.shape[:2]
    x64, w64, b64 = x.double().view(b, cin, r, r, r), w.double(), bias.double()
    ref = TF.conv3d(x64, w64, b64, padding=1)
    wmax = w64.abs().amax(dim=(1, 2, 3, 4), keepdim=True)
    mag = TF.conv3d(x64.abs() + 0.25 / scale, w64.abs() + wmax * 2.0 ** -11, b64.abs(), padding=1)
    return ref.reshape(b, -1, r ** 3), mag.reshape(b, -1, r ** 3)


# ---- CPU restatement of the kernel's arithmetic ----------------------------------------------------------------------------------------
def split16(v):
    """fp32 -> (hi, lo) fp16 terms as float32: saturate, round to nearest even, remainder (exact in fp32), round again."""
    v = v.clamp(-65504.0, 65504.0)
    hi = v.half().float()
    return hi, (v - hi).half().float()


def weight_scale(w):
    """per output channel: the power of two that takes max |w[co]| into [2^9, 2^10) (1 for an all-zero channel)"""
    mx = w.abs().amax(dim=(1, 2, 3, 4))
    ex = torch.frexp(mx)[1]
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), 10 - ex), torch.ones_like(mx))


def emulate(x, w, bias, scale, r, drop=None, shift_tap=None):
    """conv3d_h2q_kernel in plain torch: power-of-two scales, two fp16 terms per operand, the products lo.hi + hi.lo + hi.hi of each
    step of 4 taps x 8 channels added to an fp32 accumulator in the kernel's K order (chunk, tap quad, term), unscale, add bias.
    drop: leave that term out ("lo.hi" = weights' lo x activations' hi, "hi.lo", "hi.hi").  shift_tap: that tap reads the voxel one
    further along z."""
    b, cin = x.shape[:2]
    cout, c8 = w.shape[0], cdiv(cin, 8)
    ws = weight_scale(w)
    wp = torch.zeros(cout, c8 * 8, 28)
    wp[:, :cin, :27] = (w * ws.view(-1, 1, 1, 1, 1)).reshape(cout, cin, 27)
    a = wp.view(cout, c8, 8, 28).permute(0, 1, 3, 2).reshape(cout, c8 * 28 * 8)             # K order: chunk, tap, channel
    xp = torch.zeros(b, c8 * 8, r + 4, r + 4, r + 4)
    xp[:, :cin, 2:-2, 2:-2, 2:-2] = (x * scale).view(b, cin, r, r, r)
    cols = torch.zeros(b, c8, 28, 8, r ** 3)
    for t in range(27):
        dx, dy, dz = t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1 + (1 if t == shift_tap else 0)
        cols[:, :, t] = xp[:, :, 2 + dx:2 + dx + r, 2 + dy:2 + dy + r, 2 + dz:2 + dz + r].reshape(b, c8, 8, r ** 3)
    bm = cols.view(b, c8 * 28 * 8, r ** 3)
    (a_hi, a_lo), (b_hi, b_lo) = split16(a), split16(bm)
    terms = [("lo.hi", a_lo, b_hi), ("hi.lo", a_hi, b_lo), ("hi.hi", a_hi, b_hi)]     # smallest first, as the kernel issues them
    acc = torch.zeros(b, cout, r ** 3)
    for k0 in range(0, c8 * 28 * 8, 32):
        for name, at, bt in terms:
            if name != drop:
                acc = acc + torch.matmul(at[:, k0:k0 + 32], bt[:, k0:k0 + 32])
    osc = (1.0 / ws) * (1.0 / scale)
    return acc * osc.view(1, -1, 1) + bias.view(1, -1, 1)


def emulation_fraction(row, family, **mutation):
    """worst element of the restatement in units of u (|W|~ (*) |x|~ + |bias|), and in units of the bound in force"""
    b, cin, cout, r = row
    x, w, bias, scale = family_inputs(family, b, cin, cout, r, seed=17 * cin + cout)
    ref, mag = reference(x, w, bias, scale, r)
    e = float(((emulate(x, w, bias, scale, r, **mutation).double() - ref).abs() / (U * mag)).max())
    return e, e / c_bound(cin)


# ---- CPU half -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_reaches_its_variant(case):
    assert chosen_variant(case.b, case.cin, case.cout, case.r) == case.variant
    assert case.halves and set(case.halves) <= set(ALL) and "exact" in case.halves and "normal" in case.halves
    assert stat_groups(case.cout, case.variant), "no power-of-two group width >= 4 divides cout"


def test_chooser_rejects_other_resolutions_and_takes_null_pointers():
    from bdm_amd import _lib
    lib = _lib.lib()
    assert lib.bdm_conv3d_h2_variant(2, 8, 8, 16, None, None, None, None, None) == 0
    mt = ctypes.c_int(7)
    for r in (0, 4, 12, 24, 64):
        assert lib.bdm_conv3d_h2_variant(2, 8, 8, r, ctypes.byref(mt), None, None, None, None) == 3   # BDM_ERR_UNSUPPORTED
        assert mt.value == 0


def test_chooser_sweep_returns_only_covered_variants():
    """Every instance the chooser CAN return has rows in the table (at least two), in every half.  Fails the day a retune makes
    another instance reachable without a row here."""
    seen = set()
    for b in range(1, 33):
        for cout in (8, 12, 16, 24, 31, 32, 33, 40, 63, 64, 65, 72, 100, 128, 129, 136, 192, 256, 257, 384, 512):
            for r in (8, 16, 32):
                seen.add(chosen_variant(b, 64, cout, r))
    assert seen == set(VARIANTS), sorted(seen)
    for v in VARIANTS:
        assert sum(c.variant == v for c in CASES) >= 2, v
    for half in ALL:
        assert seen <= {c.variant for c in CASES if half in c.halves}, half
    # the chooser does not look at cin
    assert {chosen_variant(16, cin, 128, 16) for cin in (1, 7, 8, 35, 256, 512)} == {V16_BIG}


def test_table_covers_the_edges():
    """cin not a multiple of 8 (padded channels of the last chunk), cout not a multiple of the channel tile (M tail), cout < 16, one
    chunk and >= 32 chunks -- in the union, and the M tail and an odd cin under EVERY instance."""
    assert any(c.cin % 8 for c in CASES) and any(c.cout < 16 for c in CASES)
    assert any(c.cin <= 8 for c in CASES) and any(c.cin >= 256 for c in CASES)
    for v in VARIANTS:
        rows = [c for c in CASES if c.variant == v]
        assert any(c.cout % channel_tile(v) for c in rows), v
        assert any(c.cin % 8 for c in rows), v
        widths = [c.cout for c in rows] + [t[1] for t in INDEPENDENCE if v in t[5:]]     # statistics run in both
        assert any(8 in stat_groups(m, v) for m in widths) and any(len(stat_groups(m, v)) == 2 for m in widths), v


def c2_step_layers():
    """(b, cin, cout, r) of the second convolution of every PVConv of the C2 step (B = 16 shapes, N = 4096 points) that runs on the
    dense grid (bdm_amd/modules.py sends it to ops.conv3d_h2 or ops.conv3d_h2_gn; the others take the voxel-list kernels), read
    off the denoiser's own modules: {first module with that shape: shape}."""
    from bdm_amd.modules import PVConv
    from bdm_amd.pvcnn import PVCNN2Base
    B, N = 16, 4096
    net = PVCNN2Base(num_classes=3, embed_dim=64)
    points = [N] + [sa[1][0] for sa in net.sa_blocks]     # points per level: the centers of each set abstraction
    out = {}
    for name, m in net.named_modules():
        if not isinstance(m, PVConv):
            continue
        kind, level = name.split(".")[:2]
        n = points[int(level)] if kind == "sa_layers" else points[len(net.fp_blocks) - 1 - int(level)]
        if m.conv_impl != "fp16x3" or m.wants_compact_tail(B, n):
            continue
        conv2 = [layer for layer in m.voxel_layers if isinstance(layer, torch.nn.Conv3d)][1]
        shape = (B, conv2.in_channels, conv2.out_channels, m.resolution)
        if shape not in out.values():
            out[name] = shape
    return out


def test_c2_step_layers_are_in_the_table_verbatim():
    layers = c2_step_layers()
    assert {c.c2: (c.b, c.cin, c.cout, c.r) for c in CASES if c.c2} == layers
    assert (16, 128, 128, 16) in layers.values() and (16, 256, 256, 8) in layers.values()
    assert {V16_BIG, V8_FULL} <= {c.variant for c in CASES if c.c2}


@pytest.mark.parametrize("cin,cout,r,b_small,b_big,v_small,v_big", INDEPENDENCE)
def test_independence_shapes_change_tile_with_the_batch(cin, cout, r, b_small, b_big, v_small, v_big):
    assert chosen_variant(b_small, cin, cout, r) == v_small and chosen_variant(b_big, cin, cout, r) == v_big and v_small != v_big
    assert len(stat_groups(cout, v_small)) == 2 and 8 in stat_groups(cout, v_small)


def test_independence_covers_every_adjacent_pair():
    pairs = {(s, g) for *_, s, g in INDEPENDENCE}
    assert pairs == {(V8_TINY, V8_SMALL), (V8_SMALL, V8_FULL), (V16_SMALL, V16_BIG), (V32_SMALL, V32_BIG)}


def test_two_term_split_error_is_one_fp32_ulp_not_half():
    """Step 1 of the derivation, on the worst case: 1 + 2^-11 + 2^-22 + 2^-23 (a 24-bit fp32 value) -- hi = 1, the remainder is 2^11 + 3
    units of 2^-23, fp16 holds only the even integers there: the pair misses by one unit = 2^-23 |x| (to 2^-11), twice the header's
    2^-24; and no fp32 value in range misses by more than 2^-23 |x|."""
    v = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -22 + 2.0 ** -23], dtype=torch.float32)
    hi, lo = split16(v)
    err = float((v.double() - hi.double() - lo.double()).abs())
    assert err == 2.0 ** -23 and err > 2.0 ** -24 * float(v)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1 << 20, generator=g) * torch.exp2(torch.randint(-6, 13, (1 << 20,), generator=g).float())
    hi, lo = split16(x)
    rel = ((x.double() - hi.double() - lo.double()).abs() / x.double().abs().clamp_min(2.0 ** -2)).max()
    assert float(rel) <= 2.0 ** -23
    assert float((lo.abs() / x.abs().clamp_min(2.0 ** -2)).max()) <= 2.0 ** -11 * (1 + 2.0 ** -11)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("row", EMULATION_ROWS, ids=lambda r: "b{}_c{}_m{}_r{}".format(*r))
def test_emulation_stays_inside_the_bound(row, family):
    """The restatement of the kernel's arithmetic is within EMU_WORST u (|W|~ (*) |x|~ + |bias|) per element -- the figure the
    tightened constant 4 EMU_WORST comes from -- hence at most a quarter of the bound in force (or all of c(K), were that smaller)."""
    e, frac = emulation_fraction(row, family)
    print(f"emulation {row} {family}: worst element {e:.3f} u mag, {frac:.3f} of the bound")
    assert e <= EMU_WORST and frac <= 1.0, (e, frac)


MUTANTS = [dict(drop="lo.hi"), dict(drop="hi.lo"), dict(shift_tap=13), dict(shift_tap=26)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mutation", MUTANTS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
@pytest.mark.parametrize("row", EMULATION_ROWS, ids=lambda r: "b{}_c{}_m{}_r{}".format(*r))
def test_broken_emulation_falls_outside_the_bound(row, mutation, family):
    """One dropped partial product, or one tap shifted by a voxel, at every width and in every input family: outside the bound."""
    e, frac = emulation_fraction(row, family, **mutation)
    print(f"mutant {mutation} {row} {family}: worst element {frac:.3g} of the bound")
    assert frac > 1.0, frac


# ---- GPU half -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(hip):
    from bdm_amd import ops as o
    return o


def twice(launch):
    """Run a launch twice (fresh outputs each time) and assert bit-equal results (f); returns the first."""
    first, second = launch(), launch()
    for a, c in zip(first, second):
        assert torch.equal(a, c), "two launches of the same case differ"
    return first


def partials(ws, slices, b, groups):
    return ws.view(torch.float64)[:b * groups * slices * 2].view(b, groups, slices, 2).clone()


def run_conv(ops, x, w, bias, scale, case, groups=None):
    """to_h2 -> conv3d_h2 (groups None) or conv3d_h2_gn; every launch twice.  -> y, or (y, partials (b, groups, slices, 2), slices)"""
    b, cin, cout, r = case.b, case.cin, case.cout, case.r
    (xh,) = twice(lambda: (ops.to_h2(x, scale=scale)[0],))
    (pk, inv) = twice(lambda: ops.conv3d_h2_pack(w))
    xh2 = (xh, 1.0 / scale)
    if groups is None:
        return twice(lambda: (ops.conv3d_h2(xh2, (pk, inv), bias, cin, cout, r),))[0]

    def launch():
        y, (ws, slices) = ops.conv3d_h2_gn(xh2, (pk, inv), bias, cin, cout, r, groups)
        return y, partials(ws, slices, b, groups), torch.tensor(slices)
    y, p, s = twice(launch)
    return y, p, int(s)


def exact_inputs(pattern, case, g):
    """Small-integer activations, weights = small integers x a power of two per output channel, bias likewise."""
    b, cin, cout, r = case.b, case.cin, case.cout, case.r
    x = torch.randint(-7, 8, (b, cin, r, r, r), generator=g).float()
    if pattern == "impulse":   # one voxel at each corner, two inside next to the middle planes (brick boundaries), each in its own channel
        spots = [(i, j, k) for i in (0, r - 1) for j in (0, r - 1) for k in (0, r - 1)]
        spots += [(r // 2 - 1, r // 2, 1), (r // 2, r // 2 - 1, r - 2), (3, 4, r // 2)]
        keep = torch.zeros_like(x)
        for n, (i, j, k) in enumerate(spots):
            for bi in range(b):
                ch = (5 * n + 3 * bi) % cin
                keep[bi, ch, i, j, k] = 1 + (n + bi) % 7
        x = keep
    elif pattern == "faces":   # nonzero on the six boundary faces only
        inner = torch.zeros(r, r, r, dtype=torch.bool)
        inner[1:-1, 1:-1, 1:-1] = True
        x = x.masked_fill(inner, 0.0)
    p = torch.exp2((torch.arange(cout) % 5 - 2).float())
    w = torch.randint(-7, 8, (cout, cin, 3, 3, 3), generator=g).float() * p.view(-1, 1, 1, 1, 1)
    bias = torch.randint(-100, 101, (cout,), generator=g).float() * p
    return x, w, bias, p


def half_exact(ops, case):
    """(a) no rounding anywhere: every operand is exact in its hi term, every partial sum an integer (times the channel's power of
    two) below 2^24 -- the fp32 result IS the float64 one."""
    b, cin, cout, r = case.b, case.cin, case.cout, case.r
    g = torch.Generator().manual_seed(100 + CASE_IDS.index(case.id))
    groups = stat_groups(cout, case.variant)[0]
    for pattern in ("dense", "impulse", "faces"):
        x, w, bias, p = exact_inputs(pattern, case, g)
        xmax, wmax, bmax = float(x.abs().max()), float((w / p.view(-1, 1, 1, 1, 1)).abs().max()), float((bias / p).abs().max())
        assert 27 * cin * xmax * wmax + bmax < 2 ** 24 and xmax * 16 <= 2048 and wmax <= 2048   # the margin, before launching
        ref = TF.conv3d(x.double(), w.double(), bias.double(), padding=1).reshape(b, cout, -1)
        assert torch.equal(ref.float().double(), ref)
        xd, wd, bd = x.view(b, cin, -1).to(DEV), w.to(DEV), bias.to(DEV)
        y = run_conv(ops, xd, wd, bd, 16.0, case)
        assert torch.equal(y.cpu().double(), ref), f"{pattern}: {int((y.cpu().double() != ref).sum())} elements differ from the exact result"
        y_gn, _, _ = run_conv(ops, xd, wd, bd, 16.0, case, groups)
        assert torch.equal(y_gn, y), f"{pattern}: conv3d_h2_gn writes another output than conv3d_h2"


def unit_sums(y, groups, r):
    """Per (shape, group, canonical slice) sum, sum of squares and sum of magnitudes of y (b, cout, r^3) in float64: a slice is an
    x-plane at 8^3 and 16^3, a 2 x 8 x 32 tile (x-major) at 32^3."""
    b, cout = y.shape[:2]
    if r == 32:
        t = y.double().view(b, groups, cout // groups, 16, 2, 4, 8, 32)
        dims, s = (2, 4, 6, 7), 64
    else:
        t = y.double().view(b, groups, cout // groups, r, r * r)
        dims, s = (2, 4), r
    return (t.sum(dims).reshape(b, groups, s), (t * t).sum(dims).reshape(b, groups, s), t.abs().sum(dims).reshape(b, groups, s)), s


def check_partials(y, p, slices, groups, r, what):
    (s, q, a), expect = unit_sums(y, groups, r)
    assert slices == expect == {8: 8, 16: 16, 32: 64}[r], (slices, expect)
    n32 = 64 * (32 if r == 32 else r * r // 16)
    fs = float(((p[..., 0] - s).abs() / (n32 * U * a).clamp_min(1e-300)).max())
    fq = float(((p[..., 1] - q).abs() / ((n32 + 1) * U * q).clamp_min(1e-300)).max())
    parity(current_test() + " slice sums", fs, 1.0, note=what)
    parity(current_test() + " slice sums of squares", fq, 1.0, note=what)
    assert fs <= 1.0 and fq <= 1.0, f"{what}: a slice is {fs:.3g} / {fq:.3g} x its bound"


def half_family(ops, case, family):
    """(b) elementwise bound and whole-tensor rel-L2 on random data; for "normal" also (c) the GroupNorm slice partials."""
    b, cin, cout, r = case.b, case.cin, case.cout, case.r
    x, w, bias, scale = family_inputs(family, b, cin, cout, r, seed=1000 + CASE_IDS.index(case.id))
    ref, mag = reference(x, w, bias, scale, r)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    if family != "outlier":
        assert ops.to_h2(xd)[1] == 1.0 / scale      # the scale the bound assumes is the one ops.to_h2 picks
    y = run_conv(ops, xd, wd, bd, scale, case)
    assert bool(torch.isfinite(y).all())
    refd = ref.to(DEV)
    frac = float(((y.double() - refd).abs() / (c_bound(cin) * U * mag.to(DEV))).max())
    parity(current_test() + " elementwise", frac, 1.0, note=f"variant {case.variant}")
    l2 = float(((y.double() - refd).norm(dim=(0, 2)) / refd.norm(dim=(0, 2))).max())
    parity(current_test() + " rel-L2 per channel", l2, 2e-6, note=f"variant {case.variant}")
    assert frac <= 1.0, f"an element is {frac:.3g} x its bound {c_bound(cin):.3g} u (|W|~ (*) |x|~ + |bias|)"
    assert l2 < 2e-6, l2
    if family != "normal":
        return
    for groups in stat_groups(cout, case.variant):
        y_gn, p, slices = run_conv(ops, xd, wd, bd, scale, case, groups)
        assert torch.equal(y_gn, y), "conv3d_h2_gn writes another output than conv3d_h2"
        check_partials(y, p, slices, groups, r, f"{groups} groups of {cout // groups}")


GPU_RUNS = [(c, h) for c in CASES for h in ALL if h in c.halves]


@pytest.mark.gpu
@pytest.mark.parametrize("case,half", GPU_RUNS, ids=[f"{c.id}-{h}" for c, h in GPU_RUNS])
def test_conv3d_h2_against_float64(ops, case, half):
    assert chosen_variant(case.b, case.cin, case.cout, case.r) == case.variant
    if half == "exact":
        half_exact(ops, case)
    else:
        half_family(ops, case, half)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,r,b_small,b_big,v_small,v_big", INDEPENDENCE)
def test_results_do_not_depend_on_the_tile(ops, cin, cout, r, b_small, b_big, v_small, v_big):
    """(d) b_small shapes launched on their own and as shapes k .. k + b_small of b_big: two different kernel instances, the same
    output bits and -- the decomposition being canonical -- the same slice partials, with and without the statistics epilogue."""
    assert chosen_variant(b_small, cin, cout, r) == v_small and chosen_variant(b_big, cin, cout, r) == v_big and v_small != v_big
    x, w, bias, scale = family_inputs("normal", b_big, cin, cout, r, seed=cin + cout + r)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    k = (b_big - b_small) // 2 + (1 if b_big - b_small > 1 else 0)
    sub = xd[k:k + b_small].contiguous()
    small, big = Case("small", b_small, cin, cout, r, v_small, (), None), Case("big", b_big, cin, cout, r, v_big, (), None)
    ya, yb = run_conv(ops, sub, wd, bd, scale, small), run_conv(ops, xd, wd, bd, scale, big)
    assert torch.equal(ya, yb[k:k + b_small]), "the output depends on the tile"
    for groups in stat_groups(cout, v_small):
        ga, pa, sa = run_conv(ops, sub, wd, bd, scale, small, groups)
        gb, pb, sb = run_conv(ops, xd, wd, bd, scale, big, groups)
        assert torch.equal(ga, ya) and torch.equal(gb, yb), f"{groups} groups: the statistics epilogue changes the output"
        assert sa == sb and torch.equal(pa, pb[k:k + b_small]), f"{groups} groups: the slice partials depend on the tile"


def unpack_weights(packed, cout, cin):
    """[ceil(cin/8)][14 tap pairs][2 terms][2 taps of the pair][cout][8] fp16 -> hi, lo as (cout, 8 ceil(cin/8), 28 taps) float64"""
    c8 = cdiv(cin, 8)
    t = packed.cpu().double().view(c8, 14, 2, 2, cout, 8).permute(2, 4, 0, 5, 1, 3).reshape(2, cout, c8 * 8, 28)
    return t[0], t[1]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(1, 8), (7, 12), (35, 40)])
def test_weight_packer(ops, cin, cout):
    """(e) inv_scale is an exact power of two that takes max |w[co]| into [2^9, 2^10), also when the maximum is itself a power of two;
    an all-zero channel gets a finite scale and zero terms; hi + lo reconstructs every weight within the split's error; pad channels
    and the pad tap are zero; the convolution of the packed weights is finite and the zero channel returns the bias."""
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (10.0 ** torch.linspace(-3, 3, cout)).view(-1, 1, 1, 1, 1)
    w[0] = 0.0
    w[1] = w[1].clamp(-0.125, 0.125)
    w[1, 0, 1, 1, 1] = 0.125          # the channel's maximum is exactly 2^-3
    w[2] = w[2].clamp(-1.0, 1.0)
    w[2, cin - 1, 2, 2, 2] = -1.0
    packed, inv = twice(lambda: ops.conv3d_h2_pack(w.to(DEV)))
    inv = inv.cpu()
    assert bool(torch.isfinite(inv).all()) and bool((inv > 0).all())
    assert bool((torch.frexp(inv)[0] == 0.5).all()), "inv_scale is not a power of two"
    assert torch.equal(inv, 1.0 / weight_scale(w))
    top = w.abs().amax(dim=(1, 2, 3, 4)) / inv
    assert float(inv[0]) == 1.0 and bool(((top[1:] >= 512) & (top[1:] < 1024)).all()), top
    assert float(top[1]) == 512.0 and float(top[2]) == 512.0
    hi, lo = unpack_weights(packed, cout, cin)
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
    assert float(hi[:, cin:].abs().max() if cin % 8 else 0.0) == 0.0 and float(lo[:, cin:].abs().max() if cin % 8 else 0.0) == 0.0
    assert float(hi[..., 27].abs().max()) == 0.0 and float(lo[..., 27].abs().max()) == 0.0
    assert float(hi[0].abs().max()) == 0.0 and float(lo[0].abs().max()) == 0.0
    w64, inv64 = w.double().view(cout, cin, 27), inv.double().view(-1, 1, 1)
    e_hi, e_lo = split16(w.view(cout, cin, 27) / inv.view(-1, 1, 1))
    assert torch.equal(hi[:, :cin, :27], e_hi.double()) and torch.equal(lo[:, :cin, :27], e_lo.double())
    err = ((hi + lo)[:, :cin, :27] * inv64 - w64).abs()
    assert bool((err <= 2.0 ** -23 * w64.abs() + 2.0 ** -25 * inv64).all())
    r, b = 8, 2
    x = torch.randn(b, cin, r ** 3, generator=g)
    bias = torch.randn(cout, generator=g)
    y = ops.conv3d_h2(ops.to_h2(x.to(DEV)), (packed, inv.to(DEV)), bias.to(DEV), cin, cout, r).cpu()
    assert bool(torch.isfinite(y).all()) and torch.equal(y[:, 0], bias[0].expand(b, r ** 3))


@pytest.mark.gpu
@pytest.mark.parametrize("c,r", [(1, 8), (7, 8), (35, 16), (40, 8)])
def test_operand_producer_without_groupnorm(ops, c, r):
    """(e) to_h2 without a GroupNorm: (hi + lo) / scale is x within the two-term split's error (2^-23 |x|, or 2^-25 / scale below
    fp16's normal range), the terms are the restatement's bit for bit, fp16-representable inputs come back exactly with lo = 0, and
    the pad channels of the last chunk are zero in both planes."""
    g = torch.Generator().manual_seed(c + r)
    b, v, c8 = 2, r ** 3, cdiv(c, 8)
    x = torch.randn(b, c, v, generator=g) * torch.exp2(torch.randint(-12, 4, (b, c, v), generator=g).float())

    def planes(t, scale):
        (h2,) = twice(lambda: (ops.to_h2(t.to(DEV), scale=scale)[0],))
        assert h2.shape == (b, c8, 2, v, 8) and h2.dtype == torch.float16
        p = h2.cpu().double().permute(2, 0, 1, 4, 3).reshape(2, b, c8 * 8, v)
        return p[0], p[1]
    for scale in (256.0, 1.0):
        hi, lo = planes(x, scale)
        if c % 8:
            assert float(hi[:, c:].abs().max()) == 0.0 and float(lo[:, c:].abs().max()) == 0.0
        e_hi, e_lo = split16(x * scale)
        assert torch.equal(hi[:, :c], e_hi.double()) and torch.equal(lo[:, :c], e_lo.double())
        err = ((hi + lo)[:, :c] / scale - x.double()).abs()
        assert bool((err <= 2.0 ** -23 * x.double().abs() + 2.0 ** -25 / scale).all())
    xh = (x * 64).half().float()          # fp16-representable, in the normal range or exactly zero
    xh = torch.where(xh.abs() < 2.0 ** -14, torch.zeros_like(xh), xh)
    hi, lo = planes(xh, 1.0)
    assert torch.equal(hi[:, :c], xh.double()) and float(lo.abs().max()) == 0.0
    _, inv = ops.to_h2(x.to(DEV))         # the default scale: a power of two that puts max |x| in [2^14, 2^15)
    assert 2.0 ** 14 <= float(x.abs().max()) / inv < 2.0 ** 15 and math.frexp(inv)[0] == 0.5
