"""Every instance of the list convolutions (sconv_dil_kernel and vox_dilate_kernel, bdm_amd/csrc/sparse_conv_os.hip; the class
constants of bdm_amd/csrc/pvconv_compact.hip) ELEMENTWISE against float64, on clouds built to reach the paths no operator-level test
reaches.

The launcher picks one of twelve kernel instances <MT, NT, NW, R, H2IN>: MT = 2 (cout <= 32) or 4, R = 8 / 16 / 32 (NT = 1 / 2 / 4, NW = 8),
H2IN = first convolution (fp32 records of the occupied cells) or second (fp16 (hi, lo) rows of the once-dilated list D1 + a constant
record).  ONE case table names, per row, the instance, the cloud and the form (first convolution dense / compact / with statistics,
second convolution).

* CPU half (no GPU): `bdm_sparse_conv_dil_variant` (the launch path's own geometry) returns that instance for every row; all twelve
  are present; a sweep over cout 1 .. 256 returns nothing else; the table holds the C2 step's own list-convolution layers; the
  elementwise bound is checked against a plain torch restatement of the kernel's arithmetic ON LISTS (`emulate_list`: gathered
  neighbour through the index, absent = zero, for H2IN the constant record inside the grid and zero outside it), and the same
  restatement with one defect falls outside it.
* GPU half: the plan of the second list against a numpy restatement (exact); every row against TF.conv3d in float64 on the CPU; the
  class weight sums and class constants against their definitions.  Every row first asserts, from the tile tables the plan kernels
  WROTE, that its cloud did what it is there for (REACH below): a row that silently stops reaching its path fails.

Clouds (integer cell coordinates; the plan is built as ops.sparse_first_conv builds it, then plan_dilation + plan_dilation2):
  one_per_cell   Gaussian-like, at most one point per occupied cell           many_per_cell  several per cell, odd shapes: half in voxel 0
  single         one occupied cell: the far grid corner (even shapes), an interior cell (odd shapes)
  full           every cell occupied: some tile's input range is EXACTLY xcap rows, D1 = D2 = the grid, all 27 class counts zero
  slab           four consecutive full x-planes + a lone cell at voxel 0: some tile other than the last is short (cut at a plane boundary)
  line (32^3)    cells (0, 0, 0), (3, 0, 0), .. (30, 0, 0): ONE tile spans all 32 x-planes, (pl1 - pl0 + 1) r^2 4 > 2 (xcap + 128) 16 bytes:
                 the index planes do not fit the operand area and the kernel looks neighbours up in global memory (staged == false)
  faces          even shapes: the 27 cells {0, r/2, r-1}^3 (corners, edge and face centres, the middle): every boundary class occurs INSIDE
                 the lists; odd shapes: two cells in the middle: every class occurs OUTSIDE them, all 27 class counts > 0.  (A corner
                 class is ONE voxel: no single shape can have it on both sides, so the two sides are two shapes of one batch.)
  persistent     full shapes, tiny channel counts, as many shapes as make live tiles x channel blocks x B >= 1.25 x the CU count: the
                 launcher starts one workgroup per CU and items are dealt tile-slowest, so at least a quarter of the workgroups compute
                 a second LIVE tile on the LDS the first one left (operand tiles, zero / constant records, reduction scratch).

The elementwise bound is the one derived in the docstring of tests/test_hip_conv3d_h2.py -- this kernel issues the same MFMA sequence
on the same weight image; u = 2^-24, K = 27 * 8 * ceil(cin / 8):
       |got - ref| <= c u (|W|~ (*) |x|~ + |bias|),   c = min(1.01 (3K + 10), 4 EMU_WORST)
       |w|~ = |w| + 2^-11 max |w[co]|;   first form: |x|~ = |x| + 2^-2 / s with s the SHAPE's power of two (act_scale_from_max of
       h2_split.h, restated in act_scale: max |cell mean| s in [2^14, 2^15)); second form: the operands ARE (hi + lo) / s, exact, so
       their padding term drops: |x|~ = |x|.
x = the float32 cell means of the oracle's avg_voxelize promoted to float64 (first form; the record kernel is specified to equal
them bit for bit: asserted once against ops.avg_voxelize on the many_per_cell row) or the grid built on the host from the operands
the kernel is given: (hi + lo) / s of rows_h2 at D1's voxels, const_f32 elsewhere, zero padding outside (second form).
EMU_WORST is measured on the restatement, not on the kernel: over EMULATION_ROWS x the four input families of the dense file its worst
element is 5.18 u (|W|~ (*) |x|~ + |bias|) (per family, worst row: normal 3.06, wide 4.23, tiny 5.18, outlier 3.51; all at cin = 1 or 7,
where a listed voxel next to ONE occupied cell sums a handful of products and the representation errors of step 1 and 2 of the
derivation -- up to 10 u per product -- do not average out as they do over the dense file's full neighbourhoods; from cin = 35 on the
figures are 1.0 - 2.9).  EMU_WORST = 5.2 is asserted by test_emulation_stays_inside_the_bound, and the kernel may be 4 x that far
(another summation order inside the matrix instruction, thousands of times as many elements): c <= 20.8.
Mutants of the restatement (test_broken_emulation_falls_outside_the_bound), smallest factor outside the bound in force over
EMULATION_ROWS x families: a dropped hi.lo term 25.6 x (cin = 100, "tiny"); one tap reading the next voxel along z 5.5e4 x; one
(16-voxel block, tap quad) group skipped 4.2e4 x; H2IN: the constant record used for a neighbour outside the grid 1.3e5 x; H2IN:
zero for a neighbour inside the grid but outside D1 6.5e4 x.

GroupNorm slice partials, against the values the kernel WROTE.  Read from the epilogue of sconv_dil_kernel: a lane adds the 4
channels of one voxel (bs += v, bq = fma(v, v, bq)), row16_sum adds the 16 voxels of a block, then the tile's NBLK = TILE / 16 blocks
are added in ascending order, all in fp32: one chain over n32 = 4 * 16 * NBLK = 4 TILE values (2048 / 1024 / 512 at 32^3 / 16^3 / 8^3)
per 4-channel block; the group's blocks and everything after are fp64.  Per slice and group:
       |sum err| <= n32 u sum |v|,      |sum of squares err| <= (n32 + 1) u sum v^2      (+ 2^-50 of the magnitudes for the fp64 part)
first form: the voxels of the tile's owned linear range outside the list add nfill bias and nfill bias^2 per channel in fp64 (inside
the 2^-50); dead tiles write exact zeros; second form: the 27 slices behind the tiles' are class_count x (sum v, sum v^2) of the class
values to fp64 rounding (2^-50 relative).

Class weight sums: fp64 sums of at most 27 floats: within 27 * 2^-53 sum |w| of the numpy restatement.  Class constants:
float32(bias + wsum . const) evaluated in float64: one float32 rounding (2^-24 |value|, + 2^-149 below the normal range) plus
cin 2^-53 (|bias| + |wsum| . |const|) for the order of the fp64 sum.  On the faces cloud every class value is also compared with the
float64 CONVOLUTION at a voxel of that class outside D2, under the same bound + the float64 convolution's own 27 cin 2^-53 of the
magnitudes.

Bit-exact (torch.equal / np.array_equal): the plan, a repeated launch, compact against dense form, statistics against plain form,
strided against contiguous features, a shape alone against the same shape in its batch, the second form's listed voxels against
ops.conv3d_h2 on the densified operands, the `exact` half (small-integer data whose sums are exact in fp32), sentinels.

The operand producer bdm_group_norm_to_h2_rows and the consumers on rows (bdm_se_gate_gn_rows(_pf), bdm_devoxelize_gn_gate_add_rows(_pf))
are tested on their own, with slice partials built on the host in float64 and cut unevenly (uneven_partials of the GroupNorm file),
under that file's rule: per output element mag = the magnitude of the terms that go into it ((|x| + |mean|) rstd |gamma| + |beta| for a
normalised value, its mean over the row for a channel mean, |gamma| rstd and |beta| + |mean gamma| rstd for the affine forms,
1 + sum |w2| |hidden| for the gate, sum_i w_i mag_i |gate| + mag_add for a devoxelised point), the figure is max |got - ref64| / (u mag),
the yardstick is the same operation in plain fp32 PyTorch against the same float64 reference, and the kernel may be at most
4 x max(yardstick, 1).  The producer's (hi + lo) / s adds the two-term split's own error, derived in step 1 of the dense file's
docstring: 2 u |value| + 2^-25 / s.  Its pad channels, the rows beyond the list and the saturation word are exact.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from helpers import current_test, parity
from test_hip_conv3d_h2 import cdiv, family_inputs, pow2_below, split16, weight_scale
from test_hip_groupnorm_family import EPS, affine, channel_data, coef_ref, devox_expected, gn64, gn_module, group_totals, se_gate64, se_weights, swish, uneven_partials
from test_hip_groupnorm_family import Figures as YardstickFigures

U = 2.0 ** -24
EMU_WORST = 5.2          # bound on the worst element of the CPU restatement, in units of u (|W|~ (*) |x|~ + |bias|): see the module docstring
C_TIGHT = 4 * EMU_WORST
DEV = torch.device("cuda")
SENT = -777.0
FAMILIES = ("normal", "wide", "tiny", "outlier")
FORMS = ("dense", "compact", "stats", "second")


def c_bound(cin):
    k = 27 * 8 * cdiv(cin, 8)
    return min(1.01 * (3 * k + 10), C_TIGHT)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# variant: <MT, NT, NW, R, H2IN> of sconv_dil_kernel.  groups: GroupNorm groups of the statistics epilogue (None: a form without).
# second form: cin is the producer's C (bdm_group_norm_to_h2_rows: C <= 256).  c2: the PVConv of the C2 benchmark step (B = 16, N = 4096)
# whose first / second convolution has exactly these channels at this resolution on the list kernels (test_c2_* derives them); their
# rows run B = 1 or 2 shapes: the instance does not depend on B, and the float64 reference stays at a few seconds.
Case = namedtuple("Case", "id b cin cout groups r cloud form variant c2")


def V(mt, r, h2in):
    return (mt, {8: 1, 16: 2, 32: 4}[r], 8, r, h2in)


CASES = [
    # ---- 8^3: every channel shape (the smallest resolution that has every instance)
    Case("r8_dense_c1_m7", 2, 1, 7, None, 8, "many_per_cell", "dense", V(2, 8, 0), None),            # cin = 1; cout < 8, scalar stores
    Case("r8_compact_c7_m35", 3, 7, 35, None, 8, "one_per_cell", "compact", V(4, 8, 0), None),       # Cout % 4 = 3: the scalar store branch
    Case("r8_dense_c35_m35", 2, 35, 35, None, 8, "faces", "dense", V(4, 8, 0), None),                # cin % 8 = 3
    Case("r8_compact_c8_m7", 2, 8, 7, None, 8, "single", "compact", V(2, 8, 0), None),
    Case("r8_stats_c8_m8", 2, 8, 8, 2, 8, "many_per_cell", "stats", V(2, 8, 0), None),               # cout = 8: 24 idle channels of the block
    Case("r8_stats_c35_m40", 3, 35, 40, 10, 8, "one_per_cell", "stats", V(4, 8, 0), None),           # M tail 40 / 64
    Case("r8_stats_c7_m72", 2, 7, 72, 9, 8, "slab", "stats", V(4, 8, 0), None),                      # two blocks, tail 8 / 64; cut tiles
    Case("r8_stats_c259_m100", 2, 259, 100, 25, 8, "many_per_cell", "stats", V(4, 8, 0), None),      # 33 chunks, the last of 3; tail 36 / 64
    Case("r8_stats_c8_m136", 2, 8, 136, 17, 8, "faces", "stats", V(4, 8, 0), None),                  # three blocks, tail 8 / 64
    Case("r8_stats_c35_m32", 2, 35, 32, 8, 8, "full", "stats", V(2, 8, 0), None),                    # xcap reached exactly
    Case("r8_second_c35_m8", 2, 35, 8, 2, 8, "one_per_cell", "second", V(2, 8, 1), None),            # pad channels of the constant record
    Case("r8_second_c100_m40", 2, 100, 40, 10, 8, "faces", "second", V(4, 8, 1), None),              # 13 chunks, the last of 4
    Case("r8_second_c64_m72", 2, 64, 72, 9, 8, "slab", "second", V(4, 8, 1), None),                  # cut tiles on the second table
    Case("r8_second_c8_m100", 2, 8, 100, 25, 8, "many_per_cell", "second", V(4, 8, 1), None),
    Case("r8_second_c35_m136", 2, 35, 136, 17, 8, "single", "second", V(4, 8, 1), None),
    Case("r8_second_c32_m32", 2, 32, 32, 8, 8, "full", "second", V(2, 8, 1), None),
    Case("r8_persistent_dense", 40, 8, 100, None, 8, "persistent", "dense", V(4, 8, 0), None),
    Case("r8_persistent_compact", 40, 8, 100, None, 8, "persistent", "compact", V(4, 8, 0), None),
    Case("r8_persistent_first", 40, 8, 100, 25, 8, "persistent", "stats", V(4, 8, 0), None),
    Case("r8_persistent_second", 40, 8, 100, 25, 8, "persistent", "second", V(4, 8, 1), None),
    # ---- 16^3
    Case("r16_dense_c7_m35", 2, 7, 35, None, 16, "slab", "dense", V(4, 16, 0), None),                # cut tiles through the dense store
    Case("r16_compact_c8_m7", 2, 8, 7, None, 16, "faces", "compact", V(2, 16, 0), None),
    Case("r16_stats_c35_m40", 3, 35, 40, 10, 16, "many_per_cell", "stats", V(4, 16, 0), None),
    Case("r16_stats_c8_m32", 2, 8, 32, 8, 16, "full", "stats", V(2, 16, 0), None),
    Case("c2_fp2_first", 2, 128, 128, 8, 16, "one_per_cell", "stats", V(4, 16, 0), "fp_layers.2.1/first"),
    Case("r16_second_c35_m8", 2, 35, 8, 2, 16, "slab", "second", V(2, 16, 1), None),
    Case("r16_second_c40_m72", 2, 40, 72, 9, 16, "faces", "second", V(4, 16, 1), None),
    Case("r16_second_c8_m32", 2, 8, 32, 8, 16, "full", "second", V(2, 16, 1), None),
    Case("r16_persistent_dense", 12, 8, 72, None, 16, "persistent", "dense", V(4, 16, 0), None),      # two channel blocks
    Case("r16_persistent_compact", 12, 8, 72, None, 16, "persistent", "compact", V(4, 16, 0), None),
    Case("r16_persistent_first", 12, 8, 72, 9, 16, "persistent", "stats", V(4, 16, 0), None),
    Case("r16_persistent_second", 12, 8, 72, 9, 16, "persistent", "second", V(4, 16, 1), None),
    # ---- 32^3 (cin <= 35 but for the C2 rows)
    Case("r32_dense_c7_m35", 1, 7, 35, None, 32, "slab", "dense", V(4, 32, 0), None),
    Case("r32_dense_c8_m8_line", 2, 8, 8, None, 32, "line", "dense", V(2, 32, 0), None),             # global look-ups, one row per form
    Case("r32_compact_c8_m7_line", 2, 8, 7, None, 32, "line", "compact", V(2, 32, 0), None),
    Case("r32_stats_c35_m40_line", 2, 35, 40, 10, 32, "line", "stats", V(4, 32, 0), None),
    Case("r32_second_c35_m8_line", 2, 35, 8, 2, 32, "line", "second", V(2, 32, 1), None),
    Case("r32_stats_c35_m40", 2, 35, 40, 10, 32, "many_per_cell", "stats", V(4, 32, 0), None),
    Case("r32_stats_c8_m32_full", 1, 8, 32, 8, 32, "full", "stats", V(2, 32, 0), None),
    Case("r32_stats_c7_m40_faces", 2, 7, 40, 10, 32, "faces", "stats", V(4, 32, 0), None),
    Case("r32_second_c8_m40_slab", 1, 8, 40, 10, 32, "slab", "second", V(4, 32, 1), None),
    Case("r32_second_c8_m32_full", 1, 8, 32, 8, 32, "full", "second", V(2, 32, 1), None),
    Case("r32_second_c8_m8_faces", 2, 8, 8, 2, 32, "faces", "second", V(2, 32, 1), None),
    Case("c2_sa0_0_first", 1, 6, 32, 8, 32, "one_per_cell", "stats", V(2, 32, 0), "sa_layers.0.0/first"),
    Case("c2_sa0_1_first", 1, 32, 32, 8, 32, "one_per_cell", "stats", V(2, 32, 0), "sa_layers.0.1/first"),
    Case("c2_sa0_second", 1, 32, 32, 8, 32, "one_per_cell", "second", V(2, 32, 1), "sa_layers.0.0/second"),
    Case("c2_fp3_first", 1, 64, 64, 8, 32, "many_per_cell", "stats", V(4, 32, 0), "fp_layers.3.1/first"),
    Case("c2_fp3_second", 1, 64, 64, 8, 32, "many_per_cell", "second", V(4, 32, 1), "fp_layers.3.1/second"),
    Case("r32_persistent_dense", 6, 8, 8, None, 32, "persistent", "dense", V(2, 32, 0), None),
    Case("r32_persistent_compact", 6, 8, 8, None, 32, "persistent", "compact", V(2, 32, 0), None),
    Case("r32_persistent_first", 6, 8, 8, 2, 32, "persistent", "stats", V(2, 32, 0), None),
    Case("r32_persistent_second", 6, 8, 8, 2, 32, "persistent", "second", V(2, 32, 1), None),
]
CASE_IDS = [c.id for c in CASES]
VARIANTS = [V(mt, r, h) for mt in (2, 4) for r in (8, 16, 32) for h in (0, 1)]
# rows whose float64 references are cheap take every input family, the others "normal" (every row also runs the `exact` half)
SMALL = {c.id for c in CASES if c.b * c.cin * c.cout * c.r ** 3 <= 3 * 35 * 40 * 512 and c.cloud != "persistent"}
# small rows of the CPU restatement: (cin, cout, cloud, form), all at 8^3, two shapes each
EMULATION_ROWS = [(1, 8, "many_per_cell", "first"), (7, 8, "one_per_cell", "first"), (8, 12, "faces", "first"), (35, 16, "slab", "first"),
                  (64, 8, "full", "first"), (259, 8, "single", "first"),
                  (35, 8, "one_per_cell", "second"), (100, 8, "faces", "second"), (8, 12, "slab", "second"), (64, 8, "many_per_cell", "second")]


def chosen_variant(case_or_args):
    """(<MT, NT, NW, R, H2IN>, geometry dict) the launch path uses for this shape (host query: no GPU needed)."""
    from bdm_amd import _lib
    b, cin, cout, r, h2in, compact = case_or_args
    v = [ctypes.c_int(-1) for _ in range(9)]
    rc = _lib.lib().bdm_sparse_conv_dil_variant(b, cin, cout, r, h2in, compact, *[ctypes.byref(t) for t in v])
    assert rc == 0, rc
    mt, nt, nw, bm, ncb, tile, xcap, tiles_max, lds = (t.value for t in v)
    return (mt, nt, nw, r, h2in), dict(bm=bm, ncb=ncb, tile=tile, xcap=xcap, tiles_max=tiles_max, lds=lds)


def query(case):
    return chosen_variant((case.b, case.cin, case.cout, case.r, int(case.form == "second"), int(case.form != "dense")))


# ---- clouds and the host restatement of the plan -----------------------------------------------------------------------------------
N_ONE, N_MANY = {8: 40, 16: 200, 32: 900}, {8: 200, 16: 600, 32: 2000}


def cloud_cells(cloud, r, bi, rng):
    """(k, 3) integer cell coordinates of the points of shape `bi` of a batch"""
    grid = np.stack(np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij"), -1).reshape(-1, 3)
    if cloud in ("one_per_cell", "many_per_cell"):
        n = (N_ONE if cloud == "one_per_cell" else N_MANY)[r]
        c = np.clip(np.rint(rng.standard_normal((8 * n, 3)) * r / 8 + r / 2), 0, r - 1).astype(np.int64)
        if cloud == "one_per_cell":
            _, first = np.unique((c[:, 0] * r + c[:, 1]) * r + c[:, 2], return_index=True)
            c = c[np.sort(first)]
        c = c[:n]
        assert len(c) == n
        if cloud == "many_per_cell" and bi % 2 == 1:
            c[: n // 2] = 0
        return c
    if cloud == "single":
        return np.tile(np.array([[r - 1, r - 1, r - 1]] if bi % 2 == 0 else [[r // 2, r // 3, 2]]), (4, 1))
    if cloud in ("full", "persistent"):
        return grid[rng.permutation(r ** 3)]
    if cloud == "slab":
        p0 = r // 2 - 2
        return np.concatenate([grid[p0 * r * r:(p0 + 4) * r * r], np.zeros((1, 3), np.int64)])
    if cloud == "line":
        return np.array([[x, 0, 0] for x in range(0, r, 3)])
    assert cloud == "faces"
    if bi % 2 == 0:
        a = np.array([0, r // 2, r - 1])
        return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    return np.array([[r // 2, r // 2, r // 2], [r // 2 - 1, r // 2, r // 2]])


def batch_coords(cloud, b, r, seed, twice_each=False):
    """(b, 3, n) int32 cell coordinates: every shape padded to the longest with copies of its FIRST point.  twice_each (the `exact`
    half): every distinct cell exactly twice before the padding -- with zero features in the first cell every cell mean is exact."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = [cloud_cells(cloud, r, bi, rng) for bi in range(b)]
    if twice_each:
        out = []
        for c in shapes:
            _, first = np.unique((c[:, 0] * r + c[:, 1]) * r + c[:, 2], return_index=True)
            c = c[np.sort(first)]
            out.append(np.concatenate([c, c]))
        shapes = out
    n = max(len(c) for c in shapes)
    vc = np.stack([np.concatenate([c, np.tile(c[:1], (n - len(c), 1))]) for c in shapes])
    return torch.from_numpy(vc.transpose(0, 2, 1).copy()).to(torch.int32)


def dilate(m):
    r = m.shape[0]
    p = np.zeros((r + 2,) * 3, bool)
    p[1:-1, 1:-1, 1:-1] = m
    d = np.zeros_like(m)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                d |= p[dx:dx + r, dy:dy + r, dz:dz + r]
    return d


def voxel_class(r):
    ax = np.where(np.arange(r) == 0, 0, np.where(np.arange(r) == r - 1, 2, 1))
    return (ax[:, None, None] * 9 + ax[None, :, None] * 3 + ax[None, None, :]).reshape(-1)


HostPlan = namedtuple("HostPlan", "occ_list occ_index d1_list d1_index d2_list d2_index class_count")


def host_plan(vc_b, r):
    """The plan of one shape restated in numpy: lists in ascending voxel order, ranks (-1 outside), cells outside D2 per class."""
    lin = (vc_b[0].astype(np.int64) * r + vc_b[1]) * r + vc_b[2]
    occ = np.zeros(r ** 3, bool)
    occ[lin] = True
    d1 = dilate(occ.reshape(r, r, r))
    d2 = dilate(d1)
    out = []
    for m in (occ, d1.reshape(-1), d2.reshape(-1)):
        lst = np.flatnonzero(m)
        idx = np.full(r ** 3, -1, np.int64)
        idx[lst] = np.arange(len(lst))
        out += [lst, idx]
    cc = np.bincount(voxel_class(r)[~d2.reshape(-1)], minlength=27)
    return HostPlan(*out, cc)


def cell_means(f, vc, r):
    """avg_voxelize restated: float32 sums in point order times the float32 reciprocal of the count -> (B, C, r^3)"""
    B, C, n = f.shape
    lin = ((vc[:, 0].long() * r + vc[:, 1].long()) * r + vc[:, 2].long())
    out = torch.zeros(B, C, r ** 3)
    cnt = torch.zeros(B, r ** 3)
    for b in range(B):
        for i in range(n):
            out[b, :, lin[b, i]] += f[b, :, i]
        cnt[b].index_add_(0, lin[b], torch.ones(n))
    inv = (1.0 / cnt.clamp_min(1).double()).float()
    return out * inv[:, None, :]


def act_scale(amax):
    """act_scale_from_max (bdm_amd/csrc/h2_split.h): the power of two s with amax s in [2^14, 2^15); 1 for 0 / non-finite"""
    if not (amax > 0.0) or not np.isfinite(amax):
        return 1.0
    return float(2.0 ** (15 - np.frexp(np.float32(amax))[1]))


# ---- float64 references and the bound ------------------------------------------------------------------------------------------------
def conv64(x, w, bias, r):
    b, cin = x.shape[:2]
    return TF.conv3d(x.view(b, cin, r, r, r), w, bias, padding=1).reshape(b, -1, r ** 3)


def reference(grid, pad, w, bias, r):
    """float64 convolution of grid (B, cin, r^3) and the magnitude term |W|~ (*) (|x| + pad) + |bias|; pad (B,) per shape (0: exact operands)"""
    g64, w64, b64 = grid.double(), w.double(), bias.double()
    wmax = w64.abs().amax(dim=(1, 2, 3, 4), keepdim=True)
    padv = torch.as_tensor(pad, dtype=torch.float64).view(-1, 1, 1)
    return conv64(g64, w64, b64, r), conv64(g64.abs() + padv, w64.abs() + wmax * 2.0 ** -11, b64.abs(), r)


def first_inputs(family, case_shape, vc, seed):
    """features (B, cin, n), w, bias of a first-form row: the dense file's input families, one value per POINT"""
    b, cin, cout, r = case_shape
    x, w, bias, _ = family_inputs(family, b, cin, cout, r, seed)
    return x[:, :, :vc.shape[2]].contiguous(), w, bias


def second_inputs(family, case_shape, nd1, seed):
    """The operands of a second-form row made on the host: values (B, cin, n_rows) for the rows of D1, the constant (B, cin), the power
    of two s, split into the (hi, lo) records the kernel is given.  -> dict of float32 / fp16 CPU tensors; x_eff / c_eff = (hi + lo) / s."""
    b, cin, cout, r = case_shape
    x, w, bias, s = family_inputs(family, b, cin, cout, r, seed)
    nmax = max(int(n) for n in nd1)
    xv, cv = x[:, :, :nmax], x[:, :, r ** 3 - 1]
    hi, lo = split16(xv * s)
    chi, clo = split16(cv * s)
    x_eff, c_eff = (hi.double() + lo.double()) / s, (chi.double() + clo.double()) / s
    assert torch.equal(x_eff.float().double(), x_eff) and torch.equal(c_eff.float().double(), c_eff)     # const_f32 holds the constant exactly
    return dict(w=w, bias=bias, s=s, hi=hi, lo=lo, chi=chi, clo=clo, x_eff=x_eff.float(), c_eff=c_eff.float())


def second_grid(op, plans, r):
    """The input grid of the second form: (hi + lo) / s of the rows at D1's voxels, the constant elsewhere (B, cin, r^3) float32"""
    B, cin = op["c_eff"].shape
    grid = op["c_eff"][:, :, None].expand(B, cin, r ** 3).clone()
    for b, p in enumerate(plans):
        grid[b][:, torch.from_numpy(p.d1_list)] = op["x_eff"][b, :, :len(p.d1_list)]
    return grid


# ---- CPU restatement of the kernel's arithmetic, on lists ---------------------------------------------------------------------------
def emulate_list(rows, idx, out_list, w, bias, scale, r, const=None, drop=None, shift_tap=None, skip_group=None, const_outside=False,
                 zero_inside=False):
    """sconv_dil_kernel for ONE shape in plain torch.  rows (n_in, cin) operand values, idx (r^3,) row of a voxel or -1, out_list (n_out,)
    voxels; const (cin,) = the H2IN form's constant record, None = first form.  Power-of-two scales, two fp16 terms per operand, the
    neighbour of (voxel, tap) gathered through idx -- absent: zero; H2IN: the constant inside the grid, zero outside -- and the products
    lo.hi + hi.lo + hi.hi of each step of 4 taps x 8 channels added to an fp32 accumulator in the kernel's K order (chunk, tap quad,
    term), unscale, add bias.  -> (cout, n_out).
    Defects: drop a term; shift_tap reads the voxel one further along z; skip_group = (16-voxel block, tap quad) left out;
    const_outside: the constant also for neighbours outside the grid; zero_inside: zero for neighbours inside the grid but not in idx."""
    n_in, cin = rows.shape
    cout, c8, n_out = w.shape[0], cdiv(cin, 8), len(out_list)
    h2in = const is not None
    ws = weight_scale(w)
    wp = torch.zeros(cout, c8 * 8, 28)
    wp[:, :cin, :27] = (w * ws.view(-1, 1, 1, 1, 1)).reshape(cout, cin, 27)
    a = wp.view(cout, c8, 8, 28).permute(0, 1, 3, 2).reshape(cout, c8 * 28 * 8)             # K order: chunk, tap, channel
    recs = torch.zeros(n_in + 2, c8 * 8)                                                    # [n_in]: the constant record, [n_in + 1]: the zero record
    recs[:n_in, :cin] = rows * scale
    if h2in:
        recs[n_in, :cin] = const * scale
    ol = torch.as_tensor(out_list, dtype=torch.long)
    index = torch.as_tensor(idx, dtype=torch.long)
    vx, vy, vz = ol // (r * r), (ol // r) % r, ol % r
    cols = torch.zeros(c8, 28, 8, n_out)
    for t in range(27):
        gx, gy, gz = vx + t // 9 - 1, vy + (t // 3) % 3 - 1, vz + t % 3 - 1 + (1 if t == shift_tap else 0)
        inside = (gx >= 0) & (gx < r) & (gy >= 0) & (gy < r) & (gz >= 0) & (gz < r)
        k = torch.where(inside, index[((gx.clamp(0, r - 1) * r + gy.clamp(0, r - 1)) * r + gz.clamp(0, r - 1))], torch.full_like(gx, -1))
        takes_const = h2in & ((inside & (not zero_inside)) | ((~inside) & const_outside))
        rec = torch.where(k >= 0, k, torch.where(takes_const, torch.full_like(k, n_in), torch.full_like(k, n_in + 1)))
        cols[:, t] = recs[rec].t().reshape(c8, 8, n_out)
    bm = cols.view(c8 * 28 * 8, n_out)
    (a_hi, a_lo), (b_hi, b_lo) = split16(a), split16(bm)
    terms = [("lo.hi", a_lo, b_hi), ("hi.lo", a_hi, b_lo), ("hi.hi", a_hi, b_hi)]     # smallest first, as the kernel issues them
    acc = torch.zeros(cout, n_out)
    keep = torch.ones(n_out)
    if skip_group is not None:
        keep[16 * skip_group[0]:16 * skip_group[0] + 16] = 0.0
    for k0 in range(0, c8 * 28 * 8, 32):
        quad = (k0 // 32) % 7
        for name, at, bt in terms:
            if name == drop:
                continue
            bk = bt[k0:k0 + 32]
            if skip_group is not None and quad == skip_group[1]:
                bk = bk * keep
            acc = acc + torch.matmul(at[:, k0:k0 + 32], bk)
    osc = (1.0 / ws) * (1.0 / scale)
    return acc * osc.view(-1, 1) + bias.view(-1, 1)


def emulation_fraction(row, family, **mutation):
    """worst element of the restatement over the two shapes of an emulation row, in units of u (|W|~ (*) |x|~ + |bias|), and in units
    of the bound in force"""
    cin, cout, cloud, form = row
    r, B = 8, 2
    seed = 17 * cin + cout
    vc = batch_coords(cloud, B, r, seed)
    plans = [host_plan(vc[b].numpy(), r) for b in range(B)]
    shape = (B, cin, cout, r)
    if form == "first":
        f, w, bias = first_inputs(family, shape, vc, seed)
        vox = cell_means(f, vc, r)
        scales = [act_scale(float(vox[b].abs().max())) for b in range(B)]
        ref, mag = reference(vox, [0.25 / s for s in scales], w, bias, r)
        got = [emulate_list(vox[b][:, torch.from_numpy(p.occ_list)].t(), p.occ_index, p.d1_list, w, bias, scales[b], r, **mutation)
               for b, p in enumerate(plans)]
        lists = [p.d1_list for p in plans]
    else:
        op = second_inputs(family, shape, [len(p.d1_list) for p in plans], seed)
        w, bias = op["w"], op["bias"]
        ref, mag = reference(second_grid(op, plans, r), [0.0] * B, w, bias, r)
        got = [emulate_list(op["x_eff"][b, :, :len(p.d1_list)].t(), p.d1_index, p.d2_list, w, bias, op["s"], r, const=op["c_eff"][b], **mutation)
               for b, p in enumerate(plans)]
        lists = [p.d2_list for p in plans]
    e = 0.0
    for b in range(B):
        v = torch.from_numpy(lists[b])
        e = max(e, float(((got[b].double() - ref[b][:, v]).abs() / (U * mag[b][:, v])).max()))
    return e, e / c_bound(cin)


# ---- CPU half -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_reaches_its_variant(case):
    variant, geo = query(case)
    assert variant == case.variant
    mt, nt, nw, r, h2in = variant
    assert geo["bm"] == 16 * mt and geo["ncb"] == cdiv(case.cout, geo["bm"]) and geo["tile"] == 16 * nt * nw == {8: 128, 16: 256, 32: 512}[r]
    assert geo["xcap"] == 3 * r * r and geo["tiles_max"] == r ** 3 // geo["tile"] + r
    # the LDS of a launch: the weight chunk + both operand splits, or (dense form) the tile's results behind the reduction scratch
    operands = 16 * (14 * 4 * geo["bm"] + 2 * (geo["xcap"] + 128))
    out = 4 * ((geo["tile"] // 16 + 1) * (geo["bm"] // 16) * 8 + (geo["bm"] * geo["tile"] if case.form == "dense" else 0))
    assert geo["lds"] == max(operands, out) <= 160 * 1024
    assert case.form in FORMS and (case.groups is None) == (case.form in ("dense", "compact"))
    if case.groups:
        cg = case.cout // case.groups
        assert case.cout % case.groups == 0 and cg >= 4 and cg & (cg - 1) == 0 and geo["bm"] % cg == 0
    assert case.cloud != "line" or r == 32


def test_query_agrees_with_the_plan_and_rejects_other_resolutions():
    from bdm_amd import _lib
    lib = _lib.lib()
    for r in (8, 16, 32):
        assert chosen_variant((1, 8, 8, r, 0, 1))[1]["tiles_max"] == lib.bdm_voxel_dilate_slices(r, 0)
    assert lib.bdm_sparse_conv_dil_variant(2, 8, 8, 16, 0, 1, *([None] * 9)) == 0
    mt = ctypes.c_int(7)
    for r in (0, 4, 12, 24, 64):
        assert lib.bdm_sparse_conv_dil_variant(2, 8, 8, r, 0, 1, ctypes.byref(mt), *([None] * 8)) == 3      # BDM_ERR_UNSUPPORTED
        assert mt.value == 0
    # the second form is always compact; b and cin do not enter
    assert chosen_variant((1, 8, 40, 16, 1, 0)) == chosen_variant((16, 259, 40, 16, 1, 1))


def test_all_twelve_instances_have_rows_and_the_sweep_finds_no_other():
    seen = set()
    for cout in range(1, 257):
        for r in (8, 16, 32):
            for h2in, compact in ((0, 0), (0, 1), (1, 1)):
                seen.add(chosen_variant((3, 64, cout, r, h2in, compact))[0])
    assert len(VARIANTS) == 12 and seen == set(VARIANTS), sorted(seen)
    assert seen == {c.variant for c in CASES}
    for v in VARIANTS:
        assert sum(c.variant == v for c in CASES) >= 2, v


def test_table_covers_the_edges():
    first = [c for c in CASES if c.form != "second"]
    second = [c for c in CASES if c.form == "second"]
    plain = [c for c in CASES if c.form in ("dense", "compact")]
    assert {7, 35} <= {c.cout for c in plain if c.form == "dense"} and {7, 35} <= {c.cout for c in plain if c.form == "compact"}
    assert all(c.r == 8 for c in plain if c.id.startswith("r8_")) and {c.form for c in plain if c.r == 8} == {"dense", "compact"}
    for form in (first, second):
        stats = {(c.cout, c.groups) for c in form if c.groups and c.r == 8}
        assert {(40, 10), (72, 9), (100, 25), (136, 17)} <= stats and any(m == 8 for m, _ in stats) and any(m in (32, 64, 128) for m, _ in stats)
    assert {1, 7, 8, 35, 259} <= {c.cin for c in first if c.r == 8}
    assert {35, 100} <= {c.cin for c in second if c.r == 8} and any(c.cin % 8 == 0 for c in second if c.r == 8)
    assert all(c.cin <= 256 for c in second)
    assert all(c.cin <= 35 or (c.c2 and c.b == 1) for c in CASES if c.r == 32)
    for r in (8, 16, 32):
        for fam, clouds in ((first, {"full", "slab", "faces", "persistent"}), (second, {"full", "slab", "faces", "persistent"})):
            assert clouds <= {c.cloud for c in fam if c.r == r}, (r, clouds)
    assert {"one_per_cell", "many_per_cell", "single"} <= {c.cloud for c in first} & {c.cloud for c in second}
    assert {c.form for c in CASES if c.cloud == "line"} == set(FORMS)
    assert {(c.r, c.form) for c in CASES if c.cloud == "persistent"} == {(r, f) for r in (8, 16, 32) for f in FORMS}


def c2_list_layers():
    """{module/which: (cin, cout, groups, r)} of the convolutions of the C2 step (B = 16 shapes, N = 4096 points) that run on the list
    kernels, read off the denoiser's own modules and their routes: the first convolution where the route says "dil" (with statistics:
    compact rows), the second where the tail runs on lists.  The first module with a shape stands for its repeats."""
    from bdm_amd.modules import PVConv
    from bdm_amd.pvcnn import PVCNN2Base
    B, N = 16, 4096
    net = PVCNN2Base(num_classes=3, embed_dim=64)
    points = [N] + [sa[1][0] for sa in net.sa_blocks]
    out = {}
    for name, m in net.named_modules():
        if not isinstance(m, PVConv):
            continue
        kind, level = name.split(".")[:2]
        n = points[int(level)] if kind == "sa_layers" else points[len(net.fp_blocks) - 1 - int(level)]
        route = m.route(B, n)
        conv1, gn1, conv2, gn2 = m._parts()[:4]
        found = []
        if route.first == "dil":
            assert route.want_stats and route.compact_first
            found.append(("first", (conv1.in_channels, conv1.out_channels, gn1.num_groups, m.resolution)))
        if route.tail == "lists":
            found.append(("second", (conv2.in_channels, conv2.out_channels, gn2.num_groups, m.resolution)))
        for which, shape in found:
            if (which, shape) not in [(k.split("/")[1], v) for k, v in out.items()]:
                out[f"{name}/{which}"] = shape
    return out


def test_c2_step_layers_are_in_the_table_verbatim():
    layers = c2_list_layers()
    table = {c.c2: (c.cin, c.cout, c.groups, c.r) for c in CASES if c.c2}
    assert table == layers
    assert all(c.form == ("second" if c.c2.endswith("second") else "stats") for c in CASES if c.c2)
    assert (64, 64, 8, 32) in layers.values() and (128, 128, 8, 16) in layers.values()


def test_clouds_do_on_the_host_what_they_are_there_for():
    """The host restatement of the plan on the clouds themselves (the GPU rows assert the same from the tables the kernels wrote)."""
    for r in (8, 16, 32):
        cls = voxel_class(r)
        full = host_plan(batch_coords("full", 1, r, 1)[0].numpy(), r)
        assert len(full.occ_list) == len(full.d1_list) == len(full.d2_list) == r ** 3 and not full.class_count.any()
        one = batch_coords("one_per_cell", 2, r, 2)
        assert all(len(host_plan(one[b].numpy(), r).occ_list) == one.shape[2] for b in range(2))
        many = batch_coords("many_per_cell", 2, r, 3)
        assert len(host_plan(many[1].numpy(), r).occ_list) < many.shape[2] // 2 + 1
        single = batch_coords("single", 2, r, 4)
        a, b = host_plan(single[0].numpy(), r), host_plan(single[1].numpy(), r)
        assert len(a.occ_list) == len(b.occ_list) == 1 and len(a.d1_list) == 8 and len(b.d1_list) == 27 and len(a.d2_list) == 27 and len(b.d2_list) == 125
        faces = batch_coords("faces", 2, r, 5)
        inn, out = host_plan(faces[0].numpy(), r), host_plan(faces[1].numpy(), r)
        assert set(cls[inn.d1_list]) == set(range(27)) and (out.class_count > 0).all()
        slab = host_plan(batch_coords("slab", 1, r, 6)[0].numpy(), r)
        assert len(slab.occ_list) == 4 * r * r + 1 and slab.occ_list[0] == 0
    line = host_plan(batch_coords("line", 1, 32, 7)[0].numpy(), 32)
    assert len(line.d1_list) <= 512 and {v // 1024 for v in line.d1_list} == set(range(32))
    assert len(line.d2_list) <= 512 and {v // 1024 for v in line.d2_list} == set(range(32))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("row", EMULATION_ROWS, ids=lambda r: "c{}_m{}_{}_{}".format(*r))
def test_emulation_stays_inside_the_bound(row, family):
    """The restatement of the kernel's arithmetic is within EMU_WORST u (|W|~ (*) |x|~ + |bias|) per element -- the figure the
    tightened constant 4 EMU_WORST comes from -- hence at most a quarter of the bound in force (or all of c(K), were that smaller)."""
    e, frac = emulation_fraction(row, family)
    print(f"emulation {row} {family}: worst element {e:.3f} u mag, {frac:.3f} of the bound")
    assert e <= EMU_WORST and frac <= 1.0, (e, frac)


# (defect, the rows it applies to): the H2IN defects need a neighbour outside the grid / inside the grid and outside D1
MUTANTS = [(dict(drop="hi.lo"), None), (dict(shift_tap=13), None), (dict(skip_group=(0, 6)), None),
           (dict(const_outside=True), ("second",)), (dict(zero_inside=True), ("second",))]
MUTANT_RUNS = [(row, m) for m, forms in MUTANTS for row in EMULATION_ROWS if forms is None or row[3] in forms]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("row,mutation", MUTANT_RUNS,
                         ids=["c{}_m{}_{}_{}-".format(*r) + "-".join(f"{k}={v}" for k, v in m.items()) for r, m in MUTANT_RUNS])
def test_broken_emulation_falls_outside_the_bound(row, mutation, family):
    """One dropped partial product, one tap shifted by a voxel, one skipped (block, tap quad) group, a constant record where the
    padding is, a zero where the constant is -- at every width and in every input family: outside the bound."""
    e, frac = emulation_fraction(row, family, **mutation)
    print(f"mutant {mutation} {row} {family}: worst element {frac:.3g} of the bound")
    assert frac > 1.0, frac


# ---- GPU half: plans, launches ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(hip):
    from bdm_amd import ops as o
    return o


def twice(launch):
    """Run a launch twice (fresh outputs each time) and assert bit-equal results; returns the first."""
    first, second = launch(), launch()
    for a, c in zip(first, second):
        assert torch.equal(a, c), "two launches of the same case differ"
    return first


def build_plan(ops, vc, r):
    """The plan of integer cell coordinates (B, 3, n) as ops.sparse_first_conv builds it, with both dilated lists"""
    from bdm_amd import _lib as L
    lib = L.lib()
    B, _, n = vc.shape
    p = ops.VoxelPlan(vc, r)
    L.check(lib.bdm_voxelize_plan(B, n, r, L.ptr(vc), L.ptr(p.ind), L.ptr(p.cnt), L.ptr(p.ws), L.stream()), "voxelize_plan")
    L.check(lib.bdm_voxel_compact(B, r, p.n_max, L.ptr(p.cnt), L.ptr(p.occ_index), L.ptr(p.occ_list), L.ptr(p.n_occ), L.stream()), "voxel_compact")
    L.check(lib.bdm_voxel_row_occupancy(B, r, L.ptr(p.cnt), L.ptr(p.rowocc), L.stream()), "voxel_row_occupancy")
    ops.plan_dilation(p)
    ops.plan_dilation2(p)
    assert p.tile == 0 and p.d2_tile == 0 and p.n_dil_max == r ** 3
    return p


Tables = namedtuple("Tables", "cnt occ_index d1_list d1_index t1 d2_list d2_index t2 class_count")


def read_tables(p):
    return Tables(*(t.cpu().numpy() for t in (p.cnt, p.occ_index, p.dil_list, p.dil_index, p.tile_start, p.d2_list, p.d2_index, p.d2_tiles,
                                              p.d2_class_count)))


def live(ts_b):
    """(live tiles, list length) of one shape's tile table"""
    return int(ts_b[0, 7]), int(ts_b[-1, 1])


def assert_reach(case, tb, geo):
    """REACH: from the tables the plan kernels wrote, this row's cloud does what it is in the table for."""
    r, B = case.r, case.b
    second = case.form == "second"
    ts = tb.t2 if second else tb.t1
    tile, xcap = geo["tile"], geo["xcap"]
    lives = [live(ts[b]) for b in range(B)]
    occ = [int((tb.cnt[b] > 0).sum()) for b in range(B)]
    if case.cloud == "one_per_cell":
        assert int(tb.cnt.max()) == 1
    elif case.cloud == "many_per_cell":
        assert int(tb.cnt.max()) > 1 and (B < 2 or int(tb.cnt[1, 0]) >= case_points(case) // 2)
    elif case.cloud == "single":
        assert occ == [1] * B and int(tb.cnt[0, r ** 3 - 1]) > 0 and (B < 2 or int(tb.cnt[1, ((r // 2) * r + r // 3) * r + 2]) > 0)
    elif case.cloud in ("full", "persistent"):
        assert all(nd == r ** 3 for _, nd in lives) and occ == [r ** 3] * B
        assert any(int(ts[b, t, 5]) == xcap for b in range(B) for t in range(lives[b][0])), "no tile's input range holds exactly xcap rows"
        assert not tb.class_count.any()
    elif case.cloud == "slab":
        for b in range(B):
            nt = lives[b][0]
            assert any(int(ts[b, t, 1] - ts[b, t, 0]) < tile for t in range(nt - 1)), "the slab did not force a cut"
    elif case.cloud == "line":
        for b in range(B):
            spans = []
            for t in range(lives[b][0]):
                x0, x1 = int(ts[b, t, 6]) >> 8, int(ts[b, t, 6]) & 255
                spans.append(min(x1 + 1, r - 1) - max(x0 - 1, 0) + 1)
            assert max(spans) > 25 and max(spans) * r * r * 4 > 2 * (xcap + 128) * 16, "no tile takes the global look-up path"
    elif case.cloud == "faces":
        cls = voxel_class(r)
        lst = tb.d2_list if second else tb.d1_list
        inside = set()
        for b in range(B):
            inside |= set(cls[lst[b, :lives[b][1]]])
        assert inside == set(range(27)), "a boundary class has no voxel inside the lists"
        assert B >= 2 and (tb.class_count[1] > 0).all(), "a boundary class has no voxel outside the lists"
    if case.cloud == "persistent":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        items = sum(nt for nt, _ in lives) * geo["ncb"]
        assert items >= 1.25 * cus, f"{items} live items on {cus} CUs: no workgroup computes two live tiles in succession"
    for b in range(B):   # every row: the live tiles' input ranges fit the LDS budget the launch was sized for
        assert all(0 <= int(ts[b, t, 5]) <= xcap for t in range(lives[b][0]))


def case_points(case):
    return batch_coords(case.cloud, case.b, case.r, 1).shape[2]


def launch_first(ops, f, plan, packed, bias, cout, form, groups=None):
    """bdm_sparse_conv_dil(_gn) as ops.sparse_first_conv_os launches it, into a sentinel-filled output with 64 guard floats behind it.
    -> (y, guard) or (y, guard, partials (B, groups, tiles, 2))"""
    from bdm_amd import _lib as L
    lib = L.lib()
    fb = ops._bcl(f)
    _, B, C = fb[:3]
    r = plan.r
    xr, slots = ops._records_f32(fb, plan, extra=1)
    amax, counter = slots[:B], slots[B:]
    compact = form != "dense"
    shape = (B, plan.n_dil_max, cout) if compact else (B, cout, r ** 3)
    numel = shape[0] * shape[1] * shape[2]
    buf = torch.full((numel + 64,), SENT, device=DEV)
    y, guard = buf[:numel].view(shape), buf[numel:]
    pk, inv = packed
    args = (B, C, cout, r, plan.n_max, plan.n_dil_max, L.ptr(xr), L.ptr(amax), L.ptr(plan.occ_index), L.ptr(plan.dil_list),
            L.ptr(plan.dil_index), L.ptr(plan.tile_start), L.ptr(pk), L.ptr(inv), L.ptr(bias), L.ptr(y), 1 if compact else 0)
    if groups:
        tiles = plan.tile_start.shape[1]
        partial = torch.full((B, groups, tiles, 2), float("nan"), dtype=torch.float64, device=DEV)
        slices = ctypes.c_int(0)
        L.check(lib.bdm_sparse_conv_dil_gn(*args, int(groups), L.ptr(partial), ctypes.byref(slices), 0, L.ptr(counter), L.stream()), "sparse_conv_dil_gn")
        assert slices.value == tiles
        return y, guard, partial
    L.check(lib.bdm_sparse_conv_dil(*args, 0, L.ptr(counter), L.stream()), "sparse_conv_dil")
    return y, guard


def pack_rows(hi, lo, n_rows_max, nd, fill=60000.0):
    """(hi, lo) (B, cin, n) float32 holding fp16 values -> rows_h2 (B, C8, 2, n_rows_max, 8) fp16; rows at or beyond nd[b]: `fill`
    (finite, enormous: a kernel that reads one is off by orders of magnitude)"""
    B, cin, n = hi.shape
    c8 = cdiv(cin, 8)
    rows = torch.full((B, c8, 2, n_rows_max, 8), fill, dtype=torch.float16)
    for s, t in enumerate((hi, lo)):
        padded = torch.zeros(B, c8 * 8, n)
        padded[:, :cin] = t
        for b in range(B):
            rows[b, :, s, :nd[b]] = padded[b, :, :nd[b]].view(c8, 8, nd[b]).permute(0, 2, 1).half()
    return rows


def pack_const(chi, clo):
    B, cin = chi.shape
    c8 = cdiv(cin, 8)
    rec = torch.zeros(B, c8, 2, 8, dtype=torch.float16)
    for s, t in enumerate((chi, clo)):
        padded = torch.zeros(B, c8 * 8)
        padded[:, :cin] = t
        rec[:, :, s] = padded.view(B, c8, 8).half()
    return rec


def launch_second(ops, op_dev, plan, packed, wsum, bias, cin, cout, groups):
    """bdm_sparse_conv_dil_h2_gn + bdm_conv3d_class_constants as ops.second_conv_rows launches them, into a sentinel-filled output.
    -> (y (B, n_dil_max, cout), guard, class_vals (B, 27, cout), partials (B, groups, tiles + 27, 2))"""
    from bdm_amd import _lib as L
    lib = L.lib()
    rows_h2, const_h2, const_f32, inv_s = op_dev
    B, r = rows_h2.shape[0], plan.r
    numel = B * plan.n_dil_max * cout
    buf = torch.full((numel + 64,), SENT, device=DEV)
    y, guard = buf[:numel].view(B, plan.n_dil_max, cout), buf[numel:]
    tiles = plan.d2_tiles.shape[1]
    partial = torch.full((B, groups, tiles + 27, 2), float("nan"), dtype=torch.float64, device=DEV)
    counter = ops.amax_slots(DEV, 1)
    slices = ctypes.c_int(0)
    pk, inv = packed
    L.check(lib.bdm_sparse_conv_dil_h2_gn(B, cin, cout, r, plan.n_dil_max, plan.n_dil_max, L.ptr(rows_h2), L.ptr(const_h2), L.c_float(inv_s),
                                          L.ptr(plan.dil_index), L.ptr(plan.d2_list), L.ptr(plan.d2_index), L.ptr(plan.d2_tiles), L.ptr(pk),
                                          L.ptr(inv), L.ptr(bias), L.ptr(y), int(groups), L.ptr(partial), ctypes.byref(slices), 0,
                                          L.ptr(counter), L.stream()), "sparse_conv_dil_h2_gn")
    assert slices.value == tiles + 27
    class_vals = torch.full((B, 27, cout), SENT, device=DEV)
    L.check(lib.bdm_conv3d_class_constants(B, cin, cout, L.ptr(wsum), L.ptr(bias), L.ptr(const_f32), L.ptr(plan.d2_class_count), L.ptr(class_vals),
                                           int(groups), L.ptr(partial), tiles + 27, tiles, L.stream()), "conv3d_class_constants")
    return y, guard, class_vals, partial


class Figures:
    """The figures of one test: reported through helpers.parity as they are measured, asserted together at the end."""

    def __init__(self):
        self.bad = []

    def fraction(self, name, frac, what):
        parity(f"{current_test()} {name}", frac, 1.0, note=what)
        print(f"{name:24s} {what:50s} {frac:8.4f} of the bound")
        if not frac <= 1.0:
            self.bad.append(f"{name}, {what}: {frac:.3g} x its bound")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def elementwise(fig, name, got, ref, mag, cin, what):
    """got, ref, mag (.., n) on the CPU: the worst element in units of the bound in force"""
    assert bool(torch.isfinite(got).all()), f"{name}, {what}: not finite"
    frac = float(((got.double() - ref).abs() / (c_bound(cin) * U * mag)).max()) if got.numel() else 0.0
    fig.fraction(name, frac, what)


def check_tile_partials(fig, p, rows, ts, geo, groups, bias, what):
    """Slice partials p (B, G, S, 2) of the tiles against the rows (B, n, cout) the kernel wrote; bias: the first form's closed-form
    share of the owned linear range (None: second form)."""
    B, _, cout = rows.shape
    cg, n32 = cout // groups, 4 * geo["tile"]
    fs = fq = 0.0
    for b in range(B):
        nt, _ = live(ts[b])
        assert bool((p[b, :, nt:geo["tiles_max"]] == 0.0).all()), "a dead tile's slice is not exactly zero"
        for t in range(nt):
            j0, j1, vf, ve = (int(v) for v in ts[b, t, :4])
            v = rows[b, j0:j1].double().view(j1 - j0, groups, cg)
            s, q, a = v.sum((0, 2)), (v * v).sum((0, 2)), v.abs().sum((0, 2))
            es, eq = n32 * U * a, (n32 + 1) * U * q
            if bias is not None:
                nfill = (ve - vf) - (j1 - j0)
                bg = bias.double().view(groups, cg)
                s, q = s + nfill * bg.sum(1), q + nfill * (bg * bg).sum(1)
                a, es, eq = a + nfill * bg.abs().sum(1), es, eq
            es, eq = es + 2.0 ** -50 * (a + s.abs()), eq + 2.0 ** -50 * q
            fs = max(fs, float(((p[b, :, t, 0] - s).abs() / es.clamp_min(1e-300)).max()))
            fq = max(fq, float(((p[b, :, t, 1] - q).abs() / eq.clamp_min(1e-300)).max()))
    fig.fraction("slice sums", fs, what)
    fig.fraction("slice sums of squares", fq, what)


# ---- (2) the plan of the second list ------------------------------------------------------------------------------------------------
PLAN_CLOUDS = ("one_per_cell", "many_per_cell", "single", "full", "slab", "faces", "line")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [8, 16, 32])
def test_twice_dilated_list_and_its_tile_table(ops, r):
    """bdm_voxel_dilate_again against the numpy restatement, exactly: d2_list = the dilation of D1 in ascending voxel order, d2_index its
    ranks, class_count the cells outside D2 per boundary class, a tile table that partitions the list in tiles of at most the tile size
    whose input ranges are rows ps_D1[max(x0 - 1, 0)] .. ps_D1[min(x1 + 2, r)] of D1 (at most xcap), [7] = the live count in every
    record, dead records = the list length.  And the same once more for the first list the second is built from."""
    clouds = [c for c in PLAN_CLOUDS if c != "line" or r == 32]
    shapes = []
    for i, cloud in enumerate(clouds):
        vc = batch_coords(cloud, 2, r, 40 + i)
        shapes += [vc[0], vc[1]]
    n = max(s.shape[1] for s in shapes)
    vc = torch.stack([torch.cat([s, s[:, :1].expand(3, n - s.shape[1])], 1) for s in shapes]).contiguous()
    B = vc.shape[0]
    _, geo = chosen_variant((B, 8, 8, r, 1, 1))
    tile, xcap, tiles_max = geo["tile"], geo["xcap"], geo["tiles_max"]
    plan = build_plan(ops, vc.to(DEV), r)
    tb = read_tables(plan)
    plan_again = build_plan(ops, vc.to(DEV), r)
    for name, a, c in zip(Tables._fields, tb, read_tables(plan_again)):
        if name in ("d1_list", "d2_list"):   # entries at or beyond the list length are never written
            ts = tb.t1 if name == "d1_list" else tb.t2
            assert all(np.array_equal(a[b, :live(ts[b])[1]], c[b, :live(ts[b])[1]]) for b in range(B)), f"two plans of the same cloud differ: {name}"
        else:
            assert np.array_equal(a, c), f"two plans of the same cloud differ: {name}"
    assert tb.t1.shape == tb.t2.shape == (B, tiles_max, 16)
    cut = set()
    for b in range(B):
        hp = host_plan(vc[b].numpy(), r)
        assert np.array_equal(tb.occ_index[b], hp.occ_index)
        for ts, lst, idx, want, want_idx, src in ((tb.t1[b], tb.d1_list[b], tb.d1_index[b], hp.d1_list, hp.d1_index, hp.occ_list),
                                                  (tb.t2[b], tb.d2_list[b], tb.d2_index[b], hp.d2_list, hp.d2_index, hp.d1_list)):
            nt, nd = live(ts)
            assert nd == len(want) and np.array_equal(lst[:nd], want) and np.array_equal(idx, want_idx), (r, b)
            ps = np.concatenate([[0], np.cumsum(np.bincount(src // (r * r), minlength=r))])        # input cells in planes < x
            assert 1 <= nt <= tiles_max and (ts[:, 7] == nt).all() and ts[0, 0] == 0 and int(ts[nt - 1, 1]) == nd
            for t in range(nt):
                j0, j1, vf, ve, klo, nr = (int(v) for v in ts[t, :6])
                assert 0 < j1 - j0 <= tile and (t == 0 or j0 == int(ts[t - 1, 1]))
                assert vf == (0 if t == 0 else want[j0]) and ve == (want[j1] if t + 1 < nt else r ** 3)
                x0, x1 = want[j0] // (r * r), want[j1 - 1] // (r * r)
                assert int(ts[t, 6]) == (x0 << 8) | x1
                assert klo == ps[max(x0 - 1, 0)] and nr == ps[min(x1 + 2, r)] - klo and nr <= xcap, (r, b, t)
                assert not ts[t, 8:].any()
                if t + 1 < nt and j1 - j0 < tile:
                    cut.add((b, src is hp.d1_list))
            assert (ts[nt:, 0] == nd).all() and (ts[nt:, 1] == nd).all() and (ts[nt:, 2] == r ** 3).all() and (ts[nt:, 3] == r ** 3).all()
            assert not ts[nt:, 4:7].any() and not ts[nt:, 8:].any()
        assert np.array_equal(tb.class_count[b], hp.class_count), (r, b, tb.class_count[b], hp.class_count)
    slab = [2 * clouds.index("slab"), 2 * clouds.index("slab") + 1]
    assert all((b, False) in cut and (b, True) in cut for b in slab), "the slab was not cut on both tables"
    full = 2 * clouds.index("full")
    assert not tb.class_count[full].any() and live(tb.t2[full])[1] == r ** 3
    assert (tb.class_count[2 * clouds.index("faces") + 1] > 0).all()


# ---- (3) the two convolutions ---------------------------------------------------------------------------------------------------------
def exact_weights(cin, cout, g):
    """weights = small integers x a power of two per output channel, bias likewise"""
    p = torch.exp2((torch.arange(cout) % 5 - 2).float())
    w = torch.randint(-7, 8, (cout, cin, 3, 3, 3), generator=g).float() * p.view(-1, 1, 1, 1, 1)
    bias = torch.randint(-100, 101, (cout,), generator=g).float() * p
    assert 27 * cin * 7 * 7 + 100 < 2 ** 24
    return w, bias


def listed(ref, lst, nd):
    """ref (cout, r^3) at the first nd voxels of a list -> (nd, cout)"""
    return ref[:, torch.from_numpy(lst[:nd].astype(np.int64))].t()


def run_first(ops, oracle_ops, case, geo, half, fig):
    B, cin, cout, r, groups = case.b, case.cin, case.cout, case.r, case.groups
    seed = 1000 + CASE_IDS.index(case.id)
    exact = half == "exact"
    vc = batch_coords(case.cloud, B, r, seed, twice_each=exact)
    n = vc.shape[2]
    if exact:   # every point of a cell carries the cell's own small integers; the first cell (where the padding goes) carries zeros
        g = torch.Generator().manual_seed(seed)
        cellv = torch.randint(-7, 8, (B, cin, r ** 3), generator=g).float()
        lin = ((vc[:, 0].long() * r + vc[:, 1].long()) * r + vc[:, 2].long())
        for b in range(B):
            cellv[b, :, lin[b, 0]] = 0.0
        f = cellv.gather(2, lin[:, None, :].expand(B, cin, n)).contiguous()
        w, bias = exact_weights(cin, cout, g)
    else:
        f, w, bias = first_inputs(half, (B, cin, cout, r), vc, seed)
    vox = oracle_ops.avg_voxelize_forward(f, vc, r)[0].view(B, cin, r ** 3)
    scales = [act_scale(float(vox[b].abs().max())) for b in range(B)]
    ref, mag = reference(vox, [0.25 / s for s in scales], w, bias, r)
    if exact:
        assert torch.equal(vox, vox.round()) and float(vox.abs().max()) <= 7 and torch.equal(ref.float().double(), ref)
    fd, vcd, wd, bd = f.to(DEV), vc.to(DEV), w.to(DEV), bias.to(DEV)
    plan = build_plan(ops, vcd, r)
    tb = read_tables(plan)
    if not exact:
        assert_reach(case, tb, geo)
    if case.cloud == "many_per_cell" and half == "normal":
        assert torch.equal(ops.avg_voxelize(fd, vcd, r).cpu(), vox), "the cell means differ from the oracle's"
    packed = ops.conv3d_h2_pack(wd)
    nd = [live(tb.t1[b])[1] for b in range(B)]
    what = f"{half}, {case.form}"

    def rows_check(yc, guard):
        y = yc.cpu()
        for b in range(B):
            want = listed(ref[b], tb.d1_list[b], nd[b])
            if exact:
                assert torch.equal(y[b, :nd[b]].double(), want), f"shape {b}: {int((y[b, :nd[b]].double() != want).sum())} elements differ from the exact result"
            else:
                elementwise(fig, "elementwise", y[b, :nd[b]], want, listed(mag[b], tb.d1_list[b], nd[b]), cin, f"{what}, shape {b}")
            assert bool((y[b, nd[b]:] == SENT).all()), f"shape {b}: rows at or beyond the list length were written"
        assert bool((guard == SENT).all()), "floats behind the output were written"
        return y

    def grid_check(yd, guard):
        y = yd.cpu()
        if exact:
            assert torch.equal(y.double(), ref), f"{int((y.double() != ref).sum())} elements differ from the exact result"
        else:
            for b in range(B):
                elementwise(fig, "elementwise", y[b], ref[b], mag[b], cin, f"{what}, shape {b}, whole grid")
        assert bool((guard == SENT).all()), "floats behind the output were written"
        return y

    yd, gd = twice(lambda: launch_first(ops, fd, plan, packed, bd, cout, "dense"))
    yc, gc = twice(lambda: launch_first(ops, fd, plan, packed, bd, cout, "compact"))
    dense = grid_check(yd, gd) if case.form == "dense" else yd.cpu()
    rows = rows_check(yc, gc) if case.form != "dense" else yc.cpu()
    for b in range(B):
        assert torch.equal(rows[b, :nd[b]], listed(dense[b], tb.d1_list[b], nd[b])), f"shape {b}: compact and dense form differ"
        outside = torch.from_numpy(tb.d1_index[b] < 0)
        assert torch.equal(dense[b][:, outside], bias[:, None].expand(cout, int(outside.sum()))), f"shape {b}: a voxel outside the list is not the bias"
    if groups:
        ys, gs, ps = twice(lambda: launch_first(ops, fd, plan, packed, bd, cout, "compact", groups))
        assert torch.equal(ys, yc), "the statistics form writes other rows than the plain form"
        assert bool((gs == SENT).all())
        yds, _, pds = twice(lambda: launch_first(ops, fd, plan, packed, bd, cout, "dense", groups))
        assert torch.equal(yds, yd) and torch.equal(pds, ps), "the dense statistics form differs"
        if not exact:
            check_tile_partials(fig, ps.cpu(), rows, tb.t1, geo, groups, bias, what)
        else:
            assert bool(torch.isfinite(ps).all())
    # through the operator, and from a strided feature view
    got = ops.sparse_first_conv_os(fd, plan, packed, bd, cout, compact=True)
    wide = torch.randn(B, cin + 6, n, device=DEV)
    wide[:, 3:3 + cin] = fd
    view = ops.sparse_first_conv_os(wide[:, 3:3 + cin], plan, packed, bd, cout, compact=True)
    for b in range(B):
        assert torch.equal(got.rows[b, :nd[b]], yc[b, :nd[b]]), "ops.sparse_first_conv_os gives other rows"
        assert torch.equal(view.rows[b, :nd[b]], yc[b, :nd[b]]), "a strided feature view gives other rows"
    if B > 1:   # the last shape alone
        alone = build_plan(ops, vcd[B - 1:].contiguous(), r)
        ya, _ = launch_first(ops, fd[B - 1:].contiguous(), alone, packed, bd, cout, "compact")
        assert torch.equal(ya[0, :nd[B - 1]], yc[B - 1, :nd[B - 1]]), "a shape alone differs from the same shape in its batch"


def dense_h2_operand(op, plans_d1, r):
    """The second form's operands as the dense H2 grid ops.conv3d_h2 takes: (B, C8, 2, r^3, 8) fp16"""
    B, cin = op["chi"].shape
    c8 = cdiv(cin, 8)
    out = torch.zeros(B, c8 * 8, 2, r ** 3)
    for s, (t, c) in enumerate(((op["hi"], op["chi"]), (op["lo"], op["clo"]))):
        out[:, :cin, s] = c[:, :, None]
        for b, (lst, nd) in enumerate(plans_d1):
            out[b, :cin, s][:, torch.from_numpy(lst[:nd].astype(np.int64))] = t[b, :, :nd]
    return out.view(B, c8, 8, 2, r ** 3).permute(0, 1, 3, 4, 2).contiguous().half()


def class_sums_numpy(w):
    """wsum[k][ci][co] = the sum of the taps of w[co][ci] that stay inside the grid for boundary class k, in float64"""
    cout, cin = w.shape[:2]
    w64 = w.double().numpy().reshape(cout, cin, 3, 3, 3)
    out = np.zeros((27, cin, cout))
    for k in range(27):
        sl = [slice(1, 3) if c == 0 else (slice(0, 2) if c == 2 else slice(0, 3)) for c in (k // 9, (k // 3) % 3, k % 3)]
        out[k] = w64[:, :, sl[0], sl[1], sl[2]].sum((2, 3, 4)).T
    return out


def run_second(ops, case, geo, half, fig):
    B, cin, cout, r, groups = case.b, case.cin, case.cout, case.r, case.groups
    seed = 1000 + CASE_IDS.index(case.id)
    exact = half == "exact"
    vc = batch_coords(case.cloud, B, r, seed)
    plan = build_plan(ops, vc.to(DEV), r)
    tb = read_tables(plan)
    if not exact:
        assert_reach(case, tb, geo)
    nd1 = [live(tb.t1[b])[1] for b in range(B)]
    nd2 = [live(tb.t2[b])[1] for b in range(B)]
    if exact:   # small integers times 16: every operand exact in its hi term, lo = 0
        g = torch.Generator().manual_seed(seed)
        xv = torch.randint(-7, 8, (B, cin, max(nd1)), generator=g).float()
        cv = torch.randint(-7, 8, (B, cin), generator=g).float()
        w, bias = exact_weights(cin, cout, g)
        op = dict(w=w, bias=bias, s=16.0, hi=xv * 16, lo=torch.zeros_like(xv), chi=cv * 16, clo=torch.zeros_like(cv), x_eff=xv, c_eff=cv)
    else:
        op = second_inputs(half, (B, cin, cout, r), nd1, seed)
        w, bias = op["w"], op["bias"]
    hps = [HostPlan(None, None, tb.d1_list[b, :nd1[b]].astype(np.int64), None, None, None, None) for b in range(B)]
    ref, mag = reference(second_grid(op, hps, r), [0.0] * B, w, bias, r)
    if exact:
        assert torch.equal(ref.float().double(), ref)
    wd, bd = w.to(DEV), bias.to(DEV)
    packed = ops.conv3d_h2_pack(wd)
    (wsum,) = twice(lambda: (ops.conv_class_pack(wd),))
    op_dev = (pack_rows(op["hi"], op["lo"], r ** 3, nd1).to(DEV), pack_const(op["chi"], op["clo"]).to(DEV), op["c_eff"].to(DEV).contiguous(),
              1.0 / op["s"])
    y, guard, cvals, part = twice(lambda: launch_second(ops, op_dev, plan, packed, wsum, bd, cin, cout, groups))
    yc, cv_cpu, part = y.cpu(), cvals.cpu(), part.cpu()
    what = f"{half}, second"
    for b in range(B):
        want = listed(ref[b], tb.d2_list[b], nd2[b])
        if exact:
            assert torch.equal(yc[b, :nd2[b]].double(), want), f"shape {b}: {int((yc[b, :nd2[b]].double() != want).sum())} elements differ from the exact result"
        else:
            elementwise(fig, "elementwise", yc[b, :nd2[b]], want, listed(mag[b], tb.d2_list[b], nd2[b]), cin, f"{what}, shape {b}")
        assert bool((yc[b, nd2[b]:] == SENT).all()), f"shape {b}: rows at or beyond the list length were written"
    assert bool((guard == SENT).all()), "floats behind the output were written"
    # the operator gives the same rows, class values and partials
    rows_o, cv_o, (part_o, _) = ops.second_conv_rows(*op_dev, plan, packed, wsum, bd, cin, cout, groups)
    assert all(torch.equal(rows_o[b, :nd2[b]], y[b, :nd2[b]]) for b in range(B)) and torch.equal(cv_o, cvals) and torch.equal(part_o.cpu(), part)
    # the dense kernel on the densified operands: the same MFMA sequence on the same operands at the listed voxels
    xh = dense_h2_operand(op, [(tb.d1_list[b], nd1[b]) for b in range(B)], r).to(DEV)
    y_dense = ops.conv3d_h2((xh, 1.0 / op["s"]), packed, bd, cin, cout, r).cpu()
    for b in range(B):
        assert torch.equal(yc[b, :nd2[b]], listed(y_dense[b], tb.d2_list[b], nd2[b])), f"shape {b}: the listed voxels differ from ops.conv3d_h2"
    # class weight sums and class constants
    ws_ref = torch.from_numpy(class_sums_numpy(w))
    ws_got = wsum.cpu().view(27, cin, cout)
    wabs = w.double().abs().sum((2, 3, 4)).t()
    fig.fraction("class weight sums", float(((ws_got - ws_ref).abs() / (27 * 2.0 ** -53 * wabs).clamp_min(1e-300)).max()), what)
    c64 = op["c_eff"].double()
    cref = bias.double()[None, None, :] + torch.einsum("kio,bi->bko", ws_got, c64)
    cmag = bias.double().abs()[None, None, :] + torch.einsum("kio,bi->bko", ws_got.abs(), c64.abs())
    cerr = U * cref.abs() + 2.0 ** -149 + cin * 2.0 ** -53 * cmag
    if exact:
        assert torch.equal(cv_cpu.double(), cref)
    fig.fraction("class constants", float(((cv_cpu.double() - cref).abs() / cerr).max()), what)
    cls = voxel_class(r)
    tied = 0
    for b in range(B):   # ... and against the float64 convolution at a voxel of each class outside D2
        worst = 0.0
        for k in range(27):
            out_k = np.flatnonzero((tb.d2_index[b] < 0) & (cls == k))
            assert len(out_k) == int(tb.class_count[b, k])
            if len(out_k):
                v = int(out_k[len(out_k) // 2])
                err = (cv_cpu[b, k].double() - ref[b, :, v]).abs() / (cerr[b, k] + 27 * cin * 2.0 ** -53 * mag[b, :, v])
                worst = max(worst, float(err.max()))
                tied += 1
        fig.fraction("class constant = convolution", worst, f"{what}, shape {b}")
    assert case.cloud != "faces" or tied >= 27
    # statistics: the tiles' slices against the rows written, the 27 class slices against the class values written
    tiles = geo["tiles_max"]
    if not exact:
        check_tile_partials(fig, part[:, :, :tiles], yc, tb.t2, geo, groups, None, what)
    cg = cout // groups
    cvg = cv_cpu.double().view(B, 27, groups, cg)
    cnt = torch.from_numpy(tb.class_count.astype(np.float64))[:, :, None]
    want_s, want_q = (cnt * cvg.sum(3)).permute(0, 2, 1), (cnt * (cvg * cvg).sum(3)).permute(0, 2, 1)
    got_s, got_q = part[:, :, tiles:, 0], part[:, :, tiles:, 1]
    scale_s = (cnt * cvg.abs().sum(3)).permute(0, 2, 1)
    fig.fraction("class slices", max(float(((got_s - want_s).abs() / (2.0 ** -50 * scale_s).clamp_min(1e-300)).max()),
                                     float(((got_q - want_q).abs() / (2.0 ** -50 * want_q).clamp_min(1e-300)).max())), what)
    zero = torch.from_numpy(tb.class_count == 0)[:, None, :].expand(B, groups, 27)
    assert bool((got_s[zero] == 0.0).all()) and bool((got_q[zero] == 0.0).all()), "the slice of an empty class is not exactly 0.0"
    if B > 1:   # the last shape alone
        alone = build_plan(ops, vc[B - 1:].contiguous().to(DEV), r)
        op_alone = tuple(t[B - 1:].contiguous() for t in op_dev[:3]) + (op_dev[3],)
        ya, _, cva, pa = launch_second(ops, op_alone, alone, packed, wsum, bd, cin, cout, groups)
        assert torch.equal(ya[0, :nd2[B - 1]], y[B - 1, :nd2[B - 1]]) and torch.equal(cva[0], cvals[B - 1]) and torch.equal(pa[0].cpu(), part[B - 1]), \
            "a shape alone differs from the same shape in its batch"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_list_convolution_against_float64(ops, oracle_ops, case):
    variant, geo = query(case)
    assert variant == case.variant
    fig = Figures()
    for half in ("exact", "normal") + (FAMILIES[1:] if case.id in SMALL else ()):
        if case.form == "second":
            run_second(ops, case, geo, half, fig)
        else:
            run_first(ops, oracle_ops, case, geo, half, fig)
    fig.done()


@pytest.mark.gpu
def test_an_empty_batch_returns_and_touches_nothing(ops):
    from bdm_amd import _lib as L
    lib = L.lib()
    y = torch.full((4096,), SENT, device=DEV)
    part = torch.full((64,), SENT, dtype=torch.float64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    some = torch.zeros(4096, device=DEV)
    ints = torch.zeros(4096, dtype=torch.int32, device=DEV)
    slices = ctypes.c_int(-1)
    p = L.ptr
    assert lib.bdm_sparse_conv_dil(0, 8, 8, 8, 16, 512, p(some), p(some), p(ints), p(ints), p(ints), p(ints), p(some), p(some), p(some), p(y), 1, 0,
                                   p(counter), L.stream()) == 0
    assert lib.bdm_sparse_conv_dil_gn(0, 8, 8, 8, 16, 512, p(some), p(some), p(ints), p(ints), p(ints), p(ints), p(some), p(some), p(some), p(y), 1, 2,
                                      p(part), ctypes.byref(slices), 0, p(counter), L.stream()) == 0
    assert lib.bdm_sparse_conv_dil_h2_gn(0, 8, 8, 8, 512, 512, p(some), p(some), L.c_float(1.0), p(ints), p(ints), p(ints), p(ints), p(some), p(some),
                                         p(some), p(y), 2, p(part), ctypes.byref(slices), 0, p(counter), L.stream()) == 0
    assert lib.bdm_voxel_dilate_again(0, 8, 512, p(ints), p(ints), p(ints), p(ints), p(ints), p(ints), 0, L.stream()) == 0
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((part == SENT).all()) and int(counter) == 0 and not bool(ints.any())


# ---- (4) the operand producer on rows -------------------------------------------------------------------------------------------------
PRODUCER = [(32, 8, 8, "faces"), (35, 7, 8, "one_per_cell"), (100, 25, 16, "many_per_cell"), (256, 8, 8, "slab")]
SENT16 = -777.0          # exact in fp16


def first_conv_field(cloud, B, C, r, seed, lists):
    """A first convolution's output as the producer sees it: values at the voxels of the once-dilated list, the bias everywhere else"""
    x0 = channel_data((B, C, r ** 3), 1.3, seed)
    bias = torch.randn(C, generator=torch.Generator().manual_seed(seed + 1))
    grid = bias[None, :, None].expand(B, C, r ** 3).clone()
    for b, lst in enumerate(lists):
        v = torch.from_numpy(lst.astype(np.int64))
        grid[b][:, v] = x0[b][:, v]
    return grid, bias


def unpack_rows(rows):
    """(B, C8, 2, n, 8) fp16 -> hi, lo (B, 8 C8, n) float64"""
    B, c8, _, n, _ = rows.shape
    t = rows.cpu().double().permute(2, 0, 1, 4, 3).reshape(2, B, c8 * 8, n)
    return t[0], t[1]


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1], ids=["plain", "swish"])
@pytest.mark.parametrize("C,G,r,cloud", PRODUCER, ids=[f"c{c}_g{g}_r{r}_{cl}" for c, g, r, cl in PRODUCER])
def test_operand_producer_on_rows_against_float64(ops, C, G, r, cloud, act):
    from bdm_amd import _lib as L
    lib = L.lib()
    B, S, c8 = 2, 5, cdiv(C, 8)
    seed = 7000 + 10 * C + r
    vc = batch_coords(cloud, B, r, seed)
    plan = build_plan(ops, vc.to(DEV), r)
    tb = read_tables(plan)
    nd = [live(tb.t1[b])[1] for b in range(B)]
    lists = [tb.d1_list[b, :nd[b]] for b in range(B)]
    grid, bias = first_conv_field(cloud, B, C, r, seed, lists)
    gamma, beta = affine(C, seed + 2)
    h, mag = gn64(grid.double(), grid.abs().double(), G, gamma, beta)
    plain = TF.group_norm(grid, G, gamma, beta, EPS)
    ref, plain = (swish(h), swish(plain)) if act else (h, plain)
    partial = uneven_partials(group_totals(grid.double(), G), S, seed + S).to(DEV)
    scale = pow2_below(16384.0 / float(ref.abs().max()))
    xc = torch.full((B, r ** 3, C), float("nan"))
    for b in range(B):
        xc[b, :nd[b]] = listed(grid[b], tb.d1_list[b], nd[b])
    srcs = {0: xc.to(DEV), 1: grid.to(DEV)}
    bd, gd, btd = bias.to(DEV), gamma.to(DEV), beta.to(DEV)

    def launch(dense_in, s):
        rows = torch.full((B, c8, 2, r ** 3, 8), SENT16, dtype=torch.float16, device=DEV)
        ch2 = torch.full((B, c8, 2, 8), SENT16, dtype=torch.float16, device=DEV)
        cf = torch.full((B, C), SENT, device=DEV)
        sat = torch.zeros(1, dtype=torch.int32, device=DEV)
        L.check(lib.bdm_group_norm_to_h2_rows(B, C, r ** 3, G, L.ptr(srcs[dense_in]), dense_in, r ** 3, L.ptr(plan.dil_list), L.ptr(plan.tile_start),
                                              plan.tile_start.shape[1], L.ptr(bd), L.ptr(gd), L.ptr(btd), L.c_float(EPS), act, L.c_float(s), L.ptr(rows),
                                              L.ptr(ch2), L.ptr(cf), L.ptr(partial), S, L.ptr(sat), L.stream()), "group_norm_to_h2_rows")
        return rows, ch2, cf, sat
    rows, ch2, cf, sat = twice(lambda: launch(0, scale))
    rows_d, ch2_d, cf_d, sat_d = twice(lambda: launch(1, scale))
    assert int(sat) == 0 and int(sat_d) == 0, "the saturation word is raised by a scale that does not saturate"
    assert torch.equal(ch2.view(torch.int16), ch2_d.view(torch.int16)) and torch.equal(cf, cf_d), "compact and dense input give other constants"
    # the operator gives the same records (its own scale is another power of two: compare through ours)
    hi, lo = unpack_rows(rows)
    chi, clo = (t[..., 0] for t in unpack_rows(ch2.unsqueeze(3)))
    got, cgot = (hi + lo) / scale, (chi + clo) / scale
    assert torch.equal(cgot[:, :C].float(), cf.cpu()) and torch.equal(cgot[:, :C].float().double(), cgot[:, :C]), "const_f32 is not (hi + lo) / scale"
    if C % 8:
        assert all(float(hi[b, C:, :nd[b]].abs().max()) == 0.0 and float(lo[b, C:, :nd[b]].abs().max()) == 0.0 for b in range(B)), "pad channels of the rows"
        assert float(chi[:, C:].abs().max()) == 0.0 and float(clo[:, C:].abs().max()) == 0.0, "pad channels of the constant record"
    fig = Figures()
    for b in range(B):
        assert torch.equal(rows[b, :, :, :nd[b]].view(torch.int16), rows_d[b, :, :, :nd[b]].view(torch.int16)), "compact and dense input give other rows"
        assert bool((rows[b, :, :, nd[b]:] == SENT16).all()) and bool((rows_d[b, :, :, nd[b]:] == SENT16).all()), "rows beyond the list length were written"
        v = torch.from_numpy(lists[b].astype(np.int64))
        outside = int(np.flatnonzero(tb.d1_index[b] < 0)[0])
        r64 = torch.cat([ref[b][:, v], ref[b][:, outside:outside + 1]], 1)
        m64 = torch.cat([mag[b][:, v], mag[b][:, outside:outside + 1]], 1)
        p32 = torch.cat([plain[b][:, v], plain[b][:, outside:outside + 1]], 1).double()
        g64 = torch.cat([got[b, :C, :nd[b]], cgot[b, :C, None]], 1)
        yard = float(((p32 - r64).abs() / (U * m64)).max())
        allowed = 4.0 * max(yard, 1.0) * U * m64 + 2 * U * r64.abs() + 2.0 ** -25 / scale
        fig.fraction("rows and constant", float(((g64 - r64).abs() / allowed).max()), f"shape {b}, fp32 PyTorch {yard:.3g} u mag")
    fig.done()
    # a scale that saturates raises the word
    big = scale * 2.0 ** 8
    assert float(ref.abs().max()) * big > 65504.0
    for dense_in in (0, 1):
        assert int(launch(dense_in, big)[3]) == 1, "the saturation word stays clear under a scale that saturates"


# ---- (5) the consumers on rows -----------------------------------------------------------------------------------------------------------
CONSUMERS = [(32, 8, 16), (100, 25, 8), (256, 8, 8)]
CONSUMER_CLOUDS = ("single", "full", "faces", "one_per_cell")
PF_GROUPS, PF_POINTS = 4, 37


def points_in_occupied_cells(tb, B, r, n, seed):
    """(B, 3, n) float32 coordinates in [0, r - 1], every point inside an occupied cell (its eight corners then lie in the once-dilated
    list): offsets uniform in the cell, and every fourth point exactly on the cell centre, on a cell boundary (+- 1/2) on one axis or
    on all three; cells next to the grid faces are clamped onto the grid."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B, 3, n)
    for b in range(B):
        occ = torch.from_numpy(np.flatnonzero(tb.cnt[b] > 0))
        cell = occ[torch.randint(0, len(occ), (n,), generator=g)]
        c = torch.stack([cell // (r * r), (cell // r) % r, cell % r]).float()
        off = torch.rand(3, n, generator=g) - 0.5
        off[:, 0::4] = 0.0
        off[0, 1::8] = 0.5
        off[:, 5::8] = -0.5
        out[b] = (c + off).clamp(0.0, float(r - 1))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", CONSUMER_CLOUDS)
@pytest.mark.parametrize("C,G,r", CONSUMERS, ids=[f"c{c}_g{g}_r{r}" for c, g, r in CONSUMERS])
def test_consumers_on_rows_against_float64(ops, C, G, r, cloud):
    from bdm_amd import _lib as L
    lib = L.lib()
    B, S, PS, hidden, n = 2, 5, 3, max(C // 8, 1), 150
    seed = 9000 + 10 * C + CONSUMER_CLOUDS.index(cloud)
    vc = batch_coords(cloud, B, r, seed)
    plan = build_plan(ops, vc.to(DEV), r)
    tb = read_tables(plan)
    nd = [live(tb.t2[b])[1] for b in range(B)]
    cls = torch.from_numpy(voxel_class(r))
    # the second convolution's output: rows at D2's voxels, the value of its boundary class everywhere else
    x0 = channel_data((B, C, r ** 3), 1.3, seed)
    cvals = channel_data((B, C, 27), 1.3, seed + 1)
    grid = cvals[:, :, cls].clone()
    rows = torch.full((B, r ** 3, C), float("nan"))
    for b in range(B):
        v = torch.from_numpy(tb.d2_list[b, :nd[b]].astype(np.int64))
        grid[b][:, v] = x0[b][:, v]
        rows[b, :nd[b]] = x0[b][:, v].t()
    rows_d, cv_d = rows.to(DEV), cvals.permute(0, 2, 1).contiguous().to(DEV)
    gamma, beta = affine(C, seed + 2)
    pgamma, pbeta = affine(C, seed + 3)
    gn, pgn = gn_module(G, gamma, beta), gn_module(PF_GROUPS, pgamma, pbeta)
    w1, w2 = se_weights(C, hidden, seed + 4)
    w1d, w2d = w1.to(DEV), w2.to(DEV)
    p0 = channel_data((B, C, PF_POINTS), 1.3, seed + 5)
    stats = (uneven_partials(group_totals(grid.double(), G), S, seed + S).to(DEV), S)
    pf = ((uneven_partials(group_totals(p0.double(), PF_GROUPS), PS, seed + 50).to(DEV), PS, PF_GROUPS), pgn)
    h, mag = gn64(grid.double(), grid.abs().double(), G, gamma, beta)
    mean64, mmag = swish(h).mean(-1), mag.mean(-1)
    mean32 = swish(TF.group_norm(grid, G, gamma, beta, EPS)).mean(-1)
    gate64, gmag = se_gate64(mean64, w1, w2)
    gate32, _ = se_gate64(mean32, w1, w2)
    coef64, cmag = coef_ref(grid.double(), G, gamma, beta)
    coef32, _ = coef_ref(grid, G, gamma, beta)
    pcoef64, pmag = coef_ref(p0.double(), PF_GROUPS, pgamma, pbeta)
    pcoef32, _ = coef_ref(p0, PF_GROUPS, pgamma, pbeta)
    fig = YardstickFigures()

    def se_launch(with_pf):
        """bdm_se_gate_gn_rows(_pf) as ops.se_gate_gn_rows launches it, keeping the channel means"""
        mean = torch.full((B, C), SENT, device=DEV)
        coef = torch.full((B, C, 2), SENT, device=DEV)
        gate = torch.full((B, C), SENT, device=DEV)
        part = torch.empty(lib.bdm_se_gate_gn_rows_workspace_elems(B, C), device=DEV)
        args = (B, C, hidden, r ** 3, G, L.ptr(rows_d), r ** 3, L.ptr(plan.d2_tiles), plan.d2_tiles.shape[1], L.ptr(cv_d), L.ptr(plan.d2_class_count),
                L.ptr(stats[0]), S, L.ptr(gn.weight), L.ptr(gn.bias), L.c_float(EPS), L.ptr(w1d), L.ptr(w2d), L.ptr(part), L.ptr(mean), L.ptr(coef),
                L.ptr(gate))
        if not with_pf:
            L.check(lib.bdm_se_gate_gn_rows(*args, L.stream()), "se_gate_gn_rows")
            return mean, coef, gate
        pcoef = torch.full((B, C, 2), SENT, device=DEV)
        L.check(lib.bdm_se_gate_gn_rows_pf(*args, L.ptr(pf[0][0]), PS, PF_GROUPS, PF_POINTS, L.ptr(pgn.weight), L.ptr(pgn.bias), L.c_float(EPS),
                                           L.ptr(pcoef), L.stream()), "se_gate_gn_rows_pf")
        return mean, coef, gate, pcoef
    mean, coef, gate = twice(lambda: se_launch(False))
    mean_p, coef_p, gate_p, pcoef = twice(lambda: se_launch(True))
    assert torch.equal(mean_p, mean) and torch.equal(coef_p, coef) and torch.equal(gate_p, gate), "the point branch changes the grid's results"
    gate_o, coef_o, pcoef_o = ops.se_gate_gn_rows(rows_d, cv_d, plan, stats, gn, w1d, w2d, pf=pf, n_points=PF_POINTS)
    assert torch.equal(gate_o, gate) and torch.equal(coef_o, coef) and torch.equal(pcoef_o, pcoef), "ops.se_gate_gn_rows gives other results"
    what = f"{cloud}, class counts {int(tb.class_count.min())} .. {int(tb.class_count.max())}"
    fig.check("mean", mean, mean64, U * mmag, mean32, what)
    fig.check("coef", coef, coef64, U * cmag, coef32, what)
    fig.check("gate", gate, gate64, U * gmag, gate32, what)
    fig.check("pf_coef", pcoef, pcoef64, U * pmag, pcoef32, what)
    # devoxelisation: the points of a cloud sit in occupied cells
    g = torch.Generator().manual_seed(seed + 6)
    coords = points_in_occupied_cells(tb, B, r, n, seed + 7)
    ab = torch.stack([0.4 * torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)], -1)
    add_ab = torch.stack([0.4 * torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)], -1)
    gt = 0.05 + 0.9 * torch.rand(B, C, generator=g)
    add = channel_data((B, C, n), 1.3, seed + 8)
    cd, abd, aabd, gtd, addd = (t.to(DEV) for t in (coords, ab, add_ab, gt, add))
    wide = torch.full((B, C + 5, n), SENT, device=DEV)
    adds = wide[:, 3:3 + C]
    adds.copy_(addd)
    variants = [("no gate, no add", None, None, None), ("gate + add", gtd, addd, None), ("gate + add as a channel slice", gtd, adds, None),
                ("gate + Swish(GroupNorm(add))", gtd, addd, aabd), ("no gate, Swish(GroupNorm(add)) as a channel slice", None, adds, aabd)]
    for name, gg, ad, aab in variants:
        (got,) = twice(lambda: (ops.devoxelize_gn_gate_add_rows(cd, rows_d, cv_d, plan, abd, gate=gg, add=ad, add_coef=aab),))
        args = (coords, r, grid, ab, gt if gg is not None else None, add if ad is not None else None, add_ab if aab is not None else None)
        ref, dmag = devox_expected(torch.float64, *args)
        fig.check("devox_rows", got, ref, U * dmag, devox_expected(torch.float32, *args)[0], f"{cloud}, {name}")
    assert torch.equal(adds, addd), "the addend was changed"
    fig.done()
