"""Live per-kernel-class timing of the C-ABI launches (bench.py's roofline table).

Every kernel of the path is launched through `_lib.lib().<bdm_function>(...)`.  While a `KernelClassProfiler` is
installed the library handle is a thin proxy: every `every`-th call of each (function, shape signature) is bracketed by
two HIP events recorded on the stream the launch goes to (torch's current stream at that moment -- the main stream or one
of the side streams), so durations are measured on the device, inside the timed region, without synchronising anything.
The algorithmic work of a call (FLOPs for the matrix-core kernels, bytes for the streaming kernels) is computed from its
arguments with the per-unit formulas of SURVEY.md 8(d) / DESIGN.md section 4, so that each class gets

    share  = its part of the summed kernel time (sampled durations scaled by calls / samples)
    frac   = achieved algorithmic rate / the peak that bounds it (dense 16-bit MFMA peak / products per fp32 product for
             the split-precision convolutions and GEMMs, fp32 MFMA peak for fp32-input MFMA, HBM peak for streaming kernels)

Several kernels may sit behind one ABI function (template instantiations chosen by shape); rows are therefore keyed by
(function, shape signature) and then folded into classes.  Timing a launch with events costs two marker packets on its
queue; with every = 8 that is ~70 of ~2400 packets per reverse step.
"""
import collections

import torch

from . import _lib as L

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E ~8 TB/s
MFMA16_PEAK_TFLOPS = 2500.0      # dense fp16 / bf16 MFMA
MFMA32_PEAK_TFLOPS = 157.3       # fp32-input MFMA
VALU_TESTS_PEAK = 1024 * 64 * 2.4e9 / 4 / 6.7 / 1e9   # ball-query distance tests per ns the VALUs can issue (= 5868 G tests/s)
OCCUPANCY = {}                   # n_max -> mean occupied fraction of the sparse convolution's rows (set by bench.py)
DILATED = {}                     # r -> (once-dilated, twice-dilated) fraction of the r^3 voxels on the run's clouds (set by bench.py)


def _list_conv(a, which, products=3):
    """Cost of a LIST convolution (sparse_conv_os.hip): the matrix work it ISSUES = every (listed voxel, tap) pair of the once- (first
    convolution) or twice-dilated (second) list -- tap quads skipped inside a wave are not subtracted, so this is an upper bound of the
    issued work; the MFMA-busy counters of profiles/r0N_mfma_busy.txt are the cross-check -- against the fp16x3 peak, and next to it the
    dense-grid ALGORITHMIC flops of the operator (what a dense kernel would have to compute: not what this kernel is priced by)."""
    b, cin, cout, r = a[0], a[1], a[2], a[3]
    dense = 2.0 * 27 * cin * cout * r ** 3 * b
    frac = DILATED.get(int(r), (1.0, 1.0))[which]
    return ("mfma_list", dense * frac, MFMA16_PEAK_TFLOPS / products, dense)


def _f(flops, products):
    return ("mfma", flops, MFMA16_PEAK_TFLOPS / products)


# name -> (class, signature(args) , cost(args) -> ("mfma", flops, peak_tflops) | ("hbm", bytes) | None)
def _conv_h2(a):
    b, cin, cout, r = a[0], a[1], a[2], a[3]
    return _f(2.0 * 27 * cin * cout * r ** 3 * b, 3)


def _conv_s3(a):
    b, cin, cout, r = a[0], a[1], a[2], a[3]
    return _f(2.0 * 27 * cin * cout * r ** 3 * b, 6)


def _conv_f32(a):
    b, cin, cout, r = a[0], a[1], a[2], a[3]
    return ("mfma", 2.0 * 27 * cin * cout * r ** 3 * b, MFMA32_PEAK_TFLOPS)


def _pw(a):
    b, m, k, n = a[0], a[1], a[2], a[3]
    return ("mfma", 2.0 * b * m * k * n, MFMA32_PEAK_TFLOPS)


def _pw_s3(a):
    b, m, k, n = a[0], a[1], a[2], a[3]
    return ("mfma", 2.0 * b * m * k * n, MFMA16_PEAK_TFLOPS / 6)


def _attn(a):
    b, c, l = a[0], a[1], a[2]
    return _f(4.0 * b * c * l * l, 6) if l > 64 else ("hbm", 4.0 * 4 * b * c * l)


SPEC = {
    # dense 3x3x3 voxel convolutions
    "bdm_conv3d_3x3x3_h2": ("dense conv3d (fp16x3)", lambda a: a[:4], _conv_h2),
    "bdm_conv3d_3x3x3_h2_gn": ("dense conv3d (fp16x3)", lambda a: a[:4], _conv_h2),  # + GroupNorm partial sums in the epilogue
    "bdm_conv3d_3x3x3_s3": ("dense conv3d (bf16x6)", lambda a: a[:4], _conv_s3),
    "bdm_conv3d_3x3x3": ("dense conv3d (fp32 MFMA)", lambda a: a[:4], _conv_f32),
    "bdm_conv3d_3x3x3_sparse": ("dense conv3d (fp32 MFMA)", lambda a: a[:4], _conv_f32),
    # sparse first convolution of a PVConv (features -> GEMM -> gather).  Algorithmic work of the class = what the operator
    # has to move: read the point features once (features kernel), write the dense output grid once (gather); the GEMM's
    # intermediate is NOT algorithmic work, so the class's HBM fraction shows what that intermediate costs.  The GEMM row
    # also carries its matrix work: 2 * n_occ * cin * 27*cout with n_occ = OCCUPANCY[n_max] * n_max (measured by bench.py
    # on the final clouds after the timed region; 1.0 = upper bound when not set).
    "bdm_sparse_conv_gemm_s3": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                                lambda a: ("mfma_aux", 2.0 * a[0] * a[1] * OCCUPANCY.get(a[1], 1.0) * a[2] * a[3], MFMA16_PEAK_TFLOPS / 6)),
    "bdm_sparse_conv_gemm_h2": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                                lambda a: ("mfma_aux", 2.0 * a[0] * a[1] * OCCUPANCY.get(a[1], 1.0) * a[2] * 27 * a[3], MFMA16_PEAK_TFLOPS / 3)),
    # (+ the per-shape column addend: the time embedding's share, modules.PVConv.can_split_temb)
    "bdm_sparse_conv_gemm_s3_cb": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                                   lambda a: ("mfma_aux", 2.0 * a[0] * a[1] * OCCUPANCY.get(a[1], 1.0) * a[2] * a[3], MFMA16_PEAK_TFLOPS / 6)),
    "bdm_sparse_conv_gemm_h2_cb": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                                   lambda a: ("mfma_aux", 2.0 * a[0] * a[1] * OCCUPANCY.get(a[1], 1.0) * a[2] * 27 * a[3], MFMA16_PEAK_TFLOPS / 3)),
    "bdm_sparse_split_h2": ("sparse first conv", lambda a: (a[0], a[1], a[2]), lambda a: ("hbm", 0.0)),
    "bdm_sparse_conv_gemm": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                             lambda a: ("mfma_aux", 2.0 * a[0] * a[1] * OCCUPANCY.get(a[1], 1.0) * a[2] * a[3], MFMA32_PEAK_TFLOPS)),
    "bdm_sparse_conv_gather": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2] ** 3)),
    "bdm_sparse_conv_gather_gn": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2] ** 3)),
    # round 4: the same convolution as ONE output-stationary implicit GEMM with tap skipping (sparse_conv_os.hip): algorithmic bytes =
    # the dense output grid written once; its matrix work (live fragments only) rides along as mfma_aux
    "bdm_sparse_conv_os": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[2] * a[3] ** 3)),
    "bdm_sparse_conv_os_gn": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[2] * a[3] ** 3)),
    "bdm_sparse_conv_dil": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                            lambda a: ("hbm+list", 4.0 * a[0] * a[2] * a[3] ** 3) + _list_conv(a, 0)[1:]),
    "bdm_sparse_conv_dil_gn": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]),
                               lambda a: ("hbm+list", 4.0 * a[0] * a[2] * a[3] ** 3) + _list_conv(a, 0)[1:]),
    "bdm_voxel_dilate": ("voxelize / devoxelize", lambda a: a[:2], lambda a: ("hbm", 4.0 * a[0] * 2 * a[1] ** 3)),
    "bdm_voxel_dilate_again": ("voxelize / devoxelize", lambda a: a[:2], lambda a: ("hbm", 4.0 * a[0] * 2 * a[1] ** 3)),
    # second convolution on the twice-dilated list: priced by the matrix work it ISSUES (listed voxels x 27 taps, _list_conv); the
    # dense-grid flops of the operator (2 * 27 * cin * cout * r^3 per shape) are carried separately as `algorithmic_tflops` (VERDICT r4
    # weak 4: priced by dense flops the row read 0.79 of the ceiling against an MFMA-busy counter of 43 %)
    "bdm_sparse_conv_dil_h2_gn": ("dense conv3d (fp16x3)", lambda a: a[:4], lambda a: _list_conv(a, 1)),
    "bdm_conv3d_class_constants": ("dense conv3d (fp16x3)", lambda a: a[:3], lambda a: ("mfma", 0.0, MFMA16_PEAK_TFLOPS / 3)),
    "bdm_group_norm_to_h2_rows": ("GroupNorm(+Swish)", lambda a: a[:4], lambda a: ("hbm", (4.0 + 4.0) * a[0] * a[1] * a[2])),
    "bdm_se_gate_gn_rows": ("SE gate", lambda a: (a[0], a[1], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[3])),
    "bdm_se_gate_gn_rows_pf": ("SE gate", lambda a: (a[0], a[1], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[3])),
    "bdm_devoxelize_gn_gate_add_rows": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    "bdm_devoxelize_gn_gate_add_rows_pf": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    # hoisted conditioning (ops.Conditioning): rows of the occupied cells from the per-pixel map; algorithmic = the map rows of the points
    "bdm_sparse_conv_rows_from_map": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[4]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[4])),
    "bdm_sparse_voxel_features_s3": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2])),
    "bdm_sparse_voxel_features": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2])),
    "bdm_sparse_voxel_features_f32": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2])),
    "bdm_sparse_conv_fused": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[2] * a[3] ** 3)),
    # 1x1 convolutions / linear layers
    "bdm_pointwise_conv": ("1x1 conv GEMM (fp32 MFMA)", lambda a: a[:4], _pw),
    "bdm_pointwise_conv_gn": ("1x1 conv GEMM (fp32 MFMA)", lambda a: a[:4], _pw),  # + GroupNorm statistics / folded input GroupNorm
    "bdm_pointwise_conv_gn_bb": ("1x1 conv GEMM (fp32 MFMA)", lambda a: a[:4], _pw),   # + per-shape bias (the time embedding's share)
    "bdm_pointwise_conv_gn_add": ("1x1 conv GEMM (fp32 MFMA)", lambda a: a[:4], _pw),  # + per-element addend (hoisted conditioning share)
    "bdm_pointwise_conv_s3": ("1x1 conv GEMM (bf16x6)", lambda a: a[:4], _pw_s3),
    "bdm_pointwise_conv_gn_s3": ("1x1 conv GEMM (bf16x6)", lambda a: a[:4], _pw_s3),
    # normalisation and operand repacks: 1 read + 1 write of the tensor
    "bdm_group_norm": ("GroupNorm(+Swish)", lambda a: a[:4], lambda a: ("hbm", 8.0 * a[0] * a[1] * a[2])),
    "bdm_group_norm_to_h2": ("GroupNorm(+Swish)", lambda a: a[:4], lambda a: ("hbm", (4.0 + 4.0 + 4.0) * a[0] * a[1] * a[2])),
    "bdm_group_norm_to_h2_stats": ("GroupNorm(+Swish)", lambda a: a[:4], lambda a: ("hbm", (4.0 + 4.0) * a[0] * a[1] * a[2])),
    "bdm_group_norm_to_s3": ("GroupNorm(+Swish)", lambda a: a[:4], lambda a: ("hbm", (4.0 + 4.0 + 6.0) * a[0] * a[1] * a[2])),
    "bdm_attention_core": ("attention", lambda a: a[:3], _attn),
    "bdm_attention_core_h2": ("attention", lambda a: a[:3], lambda a: _f(4.0 * a[0] * a[1] * a[2] * a[2], 3)),
    # point operators (SURVEY.md 8d byte formulas)
    "bdm_furthest_point_sampling": ("furthest point sampling", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * (3 * a[1] + 4 * a[2]))),
    "bdm_gather_features_forward": ("furthest point sampling", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (2 * a[1] * a[3] + a[3]))),
    # the query is bound by VALU issue, not by its 3 MB of traffic: b * m * n distance tests at 6.7 VALU instructions per test per
    # lane (ISA count of ball_query_kernel<4,8>: DESIGN.md); the chip issues 1024 SIMDs x 64 lanes x 2.4 GHz / 4 cycles
    "bdm_ball_query": ("ball query (distance tests)", lambda a: (a[0], a[1], a[2], a[4]),
                       lambda a: ("valu", 1.0 * a[0] * a[1] * a[2], VALU_TESTS_PEAK, "G tests/s")),
    "bdm_sa_group": ("grouping gather + max over neighbours", lambda a: a[:5],
                     lambda a: ("hbm", 4.0 * a[0] * ((3 + a[1]) * a[2] + a[3] * a[4] + (a[1] + 3) * a[3] * a[4]))),
    # fused first set-abstraction MLP: algorithmic flops = the two layers ONCE (the three passes recompute: 3x layer 1, 2x layer 2);
    # algorithmic bytes would be the features + indices + output only, so the class is priced as a GEMM
    "bdm_sa_mlp2_fused": ("1x1 conv GEMM (fp32 MFMA)", lambda a: a[:7],
                          lambda a: ("mfma", 2.0 * a[0] * a[3] * a[4] * ((3 + a[1]) * a[5] + a[5] * a[6]), MFMA32_PEAK_TFLOPS)),
    "bdm_grouping_forward": ("grouping gather + max over neighbours", lambda a: a[:5],
                             lambda a: ("hbm", 4.0 * a[0] * (a[1] * a[2] + a[3] * a[4] + a[1] * a[3] * a[4]))),
    "bdm_max_over_neighbors": ("grouping gather + max over neighbours", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2] * (a[3] + 1))),
    "bdm_max_over_neighbors_gn": ("grouping gather + max over neighbours", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2] * (a[3] + 1))),
    "bdm_three_nn_search": ("3-NN interpolation", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 3 * a[1] + 6 * a[2]))),
    "bdm_three_nn_apply": ("3-NN interpolation", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (a[1] * a[2] + a[1] * a[3] + 6 * a[3]))),
    "bdm_fp_assemble": ("3-NN interpolation", lambda a: (a[0], a[1], a[2], a[5], a[9], a[13]),
                        lambda a: ("hbm", 4.0 * a[0] * ((a[5] + a[13]) * (a[1] + a[2]) + 2 * a[9] * a[2] + 6 * a[2]))),
    "bdm_voxelize_plan_full": ("voxelize / devoxelize", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * (4 * a[1] + 3 * a[2] ** 3))),
    "bdm_voxel_coords": ("voxelize / devoxelize", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * 9 * a[1])),
    "bdm_devoxelize_gate_add": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    # GroupNorm-folded tail of a PVConv: the row means read the conv output once; the devoxelisation reads coords and the
    # grid's 8 corners per point-channel and reads the point branch / writes the sum
    "bdm_se_gate_gn": ("SE gate", lambda a: (a[0], a[1], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[3])),
    "bdm_devoxelize_gn_gate_add": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    "bdm_se_gate_gn_pf": ("SE gate", lambda a: (a[0], a[1], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[3])),
    "bdm_devoxelize_gn_gate_add_pf": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    "bdm_devoxelize_gn_se_add": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + 10 * a[1] * a[2]))),
    "bdm_pvconv_tail_small": ("voxelize / devoxelize", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * (3 * a[2] + a[1] * a[3] ** 3 + 2 * a[1] * a[2]))),
    "bdm_sparse_conv_gather_h2_small": ("sparse first conv", lambda a: (a[0], a[1], a[2], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2] ** 3)),
    "bdm_lincomb": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 4.0 * a[0] * (a[1] + 1))),
    "bdm_se_gate": ("SE gate", lambda a: (a[0], a[1], a[3]), lambda a: ("hbm", 4.0 * a[0] * a[1] * a[3])),
    "bdm_copy_rows": ("concat / broadcast / transpose copies", lambda a: a[:3], lambda a: ("hbm", 8.0 * a[0] * a[1] * a[2])),
    "bdm_concat2_rows": ("concat / broadcast / transpose copies", lambda a: (a[0], a[1], a[2], a[6]), lambda a: ("hbm", 4.0 * a[0] * a[1] * (2 * a[2] + a[6]))),
    "bdm_broadcast_rows": ("concat / broadcast / transpose copies", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * a[1] * a[2])),
    "bdm_transpose": ("concat / broadcast / transpose copies", lambda a: a[:3], lambda a: ("hbm", 8.0 * a[0] * a[1] * a[2])),
    "bdm_rasterize_points": ("projection conditioning", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * 4 * a[1])),
    "bdm_condition_gather_cf": ("projection conditioning", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * a[1] * (2 * a[2] + 7))),
    "bdm_condition_xyz_cf": ("projection conditioning", lambda a: a[:3], lambda a: ("hbm", 4.0 * a[0] * a[1] * 6)),
    "bdm_condition_gather": ("projection conditioning", lambda a: a[:4], lambda a: ("hbm", 4.0 * a[0] * a[1] * (2 * a[2] + 7))),
    "bdm_ddpm_step": ("scheduler step / blend", lambda a: a[:1], lambda a: ("hbm", 16.0 * a[0])),
    "bdm_ddpm_step_philox": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 12.0 * a[0] * a[1])),
    "bdm_pvd_step": ("scheduler step / blend", lambda a: a[:1], lambda a: ("hbm", 16.0 * a[0])),
    "bdm_pvd_step_philox": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 12.0 * a[0] * a[1])),
    "bdm_blend_select": ("scheduler step / blend", lambda a: a[:1], lambda a: ("hbm", (36.0 + 8.0) * a[0])),
    "bdm_center_points": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 24.0 * a[0] * a[1])),
    "bdm_philox_normal": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 4.0 * a[0] * a[1])),
    "bdm_philox_bits": ("scheduler step / blend", lambda a: a[:2], lambda a: ("hbm", 8.0 * a[0] * a[1])),
    "bdm_time_embedding": ("time embedding", lambda a: a[:2], None),
}


PROBE_WEIGHT = [1]  # launches one profiled launch stands for (the tape loops profile every k-th step only: replay.run_step)


def _plain(v):
    return v.value if hasattr(v, "value") else v


class _Proxy:
    def __init__(self, handle, prof):
        self.__dict__["_h"], self.__dict__["_p"] = handle, prof

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        host_only = (not name.startswith("bdm_") or name.endswith("_bytes") or name.endswith("_elems") or name.endswith("_slices") or name.endswith("_variant")
                     or name in ("bdm_last_error", "bdm_abi_version") or name.startswith("bdm_tape_"))
        if host_only:
            return fn
        spec = SPEC.get(name, ("other", lambda a: (), None))
        prof = self._p

        def call(*args):
            if not prof.enabled or torch.cuda.is_current_stream_capturing():
                return fn(*args)
            try:
                sig = tuple(int(_plain(v)) for v in spec[1](args))
            except (TypeError, ValueError):
                sig = ()
            row = prof.rows[(name, sig)]
            row[0] += PROBE_WEIGHT[0]
            row[2] += 1
            if row[2] % prof.every:
                return fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            # the call's scalar arguments; its cost is computed from them in table(), AFTER the run (the occupancy / dilation
            # fractions the sparse and list kernels are priced with are measured on the run's final clouds)
            prof.pending.append((row, e0, e1, [_plain(v) for v in args[:16]] if spec[2] is not None else None))
            if len(prof.pending) >= 256:
                prof.drain(block=False)
            return rc
        self.__dict__[name] = call  # cache the wrapper
        return call


def row_fraction(row):
    """(bound, achieved, peak, unit, frac) of ONE (function, shape) row from its own cost and average duration; None when unpriced."""
    cost, us = row.get("cost"), row.get("avg_us")
    if cost is None or not us:
        return None
    if cost[0] in ("mfma", "mfma_list", "mfma_aux"):
        ach = cost[1] / (us * 1e-6) / 1e12
        return ("mfma", ach, cost[2], "TFLOP/s", ach / cost[2])
    if cost[0] == "valu":
        ach = cost[1] / (us * 1e-6) / 1e9
        return ("valu", ach, cost[2], cost[3], ach / cost[2])
    ach = cost[1] / (us * 1e-6) / 1e9
    return ("hbm", ach, HBM_PEAK_GBS, "GB/s", ach / HBM_PEAK_GBS)


class KernelClassProfiler:
    def __init__(self, every=8):
        self.every, self.enabled = int(every), False
        # (name, sig) -> [launches stood for, [sampled ms summed, samples, cost of one launch], calls seen]
        self.rows = collections.defaultdict(lambda: [0, [0.0, 0, None], 0])
        self.pending = collections.deque()  # (row, e0, e1, cost) of samples whose events may still be in flight
        self._saved = None

    def install(self):
        handle = L.lib()
        self._saved = handle
        L._lib = _Proxy(handle, self)
        self.enabled = True
        return self

    def remove(self):
        self.enabled = False
        if self._saved is not None:
            L._lib = self._saved
            self._saved = None

    def drain(self, block=True):
        """Fold finished samples into their rows and drop their events: thousands of LIVE HIP events slow every later stream
        operation of the process (measured: 2 x 10^4 of them cost the B = 1 loop 20 %), so they are kept only while in flight."""
        while self.pending and (block or self.pending[0][2].query()):
            row, e0, e1, cost = self.pending.popleft()
            if block:
                e1.synchronize()
            row[1][0] += e0.elapsed_time(e1)
            row[1][1] += 1
            row[1][2] = cost if row[1][2] is None else row[1][2]

    def table(self):
        """(rows, classes): rows = per (function, shape) dicts, classes = per kernel class dicts sorted by time share."""
        rows = []
        self.drain(block=True)
        for (name, sig), (calls, (ms, n, cargs), _) in self.rows.items():
            if not n:
                continue
            cost = None
            if cargs is not None:
                try:
                    cost = SPEC[name][2](cargs)
                except (TypeError, ValueError, IndexError, KeyError):
                    cost = None
            avg_us = 1e3 * ms / n
            rows.append({"function": name, "shape": list(sig), "class": SPEC.get(name, ("other",))[0], "calls": calls,
                         "sampled": n, "avg_us": avg_us, "est_total_ms": avg_us * calls / 1e3, "cost": cost})
        total = sum(r["est_total_ms"] for r in rows) or 1.0
        classes = {}
        for r in rows:
            c = classes.setdefault(r["class"], {"class": r["class"], "est_total_ms": 0.0, "calls": 0, "flops": 0.0, "bytes": 0.0,
                                                "mfma_ms": 0.0, "hbm_ms": 0.0, "peak_tflops": None, "valu": 0.0, "valu_ms": 0.0,
                                                "valu_peak": None, "valu_unit": None, "alg_flops": 0.0, "aux_peak_ms": 0.0, "aux_ms": 0.0})
            c["est_total_ms"] += r["est_total_ms"]
            c["calls"] += r["calls"]
            if r["cost"] is not None:
                if r["cost"][0] == "valu":  # VALU-issue-bound kernels: work items and the chip's issue-rate peak for them
                    c["valu"] += r["cost"][1] * r["calls"]
                    c["valu_ms"] += r["est_total_ms"]
                    c["valu_peak"], c["valu_unit"] = r["cost"][2], r["cost"][3]
                elif r["cost"][0] == "mfma_aux":  # matrix work inside a class whose algorithmic measure is bytes
                    c["flops"] += r["cost"][1] * r["calls"]
                    c["hbm_ms"] += r["est_total_ms"]
                    c["aux_peak_ms"] += r["cost"][1] * r["calls"] / (r["cost"][2] * 1e12) * 1e3   # its time at ITS peak
                    c["aux_ms"] += r["est_total_ms"]
                elif r["cost"][0] == "hbm+list":  # list first convolution: algorithmic bytes + the matrix work it issues
                    c["bytes"] += r["cost"][1] * r["calls"]
                    c["flops"] += r["cost"][2] * r["calls"]
                    c["hbm_ms"] += r["est_total_ms"]
                    c["aux_peak_ms"] += r["cost"][2] * r["calls"] / (r["cost"][3] * 1e12) * 1e3
                    c["aux_ms"] += r["est_total_ms"]
                elif r["cost"][0] in ("mfma", "mfma_list"):
                    c["flops"] += r["cost"][1] * r["calls"]
                    c["alg_flops"] += (r["cost"][3] if r["cost"][0] == "mfma_list" else r["cost"][1]) * r["calls"]
                    c["mfma_ms"] += r["est_total_ms"]
                    c["peak_tflops"] = r["cost"][2] if c["peak_tflops"] is None else max(c["peak_tflops"], r["cost"][2])
                else:
                    c["bytes"] += r["cost"][1] * r["calls"]
                    c["hbm_ms"] += r["est_total_ms"]
        out = []
        for c in classes.values():
            d = {"class": c["class"], "share": c["est_total_ms"] / total, "kernel_ms": c["est_total_ms"], "launches": c["calls"]}
            if c["valu"] > 0 and c["valu_ms"] >= max(c["mfma_ms"], c["hbm_ms"]):
                ach = c["valu"] / (c["valu_ms"] * 1e-3) / 1e9
                d.update(bound="valu", achieved=ach, peak=c["valu_peak"], unit=c["valu_unit"], frac=ach / c["valu_peak"])
            elif c["flops"] > 0 and c["mfma_ms"] > 0 and c["mfma_ms"] >= c["hbm_ms"]:
                ach = c["flops"] / (c["mfma_ms"] * 1e-3) / 1e12
                d.update(bound="mfma", achieved=ach, peak=c["peak_tflops"], unit="TFLOP/s", frac=ach / c["peak_tflops"])
                if c["alg_flops"] != c["flops"]:   # list kernels inside: the operator's dense-grid flops over the same time, for reference
                    d["algorithmic_tflops"] = c["alg_flops"] / (c["mfma_ms"] * 1e-3) / 1e12
            elif c["bytes"] > 0 and c["hbm_ms"] > 0:
                ach = c["bytes"] / (c["hbm_ms"] * 1e-3) / 1e9
                d.update(bound="hbm", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS)
                if c["flops"] > 0:
                    d["matrix_tflops"] = c["flops"] / (c["hbm_ms"] * 1e-3) / 1e12
                if c["aux_ms"] > 0:   # the class's matrix kernels against the MFMA peak of their arithmetic (issued work, own time)
                    d["mfma_frac"] = c["aux_peak_ms"] / c["aux_ms"]
            else:
                d.update(bound=None, achieved=None, peak=None, unit=None, frac=None)
            out.append(d)
        out.sort(key=lambda d: -d["share"])
        for r in rows:
            r["share"] = r["est_total_ms"] / total
        rows.sort(key=lambda r: -r["est_total_ms"])
        return rows, out
