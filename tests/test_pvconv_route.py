"""PVConv.route is THE statement of which kernels a PVConv runs (bdm_amd/modules.py): the planners and the previous module's tail read it,
forward executes it.  (1) the route table of both denoisers at the benchmark's per-GPU shapes against a literal table written from launch
dumps of the code BEFORE route() existed; (2) the coherence that used to be kept by hand between forward and its mirrors; (3) on the GPU:
the kernels on a recorded forward's tape are the ones each module's route names."""
import itertools

import pytest
import torch
import torch.nn as nn

# ---- (1) literal table: (first, gemm_impl, tail, dilate, takes_rows) per PVConv, in module order ---------------------------------
# Read off the kernel names of one recorded forward per configuration (bdm_sparse_conv_rows_from_map = "map", bdm_sparse_conv_dil_gn =
# "dil", bdm_sparse_conv_gemm_h2[_cb] / _s3[_cb] = "gemm"; bdm_sparse_conv_dil_h2_gn + bdm_devoxelize_gn_gate_add_rows = "lists",
# bdm_pvconv_tail_small = "small", bdm_devoxelize_gn_gate_add[_pf] = "folded", bdm_devoxelize_gate_add = "plain"; takes_rows = no
# bdm_sparse_voxel_features_f32 before the fp16x3 GEMM) at the commit before this file existed.
ORDER = ["sa_layers.0.0", "sa_layers.0.1", "sa_layers.1.0", "sa_layers.2.0", "fp_layers.0.1", "fp_layers.0.2", "fp_layers.0.3",
         "fp_layers.1.1", "fp_layers.1.2", "fp_layers.1.3", "fp_layers.2.1", "fp_layers.2.2", "fp_layers.3.1", "fp_layers.3.2"]
S3_FOLDED, S3_PLAIN = ("gemm", "sparse_s3", "folded", 0, False), ("gemm", "sparse_s3", "plain", 0, False)
H2_FOLDED, H2_SMALL = ("gemm", "sparse_h2", "folded", 0, False), ("gemm", "sparse_h2", "small", 0, False)
H2_SMALL_ROWS, H2_FOLDED_ROWS = ("gemm", "sparse_h2", "small", 0, True), ("gemm", "sparse_h2", "folded", 0, True)
DIL_LISTS, DIL_FOLDED, DIL_PLAIN = ("dil", None, "lists", 2, False), ("dil", None, "folded", 1, False), ("dil", None, "plain", 1, False)
MAP_FOLDED, MAP_LISTS = ("map", None, "folded", 0, False), ("map", None, "lists", 2, False)
SMALL_STAGES = [H2_FOLDED, H2_SMALL, H2_SMALL_ROWS, H2_FOLDED_ROWS, H2_SMALL, H2_SMALL_ROWS, H2_FOLDED_ROWS]   # sa2.0, fp0.1-3, fp1.1-3 (8^3)
CONFIGS = {"c1": (1, 1024), "c2": (16, 4096), "c3": (16, 4096), "c4": (8, 8192), "c5": (32, 16384)}   # bench.py: shapes per GPU, points
TABLE = {   # config -> rows after sa_layers.0.0 (whose first convolution is "map" in the PC^2 denoiser and the row's own form in PVD's)
    "c1": [S3_FOLDED, S3_FOLDED, S3_PLAIN] + SMALL_STAGES + [H2_FOLDED, H2_FOLDED, S3_FOLDED, S3_FOLDED],
    "c2": [DIL_LISTS, DIL_LISTS, S3_PLAIN] + SMALL_STAGES + [DIL_FOLDED, DIL_FOLDED, DIL_LISTS, DIL_LISTS],
    "c4": [DIL_LISTS, DIL_LISTS, S3_PLAIN] + SMALL_STAGES + [H2_FOLDED, H2_FOLDED, DIL_LISTS, DIL_LISTS],
    "c5": [DIL_LISTS, DIL_LISTS, DIL_PLAIN] + SMALL_STAGES + [DIL_FOLDED, DIL_FOLDED, DIL_LISTS, DIL_LISTS],
}
TABLE["c3"] = TABLE["c2"]
EMBED = 64


def denoiser(which, width=1):
    from bdm_amd.pvcnn import PVCNN2_PC2, PVCNN2_PVD, link_pvconvs
    net = (PVCNN2_PC2(3, EMBED, extra_feature_channels=387, width_multiplier=width) if which == "pc2"
           else PVCNN2_PVD(3, EMBED, extra_feature_channels=0, width_multiplier=width)).eval()
    for blocks in list(net.sa_layers) + list(net.fp_layers):
        if isinstance(blocks, nn.Sequential):
            link_pvconvs(blocks)
    return net


def routes(net, which, B, N):
    """{module name: (module, its route as the denoiser's forward asks for it)}: the first PVConv of the PC^2 denoiser reads the hoisted
    maps, the first PVConv of levels 1, 2 is offered the input without the time embedding, every PVConv after another is offered rows."""
    from bdm_amd.modules import PVConv
    points = [N] + [sa[1][0] for sa in net.sa_blocks]
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, PVConv):
            kind, level, index = name.split(".")
            n = points[int(level)] if kind == "sa_layers" else points[len(net.fp_blocks) - 1 - int(level)]
            split = kind == "sa_layers" and int(level) > 0
            first = kind == "sa_layers" and int(index) == 0 or kind == "fp_layers" and int(index) == 1
            out[name] = (m, m.route(B, n, hoisted=which == "pc2" and name == "sa_layers.0.0", temb_split=split,
                                    c_feat=m.in_channels - EMBED if split else None, rows_offered=not first), n)
    return out


@pytest.mark.parametrize("which", ["pc2", "pvd"])
def test_route_table_of_the_benchmark_configurations(which):
    net = denoiser(which)
    for config, (B, N) in CONFIGS.items():
        got = routes(net, which, B, N)
        assert list(got) == ORDER
        want = [(MAP_LISTS if TABLE[config][0] == DIL_LISTS else MAP_FOLDED) if which == "pc2" else TABLE[config][0]] + TABLE[config][1:]
        for name, row in zip(ORDER, want):
            r = got[name][1]
            assert (r.first, r.gemm_impl, r.tail, r.dilate, r.takes_rows) == row, (config, name, r)
        # the dumps' bdm_sparse_conv_gemm_*_cb launches: levels 1, 2 take the time embedding as per-shape terms unless they run "dil"
        assert [got[n][1].temb_split for n in ("sa_layers.1.0", "sa_layers.2.0")] == [TABLE[config][2][0] != "dil", True], config


# ---- (2) coherence over sizes and knobs --------------------------------------------------------------------------------------------
ALL_R = {8, 16, 32}
KNOBS = {
    "defaults": {}, "conv_bf16x6": {"conv_impl": "bf16x6"}, "conv_fp32": {"conv_impl": "fp32"},
    "gemm_fp32": {"sparse_gemm": "sparse"}, "gemm_s3": {"sparse_gemm": "sparse_s3"}, "gemm_fused": {"sparse_gemm": "sparse_fused"},
    "conv_gemm": {"sparse_conv": "gemm"}, "dil_always": {"sparse_dil_always": True, "sparse_dil_resolutions": ALL_R},
    "compact_always": {"compact_tail": "always", "compact_tail_resolutions": ALL_R}, "compact_0": {"compact_tail": "0"},
    "lists_everywhere": {"sparse_dil_always": True, "sparse_dil_resolutions": ALL_R, "compact_tail": "always", "compact_tail_resolutions": ALL_R},
    "fold_gn1_off": {"fold_gn1": False}, "fold_gn2_off": {"fold_gn2": False}, "fold_pf_off": {"fold_pf": False},
    "se_in_devox": {"se_in_devox": True}, "temb_split_off": {"temb_split": False}, "sparse_first_conv_off": {"sparse_first_conv": False},
}
# (B, N) on both sides of ops.SPARSE_DIL_MIN_ITEMS = 160 (32^3: B * min(64, 2N / 512) * (2 if C > 64)) and COMPACT_16_MIN_ITEMS = 336
# (16^3, <= 64 channels: B * min(16, 3 * 1024 / 256) = 12 B: 27 / 28 shapes)
GRID = [(1, 1024), (2, 2048), (9, 4096), (10, 4096), (13, 4096), (14, 4096), (16, 4096), (27, 4096), (28, 4096), (8, 8192), (32, 16384)]


def check_coherence(net, which, B, N, what):
    got = routes(net, which, B, N)
    for name, (m, r, n) in got.items():
        tag = (what, B, N, name, r)
        assert (r.dilate == 2) == (r.tail == "lists"), tag
        assert (r.dilate >= 1) == (r.first == "dil" or r.tail == "lists"), tag
        assert not (r.first == "dil" and r.temb_split), tag
        assert r.compact_first == (r.first == "dil" and r.want_stats) and (r.tail != "lists" or r.want_stats), tag
        assert (r.plan_args is None) == r.first.startswith("dense") and (r.gemm_impl is not None) == (r.first in ("gemm", "gemm_split")), tag
        # a tail carries a head exactly when it is the one-launch small-grid tail and the successor's route takes the rows
        nxt = m._next_pv
        takes = nxt is not None and got[name[:-1] + str(int(name[-1]) + 1)][1].takes_rows
        assert r.head == (r.tail == "small" and takes), tag
        if nxt is None:
            assert not r.head, tag
        # what the side-stream planner builds ahead (no flags: it knows the sizes only) is what the forward will want
        ahead = m.route(B, n)
        if not (r.first == "map"):
            assert (ahead.plan_args, ahead.dilate) == (r.plan_args, r.dilate), tag
        assert m.wants_compact_tail(B, n) == (ahead.tail == "lists"), tag


@pytest.mark.parametrize("which", ["pc2", "pvd"])
def test_route_coherence_over_sizes_and_knobs(monkeypatch, which):
    from bdm_amd import ops
    from bdm_amd.modules import PVConv
    net = denoiser(which)
    assert ops.SPARSE_DIL_MIN_ITEMS == 160 and ops.COMPACT_16_MIN_ITEMS == 336   # (the grid above straddles these)
    seen = set()
    for knob, values in KNOBS.items():
        with monkeypatch.context() as mp:
            for k, v in values.items():
                mp.setattr(PVConv, k, v)
            for B, N in GRID:
                check_coherence(net, which, B, N, knob)
                seen |= {(r.first, r.tail) for _, r, _ in routes(net, which, B, N).values()}
    pv = next(m for m in net.modules() if isinstance(m, PVConv) and m.resolution == 32 and m is not net.sa_layers[0][0])
    pv.h2_saturated = True     # (ops.poll_h2_saturation: the layer leaves every fp16x3 form)
    for B, N in GRID:
        check_coherence(net, which, B, N, "saturated")
        r = pv.route(B, N)
        assert (r.first, r.tail, r.second, r.want_stats, r.dilate) == ("gemm", "plain", "bf16x6", False, 0)
    for glue, tail_only in itertools.product((True, False), repeat=2):
        with monkeypatch.context() as mp:
            mp.setattr(ops, "SMALL_GLUE", glue)
            mp.setattr(ops, "SMALL_GLUE_TAIL_ONLY", tail_only)
            check_coherence(net, which, 2, 1024, f"SMALL_GLUE={glue}, TAIL_ONLY={tail_only}")
            small = [r.tail == "small" for _, r, _ in routes(net, which, 2, 1024).values()]
            assert any(small) == glue
    # the sweep reaches every first-convolution form but the experimental gather-with-split, and every tail form
    assert {f for f, _ in seen} == {"map", "dil", "gemm", "dense_s3", "dense_fp32"} - ({"map"} if which == "pvd" else set())
    assert {t for _, t in seen} == {"lists", "small", "se_devox", "folded", "plain"}


# ---- (3) GPU: the route is what runs -----------------------------------------------------------------------------------------------
FIRST_KERNEL = {"map": "bdm_sparse_conv_rows_from_map", "dense_s3": "bdm_avg_voxelize_s3", "sparse_h2": "bdm_sparse_conv_gemm_h2",
                "sparse_s3": "bdm_sparse_conv_gemm_s3", "sparse": "bdm_sparse_conv_gemm"}
FIRST_KERNELS = {"bdm_sparse_conv_rows_from_map", "bdm_avg_voxelize_s3", "bdm_sparse_conv_dil", "bdm_sparse_conv_dil_gn", "bdm_sparse_conv_gemm",
                 "bdm_sparse_conv_gemm_h2", "bdm_sparse_conv_gemm_h2_cb", "bdm_sparse_conv_gemm_s3", "bdm_sparse_conv_gemm_s3_cb"}
TAIL_KERNEL = {"lists": "bdm_devoxelize_gn_gate_add_rows", "small": "bdm_pvconv_tail_small", "se_devox": "bdm_devoxelize_gn_se_add",
               "folded": "bdm_devoxelize_gn_gate_add", "plain": "bdm_devoxelize_gate_add"}
SECOND_KERNEL = {("fp16x3", True): "bdm_conv3d_3x3x3_h2_gn", ("fp16x3", False): "bdm_conv3d_3x3x3_h2", ("bf16x6", False): "bdm_conv3d_3x3x3_s3"}
GPU_KNOBS = ["defaults", "dil_always", "lists_everywhere", "conv_bf16x6", "gemm_s3", "gemm_fp32", "conv_gemm", "compact_0", "fold_gn1_off",
             "fold_gn2_off", "fold_pf_off", "se_in_devox", "temb_split_off", "sparse_first_conv_off", "small_glue_off", "saturated"]


@pytest.mark.gpu
@pytest.mark.parametrize("which,knob", [("pvd", k) for k in GPU_KNOBS] + [("pc2", k) for k in ("defaults", "lists_everywhere")])
def test_the_recorded_forward_runs_what_the_routes_name(hip, monkeypatch, which, knob):
    """One forward of a denoiser (B = 2, N = 1024) recorded on the launch tape under knobs that the suite's parity tests already force: per
    PVConv the first-convolution, second-convolution and tail kernels between its first and last launch are the ones its route() names;
    rows that a tail left are consumed (no feature pass); and no bdm_voxel_dilate* launch sits inside a PVConv whose plan the side-stream
    planner built for it (sa_layers.1.0, sa_layers.2.0, fp_layers.0.1) -- a planner that disagrees with forward about the lists shows up
    there.  (Later PVConvs that share a plan built for another module's route may still add their list: fp_layers.2.1 at B = 16.)"""
    from bdm_amd import ops, tape
    from bdm_amd.modules import PVConv
    from bdm_amd.pvcnn import PVCNN2_PC2, PVCNN2_PVD
    from bdm_amd.utils.procedural import fill_module_
    for k, v in KNOBS.get(knob, {}).items():
        monkeypatch.setattr(PVConv, k, v)
    if knob == "small_glue_off":
        monkeypatch.setattr(ops, "SMALL_GLUE", False)
    B, N, extra = 2, 1024, (32 if which == "pc2" else 0)
    net = fill_module_((PVCNN2_PC2 if which == "pc2" else PVCNN2_PVD)(3, EMBED, extra_feature_channels=extra).eval(), seed=9).cuda()
    if knob == "saturated":
        net.fp_layers[3][1].h2_saturated = True
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(B, 3, N, generator=g) * 0.4, torch.randn(B, extra, N, generator=g)], dim=1).cuda()
    t = torch.tensor([900, 3]).cuda()
    net(x, t)                                # (weight packs, workspaces: everything lazy stays off the tape)
    torch.cuda.synchronize()
    spans, asked = [], []
    real_forward, real_route = PVConv.forward, PVConv.route
    monkeypatch.setattr(PVConv, "route", lambda self, *a, **k: (asked.append((self, real_route(self, *a, **k))), asked[-1][1])[1])

    def forward(self, inputs):
        lo = len(tp.calls)
        out = real_forward(self, inputs)
        spans.append((self, lo, len(tp.calls), [r for m, r in asked if m is self][-1]))   # (forward's own question is the module's last)
        return out
    monkeypatch.setattr(PVConv, "forward", forward)
    with ops.static_step(), tape.record() as tp:
        net(x, t)
    torch.cuda.synchronize()
    assert not tp.broken and len(spans) == 14
    names = [getattr(fn, "__name__", "") for fn, _ in tp.calls]
    took_rows = 0
    for m, lo, hi, r in spans:
        mine, tag = names[lo:hi], (m.bdm_name, r)
        if r.first == "dil":
            first = "bdm_sparse_conv_dil_gn" if r.want_stats else "bdm_sparse_conv_dil"
        else:
            first = FIRST_KERNEL[r.first if r.gemm_impl is None else r.gemm_impl] + ("_cb" if r.temb_split else "")
        assert [k for k in mine if k in FIRST_KERNELS] == [first], tag
        assert ("bdm_sparse_conv_gather_gn" in mine) == (r.want_stats and r.first in ("map", "gemm")), tag
        if r.tail == "lists":
            assert "bdm_sparse_conv_dil_h2_gn" in mine and "bdm_group_norm_to_h2_rows" in mine, tag
        else:
            assert SECOND_KERNEL[(r.second, r.tail not in ("plain",))] in mine, tag
        tails = [k[:-3] if k.endswith("_pf") else k for k in mine if k.startswith("bdm_devoxelize") or k == "bdm_pvconv_tail_small"]
        assert tails == [TAIL_KERNEL[r.tail]], tag
        if r.gemm_impl == "sparse_h2":
            assert ("bdm_sparse_voxel_features_f32" not in mine) == r.takes_rows, tag
            took_rows += r.takes_rows
        if m.bdm_name in ("sa_layers.1.0", "sa_layers.2.0", "fp_layers.0.1"):
            assert not [k for k in mine if k.startswith("bdm_voxel_dilate")], tag
            assert (r.first == "dil" or r.tail == "lists") or knob not in ("dil_always", "lists_everywhere") or m.bdm_name == "sa_layers.1.0", tag
    heads = sum(r.head for _, _, _, r in spans)
    assert took_rows == heads, (knob, took_rows, heads)     # every operand a tail left was consumed, and none was formed in vain
    assert heads == {"defaults": 4, "small_glue_off": 0}.get(knob, heads), (knob, heads)   # (FP0 and FP1: two hand-overs each)
