"""The colouring model on the GPU against the float64 restatement (tests/color_ref.py; its inner PVCNN is the float32 oracle).

* teacher-forced block: the restatement's PVCNN is given the GPU's own fp32 norm0 output, so both sides sample and group on
  identical coordinates; sample / neighbour indices bit for bit, block output within 5e-6 relative L2 (the per-step figure of the
  teacher-forced suite, tests/test_hip_teacher_forced.py);
* free-running transformer, one and two layers: colours within the project's standing 1e-3 relative L2, for seeds at which the
  restatement run in float32 and in float64 picks identical FPS / ball-query indices in every block (checked here on the CPU,
  per host, before anything runs on the GPU: a flipped neighbour would otherwise be a property of the input, not of the kernels);
* the model's contract: Pointclouds with the input points and features in [0, 1], the reference's state-dict keys, determinism.

Sizes: B = 2, N = 1024 (the first set-abstraction level's centre count) and N = 1100 (no multiple of any tile).
"""
import pytest
import torch

import color_ref as R
from helpers import check_rel_l2, point_cloud_inputs

IN_CHANNELS = 3 + 3 + 384
CASES = [(1024, 1), (1024, 2), (1100, 1), (1100, 2)]
# Seeds are tried in this order and the first one that passes the index check below ON THIS HOST is used.  The check cannot be settled
# once and for all: the float32 side goes through the oracle PVCNN, whose last bits (and with them the second block's "coordinates")
# depend on the host's BLAS and thread count.  22 passes all four cases on the hosts this was written on; about one seed in two
# passes a one-layer case, one in five a two-layer case.
CANDIDATE_SEEDS = (22,) + tuple(s for s in range(20, 80) if s != 22)
# Two layers run at head scale 0.03 (see `transformer`): at head 1 a last-bit difference in the first block's input comes out of its
# PVCNN large enough to move a neighbour of the second block for 39 seeds in 40, so that no seed would hold from one host to the next.
# One layer runs at head 1, and so does the teacher-forced block, which is what pins the PVCNN at these widths.
TWO_LAYER_HEAD = 0.03

REFERENCE_KEYS = """
input_projection.weight input_projection.bias norm.weight norm.bias output_projection.weight output_projection.bias
blocks.{i}.norm0.weight blocks.{i}.norm0.bias blocks.{i}.norm2.weight blocks.{i}.norm2.bias
blocks.{i}.mlp.fc1.weight blocks.{i}.mlp.fc1.bias blocks.{i}.mlp.fc2.weight blocks.{i}.mlp.fc2.bias
""".split()


def transformer(layers, seed, head=1.0):
    """Procedural weights; `head` scales the last classifier layer of every inner PVCNN: the suite's "head scale"
    (tests/trajectory_case.py).  The reference initialises that layer at N(0, 1e-6); at head 1 the procedural
    PVCNN amplifies a last-bit difference of its input by orders of magnitude."""
    from bdm_amd.transformer import PointCloudTransformerModel
    from bdm_amd.utils.procedural import fill_module_
    net = fill_module_(PointCloudTransformerModel(num_layers=layers, model_type="pvcnn", in_channels=IN_CHANNELS, out_channels=3,
                                                  embed_dim=64).eval(), seed=seed)
    with torch.no_grad():
        for blk in net.blocks:
            last = blk.point_cloud_model.model.classifier[-1]
            last.weight.mul_(head)
            last.bias.mul_(head)
    return net, {k: v.clone() for k, v in net.state_dict().items()}


def conditioned_input(B, N, seed):
    """(B, N, 390): coordinates 0.5 N(0, 1), feature channels N(0, 1) (the draw of the denoiser goldens)."""
    return point_cloud_inputs(B, IN_CHANNELS, N, seed).transpose(1, 2).contiguous()


def gpu_sa_indices(hip, coords):
    from oracle.ref_net import SA_BLOCKS
    out, c = [], coords.contiguous()
    for _, (m, radius, u, _) in SA_BLOCKS:
        idx = hip.furthest_point_sampling(c, m)
        centers = hip.gather_features_forward(c, idx)
        out.append((idx.cpu(), hip.ball_query(centers, c, radius, u).cpu()))
        c = centers
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1100])
def test_block_teacher_forced(hip, oracle_ops, N):
    B, seed = 2, 31
    net, sd = transformer(1, seed)
    x = conditioned_input(B, N, seed)
    trace = []
    net.cuda().forward_colors(x.cuda(), 0.5, 0.5, trace=trace)
    h, ln, p, y = (t.transpose(1, 2).cpu() for t in trace[0])   # (B, N, E)
    ours = gpu_sa_indices(hip, trace[0][1][:, :3])
    for lvl, ((fi, bi), (fr, br)) in enumerate(zip(ours, R.sa_indices(ln.transpose(1, 2)[:, :3]))):
        assert torch.equal(fi, fr), f"level {lvl}: furthest point samples differ"
        assert torch.equal(bi, br), f"level {lvl}: ball-query neighbours differ"
    h64 = R.linear(x.double(), sd["input_projection.weight"], sd["input_projection.bias"])
    check_rel_l2(h.double(), h64, 5e-6, "input projection")
    y64, ln64, p64 = R.block(sd, "blocks.0.", h64, pvcnn_input=ln)
    check_rel_l2(ln.double(), ln64, 5e-6, "norm0")
    check_rel_l2(p.double(), p64, 5e-6, "PVCNN on the GPU's norm0 output")
    check_rel_l2(y.double(), y64, 5e-6, "block output")


def same_indices(ln32, ln64):
    """Do the float32 and the float64 norm0 outputs (B, N, E) lead to identical FPS / ball-query indices on all four levels?"""
    ia, ib = R.sa_indices(ln32.transpose(1, 2)[:, :3]), R.sa_indices(ln64.float().transpose(1, 2)[:, :3])
    return all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(ia, ib))


def restatement_pair(sd, x, layers):
    """The restatement in float32 and in float64, block by block, given up at the first block whose PVCNN would sample or group
    differently in the two (-> None); else the float64 colours.  The check comes BEFORE each PVCNN: a rejected seed costs little."""
    h32 = R.linear(x, sd["input_projection.weight"], sd["input_projection.bias"])
    h64 = R.linear(x.double(), sd["input_projection.weight"], sd["input_projection.bias"])
    for i in range(layers):
        pre = f"blocks.{i}."
        ln32, ln64 = (R.layer_norm(h, sd[pre + "norm0.weight"], sd[pre + "norm0.bias"]) for h in (h32, h64))
        if not same_indices(ln32, ln64):
            return None
        h64 = R.block_tail(sd, pre, h64, R.pvcnn(sd, pre, ln64, torch.float64))
        if i + 1 < layers:
            h32 = R.block_tail(sd, pre, h32, R.pvcnn(sd, pre, ln32, torch.float32))
    return torch.clamp(R.linear(h64, sd["output_projection.weight"], sd["output_projection.bias"]) * 0.5 + 0.5, 0, 1)


def seeded_case(B, N, layers, head=1.0):
    """The first candidate seed at which the restatement run in float32 and in float64 selects identical FPS / ball-query indices
    in every block, with its network, input and float64 colours."""
    for seed in CANDIDATE_SEEDS:
        net, sd = transformer(layers, seed, head)
        x = conditioned_input(B, N, seed)
        ref = restatement_pair(sd, x, layers)
        if ref is not None:
            return seed, net, sd, x, ref
    pytest.fail(f"none of the seeds {CANDIDATE_SEEDS[0]} .. {CANDIDATE_SEEDS[-1]} passes the float32 / float64 index check")


def test_restatement_pair_is_the_restatement(oracle_ops):
    """(CPU) restatement_pair computes color_ref.colors, and refuses an input on which float32 and float64 sample differently."""
    net, sd = transformer(1, 3)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 1100, IN_CHANNELS, generator=g)
    t32, t64 = [], []
    R.colors(sd, x, trace=t32)
    whole = R.colors(sd, x.double(), trace=t64)
    got = restatement_pair(sd, x, 1)
    if same_indices(t32[0][1], t64[0][1]):
        assert torch.equal(got, whole)
    else:
        assert got is None
    x[0, 1] = x[0, 0]   # two identical points: an exact tie in every distance comparison, same in both precisions -- still equal indices
    ln = torch.randn(1, 1100, 64, generator=g)
    assert same_indices(ln, ln.double())
    far = ln.double().clone()
    far[0, :, 0] += torch.linspace(0, 1, 1100, dtype=torch.float64)   # another cloud: other samples
    assert not same_indices(ln, far)


@pytest.mark.gpu
@pytest.mark.parametrize("N,layers", CASES)
def test_free_running_colours(hip, oracle_ops, N, layers):
    B = 2
    seed, net, sd, x, ref = seeded_case(B, N, layers, head=TWO_LAYER_HEAD if layers > 1 else 1.0)
    print(f"N {N}, {layers} layer(s): seed {seed}")
    from bdm_amd import transformer as T
    default, net = T.TAIL_IMPL, net.cuda()
    try:
        for impl in ("fused", "composed"):   # the fused tail kernel and the route composed from existing launches
            T.TAIL_IMPL = impl
            got = net.forward_colors(x.cuda(), 0.5, 0.5).cpu()
            assert got.shape == (B, N, 3) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
            check_rel_l2(got.double(), ref, 1e-3, f"{layers} layer(s), {impl} tail")
    finally:
        T.TAIL_IMPL = default
    raw = net(x.cuda()).cpu()   # the reference's forward: the raw output projection
    check_rel_l2(torch.clamp(raw * 0.5 + 0.5, 0, 1).double(), ref, 1e-3, "through forward()")


@pytest.mark.gpu
def test_composed_tail_agrees_with_the_fused_kernel(hip):
    """The yardstick route of tools/coloring_bench.py (existing launches) computes the same block output and colours."""
    from bdm_amd import transformer as T
    net, _ = transformer(2, 7)
    net = net.cuda()
    g = torch.Generator().manual_seed(0)
    h, p = torch.randn(2, 64, 1100, generator=g).cuda(), torch.randn(2, 64, 1100, generator=g).cuda()
    blk = net.blocks[0]
    for kw in ({}, {"next_norm": net.blocks[1].norm0}, {"head": (net.output_projection, 0.5, 0.5)}):
        default = T.TAIL_IMPL
        try:
            T.TAIL_IMPL = "fused"
            fused = blk.tail(h, p, **kw)
            T.TAIL_IMPL = "composed"
            composed = blk.tail(h, p, **kw)
        finally:
            T.TAIL_IMPL = default
        for a, b in zip(fused, composed):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.shape == b.shape
                check_rel_l2(a, b, 2e-6, "fused vs composed")


@pytest.mark.gpu
def test_model_contract(hip):
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.config import PointCloudColoringModelConfig, ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.model import get_coloring_model
    from bdm_amd.utils.procedural import fill_module_
    cfg = ProjectConfig()
    cfg.model = PointCloudColoringModelConfig()
    model = get_coloring_model(cfg).eval()
    keys = sorted(k.format(i=0) for k in REFERENCE_KEYS)
    own = [k[len("point_cloud_model."):] for k in model.state_dict() if k.startswith("point_cloud_model.")
           and not k.startswith("point_cloud_model.blocks.0.point_cloud_model.model.")]
    assert sorted(own) == keys
    # a state dict with exactly the reference's key list loads strictly: the transformer's own keys, the inner PVCNN's under
    # blocks.0.point_cloud_model.model.* (PointCloudModel / PVCNN2_PC2, as in the diffusion model) and the feature model's
    from bdm_amd.model import PointCloudModel
    inner = PointCloudModel(model_type="pvcnn", in_channels=64, out_channels=64, embed_dim=64).state_dict()
    expected = ["point_cloud_model." + k for k in keys] + ["point_cloud_model.blocks.0.point_cloud_model." + k for k in inner] + \
        [k for k in model.state_dict() if k.startswith("feature_model.")]
    sd = {k: torch.zeros_like(model.state_dict()[k]) for k in expected}
    assert set(sd) == set(model.state_dict())
    model.load_state_dict(sd, strict=True)
    fill_module_(model, seed=4)
    model = model.cuda()
    B, N = 2, 1100
    batch = next(iter(SyntheticShapes(range(B), B, seed=4, image_size=224, num_points=N))).to("cuda")
    pc = batch.sequence_point_cloud
    pts = pc.points_padded() if isinstance(pc, Pointclouds) else pc
    out = model(batch, return_point_cloud=True)
    assert isinstance(out, Pointclouds)
    assert torch.equal(out.points_padded(), pts * model.scale_factor / model.scale_factor)
    f = out.features_padded()
    assert f.shape == (B, N, 3) and bool(torch.isfinite(f).all()) and float(f.min()) >= 0.0 and float(f.max()) <= 1.0
    assert torch.equal(model(batch, return_point_cloud=True, noise_std=0).features_padded(), f), "noise_std = 0 is deterministic"
    noisy = model(batch, return_point_cloud=True, noise_std=0.05)
    assert torch.equal(noisy.points_padded(), pts) and not torch.equal(noisy.features_padded(), f)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        model(batch)


@pytest.mark.gpu
def test_shape_model_is_unchanged(hip):
    from bdm_amd.config import ProjectConfig
    from bdm_amd.model import get_model
    model = get_model(ProjectConfig())
    assert (model.in_channels, model.out_channels) == (3 + 3 + 384, 3)
    assert model.point_cloud_model.model.classifier[-1].weight.shape[0] == 3
