"""The simple and PVCNN++ denoisers on the HIP path (csrc/simple_point.hip, bdm_amd/simple.py): the reference's goldens, the
fused layer kernel against a float64 evaluation of the same layer, the pooled max / std, batch invariance, the launch tape,
and the Blending CLI with model.point_cloud_model=simple."""
import numpy as np
import pytest
import torch

from simple_ref import E, S, filled, golden, layer

pytestmark = pytest.mark.gpu


def _net(kind, seed):
    from bdm_amd.model import PointCloudModel
    m = PointCloudModel(model_type="simple" if kind == "simple" else "pvcnnplusplus", in_channels=3 + S, embed_dim=E).model
    return filled(m.eval(), seed)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("kind,N,tol", [("simple", 1024, 1e-5), ("simple", 1100, 1e-5), ("pvcnnpp", 1024, 1e-4),
                                        ("pvcnnpp", 1100, 1e-4)])
def test_forward_matches_reference_golden(hip, kind, N, tol):
    from oracle.gen_golden import point_cloud_inputs
    g = golden(f"{kind}_full_n{N}.npz")
    net = _net(kind, int(g["weight_seed"])).cuda()
    x = point_cloud_inputs(int(g["B"]), 3 + int(g["S"]), N, seed=int(g["input_seed"])).cuda()
    y = net(x, torch.from_numpy(g["t"]).cuda())
    err = _rel(y, torch.from_numpy(g["out"]))
    print(f"{kind} N={N}: rel L2 vs reference golden {err:.2e}")
    assert err <= tol


@pytest.mark.parametrize("B,N", [(1, 1024), (3, 1100), (1, 16384), (3, 16384)])
def test_fused_layer_against_float64(hip, B, N):
    """Every layer kernel against a float64 evaluation of the same layer on the same input; pooled max bit-equal to
    torch.amax, pooled std within 1e-6 of float64 torch.std."""
    from oracle.gen_golden import point_cloud_inputs
    net = _net("simple", 7).cuda()
    x = point_cloud_inputs(B, 3 + S, N, seed=40 + B).cuda()
    trace = []
    net(x, torch.tensor([10, 400, 990][:B]).cuda(), _trace=trace)
    sd = {k: v.double().cpu() for k, v in net.state_dict().items()}
    worst = 0.0
    for i, (xi, pooled) in enumerate(trace[:-1]):
        xi_n = xi.transpose(1, 2)                                     # (B, N, 128)
        assert torch.equal(pooled[:, :128], xi_n.amax(dim=1)), f"layer {i}: max"
        std64 = xi_n.double().std(dim=1)
        assert float(((pooled[:, 128:].double() - std64).abs() / std64.abs().clamp_min(1e-30)).max()) <= 1e-6, f"layer {i}: std"
        nxt = trace[i + 1]
        nxt = nxt[0] if isinstance(nxt, tuple) else nxt
        ref = layer(sd, f"layers.{i}.", xi_n.double().cpu())
        err = _rel(nxt.transpose(1, 2), ref)
        worst = max(worst, err)
        assert err <= 5e-6, f"layer {i}: {err:.2e}"
    print(f"B={B} N={N}: worst layer rel L2 vs float64 {worst:.2e}")


def test_batch_invariance(hip):
    """Shape k of a B = 16 forward has the bits of the same shape run alone."""
    from oracle.gen_golden import point_cloud_inputs
    net = _net("simple", 8).cuda()
    B, N = 16, 1100
    x = point_cloud_inputs(B, 3 + S, N, seed=50).cuda()
    t = torch.arange(B).cuda() * 60 + 5
    y = net(x, t)
    for k in (0, 7, 15):
        assert torch.equal(net(x[k:k + 1].contiguous(), t[k:k + 1]), y[k:k + 1]), k


def test_launch_tape_replay_equals_eager_loop(hip, monkeypatch):
    """A Blending-style reverse loop with a `simple` recon model: the recorded and replayed step gives the eager bits; the early
    furthest-point sampler stays off for both new networks."""
    import bdm_amd.model as M
    from bdm_amd import pvcnn
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 10
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    cfg.model.point_cloud_model = "simple"
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    assert pvcnn.early_first_sampler(model.point_cloud_model.model, x0) is None
    assert pvcnn.early_first_sampler(_net("pvcnnpp", 1).cuda(), x0) is None
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    noise = [torch.randn(B, N, 3, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(steps)]

    def run(mode):
        monkeypatch.setattr(M, "TAPE_STEPS", mode)
        it = iter(noise)
        model.scheduler.noise_source = lambda shape, device: next(it)
        try:
            return model.interaction_sample(x0.clone(), batch.camera, batch.image_rgb, None, start_time=500,
                                            end_time=500 - steps).cpu()
        finally:
            model.scheduler.noise_source = None

    eager = run("0")
    taped = run("1")
    g = model._tape_cache
    assert g["off"] is None, g["off"]
    assert g["tape"] is not None
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, taped)


def test_main_blending_with_simple_model(hip, tmp_path):
    import main_blending
    from bdm_amd.io import load_pointcloud_ply
    out = main_blending.main(["run.job=sample_bdm_blending", f"run.save_dir={tmp_path}", "dataset=synthetic",
                              "dataset.max_points=512", "dataset.num_shapes=2", "dataloader.batch_size=2",
                              "run.num_inference_steps=1000", "run.diffusion_scheduler=ddpm", "aux_run.roll_step=1",
                              "aux_run.milestones=[1000,998,996,995]", "run.name=simple_cli", "model.point_cloud_model=simple"])
    files = sorted((out / "pred" / "chair").iterdir())
    assert len(files) == 2
    for f in files:
        p = load_pointcloud_ply(f)
        assert p.shape == (512, 3) and np.isfinite(p).all()


@pytest.mark.parametrize("kind,sched", [("simple", "ddim"), ("pvcnnplusplus", "ddpm")])
def test_main_sample_with_new_model_types(hip, tmp_path, kind, sched):
    import main as main_sample
    from bdm_amd.io import load_pointcloud_ply
    out = main_sample.main(["run.job=sample", f"run.save_dir={tmp_path}", "dataset=synthetic", "dataset.max_points=512",
                            "dataset.num_shapes=2", "dataloader.batch_size=2", "run.num_inference_steps=10",
                            f"run.diffusion_scheduler={sched}", "run.name=simple_cli", f"model.point_cloud_model={kind}"])
    files = sorted((out / "pred" / "chair").iterdir())
    assert len(files) == 2
    for f in files:
        p = load_pointcloud_ply(f)
        assert p.shape == (512, 3) and np.isfinite(p).all()
