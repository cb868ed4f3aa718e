"""Config C1 of BASELINE.json -- vanilla PC^2 sampling of ONE shape, N = 1024 points, 100 DDPM steps (leading spacing:
t = 990, 980, ..., 0), projection conditioning at every step, identical injected noise on both sides -- as a CHAOS MONITOR, plus
the bit-equality tests of the recorded forms of the reverse loop (hipGraph, launch tape).

Free-running C1 at the literal 1e-3 (round 6): head scale 0.3, the largest the head-scale rule allows for this configuration
(test_c1_free_running_final_cloud_vs_oracle_fixture).  At head scale 1 the random-init sampler amplifies 1-ulp changes through its
discrete decisions (pixel ownership, ball-query membership, FPS arg-max, voxel rounding), so a free-running comparison there measures
chaos: that case stays as a monitor -- 1e-5 until the first flip (first 10 steps), afterwards no faster than
the oracle diverges from ITSELF (1 ulp away / another reduction order).  Per-step parity at head scale 1 is held by
tests/test_hip_teacher_forced.py (every timestep, <= 1e-5 per step)."""
import pytest
import torch

from helpers import rel_l2, seeded

pytestmark = pytest.mark.gpu


def _c1_fixture(name):
    import os
    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(here, f"traj_{name}.npz"))
    alt = np.load(os.path.join(here, f"traj_{name}_alt.npz"))
    return {k: g[k] for k in g.files}, {k: alt[k] for k in alt.files}


@pytest.mark.parametrize("name", ["c1_n1024_h03", "c1_n1024_h01"])
def test_c1_free_running_final_cloud_vs_oracle_fixture(hip, name):
    """C1 as the reference runs it (model/model.py:182-201): vanilla PC^2, ONE shape, N = 1024, 100 FREE-RUNNING steps, projection
    conditioning at every step -- final cloud against the oracle's (tests/golden/traj_<name>.npz, oracle/gen_golden_traj.py) at the
    LITERAL 1e-3.  Head scale 0.3 = the largest of {1, 0.3, 0.1, 0.03} at which the oracle's own 1-ulp
    self-sensitivity over these 100 steps stays below 1e-4 (7.1e-3 / 8.2e-6 / 2.6e-7 / 2.0e-7: the rule of
    tests/test_hip_full_trajectory.py applied to this configuration).  The oracle at ANOTHER reduction order (the `_alt` fixture: 1
    thread against 2) says more than that single probe: at 0.3 it ends 1.05e-3 from the fixture of record -- one discrete decision
    (pixel ownership / ball membership) flips between steps 30 and 40 -- at 0.1 it stays at the fp32 floor.  Both head scales are
    held to the literal bound; the 3e-4 early-warning line (the C2 / C3 fixtures') is asserted where the oracle agrees with itself
    (0.1: there the HIP path ends 1.4e-4 away after two discrete flips of its own, steps 20 - 50, which neither oracle variant nor
    the 1-ulp probe shares -- its per-forward distance from exact arithmetic is ~1e-6 against the oracle variants' 5e-7 from each
    other).  Both oracle yardsticks travel with the fixtures and go on the record beside the figure."""
    import trajectory_case as case
    from helpers import parity
    g, alt = _c1_fixture(name)
    h = float(g["head_scale"])
    c = case.build_c1(h, num_points=int(g["N"]), steps=int(g["steps"]))
    final, snaps = case.run_hip_c1(c)
    assert bool(torch.isfinite(final).all())
    curve = [rel_l2(x, torch.from_numpy(g[f"snap_{i}"])) for i, x in enumerate(snaps)]
    d_oo = rel_l2(torch.from_numpy(alt["final"]), torch.from_numpy(g["final"]))
    calm = d_oo < 1e-4
    err = parity(f"traj_{name} final cloud (C1: vanilla PC^2, 100 free-running steps, head {h:g})", rel_l2(final, torch.from_numpy(g["final"])), 1e-3,
                 note="margin line 3e-4" if calm else f"oracle vs oracle {d_oo:.1e}: no margin line")
    parity(f"traj_{name} oracle 1-ulp self-sensitivity (context)", float(g["self_sensitivity"]), 1e-4)
    parity(f"traj_{name} oracle vs oracle at another reduction order (context)", d_oo, 1.0)
    print(f"C1 free-running, head {h:g}: every 10th step", " ".join(f"{e:.1e}" for e in curve), f"final {err:.3e}; oracle vs oracle {d_oo:.3e}")
    assert float(g["self_sensitivity"]) < 1e-4
    assert err <= 1e-3, f"final rel-L2 {err:.3e}; every 10th step {['%.1e' % e for e in curve]}"
    if calm:
        assert err <= 3e-4, f"margin gone: {err:.3e} is inside 1e-3 but past the 3e-4 early-warning line"


def test_c1_chaos_monitor_divergence_no_faster_than_the_oracles_own(hip):
    """Head scale 1 (a random-init network at full gain): the HIP path tracks the oracle to 1e-5 over the first 10 steps and afterwards
    diverges no faster than the ORACLE diverges from itself -- started one float32 ulp away (`self_sensitivity` of the fixture) or run at
    another reduction order (`traj_c1_n1024_h1_alt.npz`): final rel-L2 <= max(1e-3, 4 x the larger of the two).  Both yardsticks are
    oracle-vs-oracle, generated once in the build container (the live oracle runs of rounds 2 - 5 cost the GPU suite ~100 s of host time)."""
    import trajectory_case as case
    from helpers import parity
    g, alt = _c1_fixture("c1_n1024_h1")
    c = case.build_c1(1.0, num_points=int(g["N"]), steps=int(g["steps"]))
    final, snaps = case.run_hip_c1(c)
    curve = [rel_l2(x, torch.from_numpy(g[f"snap_{i}"])) for i, x in enumerate(snaps)]
    d_oo = rel_l2(torch.from_numpy(alt["final"]), torch.from_numpy(g["final"]))
    yard = max(float(g["self_sensitivity"]), d_oo)
    err = rel_l2(final, torch.from_numpy(g["final"]))
    print("C1 chaos monitor, head 1: every 10th step", " ".join(f"{e:.1e}" for e in curve),
          f"final {err:.3e}; oracle 1-ulp self-sensitivity {float(g['self_sensitivity']):.3e}, oracle vs oracle {d_oo:.3e}")
    parity("c1 trajectory (head scale 1, chaos monitor): first 10 steps", curve[0], 1e-5)
    parity("c1 trajectory (head scale 1, chaos monitor): final vs 4x the oracle's own spread", err, max(1e-3, 4 * yard))
    assert curve[0] < 1e-5
    assert err <= max(1e-3, 4 * yard)


def test_graph_replay_equals_eager_loop(hip, monkeypatch):
    """The hipGraph form of the reverse loop (one captured step replayed per timestep) gives the bits of the eager loop."""
    import bdm_amd.model as M
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 12
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    noise = [torch.randn(B, N, 3, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(steps)]

    def run(graph):
        monkeypatch.setattr(M, "GRAPH_STEPS", graph)
        it = iter(noise)
        model.scheduler.noise_source = lambda shape, device: next(it)
        try:
            return model.interaction_sample(x0.clone(), batch.camera, batch.image_rgb, None, start_time=500,
                                            end_time=500 - steps).cpu()
        finally:
            model.scheduler.noise_source = None

    eager, graphed = run(False), run(True)
    assert getattr(model, "_graph_cache", None) is not None  # the graph path was taken
    assert torch.equal(eager, graphed)
    again = run(True)  # second use replays the cached graph
    assert torch.equal(eager, again)


def test_launch_tape_replay_equals_eager_loop(hip, monkeypatch):
    """The launch-tape form of the reverse loop (bdm_amd/tape.py: one step recorded as a flat list of C-ABI calls, replayed
    per timestep) gives the bits of the eager loop, records every launch of the step, and is re-used by the next trajectory."""
    import bdm_amd.model as M
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 12
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()
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
    assert getattr(model, "_tape_cache", None) is None
    taped = run("1")
    g = model._tape_cache
    assert g["off"] is None, g["off"]
    assert g["tape"] is not None and len(g["tape"]) > 150  # the whole step is on the tape
    print("launch tape:", len(g["tape"]), "entries,", len(g["tape"].torch_ops), "torch operators:", sorted(set(g["tape"].torch_ops)))
    assert torch.equal(eager, taped)
    tape_before = g["tape"]
    again = run("auto")  # B * N is below the host-bound threshold: the default takes the tape, and re-uses the recorded one
    assert model._tape_cache["tape"] is tape_before
    assert torch.equal(eager, again)
    # rewriting a weight invalidates the recording (it holds the addresses of packs derived from the old values)
    with torch.no_grad():
        conv = next(m for m in model.point_cloud_model.modules() if isinstance(m, torch.nn.Conv3d))
        conv.weight.mul_(1.25)
    changed_tape, changed_eager = run("1"), run("0")
    assert model._tape_cache["tape"] is not tape_before
    assert torch.equal(changed_tape, changed_eager) and not torch.equal(changed_tape, eager)


def test_launch_tape_counts_steps_and_is_reused_across_segments(hip, monkeypatch):
    """Two interaction_sample segments of one trajectory on the launch tape (the samplers run the PC^2 loop in segments): the record's
    step counter runs on across them (replay.run_step), the second segment replays the first's recording, and the result has the
    bits of the same two segments run eagerly."""
    import bdm_amd.model as M
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 12
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    noise = [torch.randn(B, N, 3, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(2 * steps)]

    def run(mode):
        monkeypatch.setattr(M, "TAPE_STEPS", mode)
        it = iter(noise)
        model.scheduler.noise_source = lambda shape, device: next(it)
        tapes = []
        try:
            x = x0.clone()
            for start in (500, 500 - steps):
                x = model.interaction_sample(x, batch.camera, batch.image_rgb, None, start_time=start, end_time=start - steps)
                tapes.append((getattr(model, "_tape_cache", None) or {}).get("tape"))
            return x.cpu(), tapes
        finally:
            model.scheduler.noise_source = None

    eager, tapes = run("0")
    assert tapes == [None, None]
    taped, tapes = run("1")
    g = model._tape_cache
    assert g["off"] is None, g["off"]
    assert g["steps"] == 2 * steps - 1
    assert tapes[0] is not None and tapes[1] is tapes[0] and g["tape"] is tapes[0]
    assert torch.equal(eager, taped)


def test_prior_loop_replayed_from_a_tape_equals_the_eager_loop(hip, monkeypatch):
    """pvd.Model.gen_samples in launch-tape form (the prior's 16-step segments of the BDM recipes, pvd/__init__.py:226-270 through
    generate_pvd_xyz :450-473): the bits of the eager loop, with the reference's global-generator noise and with the per-shape Philox
    streams; the recording is re-used by the next segment and dropped when a weight changes."""
    from bdm_amd import rng
    from bdm_amd.pvd import Model, generate_pvd_xyz, prepare_pvd_model
    B, N, steps = 2, 1024, 8
    pvd = prepare_pvd_model({"model": None, "nc": 3, "embed_dim": 64, "attention": True, "dropout": 0.1}, torch.device("cuda"))
    x0 = (torch.randn(B, 3, N, generator=torch.Generator().manual_seed(5)) * 0.5).cuda()

    def run(taped, philox):
        monkeypatch.setattr(Model, "tape_pvd", taped)
        pvd.diffusion.streams = rng.ShapeStreams(7, range(B), torch.device("cuda")) if philox else None
        if not philox:
            torch.manual_seed(11)
            torch.cuda.manual_seed_all(11)
        try:
            first = generate_pvd_xyz(pvd, x0.clone(), 400, 400 - steps)
            return generate_pvd_xyz(pvd, first, 300, 300 - steps).cpu()      # a second segment
        finally:
            pvd.diffusion.streams = None

    for philox in (False, True):
        pvd._tape_cache = None
        eager = run(False, philox)
        assert getattr(pvd, "_tape_cache", None) is None
        taped = run(True, philox)
        g = pvd._tape_cache
        assert g["off"] is None, g["off"]
        assert g["tape"] is not None and len(g["tape"]) > 120 and g["steps"] == 2 * steps - 1
        assert torch.equal(eager, taped), philox
    tape_before = pvd._tape_cache["tape"]
    again = run(True, True)
    assert pvd._tape_cache["tape"] is tape_before and torch.equal(again, taped)
    with torch.no_grad():
        conv = next(m for m in pvd.model.modules() if isinstance(m, torch.nn.Conv3d))
        conv.weight.mul_(1.25)
    changed_tape, changed_eager = run(True, True), run(False, True)
    assert pvd._tape_cache["tape"] is not tape_before
    assert torch.equal(changed_tape, changed_eager) and not torch.equal(changed_tape, taped)


def test_saturation_reroute_reaches_a_recorded_step(hip, monkeypatch):
    """a recorded reverse step has a layer's fp16x3 kernels baked in.  When poll_h2_saturation() switches
    that layer to bf16x6, the recording must not be replayed: the cache key carries ops.saturation_epoch(), the next loop
    re-records, and the new tape launches the bf16x6 convolution for the flagged layer."""
    import warnings
    import bdm_amd.model as M
    from bdm_amd import ops
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.modules import PVConv
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 1, 1024, 10
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    monkeypatch.setattr(M, "TAPE_STEPS", "1")

    def run():
        it = iter(torch.randn(B, N, 3, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(steps))
        model.scheduler.noise_source = lambda shape, device: next(it)
        try:
            return model.interaction_sample(x0.clone(), batch.camera, batch.image_rgb, None, start_time=500, end_time=500 - steps).cpu()
        finally:
            model.scheduler.noise_source = None

    def names(tp):
        return [getattr(fn, "__name__", "") for fn, _ in tp.calls]

    before = run()
    tape0 = model._tape_cache["tape"]
    assert tape0 is not None and model._tape_cache["off"] is None
    n_s3_before = sum(n == "bdm_conv3d_3x3x3_s3" for n in names(tape0))
    # a degenerate cloud would do this: raise the sticky word of ONE fp16x3 layer
    pv = next(m for m in model.point_cloud_model.modules() if isinstance(m, PVConv) and getattr(m, "conv_impl", "") == "fp16x3")
    ops.saturation_slot(pv, x0.device).fill_(1)
    epoch = ops.saturation_epoch()
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        assert ops.poll_h2_saturation() == [pv]
    assert ops.saturation_epoch() == epoch + 1 and pv.h2_saturated
    after = run()
    tape1 = model._tape_cache["tape"]
    assert tape1 is not tape0, "the recorded step with the clamped fp16x3 kernels was replayed"
    assert sum(n == "bdm_conv3d_3x3x3_s3" for n in names(tape1)) == n_s3_before + 1   # the flagged layer's second convolution
    assert float((after - before).norm() / before.norm()) < 1e-3                       # same sampler, bf16x6 in one layer


def test_recorded_step_pins_the_buffers_it_did_not_allocate(hip, monkeypatch):
    """a step recorded into the tape's private pool also bakes in addresses of buffers allocated OUTSIDE the
    recording -- `ops._ws_cache` workspaces (replaced when a larger request arrives), the packed cameras (a single-entry cache
    replaced by any call with another camera), weight packs.  The tape pins them: after an eager call has replaced the rasteriser
    workspace and the camera pack, replaying the OLD recording still gives the eager loop's bits."""
    import bdm_amd.model as M
    from bdm_amd import ops
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 10
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=3).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    other = next(iter(SyntheticShapes(range(7, 7 + 2 * B), 2 * B, num_points=N))).to("cuda")   # another camera, a larger batch
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(5)).cuda()

    def run(mode, b=batch, x=x0, n=steps):
        monkeypatch.setattr(M, "TAPE_STEPS", mode)
        it = iter(torch.randn(x.shape, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(n))
        model.scheduler.noise_source = lambda shape, device: next(it)
        try:
            return model.interaction_sample(x.clone(), b.camera, b.image_rgb, None, start_time=500, end_time=500 - n).cpu()
        finally:
            model.scheduler.noise_source = None

    eager = run("0")
    taped = run("1")
    tp = model._tape_cache["tape"]
    assert tp is not None and tp.pool is not None and torch.equal(eager, taped)
    pinned = {t.untyped_storage().data_ptr() for t in tp.keep if isinstance(t, torch.Tensor)}
    cam_ptr = model._cam_cache[1].untyped_storage().data_ptr()
    ws_ptrs = {k: v.untyped_storage().data_ptr() for k, v in ops._ws_cache.items()}
    assert cam_ptr in pinned, "the packed cameras' address is baked into the step but not pinned by the tape"
    assert pinned & set(ws_ptrs.values()), "no cached workspace is pinned although the step's kernels use them"
    assert not (pinned & tp.pool_storages)
    g = model._tape_cache

    def replay_once():   # the recorded step by hand, on its own static buffers
        g["x"].copy_(x0)
        g["t"].fill_(400)
        tp.replay()
        torch.cuda.synchronize()
        return g["eps"].clone()
    eps_before = replay_once()
    # an eager call with another camera and twice the batch: replaces the camera pack and outgrows the workspaces
    x_big = torch.randn(2 * B, N, 3, generator=torch.Generator().manual_seed(9)).cuda()
    run("0", b=other, x=x_big, n=3)
    assert model._cam_cache[1].untyped_storage().data_ptr() != cam_ptr
    assert any(v.untyped_storage().data_ptr() != ws_ptrs.get(k) for k, v in ops._ws_cache.items())
    junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(64)]   # whatever was freed is overwritten
    del junk
    # the OLD recording still reads and writes only memory it owns or pinned
    assert torch.equal(replay_once(), eps_before) and bool(torch.isfinite(eps_before).all())


def test_first_level_sampled_ahead_of_the_conditioning_same_bits(hip, monkeypatch):
    """pvcnn.early_first_sampler: the first set-abstraction level's furthest point sampling starts from x_t on the sampler's stream
    before the step's projection conditioning; the forward that follows uses those centres.  Same bits as sampling inside the
    encoder, eagerly and on a replayed tape; a forward whose input is NOT the conditioned tensor of that call samples for itself."""
    import bdm_amd.model as M
    import bdm_amd.pvcnn as PV
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N, steps = 2, 1024, 6
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=4).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(6)).cuda()
    noise = [torch.randn(B, N, 3, generator=torch.Generator().manual_seed(200 + i)).cuda() for i in range(steps)]

    def run(early, mode):
        monkeypatch.setattr(PV, "EARLY_SAMPLER", early)
        monkeypatch.setattr(M, "TAPE_STEPS", mode)
        model._tape_cache = None
        it = iter(noise)
        model.scheduler.noise_source = lambda shape, device: next(it)
        try:
            return model.interaction_sample(x0.clone(), batch.camera, batch.image_rgb, None, start_time=400, end_time=400 - steps).cpu()
        finally:
            model.scheduler.noise_source = None

    ref = run(False, "0")
    assert torch.equal(run(True, "0"), ref)
    assert torch.equal(run(True, "1"), ref)
    # the handle vouches for ONE tensor: a copy of the conditioned input carries no handle and is sampled inside the encoder
    monkeypatch.setattr(PV, "EARLY_SAMPLER", True)
    t = torch.full((B,), 300, dtype=torch.int64, device="cuda")
    x_in = model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t)
    assert x_in._bdm_cond.early is not None
    with_handle = model.point_cloud_model(x_in, t)
    plain = model.point_cloud_model(x_in.clone(), t)
    assert torch.allclose(with_handle, plain, rtol=0, atol=1e-5)   # (the clone also leaves the hoisted-conditioning path: not the same bits)


def test_lazily_conditioned_input_is_either_unread_or_completed(hip, monkeypatch):
    """model.get_input_with_conditioning(lazy=True) (the reverse loops): only the coordinate rows of the (B, 3 + C, N) input are written.
    (a) With every reader of the feature rows on a hoisted map the forward gives the bits of the complete input -- also when rows 3..
    are poisoned with NaN, so nothing reads them; (b) when a reader is NOT hoisted (here: the hoisted first convolution switched off)
    the denoiser completes the tensor first; (c) completing is idempotent."""
    import bdm_amd.model as M
    from bdm_amd import modules, ops
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.utils.procedural import fill_module_
    B, N = 2, 1024
    cfg = ProjectConfig()
    cfg.dataset.max_points = N
    model = fill_module_(M.get_model(cfg).eval(), seed=5).cuda()
    batch = next(iter(SyntheticShapes(range(B), B, num_points=N))).to("cuda")
    x0 = (torch.randn(B, N, 3, generator=torch.Generator().manual_seed(8)) * 0.5).cuda()
    t = torch.full((B,), 321, dtype=torch.int64, device="cuda")
    full = model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t)
    assert full._bdm_cond.features_ready
    ref = model.point_cloud_model(full, t).clone()
    lazy = model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t, lazy=True)
    cond = lazy._bdm_cond
    assert not cond.features_ready and torch.equal(cond.x_cf[:, :3], full._bdm_cond.x_cf[:, :3])
    cond.x_cf[:, 3:].fill_(float("nan"))                       # (a) poisoned: a reader would spread NaN
    got = model.point_cloud_model(lazy, t)
    assert not cond.features_ready and torch.equal(got, ref)
    # (b) a generic reader: the tensor is completed, and the result is that of the complete input
    lazy2 = model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t, lazy=True)
    monkeypatch.setattr(modules.PVConv, "sparse_first_conv", False)
    ref_b = model.point_cloud_model(model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t), t).clone()
    got_b = model.point_cloud_model(lazy2, t)
    assert lazy2._bdm_cond.features_ready and torch.equal(lazy2._bdm_cond.x_cf, full._bdm_cond.x_cf) and torch.equal(got_b, ref_b)
    monkeypatch.setattr(modules.PVConv, "sparse_first_conv", True)
    # (c) completing is idempotent and leaves the complete tensor
    lazy3 = model.get_input_with_conditioning(x0, batch.camera, batch.image_rgb, None, t, lazy=True)
    lazy3._bdm_cond.ensure_features()
    lazy3._bdm_cond.ensure_features()
    assert lazy3._bdm_cond.features_ready and torch.equal(lazy3._bdm_cond.x_cf, full._bdm_cond.x_cf)
