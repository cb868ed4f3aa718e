"""bench.py -- sampled shapes/sec of the BDM coupled-diffusion sampling hot path on MI355X.

Metric (BASELINE.json): sampled shapes/sec (4096 pts, 1000 DDPM steps).  One "step" = ONE COMPLETE
BDM-Blending trajectory of a batch of 16 shapes per GPU (config C2: N = 4096, milestones
[1000,968,936,872,128,64,32,0], roll_step 16 -> 1000 PC^2 denoiser steps with per-step projection
conditioning + 80 PVD prior steps + 5 blends, plus the hoisted image encoder once per batch), on
synthetic inputs and procedural random-init weights (no datasets / checkpoints offline).  Nothing is
skipped inside the timed region.  N GPUs = N independent shards of 16 shapes (weak scaling, no
collective on the data path; one barrier + MAX-over-ranks for timing).

    python bench.py                          # 1 GPU, 1 trajectory (about a minute)
    python bench.py --gpus N                 # no WORLD_SIZE in the environment: starts its own N workers (one per GPU) through
                                             # `python -m torch.distributed.run` BEFORE anything touches a GPU, relays rank 0's line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --config c3              # the other BASELINE.json configurations at their per-GPU batch:
                                             #   c2 Blending N=4096 B=16 (default, the metric's workload) | c3 Merging N=4096 B=16
                                             #   c4 Blending N=8192 B=8 | c5 Blending N=16384 B=32
    python bench.py --full                   # also the kernel-class profile, roofline figures and CPU baselines below
    python bench.py --dump-outputs DIR       # after the timed steps: DIR/points.npy = the (shapes, points, 3) float32 clouds
                                             # of the last timed trajectory (same arguments -> same inputs)

A plain run sets up, warms up, times --steps trajectories and prints the headline line (metric, value, unit, ms_per_step, ...).
Nothing else runs: no profiler is installed in the timed region and no step of the replayed loops is diverted to an eager probe.

Extra objects on the JSON line, with --full only (the timed region then also runs every 50th replayed step eagerly and samples
launches with HIP events, as the kernel-class profile needs):
  roofline       -- the kernel CLASS with the largest share of kernel time (live HIP-event sampling of every 32nd launch of
                    every C-ABI function inside the timed region, bdm_amd/profiling.py): achieved = algorithmic FLOPs (or
                    bytes) of its launches / their summed duration, against the peak that bounds it (dense 16-bit MFMA peak
                    / 3 partial products for the fp16x3 convolution); `kernel` names the heaviest (function, shape) row of
                    the class, whose avg_launch_us is the number to compare with the rocprofv3 summary under profiles/.
                    `traffic` comes from the committed PMC pass profiles/r0N_pmc_traffic.json (newest round first; separate rocprofv3 --pmc runs of one
                    forward, same kernel; `traffic_commit` = the commit it was measured at -- not measured inside this run).
  roofline_table -- every kernel class: share of kernel time, launches, achieved vs peak.
  cpu_baseline   -- the CPU oracle ("port": oracle/ref_net.py + oracle/pvcnn_ops_ref.c, the reference has no CPU
                    path) timed on this box's host cores on a bounded sample and extrapolated to a trajectory.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md, "Peak BF16/FP16 MFMA ~2.5 PF dense"
CONV_IMPL = os.environ.get("BDM_CONV", "fp16x3")
SPLIT_PRODUCTS = 3 if CONV_IMPL == "fp16x3" else 6  # 16-bit MFMA products issued per fp32 multiply-add by the convolution
MILESTONES = [1000, 968, 936, 872, 128, 64, 32, 0]


def host_cores():
    """CPUs this process may actually use: min(affinity mask, cgroup v2 cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(model, pvd_model, n_points, budget_s=25.0):
    """Oracle ("port") timed on the host cores: PC^2 and PVD denoiser forwards + scheduler steps at B = 1."""
    from oracle import ref_net, ref_sampler
    cores = host_cores()
    torch.set_num_threads(cores)
    sd_pc2 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    sd_pvd = {k: v.detach().cpu() for k, v in pvd_model.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, n_points, 3, generator=g) * 0.5
    feats = torch.randn(1, n_points, 387, generator=g)
    x_in = torch.cat([x, feats], dim=2)
    t = torch.tensor([500])
    ddpm, gd = ref_sampler.RefDDPM(), ref_sampler.RefPVDDiffusion()

    def pc2_step():
        eps = ref_net.point_cloud_model_forward(sd_pc2, x_in, t, prefix="point_cloud_model.model.")
        return ddpm.step(eps, 500, x, torch.zeros_like(x))

    def pvd_step():
        xp = x.permute(0, 2, 1).contiguous()
        eps = ref_net.pvcnn_forward(sd_pvd, xp, t, prefix="model.module.")
        return gd.step(eps, 500, xp, torch.zeros_like(xp))

    def timed(fn, budget):
        fn()  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            el = time.perf_counter() - t0
            if el > budget or n >= 20:
                return el / n, n

    s_pc2, n_pc2 = timed(pc2_step, budget_s * 0.6)
    s_pvd, n_pvd = timed(pvd_step, budget_s * 0.3)
    t_shape = 1000 * s_pc2 + 80 * s_pvd
    return {"value": 1.0 / t_shape, "unit": "shapes/s", "cores": cores, "kind": "port",
            "sample": f"{n_pc2} PC2 + {n_pvd} PVD denoiser steps at B=1, N={n_points} (denoiser forward + scheduler step; "
                      f"projection conditioning excluded); {s_pc2:.3f} s / {s_pvd:.3f} s per step, EXTRAPOLATED to "
                      f"1000 PC2 + 80 PVD steps per shape",
            "s_per_pc2_step": s_pc2, "s_per_pvd_step": s_pvd}


def c1_full(device, n_points=1024, steps=100):
    """Config C1 (BASELINE.json configs[0], the reference's own CPU-runnable case) IN FULL on both sides: vanilla PC^2
    sampling of one shape, 100 DDPM steps with projection conditioning at every step (image encoder hoisted on both
    sides).  Returns seconds per trajectory: HIP path on the GPU, CPU oracle on the host cores."""
    from bdm_amd.cameras import join_cameras
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.model import get_model
    from bdm_amd.utils.procedural import fill_module_
    from oracle import ref_net, ref_sampler as R, ref_vit
    cfg = ProjectConfig()
    cfg.dataset.max_points = n_points
    model = fill_module_(get_model(cfg).eval(), seed=11)
    batch = next(iter(SyntheticShapes(range(1), 1, seed=5, image_size=224, num_points=n_points)))
    ts = list(range(1000 - 1000 // steps, -1, -(1000 // steps)))
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(1, n_points, 3, generator=g)
    noise = {t: torch.randn(1, n_points, 3, generator=g) for t in ts}
    sd = model.state_dict()
    t0 = time.perf_counter()
    local = ref_vit.local_conditioning(sd, batch.image_rgb)
    cams = join_cameras(batch.camera).packed()
    ddpm, x = R.RefDDPM(), x0.clone()
    for t in ts:
        x_in = R.get_input_with_conditioning(x, cams, local)
        eps = ref_net.point_cloud_model_forward(sd, x_in, torch.full((1,), t), prefix="point_cloud_model.model.")
        x = ddpm.step(eps, t, x, noise[t] if t > 0 else None, prev_t=t - 1000 // steps)
    cpu_s = time.perf_counter() - t0
    model = model.to(device)
    b = batch.to(device)

    def gpu_run():
        model._cond_cache = None
        return model.forward_sample(num_points=n_points, camera=b.camera, image_rgb=b.image_rgb, mask=None,
                                    scheduler="ddpm", num_inference_steps=steps)
    gpu_run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = gpu_run()
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    assert torch.isfinite(out.points_padded()).all() and torch.isfinite(x).all()
    return {"workload": f"C1: vanilla PC2, 1 shape, N={n_points}, {steps} DDPM steps, conditioning every step", "gpu_s": gpu_s,
            "cpu_s": cpu_s, "speedup": cpu_s / gpu_s}


CONFIGS = {  # BASELINE.json configs[1..4] at their per-GPU share (batch / 8 GPUs)
    "c2": dict(kind="blending", points=4096, batch=16, label="C2: BDM-Blending, N=4096 pts, 1000 DDPM steps, batch=16 per GPU"),
    "c3": dict(kind="merging", points=4096, batch=16, label="C3: BDM-Merging, N=4096 pts, 1000 DDPM steps, batch=16 per GPU (128 over 8)"),
    "c4": dict(kind="blending", points=8192, batch=8, label="C4: BDM-Blending, N=8192 pts, 1000 DDPM steps, batch=8 per GPU (64 over 8)"),
    "c5": dict(kind="blending", points=16384, batch=32, label="C5: BDM-Blending, N=16384 pts, 1000 DDPM steps, batch=32 per GPU (256 over 8)"),
}


DUMP_MAX_BYTES = 64 * 2 ** 20


def dump_outputs(path, out, total_shapes, rank, world, dist_backend):
    """--dump-outputs: the final clouds of the last timed trajectory (what bdm_blending / bdm_merging hand their caller, as
    points_padded()) -> path/points.npy, float32, all ranks' shapes in global order.  Above DUMP_MAX_BYTES a fixed seeded
    sample of whole shapes (ascending global index) is written instead.  Collective: every rank calls it."""
    import numpy as np
    from bdm_amd.distributed import gather_clouds
    local = out.float() if dist_backend in (None, "nccl") else out.float().cpu()   # gloo gathers host tensors
    clouds = gather_clouds(local, total_shapes, rank, world).cpu()
    if rank != 0:
        return
    per_shape = clouds[0].numel() * 4
    if clouds.numel() * 4 > DUMP_MAX_BYTES:
        keep = max(1, DUMP_MAX_BYTES // per_shape)
        pick = torch.randperm(clouds.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values
        clouds = clouds[pick]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "points.npy"), clouds.numpy())


def self_launch(args):
    """`python bench.py --gpus N` without a torch.distributed.run environment: start the N workers ourselves (child processes, one
    rank per GPU over RCCL), BEFORE this process has touched a GPU, relay their output and exit with their status.  The reference
    shards with accelerator.prepare(dataloader) under `accelerate launch` (experiments/main_blending.py:115-124)."""
    import socket
    import subprocess
    env = dict(os.environ)
    have = torch.cuda.device_count()  # counting devices does not initialise the GPU
    if have < args.gpus:
        if env.get("BDM_SHARE_GPU") != "1":
            print(f"bench.py: --gpus {args.gpus} but only {have} GPU(s) visible (BDM_SHARE_GPU=1 runs the ranks on one GPU over gloo: "
                  "a functional check, not a measurement)", file=sys.stderr)
            return 2
        env.setdefault("BDM_DIST_BACKEND", "gloo")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in proc.stdout.splitlines():
        if ln not in lines:
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or len(lines) != 1:
        print(f"bench.py: worker group failed (exit {proc.returncode}, {len(lines)} result lines)", file=sys.stderr)
        return proc.returncode or 1
    print(lines[0], flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1, help="timed trajectories (each = 1000 DDPM steps of a 16-shape batch)")
    ap.add_argument("--warmup", type=int, default=0, help="untimed trajectories before the timed ones")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2", help="BASELINE.json configuration (default c2: the metric's)")
    ap.add_argument("--batch", type=int, default=None, help="shapes per GPU (default: the configuration's)")
    ap.add_argument("--points", type=int, default=None, help="points per shape (default: the configuration's)")
    ap.add_argument("--ddpm-steps", type=int, default=1000, help="ONLY for smoke runs; any value != 1000 marks the line invalid")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out cpu_baseline (and its c1_full)")
    ap.add_argument("--full", action="store_true",
                    help="also profile the timed region by kernel class and report roofline figures and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed trajectory's clouds to DIR/points.npy (float32)")
    args = ap.parse_args()
    conf = CONFIGS[args.config]
    custom = (args.batch is not None and args.batch != conf["batch"]) or (args.points is not None and args.points != conf["points"])
    args.batch = conf["batch"] if args.batch is None else args.batch
    args.points = conf["points"] if args.points is None else args.points
    merging = conf["kind"] == "merging"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    from bdm_amd import _lib
    from bdm_amd.config import ProjectConfig
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.distributed import barrier, init_from_env, max_over_ranks, per_rank_values, pin_to_gpu_numa_node, shard_indices
    from bdm_amd.model import get_fusion_model, get_model
    from bdm_amd.pvd import prepare_pvd_model
    from bdm_amd.sampling import batch_streams, bdm_blending, bdm_merging, count_forwards
    from bdm_amd.utils.procedural import fill_module_

    # before anything touches the GPU: this worker onto the host cores next to ITS GPU (no-op when the topology cannot be read)
    lr_env = 0 if os.environ.get("BDM_SHARE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    affinity = pin_to_gpu_numa_node(lr_env) if os.environ.get("BDM_PIN_NUMA", "1") == "1" else {"numa_node": None, "why": "BDM_PIN_NUMA=0"}
    rank, local_rank, world = init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    rccl_ranks = torch.distributed.get_world_size() if world > 1 else 1  # the world size the process group really has
    dist_backend = torch.distributed.get_backend() if world > 1 else None
    if os.environ.get("BDM_SHARE_GPU") == "1":  # test aid: every rank on cuda:0 (with BDM_DIST_BACKEND=gloo) on a 1-GPU box
        local_rank = 0
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    _lib.lib()  # fail loudly if the HIP extension is missing

    cfg = ProjectConfig()
    cfg.dataset.max_points = args.points
    cfg.aux_run.roll_step = 16
    if args.ddpm_steps == 1000:
        cfg.aux_run.milestones = MILESTONES
    else:  # smoke only: a short schedule with one coupling point (recon + prior branch + blend)
        s = args.ddpm_steps
        cfg.aux_run.milestones, cfg.aux_run.roll_step = [1000, 1000 - s // 3, 1000 - 2 * s // 3, 1000 - s], 1
    torch.manual_seed(cfg.run.seed + rank)
    model = fill_module_(get_model(cfg).eval(), seed=cfg.run.seed).to(device)
    pvd_model = prepare_pvd_model({"model": None, "nc": 3, "embed_dim": 64, "attention": True, "dropout": 0.1}, device)
    fusion = None
    if merging:  # PVCNN_fuse over copies of both denoisers (main_merging.py:565-575); the "zero convolutions" get procedural weights
        fusion = get_fusion_model(cfg, pvd_model, model)
        fill_module_(fusion.fusion_model.model.projs, seed=cfg.run.seed + 2, prefix="projs.")
        fill_module_(fusion.feature_model, seed=cfg.run.seed, prefix="feature_model.")
        fusion = fusion.eval().to(device)
    total_shapes = args.batch * world
    batch = next(iter(SyntheticShapes(shard_indices(total_shapes, rank, world), args.batch, seed=cfg.run.seed,
                                      image_size=224, num_points=args.points))).to(device)
    cfg.run.rng = "per_shape"  # every draw from the shapes' own Philox streams keyed by (seed, GLOBAL shape index): the
    counter = [0]              # samples do not depend on the number of ranks

    def sample(c, **kw):
        if merging:
            return bdm_merging(None, batch, c, pvd_model, model, fusion, **kw)
        return bdm_blending(None, batch, c, model, pvd_model, **kw)

    def trajectory():
        model._cond_cache = None  # the hoisted image encoder runs once per trajectory, inside the timed region
        if fusion is not None:
            fusion._cond_cache = None
        counter[0] += 1
        return sample(cfg, streams=batch_streams(cfg, batch, device, sample_idx=counter[0])).points_padded()

    # prime allocator / code objects (not a "step": a 2-forward schedule)
    prime_cfg = ProjectConfig()
    prime_cfg.dataset.max_points = args.points
    prime_cfg.aux_run.milestones, prime_cfg.aux_run.roll_step = ([1000, 996, 993, 990], 2) if merging else ([1000, 998, 996], 1)
    prime_cfg.run.rng = "per_shape"
    sample(prime_cfg)
    for _ in range(args.warmup):
        trajectory()

    prof = None
    if args.full:
        model.eager_probe_every = 50  # replayed loops (launch tape, BDM_GRAPH=1): every 50th step runs eagerly so that single launches
                                      # can be timed; the profiler counts each of its launches 50 times (profiling.PROBE_WEIGHT)
        pvd_model.eager_probe_every = model.eager_probe_every   # (the prior's replayed loop likewise: pvd.Model._gen_samples_tape)
        from bdm_amd.profiling import KernelClassProfiler
        prof = KernelClassProfiler(every=4).install()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = trajectory()
    torch.cuda.synchronize()
    own = time.perf_counter() - t0                      # this rank's own work, BEFORE the closing barrier equalises the clocks
    barrier()
    mine = time.perf_counter() - t0
    elapsed = max_over_ranks(mine, device)
    per_rank_s = per_rank_values(own, device)           # after the timed region: which rank was the slow one, and by how much
    per_rank_numa = per_rank_values(float(-1 if affinity.get("numa_node") is None else affinity["numa_node"]), device)
    if prof is not None:
        prof.remove()
    assert torch.isfinite(out).all()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, total_shapes, rank, world, dist_backend)

    if rank == 0:
        pc2_f, pvd_f, fuse_f = count_forwards(cfg.aux_run.milestones, cfg.aux_run.roll_step, merging=merging)
        value = total_shapes * args.steps / elapsed
        line = {
            "metric": f"sampled shapes/sec ({args.points} pts, 1000 DDPM steps)", "value": value, "unit": "shapes/s",
            "n_gpus": world, "rccl_ranks": rccl_ranks, "dist_backend": dist_backend, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed * 1e3 / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "per_rank_s": [round(v, 4) for v in per_rank_s], "rank_spread": max(per_rank_s) / max(min(per_rank_s), 1e-9),
            "per_rank_numa_node": [int(v) for v in per_rank_numa], "affinity_rank0": affinity,
            "rng": "per-shape Philox4x32-10 streams keyed by (seed, global shape index), noise generated inside the step kernels",
            "conv_arithmetic": CONV_IMPL + (" (fp32-grade: operands as two fp16 terms after power-of-two scaling, three partial "
                                                    "products, fp32 accumulate; first conv of each PVConv: on the occupied voxels only -- fp16x3 (list kernel or 8^3 GEMM) or "
                                                    "bf16x6 (exact 3-way bf16 split, six products: the GEMM + gather form a layer takes when the batch is too "
                                                    "small for the list kernel, ops.sparse_dil_pays), or the hoisted fp32 map at SA0.0)"
                                                    if CONV_IMPL == "fp16x3" else " (fp32-grade: exact 3-way bf16 operand split, "
                                                    "six partial products, fp32 accumulate)"),
            "config": {"workload": conf["label"] + ", synthetic R2N2-style inputs, procedural random-init PC2 + PVD"
                                   + (" + fusion" if merging else "") + " weights",
                       "name": args.config, "shapes_per_gpu": args.batch, "points": args.points, "pc2_forwards": pc2_f,
                       "pvd_forwards": pvd_f, "fusion_forwards": fuse_f,
                       "milestones": cfg.aux_run.milestones, "roll_step": cfg.aux_run.roll_step},
        }
        if args.ddpm_steps != 1000 or custom:
            line["invalid"] = "smoke / custom configuration: not one of BASELINE.json's workloads"
        elif args.config != "c2":
            line["note"] = "not the headline workload (the metric is quoted on C2); same trajectory definition at this configuration's size"
        if args.full:  # kernel-class profile of the timed region, roofline figures (after the timed region)
            # occupied fraction of the sparse convolutions' rows on the final clouds (after the timed region), per level
            from bdm_amd import functional as BF, ops as bops, profiling
            # ... on the clouds the trajectory ENDS with and on clouds like the ones it STARTS with (centred Gaussian noise): the listed
            # fraction of the grid shrinks as the cloud condenses, the mean of the two ends prices the kernels of the whole trajectory
            ends = [out.transpose(1, 2).contiguous(), torch.randn(out.shape[0], 3, args.points, device=out.device)]
            ends[1] = ends[1] - ends[1].mean(dim=2, keepdim=True)
            acc_occ, acc_dil = {}, {}
            for pts in ends:
                for r_, n_ in ((32, args.points), (16, 1024), (8, 256), (8, 64)):
                    if pts.shape[2] > n_:
                        pts = BF.furthest_point_sample(pts, n_)
                    bops.clear_plan_cache()
                    plan = bops.voxel_plan(pts, r_, dilate=2 if r_ in (16, 32) else 0)
                    acc_occ.setdefault(plan.n_max, []).append(float(plan.n_occ.float().mean()) / plan.n_max)
                    if getattr(plan, "d2_tiles", None) is not None:   # once- / twice-dilated fraction of the grid: what the list convolutions compute
                        d1 = float(plan.tile_start[:, :, 1].max(dim=1).values.float().mean()) / r_ ** 3
                        d2 = float(plan.d2_tiles[:, :, 1].max(dim=1).values.float().mean()) / r_ ** 3
                        acc_dil.setdefault(r_, []).append((d1, d2))
            for k, v in acc_occ.items():
                profiling.OCCUPANCY[k] = sum(v) / len(v)
            for k, v in acc_dil.items():
                profiling.DILATED[k] = (sum(a for a, _ in v) / len(v), sum(b for _, b in v) / len(v))
                line.setdefault("dilated_fraction_final_and_initial", {})[str(k)] = [[round(a, 4), round(b, 4)] for a, b in v]
            rows, classes = prof.table()
            if classes:
                # dominant class of the MAIN stream: the furthest-point sampler runs concurrently on its own stream (a chain of M - 1
                # dependent rounds on one CU per shape: neither a bandwidth nor a matrix kernel); it is listed in roofline_table
                top = next((c for c in classes if c["class"] != "furthest point sampling"), classes[0])
                top_rows = [r for r in rows if r["class"] == top["class"]]
                head = top_rows[0]
                traffic, traffic_commit = None, None
                try:  # HBM bytes per launch of that kernel from the committed PMC pass (separate rocprofv3 --pmc runs)
                    pm_path = next(p for p in (os.path.join(ROOT, "profiles", f) for f in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json")) if os.path.exists(p))
                    pm = json.load(open(pm_path))
                    key = f"{head['function']}{tuple(head['shape'])}"
                    ent = (pm["kernels"].get(key) or pm["kernels"].get(key.replace("_h2_gn(", "_h2("))  # same kernels + GN epilogue
                           or pm["kernels"].get(key.replace("_gather_gn(", "_gather(")))
                    if ent:
                        traffic, traffic_commit = ent["bytes_per_launch"], pm.get("commit")
                except (OSError, KeyError, ValueError, StopIteration):
                    pass
                own = profiling.row_fraction(head) or (top["bound"], top["achieved"], top["peak"], top["unit"], top["frac"])
                line["roofline"] = {"bound": own[0], "achieved": own[1], "peak": own[2], "unit": own[3],
                                    "frac": own[4], "traffic": traffic, "traffic_commit": traffic_commit,
                                    "kernel_class": top["class"], "class_frac": top["frac"], "share_of_kernel_time": top["share"],
                                    "kernel": f"{head['function']}{tuple(head['shape'])}", "avg_launch_us": head["avg_us"],
                                    "launches_timed": sum(r["sampled"] for r in top_rows),
                                    "launches_total": sum(r["calls"] for r in top_rows),
                                    "note": "`kernel` = the heaviest (function, shape) row of the class with the largest share of kernel time; achieved / "
                                            "frac are THAT kernel's own (its algorithmic flops per launch / its average launch duration); class_frac = the "
                                            "whole class (list convolutions priced by the matrix work they issue: listed voxels x 27 taps); durations: (HIP events on the launching stream around every 4th launch of the eagerly run steps: every "
                                            "50th PC2 step of the replayed loop and the PVD / fusion forwards); the sampler stream's class is excluded; for the "
                                            "fp16x3 convolution every fp32 product is 3 fp16 MFMA products: peak = 2500 TFLOP/s / 3"}
                line["roofline"]["sparse_rows_occupied_fraction"] = {str(k): round(v, 4) for k, v in profiling.OCCUPANCY.items()}
                line["roofline"]["dilated_fraction_of_grid"] = {str(k): [round(v[0], 4), round(v[1], 4)] for k, v in profiling.DILATED.items()}
                line["roofline_table"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in c.items()} for c in classes]
                def _own(r):
                    f = profiling.row_fraction(r)
                    return {} if f is None else {"bound": f[0], "frac": round(f[4], 4)}
                line["roofline_rows"] = [dict({"kernel": f"{r['function']}{tuple(r['shape'])}", "class": r["class"], "share": round(r["share"], 4),
                                               "avg_us": round(r["avg_us"], 2), "launches": r["calls"]}, **_own(r)) for r in rows[:12]]
                # north-star target g1 (">= 40 % of the HBM roofline on the ball-query / gather kernel"): the first set-abstraction level
                # (n points -> 1024 centres x 32 neighbours) from the in-run events of THIS run -- the query priced against the VALU issue rate
                # that bounds it (profiling.VALU_TESTS_PEAK) and against HBM, the grouping gather (point-major repack + gather: one ABI call,
                # two launches) against HBM, and the pair against HBM (SURVEY.md 8d byte formula of the pair)
                def _row(fn, pred):
                    return next((r for r in rows if r["function"] == fn and pred(r["shape"])), None)
                bq = _row("bdm_ball_query", lambda sh: sh[1] == args.points and sh[2] == 1024)
                sg = _row("bdm_sa_group", lambda sh: sh[2] == args.points and sh[3] == 1024)
                fused = _row("bdm_sa_mlp2_fused", lambda sh: sh[2] == args.points and sh[3] == 1024)
                in_path = sg is not None
                if bq and sg is None and fused is not None:
                    # round 4: the first level's grouped MLP re-gathers the neighbours' rows inside its three passes (bdm_sa_mlp2_fused), so
                    # the standalone gather no longer runs there.  It still ships (levels 1-3, and level 0 with BDM_SA_FUSED=0): timed here
                    # OUTSIDE the timed region on the level-0 shape, 20 launches between two events on the launching stream.
                    b_, c_, n_, m_, u_ = fused["shape"][:5]
                    gq = torch.Generator().manual_seed(1)
                    pts_ = out.transpose(1, 2).contiguous()   # the final clouds of this run (the neighbourhoods the path sees)
                    fts_ = torch.randn(b_, c_, n_, generator=gq).to(device)
                    cen_ = BF.furthest_point_sample(pts_, m_)
                    idx_ = BF.ball_query(cen_, pts_, 0.1, u_)
                    for _ in range(3):
                        bops.sa_group(pts_, cen_, fts_, idx_)
                    e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0_.record()
                    for _ in range(20):
                        bops.sa_group(pts_, cen_, fts_, idx_)
                    e1_.record()
                    torch.cuda.synchronize()
                    sg = {"shape": (b_, c_, n_, m_, u_), "avg_us": e0_.elapsed_time(e1_) / 20 * 1e3}
                if bq and sg:
                    b_, c_, n_, m_, u_ = sg["shape"][:5]
                    gather_bytes = 4.0 * b_ * ((3 + c_) * n_ + m_ * u_ + (c_ + 3) * m_ * u_)
                    query_bytes = 4.0 * b_ * (3 * n_ + 3 * m_ + m_ * u_)
                    tests = 1.0 * b_ * m_ * n_
                    line["g1_ball_query_and_grouping"] = {
                        "level": f"SA0: {b_} x {n_} points -> {m_} centres x {u_} neighbours, {c_} feature channels",
                        "grouping_gather": {"kernel": f"bdm_sa_group{tuple(sg['shape'])}", "avg_us": round(sg["avg_us"], 2), "in_timed_path": in_path,
                                            "algorithmic_mb": round(gather_bytes / 2 ** 20, 1), "achieved_gbs": round(gather_bytes / sg["avg_us"] / 1e3, 1),
                                            "hbm_frac": round(gather_bytes / sg["avg_us"] / 1e3 / profiling.HBM_PEAK_GBS, 3)},
                        "ball_query": {"kernel": f"bdm_ball_query{tuple(bq['shape'])}", "avg_us": round(bq["avg_us"], 2),
                                       "distance_tests_g": round(tests / 1e9, 3), "achieved_gtests_s": round(tests / bq["avg_us"] / 1e3, 1),
                                       "valu_frac": round(tests / bq["avg_us"] / 1e3 / profiling.VALU_TESTS_PEAK, 3),
                                       "hbm_frac": round(query_bytes / bq["avg_us"] / 1e3 / profiling.HBM_PEAK_GBS, 4)},
                        "pair_hbm_frac": round((gather_bytes + query_bytes - 4.0 * b_ * m_ * u_) / (sg["avg_us"] + bq["avg_us"]) / 1e3 / profiling.HBM_PEAK_GBS, 3),
                        "note": "the query is bound by VALU issue (6.7 instructions per distance test), not by its 3 MB of traffic; the gather meets "
                                "the 40 % target on its own, the pair cannot by memory tuning (DESIGN.md 7.6)"}
                    # the pair that DOES run inside the timed region: set-abstraction level 1 (n / 4 points -> n / 16 centres), ball query on the
                    # sampler's stream + the grouping gather from LDS-staged channel rows (round 6: sa_group_lds_kernel) on the main stream
                    bq1 = _row("bdm_ball_query", lambda sh: sh[1] == args.points // 4 and sh[2] == args.points // 16)
                    sg1 = _row("bdm_sa_group", lambda sh: sh[2] == args.points // 4 and sh[3] == args.points // 16)
                    if bq1 and sg1:
                        b1_, c1_, n1_, m1_, u1_ = sg1["shape"][:5]
                        pair_bytes = 4.0 * b1_ * (3 * n1_ + 3 * m1_ + c1_ * n1_ + m1_ * u1_ + (c1_ + 3) * m1_ * u1_)
                        gather1 = 4.0 * b1_ * ((3 + c1_) * n1_ + m1_ * u1_ + (c1_ + 3) * m1_ * u1_)
                        line["g1_ball_query_and_grouping"]["in_path_pair_level1"] = {
                            "level": f"SA1: {b1_} x {n1_} points -> {m1_} centres x {u1_} neighbours, {c1_} feature channels", "in_timed_path": True,
                            "ball_query_us": round(bq1["avg_us"], 2), "grouping_gather_us": round(sg1["avg_us"], 2),
                            "algorithmic_mb": round(pair_bytes / 2 ** 20, 1),
                            "gather_hbm_frac": round(gather1 / sg1["avg_us"] / 1e3 / profiling.HBM_PEAK_GBS, 3),
                            "pair_hbm_frac": round(pair_bytes / (bq1["avg_us"] + sg1["avg_us"]) / 1e3 / profiling.HBM_PEAK_GBS, 3),
                            "note": "both kernels timed by the in-run events of the timed region; why the pair stays below 0.40 at every level: "
                                    "profiles/r06_g1_query_and_gather.txt (the gather alone is write-bound at 0.41 - 0.49)"}
                    if fused is not None:
                        fb_, fc_, fn_, fm_, fu_, f1_, f2_ = fused["shape"][:7]
                        flops_ = 2.0 * fb_ * fm_ * fu_ * ((3 + fc_) * f1_ + f1_ * f2_)
                        line["g1_ball_query_and_grouping"]["fused_grouped_mlp"] = {
                            "kernel": f"bdm_sa_mlp2_fused{tuple(fused['shape'])}", "avg_us": round(fused["avg_us"], 2),
                            "algorithmic_gflop": round(flops_ / 1e9, 2), "achieved_tflops": round(flops_ / fused["avg_us"] / 1e6, 1),
                            "fp32_mfma_frac": round(flops_ / fused["avg_us"] / 1e6 / FP32_MFMA_PEAK_TFLOPS, 3),
                            "bytes_not_moved_mb": round(4.0 * fb_ * fm_ * fu_ * (2 * (3 + fc_) + 2 * f1_ + f2_) / 2 ** 20, 1),
                            "note": "grouping + 2-layer SharedMLP + max over neighbours in four launches (row repack + three recompute passes): the "
                                    "grouped tensor and both layer outputs (bytes_not_moved_mb: each written once and read once by the operator chain) "
                                    "never exist; replaces sa_group + two 1x1 GEMMs + the folded max at this level (204 -> 112 us at B = 16)"}
        # whole-path view: algorithmic FLOPs of SURVEY.md 8d per trajectory
        tflop_per_shape = (pc2_f * 103.64 + pvd_f * 81.22) / 1e3 if args.points == 4096 and not merging else None
        if tflop_per_shape:
            line["path_tflops"] = value * tflop_per_shape
            line["path_frac_of_fp32_mfma_peak"] = value * tflop_per_shape / (FP32_MFMA_PEAK_TFLOPS * world)
            # against the ceiling the split-precision kernels can reach: dense 16-bit MFMA peak / 3 products per fp32 product
            line["path_frac_of_fp16x3_peak"] = value * tflop_per_shape / (BF16_MFMA_PEAK_TFLOPS / 3 * world)
        if args.full and not args.no_cpu_baseline and world == 1 and args.config == "c2":
            line["cpu_baseline"] = cpu_baseline(model, pvd_model, args.points)
            line["speedup_vs_cpu_baseline"] = value / line["cpu_baseline"]["value"]
            line["cpu_baseline"]["c1_full"] = c1_full(device)  # the reference's CPU-runnable config, run in full on both sides
        print(json.dumps(line), flush=True)
    barrier()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
