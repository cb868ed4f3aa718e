"""Times the occupancy-grid kernel behind the JSD measure: bdm_amd.metrics.occupancy_grid at S = 400 clouds of
N = 2048 points on the 28^3 sphere-clipped grid, once on clouds normalised to radius 0.5 (nearly every point rounds to a kept cell:
the fast path) and once on the same clouds normalised to radius 1 (most points lie outside the sphere: the slow path), each beside a
numpy restatement of the same two-path algorithm on the host's cores, with the share of points that took the slow path.
GPU times: median of the timed repeats, HIP events around each repeat, after warm-up; they include the wrapper's two range checks
and the gather of the kept cells.  `kernel_ms` times the bare C call.  The host restatement runs on `--host-clouds` clouds spread over
`--host-threads` threads and is scaled to S clouds (its cost is per cloud); its counts are compared with the kernel's on those clouds.

    python tools/metrics_jsd_bench.py [--clouds 400] [--points 2048] [--resolution 28] [--repeats 10] [--host-clouds 32] [--host-threads 16]
"""
import argparse
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L, metrics as M  # noqa: E402


def median_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return sorted(times)[len(times) // 2]


def host_cells(cloud, r, mask, kept_xyz, kept_flat):
    """Flat cell index of every point of one cloud, float32, fast path by rounding and slow path by brute force over the kept cells;
    also the number of slow points."""
    idx = np.clip(np.rint((cloud + np.float32(0.5)) * np.float32(r - 1)), 0, r - 1).astype(np.int64)
    flat = (idx[:, 0] * r + idx[:, 1]) * r + idx[:, 2]
    slow = np.flatnonzero(~mask[flat])
    for p0 in range(0, len(slow), 128):
        p = cloud[slow[p0:p0 + 128]]
        dx, dy, dz = (p[:, None, a] - kept_xyz[None, :, a] for a in range(3))
        flat[slow[p0:p0 + 128]] = kept_flat[((dx * dx + dy * dy) + dz * dz).argmin(axis=1)]
    return flat, len(slow)


def host_occupancy(clouds, r, threads):
    grid, _ = M.unit_cube_grid_point_cloud(r)
    flat_grid = grid.reshape(-1, 3)
    mask = np.linalg.norm(flat_grid, axis=1) <= 0.5
    kept_flat = np.flatnonzero(mask)
    kept_xyz = flat_grid[kept_flat]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        cells = list(pool.map(lambda c: host_cells(c, r, mask, kept_xyz, kept_flat), clouds))
    hits, active = np.zeros(r ** 3, dtype=np.int64), np.zeros(r ** 3, dtype=np.int64)
    for flat, _ in cells:
        per_cloud = np.bincount(flat, minlength=r ** 3)
        hits += per_cloud
        active += per_cloud > 0
    seconds = time.perf_counter() - t0
    return hits[kept_flat], active[kept_flat], sum(n for _, n in cells), seconds


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=400)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-clouds", type=int, default=32)
    ap.add_argument("--host-threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    warnings.simplefilter("ignore")   # radius 1 is outside cube and sphere on purpose
    S, N, r = args.clouds, args.points, args.resolution
    rng = np.random.Generator(np.random.PCG64(0))
    unit = M.normalize_unit_sphere(rng.uniform(-1.0, 1.0, (S, N, 3)).astype(np.float32))   # filled cubes, farthest corner at radius 1
    out = {"clouds": S, "points": N, "resolution": r, "host_clouds": min(args.host_clouds, S), "host_threads": args.host_threads}
    for name, clouds in (("radius_0.5", (unit * np.float32(0.5))), ("radius_1", unit)):
        d = torch.from_numpy(clouds).cuda()
        axis, mask, kept = M._device_grid(r, True, d.device)
        raw = torch.empty(2, r ** 3, dtype=torch.int32, device=d.device)
        call = lambda: L.check(L.lib().bdm_occupancy_grid(S, N, r, L.ptr(d), L.ptr(axis), L.ptr(mask), L.ptr(raw[0]), L.ptr(raw[1]),
                                                          L.stream()), "occupancy_grid")
        kernel_ms = median_ms(call, args.repeats)
        gpu_ms = median_ms(lambda: M.occupancy_grid(d, r), args.repeats)
        h = min(args.host_clouds, S)
        hits, active, nslow, seconds = host_occupancy(clouds[:h], r, args.host_threads)
        g_hits, g_active = (t.cpu().numpy() for t in M.occupancy_grid(d[:h], r))
        rounded = torch.clamp(torch.round((d + 0.5) * (r - 1)), 0, r - 1).long()
        slow_share = 1.0 - float(mask[(rounded[..., 0] * r + rounded[..., 1]) * r + rounded[..., 2]].float().mean())
        out[name] = {"occupancy_grid_ms": round(gpu_ms, 3), "kernel_ms": round(kernel_ms, 3), "points_per_s": S * N / (kernel_ms * 1e-3),
                     "slow_path_share": round(slow_share, 4), "host_slow_path_share": round(nslow / (h * N), 4),
                     "host_numpy_ms_measured": round(seconds * 1e3, 1), "host_numpy_ms_scaled_to_all_clouds": round(seconds * 1e3 * S / h, 1),
                     "cells_where_host_and_gpu_hits_differ": int((hits != g_hits).sum()),
                     "cells_where_host_and_gpu_active_differ": int((active != g_active).sum())}
    print(json.dumps(out))
