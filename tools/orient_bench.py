"""Times the visibility-voting orientation (bdm_orient_normals) beside the estimator it follows
(bdm_estimate_normals at k = 50) on B = 16 clouds of N = 4096 and N = 16384 points, default parameters (32 views, 128 x 128
z-buffer, splat 2, 8 fallback neighbours, 8 rounds), and the step's share of `python -m bdm_amd.normals` per file.

Kernel-side times: HIP events around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows
divided by the launches, the two functions alternating in one run (the figure to read is the ratio in the same run).  LDS atomics
counted from the shapes: n (2 splat + 1)^2 per cloud and view.  Per-file times: a host clock around process_tree's estimate_fn (it
ends in device-to-host copies), with and without the orientation, over a tree of `--files` synthetic clouds.  One JSON line.

    python tools/orient_bench.py [--repeats 7] [--launches 10] [--files 32]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import normals as N  # noqa: E402


def window_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def shapes(b, n, generator):
    """b closed surfaces of n points: ellipsoids of random axes (what the orientation is for; a Gaussian blob has no outside)."""
    d = torch.nn.functional.normalize(torch.randn(b, n, 3, device="cuda", generator=generator), dim=-1)
    return d * (0.2 + 0.3 * torch.rand(b, 1, 3, device="cuda", generator=generator))


def kernel_rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for b, n in ((16, 4096), (16, 16384)):
        pts = shapes(b, n, gen)
        normals, idx, _ = N._estimate(pts, 50, N.ORIENT_CANONICAL, want_idx=True)
        calls = {"estimate_k50": lambda: N._estimate(pts, 50, N.ORIENT_CANONICAL, want_idx=True),
                 "orient": lambda: N.orient_normals_by_visibility(pts, normals, idx)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():                         # alternating: both see the same machine
                times[name].append(window_ms(fn, args.launches))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        _, info = N.orient_normals_by_visibility(pts, normals, idx, return_info=True)
        atomics = b * 32 * n * 25
        rows.append({"clouds": b, "points": n, "estimate_k50_ms": round(med["estimate_k50"], 4), "orient_ms": round(med["orient"], 4),
                     "orient_ms_min_max": [round(min(times["orient"]), 4), round(max(times["orient"]), 4)],
                     "orient_over_estimate": round(med["orient"] / med["estimate_k50"], 4),
                     "lds_atomics_per_s": atomics / (med["orient"] * 1e-3), "undecided": int(info["undecided"].sum())})
    return rows


def per_file(args):
    from bdm_amd.io import save_pointcloud_ply
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for j, cloud in enumerate(shapes(args.files, 4096, gen).cpu().numpy()):
            save_pointcloud_ply(cloud, os.path.join(tmp, "in", f"{j:04d}.ply"))
        for orient in ("neighbours", "visibility", "neighbours", "visibility"):     # the first pair warms up, the second is kept
            spent = [0.0]

            def estimate_fn(points, orient=orient, spent=spent):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev = points.cuda()
                if orient == "visibility":
                    normals, idx, curv = N._estimate(dev, 50, N.ORIENT_CANONICAL, want_idx=True, want_curvatures=True)
                    normals, info = N.orient_normals_by_visibility(dev, normals, idx, return_info=True)
                    res = normals.cpu(), curv.cpu(), int(info["undecided"].sum())
                else:
                    normals, curv = N.estimate_pointcloud_normals(dev, 50, True, return_curvatures=True)
                    res = normals.cpu(), curv.cpu()
                spent[0] += time.perf_counter() - t0
                return res

            t0 = time.perf_counter()
            N.process_tree(os.path.join(tmp, "in"), os.path.join(tmp, "out_" + orient), estimate_fn, 16)
            out[orient] = {"gpu_step_ms_per_file": round(1e3 * spent[0] / args.files, 4),
                           "whole_ms_per_file": round(1e3 * (time.perf_counter() - t0) / args.files, 4)}
    extra = out["visibility"]["gpu_step_ms_per_file"] - out["neighbours"]["gpu_step_ms_per_file"]
    out["orientation_share_of_a_file"] = round(extra / out["visibility"]["whole_ms_per_file"], 4)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--files", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "kernels": kernel_rows(args),
                      "per_file_n4096_k50": per_file(args)}))
