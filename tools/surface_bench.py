"""Times the mesher (reconstruct_surface: bdm_surface_grid + bdm_surface_extract) beside the estimator whose
normals it consumes (bdm_estimate_normals at k = 50) on B = 16 clouds of N = 4096 points at R = 64 and of N = 16384 points at
R = 128, support 3.

HIP events around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows divided by the launches,
the functions alternating in one run (the figure to read is the ratio in the same run).  reconstruct_surface reads the counts
between its two ABI calls, so its window contains one host synchronisation per call; "grid" and "extract" time the two ABI calls
alone on preallocated outputs.  One JSON line.

    python tools/surface_bench.py [--repeats 7] [--launches 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import normals as N  # noqa: E402
from bdm_amd import surface as S  # noqa: E402


def window_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def shapes(b, n, generator):
    """b ellipsoids of random axes with their analytic outward normals."""
    d = torch.nn.functional.normalize(torch.randn(b, n, 3, device="cuda", generator=generator), dim=-1)
    axes = 0.2 + 0.3 * torch.rand(b, 1, 3, device="cuda", generator=generator)
    return (d * axes).contiguous(), torch.nn.functional.normalize(d / axes, dim=-1).contiguous()


def rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.lib()
    out = []
    for b, n, R, s in ((16, 4096, 64, 3), (16, 16384, 128, 3)):
        pts, nrm = shapes(b, n, gen)
        ws = torch.empty(lib.bdm_surface_workspace_bytes(b, n, R, s), dtype=torch.uint8, device="cuda")
        counts = torch.empty(b, 4, dtype=torch.int32, device="cuda")

        def grid():
            L.check(lib.bdm_surface_grid(b, n, R, s, 0.0, L.ptr(pts), L.ptr(nrm), L.ptr(counts), L.ptr(ws), L.stream()), "surface_grid")

        grid()
        host = counts.cpu()
        nv, nf = host[:, 0].long(), host[:, 1].long()
        offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).cuda()
        verts = torch.empty(int(nv.sum()), 3, dtype=torch.float32, device="cuda")
        faces = torch.empty(int(nf.sum()), 3, dtype=torch.int32, device="cuda")

        def extract():
            L.check(lib.bdm_surface_extract(b, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream()),
                    "surface_extract")

        calls = {"estimate_k50": lambda: N._estimate(pts, 50, N.ORIENT_CANONICAL, want_idx=True),
                 "reconstruct": lambda: S.reconstruct_surface(pts, nrm, resolution=R, support=s), "grid": grid, "extract": extract}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():                         # alternating: all see the same machine
                times[name].append(window_ms(fn, args.launches))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        out.append({"clouds": b, "points": n, "resolution": R, "support": s, "vertices": int(nv.sum()), "faces": int(nf.sum()),
                    "skipped_quads": int(host[:, 2].sum()), **{f"{name}_ms": round(v, 4) for name, v in med.items()},
                    "reconstruct_ms_min_max": [round(min(times["reconstruct"]), 4), round(max(times["reconstruct"]), 4)],
                    "reconstruct_over_estimate": round(med["reconstruct"] / med["estimate_k50"], 4),
                    "integer_atomics_per_s": 2 * b * n * (2 * s) ** 3 / (med["grid"] * 1e-3)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rows": rows(args)}))
