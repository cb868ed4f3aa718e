"""Times one bdm_estimate_normals call at (B = 16, N = 4096, k = 50) and (B = 16, N = 16384, k = 50), beside
what a user would otherwise run on the same GPU: torch.cdist + topk + torch.linalg.eigh through PyTorch-ROCm, cloud by cloud (the
(N, N) distance matrix of all 16 clouds of 16384 points at once would be 17 GB).  There is no earlier implementation to compare
with.  Times: median of the timed repeats, HIP events around each repeat, after warm-up.  The torch path gets fewer repeats when
one takes long (its repeat count is reported).  Also printed: the bytes the call must move and the distance evaluations it makes,
computed from the shapes, and how far the two paths' normals are apart (they pick neighbours by different arithmetic).

    python tools/normals_bench.py [--batch 16] [--points 4096 16384] [--k 50] [--repeats 30]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402


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


def torch_normals(points, k):
    """cdist + topk + eigh, one cloud at a time: (B, N, 3) unit eigenvectors of the smallest eigenvalue (sign as eigh returns it)."""
    out = torch.empty_like(points)
    for b, p in enumerate(points):
        idx = torch.cdist(p, p).topk(k, dim=1, largest=False).indices
        e = p[idx] - p[:, None, :]
        d = e - e.mean(dim=1, keepdim=True)
        cov = torch.einsum("nki,nkj->nij", d, d) / k
        out[b] = torch.linalg.eigh(cov).eigenvectors[:, :, 0]
    return out


def sphere_clouds(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, N, 3, generator=g)
    return (d / d.norm(dim=-1, keepdim=True) * (0.3 + 0.003 * torch.randn(B, N, 1, generator=g))).cuda()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    B, k = args.batch, args.k
    out = {"batch": B, "k": k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for N in args.points:
        pts = sphere_clouds(B, N)
        normals = torch.empty(B, N, 3, device="cuda")
        curv = torch.empty(B, N, 3, device="cuda")
        idx = torch.empty(B, N, k, dtype=torch.int32, device="cuda")

        def call(with_all=False):
            L.check(L.lib().bdm_estimate_normals(B, N, k, 1, L.ptr(pts), None, L.ptr(idx) if with_all else None, L.ptr(normals),
                                                 L.ptr(curv) if with_all else None, None, L.stream()), "estimate_normals")

        kernel_ms = median_ms(call, args.repeats)
        kernel_all_ms = median_ms(lambda: call(True), args.repeats)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch_normals(pts, k)                                                # first call: library set-up, not timed
        t0.record()
        want = torch_normals(pts, k)
        t1.record()
        t1.synchronize()
        once_ms = t0.elapsed_time(t1)
        torch_repeats = max(3, min(args.repeats, int(15000.0 / max(once_ms, 1e-3))))
        torch_ms = median_ms(lambda: torch_normals(pts, k), torch_repeats, warmup=0)
        call()
        cross = torch.linalg.cross(normals, want).norm(dim=-1)
        out[f"n{N}"] = {
            "kernel_ms": round(kernel_ms, 3), "kernel_with_idx_and_curvatures_ms": round(kernel_all_ms, 3),
            "torch_cdist_topk_eigh_ms": round(torch_ms, 3), "torch_repeats": torch_repeats, "torch_over_kernel": round(torch_ms / kernel_ms, 2),
            "bytes_that_must_move": B * N * 3 * 4 * 2, "bytes_with_idx_and_curvatures": B * N * (3 * 4 * 3 + k * 4),
            "distance_evaluations": B * N * N, "distance_evaluations_per_s": B * N * N / (kernel_ms * 1e-3),
            "queries_per_s": B * N / (kernel_ms * 1e-3),
            "median_abs_cross_between_paths": float(cross.median()), "share_of_points_beyond_1e-3": float((cross > 1e-3).float().mean())}
    print(json.dumps(out))
