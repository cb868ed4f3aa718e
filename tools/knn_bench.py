"""Times bdm_knn_points and bdm_knn_interpolate.  Times as tools/normals_bench.py takes them: the median of
the timed calls, HIP events around each call, after warm-up; the yardstick is timed in the same run.  Every timing comes with its
spread (the fastest and the slowest of the timed calls), so that two medians can be told apart from run-to-run noise.

  Same-set case: B clouds searched against themselves (p1 = p2) at K = 50, beside bdm_estimate_normals on the same clouds: the new
    search does a strict subset of that kernel's work (the same scan and insertions, no covariance, no Jacobi).
  Colour-transfer workload: B meshes from reconstruct_surface at 64^3 of 4096-point clouds, the queries are the vertices, K = 3;
    the yardstick is torch.cdist + topk on the same GPU, entry by entry.  Then bdm_knn_interpolate (inverse squared distance, 3
    channels) on the result, against the bytes it must move.

    python tools/knn_bench.py [--batch 16] [--points 4096 16384] [--k 50] [--repeats 30]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402


def timed_ms(fn, repeats, warmup=3):
    """{"median", "min", "max"} in milliseconds of `repeats` calls between HIP events, after `warmup` calls."""
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
    times.sort()
    return {"median": round(times[len(times) // 2], 4), "min": round(times[0], 4), "max": round(times[-1], 4)}


def sphere_clouds(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, N, 3, generator=g)
    return (d / d.norm(dim=-1, keepdim=True) * (0.3 + 0.003 * torch.randn(B, N, 1, generator=g))).cuda()


def knn_call(queries, refs, q_first, r_first, k, idx, d2):
    lib = L.lib()
    B = q_first.numel() - 1
    ws = torch.empty(lib.bdm_knn_points_workspace_bytes(B, int(q_first[-1]), k), dtype=torch.uint8, device="cuda")

    def call():
        L.check(lib.bdm_knn_points(B, k, L.ptr(queries), L.ptr(refs), q_first.data_ptr(), r_first.data_ptr(), L.ptr(idx), L.ptr(d2),
                                   L.ptr(ws), L.stream()), "knn_points")
    return call


def same_set(B, N, k, repeats):
    pts = sphere_clouds(B, N)
    first = torch.arange(B + 1, dtype=torch.int64) * N
    idx = torch.empty(B * N, k, dtype=torch.int32, device="cuda")
    d2 = torch.empty(B * N, k, device="cuda")
    normals = torch.empty(B, N, 3, device="cuda")
    nidx = torch.empty(B, N, k, dtype=torch.int32, device="cuda")

    def normals_call():
        L.check(L.lib().bdm_estimate_normals(B, N, k, 0, L.ptr(pts), None, L.ptr(nidx), L.ptr(normals), None, None, L.stream()), "estimate_normals")
    # interleaved: knn, normals, knn again, so that a drift of the clocks shows as a difference between the two knn timings
    knn_a = timed_ms(knn_call(pts, pts, first, first, k, idx, d2), repeats)
    nrm = timed_ms(normals_call, repeats)
    knn_b = timed_ms(knn_call(pts, pts, first, first, k, idx, d2), repeats)
    same = bool(torch.equal(idx.view(B, N, k), nidx))
    return {"knn_points_ms": knn_a, "knn_points_again_ms": knn_b, "estimate_normals_with_idx_ms": nrm,
            "knn_over_normals": round(min(knn_a["median"], knn_b["median"]) / nrm["median"], 3), "same_indices_as_the_normals_kernel": same,
            "distance_evaluations": B * N * N, "distance_evaluations_per_s": B * N * N / (min(knn_a["median"], knn_b["median"]) * 1e-3),
            "bytes_that_must_move": B * N * (3 * 4 * 2 + k * 8)}


def colour_transfer(B, repeats, k=3, c=3):
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import reconstruct_surface
    pts = sphere_clouds(B, 4096, seed=1)
    verts, _ = reconstruct_surface(pts, estimate_pointcloud_normals(pts, 50, "visibility"), resolution=64)
    nv = [int(v.shape[0]) for v in verts]
    queries, refs = torch.cat(verts).contiguous(), pts.reshape(-1, 3).contiguous()
    q_first = torch.tensor([0] + nv, dtype=torch.int64).cumsum(0)
    r_first = torch.arange(B + 1, dtype=torch.int64) * 4096
    sum_p = int(q_first[-1])
    idx = torch.empty(sum_p, k, dtype=torch.int32, device="cuda")
    d2 = torch.empty(sum_p, k, device="cuda")
    knn = timed_ms(knn_call(queries, refs, q_first, r_first, k, idx, d2), repeats)

    def torch_knn():
        return [torch.cdist(v, p).topk(k, dim=1, largest=False) for v, p in zip(verts, pts)]
    yard = timed_ms(torch_knn, repeats)
    agree = sum(int((t.indices == i).sum()) for t, i in zip(torch_knn(), idx.long().split(nv))) / (sum_p * k)
    attr = ((refs + 1.0) / 2.0).contiguous()
    out = torch.empty(sum_p, c, device="cuda")
    lib = L.lib()
    ws = torch.empty(lib.bdm_knn_interpolate_workspace_bytes(B), dtype=torch.uint8, device="cuda")

    def interp():
        L.check(lib.bdm_knn_interpolate(B, k, c, 1, 1e-8, 0.5, L.ptr(attr), L.ptr(idx), L.ptr(d2), q_first.data_ptr(), r_first.data_ptr(),
                                        L.ptr(out), L.ptr(ws), L.stream()), "knn_interpolate")
    itp = timed_ms(interp, repeats)
    evals = sum(n * 4096 for n in nv)
    knn_bytes = sum_p * (12 + k * 8) + B * 4096 * 12
    itp_bytes = sum_p * (k * 8 + c * 4) + sum_p * k * c * 4       # lists in, colours out, one gathered row per neighbour
    return {"meshes": B, "vertices": sum_p, "vertices_per_mesh_min_max": [min(nv), max(nv)], "k": k,
            "knn_points_ms": knn, "torch_cdist_topk_ms": yard, "torch_over_kernel": round(yard["median"] / knn["median"], 2),
            "share_of_indices_equal_to_torch": round(agree, 6),
            "distance_evaluations": evals, "distance_evaluations_per_s": evals / (knn["median"] * 1e-3), "knn_bytes_that_must_move": knn_bytes,
            "knn_interpolate_ms": itp, "interpolate_bytes_that_must_move": itp_bytes,
            "interpolate_gb_per_s": round(itp_bytes / (itp["median"] * 1e-3) / 1e9, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"batch": args.batch, "k": args.k, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for N in args.points:
        out[f"same_set_n{N}"] = same_set(args.batch, N, args.k, args.repeats)
    out["colour_transfer"] = colour_transfer(args.batch, args.repeats)
    print(json.dumps(out))
