"""Times the alignment kernels.  Times as tools/knn_bench.py takes them: the median of the timed calls, HIP
events around each call, after warm-up, with the fastest and the slowest beside it; the composed route is timed in the same run.

  The match alone: bdm_align_moments (state, amax, one match, the copy of the moments), beside bdm_knn_points at K = 1.
  One iteration: bdm_icp_rounds with rounds = 1 (match + solve + the counter) on a state that bdm_icp_init wrote just before, so
    every timed call does the first iteration's work.  Beside it the composed route the repository offered before: bdm_knn_points at
    K = 1, a torch gather of the partners, float64 moments and torch.linalg.svd with the determinant correction, and the host
    read-back of the mean squared residual that its stopping test needs.  bdm_knn_points at K = 1 is also timed alone: the pair rate
    of the two searches.
  Full run: bdm_amd.alignment.iterative_closest_point, its read-backs included, with the iteration counts it took.

  Shapes: B = 16 entries of 4096 against 4096 points, and one entry of 16384 against 16384.

    python tools/align_bench.py [--repeats 30]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from tools.knn_bench import knn_call, timed_ms  # noqa: E402


def clouds(B, N, seed=0):
    """A box cloud per entry and a rotated (8 degrees about (1, 2, 3)), shifted, permuted copy with a little noise."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, N, 3, generator=g) - 0.5) * torch.tensor([1.0, 0.6, 0.3])
    a = [v / math.sqrt(14.0) for v in (1.0, 2.0, 3.0)]
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = math.radians(8.0)
    R = (torch.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)).T
    y = x @ R + torch.tensor([0.03, -0.02, 0.01]) + 0.002 * torch.randn(B, N, 3, generator=g)
    y = torch.stack([y[i, torch.randperm(N, generator=g)] for i in range(B)])
    return x.cuda().contiguous(), y.cuda().contiguous()


def shape(B, N, repeats):
    lib = L.lib()
    x, y = clouds(B, N)
    first = torch.arange(B + 1, dtype=torch.int64) * N
    xp, yp = x.view(-1, 3), y.view(-1, 3)
    ws = torch.empty(lib.bdm_align_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    active = torch.zeros(1, dtype=torch.int32, device="cuda")

    def init():
        L.check(lib.bdm_icp_init(B, L.ptr(xp), L.ptr(yp), first.data_ptr(), first.data_ptr(), None, L.ptr(ws), L.stream()), "icp_init")

    def fused():
        init()
        L.check(lib.bdm_icp_rounds(B, 1, 100, 0, 1e-6, 1e-9, L.ptr(xp), L.ptr(yp), first.data_ptr(), first.data_ptr(), None, L.ptr(active), L.ptr(ws),
                                   L.stream()), "icp_rounds")
        return int(active.item())   # the read-back of the loop

    moments = torch.empty(B, 18, dtype=torch.int64, device="cuda")

    def match_only():   # state, amax, one match and the copy of the moments: an iteration without solve, counter and read-back
        L.check(lib.bdm_align_moments(B, 0, L.ptr(xp), L.ptr(yp), first.data_ptr(), first.data_ptr(), None, L.ptr(moments), None, None, L.ptr(ws),
                                      L.stream()), "align_moments")

    idx = torch.empty(B * N, 1, dtype=torch.int32, device="cuda")
    d2 = torch.empty(B * N, 1, device="cuda")
    search = knn_call(xp, yp, first, first, 1, idx, d2)
    base = (torch.arange(B, device="cuda") * N)[:, None]

    def composed():
        search()
        part = yp[(idx.view(B, N).long() + base).view(-1)].view(B, N, 3).double()
        xd = x.double()
        mx, my = xd.mean(1, keepdim=True), part.mean(1, keepdim=True)
        M = (xd - mx).transpose(1, 2) @ (part - my) / N
        U, _, Vh = torch.linalg.svd(M)
        E = torch.eye(3, dtype=torch.float64, device="cuda").repeat(B, 1, 1)
        E[:, 2, 2] = torch.det(U @ Vh)
        R = U @ E @ Vh
        T = my[:, 0] - (mx @ R)[:, 0]
        mse = ((xd @ R + T[:, None] - part) ** 2).sum(-1).mean(1)
        return mse.cpu()   # the read-back of the stopping test

    init_ms = timed_ms(init, repeats)
    fused_a = timed_ms(fused, repeats)
    comp = timed_ms(composed, repeats)
    knn1 = timed_ms(search, repeats)
    match_ms = timed_ms(match_only, repeats)
    fused_b = timed_ms(fused, repeats)   # again: a drift of the clocks shows as a difference between the two

    from bdm_amd.alignment import iterative_closest_point
    sol = {}

    def full():
        sol["s"] = iterative_closest_point(x, y)
    full_ms = timed_ms(full, max(repeats // 3, 3), warmup=1)
    iters = len(sol["s"].t_history)
    best = min(fused_a["median"], fused_b["median"])
    pairs = B * N * N
    return {"entries": B, "points": N, "icp_init_ms": init_ms, "fused_iteration_with_init_ms": fused_a, "fused_iteration_with_init_again_ms": fused_b,
            "fused_iteration_ms": round(best - init_ms["median"], 4), "composed_iteration_ms": comp, "knn_points_k1_ms": knn1,
            "match_with_init_ms": match_ms, "pairs_per_s_match_with_init": pairs / (match_ms["median"] * 1e-3),
            "composed_over_fused": round(comp["median"] / (best - init_ms["median"]), 2), "pairs": pairs,
            "pairs_per_s_fused_iteration": pairs / ((best - init_ms["median"]) * 1e-3), "pairs_per_s_knn_points_k1": pairs / (knn1["median"] * 1e-3),
            "full_run_ms": full_ms, "full_run_iterations": iters, "full_run_converged": int(sol["s"].converged.sum())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"repeats": args.repeats, "device": torch.cuda.get_device_name(0), "b16_n4096": shape(16, 4096, args.repeats), "b1_n16384": shape(1, 16384, args.repeats)}
    print(json.dumps(out))
