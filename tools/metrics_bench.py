"""Times the generation-metric kernels on the GPU: pairwise_chamfer at S = R = 64, n = 2048 against the route
that existed before it (bdm_nn_sqdist twice on inputs expanded to (S R, n, 3), the expansion included), and pairwise_emd in pairs/s.
Median of the timed repeats, HIP events around each repeat, after warm-up.  Rates are set against the fp32 vector-issue peak
(256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-instructions/s; transcendentals issue at half of it).

    python tools/metrics_bench.py [--clouds 64] [--points 2048] [--repeats 10] [--emd-clouds 32]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import evaluation as E, metrics as M  # noqa: E402

VALU_PEAK = 256 * 4 * 32 * 2.4e9


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


def old_route(a, b):
    S, R, n = a.shape[0], b.shape[0], a.shape[1]
    ea = a[:, None].expand(S, R, n, 3).reshape(S * R, n, 3).contiguous()
    eb = b[None].expand(S, R, b.shape[1], 3).reshape(S * R, b.shape[1], 3).contiguous()
    return (E.nn_sqdist(ea, eb).mean(dim=1) + E.nn_sqdist(eb, ea).mean(dim=1)).view(S, R)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--emd-clouds", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    S, n = args.clouds, args.points
    gen = torch.Generator(device="cuda").manual_seed(0)
    a = 0.5 * torch.randn(S, n, 3, device="cuda", generator=gen)
    b = torch.rand(S, n, 3, device="cuda", generator=gen) * 2 - 1
    new_ms = median_ms(lambda: M.pairwise_chamfer(a, b), args.repeats)
    old_ms = median_ms(lambda: old_route(a, b), args.repeats)
    rel = float(((M.pairwise_chamfer(a, b) - old_route(a, b)).abs() / old_route(a, b)).max())
    dist = 2.0 * S * S * n * n                        # point-to-point distances of both directions
    e = args.emd_clouds
    emd_ms = median_ms(lambda: M.pairwise_emd(a[:e], b[:e]), args.repeats)
    pairs = e * e
    elems = pairs * 30.0 * n * n                      # ten levels x three passes over the n x n kernel matrix
    # instructions per element of the inner loops (ISA of csrc/metrics.hip): Chamfer 3.5 VALU per distance; EMD passes 1, 2: 4 VALU + 1 exp,
    # pass 3: 5.5 VALU + exp + sqrt; a transcendental costs two issue slots
    emd_slots = pairs * 10.0 * n * n * (2 * (4 + 2) + (5.5 + 4))
    out = {"clouds": S, "points": n,
           "chamfer_ms": round(new_ms, 3), "nn_sqdist_expanded_ms": round(old_ms, 3), "speedup": round(old_ms / new_ms, 2),
           "max_rel_difference_of_the_two_routes": rel,
           "expanded_copies_avoided_bytes": 2 * S * S * n * 12 + 2 * S * S * n * 4,
           "chamfer_distances_per_s": dist / (new_ms * 1e-3),
           "chamfer_valu_fraction": 3.5 * dist / (new_ms * 1e-3) / VALU_PEAK,
           "emd_clouds": e, "emd_ms": round(emd_ms, 3), "emd_pairs_per_s": round(pairs / (emd_ms * 1e-3), 1),
           "emd_exp_per_s": elems / (emd_ms * 1e-3), "emd_transcendental_fraction": (elems * 4.0 / 3.0) / (emd_ms * 1e-3) / (VALU_PEAK / 2),
           "emd_issue_fraction": emd_slots / (emd_ms * 1e-3) / VALU_PEAK}
    print(json.dumps(out))
