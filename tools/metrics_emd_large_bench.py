"""Times the any-size approximate-match EMD kernel on the GPU: 32 x 32 pairs at n = 4096 (resident form),
16 x 16 at n = 8192 and at n = 16384 (streamed form) and, for scale, both kernels and both forms at n = 2048 on 32 x 32 pairs.
Median of the timed repeats, HIP events around each repeat, after warm-up, as tools/metrics_bench.py does.  Rates are set against the
fp32 vector-issue peak (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-instructions/s) with the per-element issue
slots of the old kernel's inner loops (passes 1, 2: 4 packed + exp, pass 3: 5.5 packed + exp + sqrt; a transcendental takes two slots).
One JSON line.

    python tools/metrics_emd_large_bench.py [--repeats 5] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import metrics as M  # noqa: E402

VALU_PEAK = 256 * 4 * 32 * 2.4e9
CUS = 256


def median_ms(fn, repeats, warmup=1):
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


def row(name, clouds, n, ms):
    pairs = clouds * clouds
    elems = pairs * 30.0 * n * n                                   # ten levels x three passes over the n x n kernel matrix
    slots = pairs * 10.0 * n * n * (2 * (4 + 2) + (5.5 + 4))
    rounds = -(-pairs // CUS)                                      # pairs one workgroup of the persistent grid walks
    return {"case": name, "clouds": clouds, "points": n, "ms": round(ms, 3), "pairs_per_s": round(pairs / (ms * 1e-3), 1),
            "ms_per_pair_and_cu": round(ms / rounds, 3), "exp_per_s": elems / (ms * 1e-3), "issue_fraction": round(slots / (ms * 1e-3) / VALU_PEAK, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="n = 2048 and 4096 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    gen = torch.Generator(device="cuda").manual_seed(0)

    def clouds(count, n):
        return 0.5 * torch.randn(count, n, 3, device="cuda", generator=gen), torch.rand(count, n, 3, device="cuda", generator=gen) * 2 - 1

    rows = []
    a, b = clouds(32, 2048)
    rows.append(row("pairwise_emd (old kernel)", 32, 2048, median_ms(lambda: M.pairwise_emd(a, b), args.repeats)))
    rows.append(row("pairwise_emd_large resident", 32, 2048, median_ms(lambda: M.pairwise_emd_large(a, b, mode=1), args.repeats)))
    rows.append(row("pairwise_emd_large streamed", 32, 2048, median_ms(lambda: M.pairwise_emd_large(a, b, mode=2), args.repeats)))
    a, b = clouds(32, 4096)
    rows.append(row("pairwise_emd_large resident", 32, 4096, median_ms(lambda: M.pairwise_emd_large(a, b), args.repeats)))
    rows.append(row("pairwise_emd_large streamed", 32, 4096, median_ms(lambda: M.pairwise_emd_large(a, b, mode=2), args.repeats)))
    if not args.quick:
        for n in (8192, 16384):
            a, b = clouds(16, n)
            rows.append(row("pairwise_emd_large streamed", 16, n, median_ms(lambda: M.pairwise_emd_large(a, b), args.repeats)))
    print(json.dumps({"rows": rows}))
