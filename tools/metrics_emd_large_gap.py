"""Prints g_large, the largest relative gap between the float32 and the float64 row-blocked restatement of the approximate-match EMD
over the case list of tests/metrics_large_ref.py (every pair in natural and in reversed point order, n = 1 to 8192).  CPU only; the
GPU test's tolerance is 32 g_large (tests/test_hip_metrics_emd_large.py: EMD_G_LARGE).  Minutes of CPU.

    python tools/metrics_emd_large_gap.py [--jobs 4] [--max-n N]
"""
import argparse
import os
import sys
from multiprocessing import Pool

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import metrics_large_ref as LR  # noqa: E402


def _one(task):
    name, a, b = task
    g, r64 = LR.gap(a, b)
    return name, g, r64


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--max-n", type=int, default=None)
    args = ap.parse_args()
    tasks = sorted(LR.large_case_pairs(args.max_n), key=lambda t: -len(t[1]))   # longest first
    worst = 0.0
    with Pool(args.jobs) as pool:
        for name, g, r64 in pool.imap_unordered(_one, tasks, chunksize=1):
            worst = max(worst, g)
            print(f"{name:<18s} float64 {r64:.9f}  gap {g:.3e}", flush=True)
    print(f"g_large = {worst:.5e}   32 g_large = {32 * worst:.5e}")
