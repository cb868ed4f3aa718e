"""Prints g, the largest relative gap between the float32 and the float64 restatement of the approximate-match EMD over the case
list of tests/metrics_ref.py (each pair in natural and in reversed point order).  CPU only; the GPU test's tolerance is 32 g
(tests/test_hip_metrics.py: EMD_G).

    python tools/metrics_emd_gap.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import metrics_ref as R  # noqa: E402

if __name__ == "__main__":
    worst = 0.0
    for name, a, b in R.emd_case_pairs():
        r64, r32 = R.emd_approx_ref(a, b, np.float64), R.emd_approx_ref(a, b, np.float32)
        gap = abs(r32 - r64) / abs(r64)
        worst = max(worst, gap)
        print(f"{name:<18s} float64 {r64:.9f}  float32 {r32:.9f}  gap {gap:.3e}", flush=True)
    print(f"g = {worst:.3e}   32 g = {32 * worst:.3e}")
