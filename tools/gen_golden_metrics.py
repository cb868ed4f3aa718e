"""Writes tests/golden/metrics_e2e.npz: the float64 Chamfer and approximate-match EMD matrices (sample x ref, sample x sample,
ref x ref) of the end-to-end case of tests/metrics_ref.py (E2E), from the CPU references alone (no kernel involved), and prints the
smallest relative best-to-second-best gap of each distance.  tests/test_hip_metrics.py needs that gap above 10 x its elementwise
bound; if it is not, choose other seeds in metrics_ref.E2E and run again.  Minutes of CPU.

    python tools/gen_golden_metrics.py [--jobs 8]
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_ref as R  # noqa: E402


def _emd_row(args):
    p, b = args
    return [R.emd_approx_ref(p, q) for q in b]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    jobs = ap.parse_args().jobs
    x, y = R.e2e_clouds()
    out = {}
    with Pool(jobs) as pool:
        for key, (a, b) in {"xy": (x, y), "xx": (x, x), "yy": (y, y)}.items():
            out[f"cd_{key}"] = R.chamfer_sum_matrix_ref(a, b)
            out[f"emd_{key}"] = np.array(pool.map(_emd_row, [(p, b) for p in a]))
    for d in ("cd", "emd"):
        print(d, "smallest relative gap", R.e2e_min_gap(out[f"{d}_xx"], out[f"{d}_xy"], out[f"{d}_yy"]))
    path = os.path.join(ROOT, "tests", "golden", "metrics_e2e.npz")
    np.savez_compressed(path, **out, **{k: np.int64(v) for k, v in R.E2E.items()})
    print("wrote", path)
