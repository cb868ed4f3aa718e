"""Writes tests/golden/metrics_emd_large.npz: the float64 approximate-match EMD of the "golden" cases of tests/metrics_large_ref.py
(n = 2600 to 8192: seconds to a minute per pair, too slow to restate inside the GPU suite), from the row-blocked CPU restatement
alone (no kernel involved).  The file holds numbers and seeds only: `cases` (n, s, r, seed) and one (s, r) matrix `emd_n<n>` each.
Minutes of CPU.

    python tools/gen_golden_metrics_emd_large.py [--jobs 4]
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_large_ref as LR  # noqa: E402
import metrics_ref as R  # noqa: E402


def _one(task):
    n, s, r, seed, i, j = task
    a, b = R.emd_case(n, s, r, seed)
    return LR.emd_approx_blocked(a[i], b[j], np.float64)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    jobs = ap.parse_args().jobs
    cases = [c[:4] for c in LR.LARGE_CASES if c[4] == "golden"]
    tasks = [(n, s, r, seed, i, j) for n, s, r, seed in cases for i in range(s) for j in range(r)]
    with Pool(jobs) as pool:
        values = dict(zip(tasks, pool.map(_one, tasks, chunksize=1)))
    out = {"cases": np.array(cases, dtype=np.int64)}
    for n, s, r, seed in cases:
        out[f"emd_n{n}"] = np.array([[values[(n, s, r, seed, i, j)] for j in range(r)] for i in range(s)])
        print(n, out[f"emd_n{n}"].tolist())
    path = os.path.join(ROOT, "tests", "golden", "metrics_emd_large.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)
