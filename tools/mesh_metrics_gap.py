"""Prints, per distance case of tests/mesh_metrics_ref.py, the largest gap between the float32 restatement of the point-to-face rule
(bdm_hip.h section 14) and the float64 evaluation of the same formulas on the same inputs, over every (point, valid face) pair with
a finite point: the largest absolute gap, and the largest gap relative to the float64 value over the pairs whose float64 value
is at least 1e-6.  CPU only, seconds.  tests/test_mesh_metrics_host.py asserts twice these figures (mesh_metrics_ref.GAP).

    python tools/mesh_metrics_gap.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mesh_metrics_ref as M  # noqa: E402

if __name__ == "__main__":
    print("GAP = {")
    for name in M.DIST_CASES:
        a, r, n = M.pair_gap(name)
        print(f'    "{name}": ({a:.3e}, {r:.3e}),   # {n} pairs')
    print("}")
