"""Measures what tests/test_align_host.py bounds: the largest gap of R, T, s between the alignment solve's float32-rounded outputs
(the restatement tests/align_ref.py, which the kernel equals bit for bit) and the float64 SVD definition, over the test's own cases.
The near-reflection cases get a figure of their own (their smallest singular value is small, so the rotation is less well
determined); every other case shares one.  The test's constants are four times these figures.  No GPU needed.

    python tools/align_gap.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import align_ref as A   # noqa: E402


def main():
    gaps, sweeps = {}, {}
    for name, rows in A.solve_cases().items():
        gaps[name] = max(A.solve_gap(m, e, es, collinear=name == "collinear") for m, e, es in rows)
        worst = 0
        for m, e, _ in rows:   # the first sweep count after which the off-diagonal is below 1e-17 of the largest eigenvalue
            M = A.central_moments(m, e)[3]
            worst = max(worst, next((k for k in range(1, 21) if A.horn_rotation(M, k, return_offdiag=True)[1] < 1e-17), 21))
        sweeps[name] = worst
    out = {"gap": gaps, "gap_general": max(v for k, v in gaps.items() if k != "near_reflection"), "gap_near_reflection": gaps["near_reflection"],
           "sweeps_to_1e-17": sweeps}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
