"""CPU reference and case list of the any-size approximate-match EMD (csrc/metrics_emd_large.hip, bdm_amd.metrics.pairwise_emd_large /
paired_emd); numpy only, owes nothing to a kernel.

* emd_approx_blocked: metrics_ref.emd_approx_ref restated over ROW BLOCKS of the n x n kernel matrix, so that n = 8192 needs
  block x n elements at a time and not n x n.  The blocks of d^2 are kept while they fit `cache_bytes` (n <= 4096 in float64)
  and recomputed per pass above it: the same values either way.  With one block it is emd_approx_ref operation for operation.
* LARGE_CASES: (n, s, r, seed, kind) on metrics_ref.emd_case inputs.  "live" cases are restated in float64 inside the GPU test,
  "golden" ones (seconds to a minute per pair) come from tests/golden/metrics_emd_large.npz (tools/gen_golden_metrics_emd_large.py).
  tools/metrics_emd_large_gap.py measures the float32-vs-float64 gap g_large on all of them.
"""
import numpy as np

import metrics_ref as R

# what bdm_pairwise_emd_large_variant reports for the streamed form; the GPU test pins the table through it
STAGE, THREADS, KPT = 1024, 512, 4
BOUNDARY_NS = (STAGE - 1, STAGE, STAGE + 1, THREADS * KPT - 1, THREADS * KPT + 1, 2049)   # 2049 = THREADS * KPT + 1 names one case

# g_large as tools/metrics_emd_large_gap.py measured it over LARGE_CASES, 1.33819e-6 at n256[0,1], rounded UP to four digits (the GPU
# bound is 32 g_large; the CPU suite re-measures the cases with n <= 2049)
EMD_G_LARGE = 1.339e-6

LARGE_CASES = [(n, s, r, seed, "live") for n, s, r, seed in R.EMD_CASES if n <= 1000]
LARGE_CASES += [(n, 1, 1, 300 + n, "live") for n in sorted(set(BOUNDARY_NS))]
LARGE_CASES += [(2600, 2, 2, 401, "golden"), (4096, 1, 1, 402, "golden"), (4097, 1, 1, 403, "golden"), (8192, 1, 1, 404, "golden")]


def large_case(n):
    """(a (s, n, 3), b (r, n, 3)) of the case with n points."""
    (n, s, r, seed, _), = [c for c in LARGE_CASES if c[0] == n]
    return R.emd_case(n, s, r, seed)


def large_case_pairs(max_n=None):
    """Every (name, a_i, b_j) of LARGE_CASES (n <= max_n), each in natural and in reversed point order."""
    for n, s, r, seed, _ in LARGE_CASES:
        if max_n is not None and n > max_n:
            continue
        a, b = R.emd_case(n, s, r, seed)
        for i in range(s):
            for j in range(r):
                yield f"n{n}[{i},{j}]", a[i], b[j]
                yield f"n{n}[{i},{j}]rev", a[i, ::-1], b[j, ::-1]


def emd_approx_blocked(a, b, dtype=np.float64, block=512, cache_bytes=1 << 28):
    """cost(a, b) / n of the approximate match, one block of `block` rows of the match matrix at a time."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    n = a.shape[0]
    assert b.shape[0] == n
    eps, one, zero = dtype(1e-9), dtype(1.0), dtype(0.0)
    blocks = [(i0, min(n, i0 + block)) for i0 in range(0, n, block)]
    keep = n * n * np.dtype(dtype).itemsize <= cache_bytes
    d2_kept = [R.sqdist_matrix(a[i0:i1], b, dtype) for i0, i1 in blocks] if keep else None

    def d2_block(bi):
        return d2_kept[bi] if keep else R.sqdist_matrix(a[blocks[bi][0]:blocks[bi][1]], b, dtype)

    rem_l, rem_r = np.ones(n, dtype), np.ones(n, dtype)
    cost = zero
    for j in R.LEVELS:
        level = zero if j == -2 else dtype(-(4.0 ** j))
        k_kept = [np.exp(level * d2) for d2 in d2_kept] if keep and 2 * n * n * np.dtype(dtype).itemsize <= cache_bytes else None

        def k_block(bi):
            return k_kept[bi] if k_kept is not None else np.exp(level * d2_block(bi))

        ratio_l = np.empty(n, dtype)
        for bi, (i0, i1) in enumerate(blocks):
            ratio_l[i0:i1] = rem_l[i0:i1] / (eps + (k_block(bi) * rem_r[None, :]).sum(axis=1))
        col = np.zeros(n, dtype)
        for bi, (i0, i1) in enumerate(blocks):
            col = col + (k_block(bi) * ratio_l[i0:i1, None]).sum(axis=0)
        sumr = rem_r * col
        ratio_r = rem_r * np.minimum(rem_r / (sumr + eps), one)
        rem_r = np.maximum(zero, rem_r - sumr)
        for bi, (i0, i1) in enumerate(blocks):
            w = k_block(bi) * ratio_l[i0:i1, None] * ratio_r[None, :]
            cost = cost + (w * np.sqrt(d2_block(bi))).sum(dtype=dtype)
            rem_l[i0:i1] = np.maximum(zero, rem_l[i0:i1] - w.sum(axis=1))
            assert w.dtype == dtype
    assert rem_l.dtype == dtype and rem_r.dtype == dtype and np.asarray(cost).dtype == dtype
    return float(cost) / n


def gap(a, b):
    """(relative gap between the float32 and the float64 blocked restatement, the float64 value)."""
    r64, r32 = emd_approx_blocked(a, b, np.float64), emd_approx_blocked(a, b, np.float32)
    return abs(r32 - r64) / abs(r64), r64
