"""CPU references for the generation metrics (bdm_amd/metrics.py, csrc/metrics.hip), in numpy; owe nothing to any kernel.

* chamfer_ref: float64 mean of nearest squared distances in the difference form.  sqdist_matrix(..., np.float32, expanded=True)
  is the MUTANT |p|^2 + |q|^2 - 2 p.q whose cancellation the elementwise bound of the GPU test must catch (in float32: in float64
  the expanded form is exact on fp32 inputs).
* emd_approx_ref: the approximate-match EMD (Fan et al.'s approxmatch + matchcost, the EMD that PointFlow and PVD report),
  restated from the published algorithm as DESIGN.md section 10 writes it down; float64 or float32.  `level_order` and `clamp`
  produce the mutants of tests/test_metrics_host.py.
* emd_exact: the true earth mover's distance of two equal-sized clouds (optimal assignment on the Euclidean distance).
* the case lists the CPU and GPU tests share (tools/metrics_emd_gap.py measures the restatement's float32-vs-float64 gap on them).
"""
import numpy as np

LEVELS = (7, 6, 5, 4, 3, 2, 1, 0, -1, -2)   # level = -4^j, 0 at j = -2


def sqdist_matrix(a, b, dtype=np.float64, expanded=False):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    if expanded:
        return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    dx, dy, dz = (a[:, None, c] - b[None, :, c] for c in range(3))
    return dx * dx + dy * dy + dz * dz


def chamfer_ref(a, b):
    """a (n, 3), b (m, 3) -> (mean_p min_q |p - q|^2, mean_q min_p |p - q|^2) in float64."""
    d2 = sqdist_matrix(a, b, np.float64)
    return float(d2.min(axis=1).mean()), float(d2.min(axis=0).mean())


def chamfer_matrix_ref(a, b):
    """a (s, n, 3), b (r, m, 3) -> out_ab, out_ba (s, r) float64."""
    ab, ba = np.zeros((len(a), len(b))), np.zeros((len(a), len(b)))
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            ab[i, j], ba[i, j] = chamfer_ref(ai, bj)
    return ab, ba


def emd_approx_ref(a, b, dtype=np.float64, level_order=LEVELS, clamp=True, return_mass=False):
    """cost(a, b) / n of the approximate match; with return_mass also the total matched mass sum_kl w(k, l)."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    n = a.shape[0]
    assert b.shape[0] == n
    eps, one, zero = dtype(1e-9), dtype(1.0), dtype(0.0)
    d2 = sqdist_matrix(a, b, dtype)
    d = np.sqrt(d2)
    rem_l, rem_r = np.ones(n, dtype), np.ones(n, dtype)
    cost, mass = zero, zero
    for j in level_order:
        level = zero if j == -2 else dtype(-(4.0 ** j))
        k = np.exp(level * d2)
        ratio_l = rem_l / (eps + (k * rem_r[None, :]).sum(axis=1))
        sumr = rem_r * (k * ratio_l[:, None]).sum(axis=0)
        frac = rem_r / (sumr + eps)
        ratio_r = rem_r * (np.minimum(frac, one) if clamp else frac)
        rem_r = np.maximum(zero, rem_r - sumr)
        w = k * ratio_l[:, None] * ratio_r[None, :]
        cost = cost + (w * d).sum(dtype=dtype)
        mass = mass + w.sum(dtype=dtype)
        rem_l = np.maximum(zero, rem_l - w.sum(axis=1))
        assert k.dtype == dtype and w.dtype == dtype and rem_l.dtype == dtype
    out = float(cost) / n
    return (out, float(mass)) if return_mass else out


def emd_exact(a, b):
    """True EMD / n: the optimal one-to-one assignment on sqrt(d^2) (float64)."""
    from scipy.optimize import linear_sum_assignment
    d = np.sqrt(sqdist_matrix(a, b, np.float64))
    rows, cols = linear_sum_assignment(d)
    return float(d[rows, cols].sum()) / len(a)


# ---- the shared case lists ---------------------------------------------------------------------------------------------------
def gaussian(count, n, seed, scale=0.5, offset=0.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (offset + scale * rng.standard_normal((count, n, 3))).astype(np.float32)


def uniform(count, n, seed, half=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-half, half, (count, n, 3)).astype(np.float32)


# EMD cases: (n, s, r, seed).  a = s Gaussian clouds (sigma 0.5), b = r clouds uniform in [-1, 1]^3: unlike distributions, so that
# every level of the match moves mass.  Few pairs at 2048 (the float64 restatement takes seconds per pair there).
EMD_CASES = [(1, 2, 3, 101), (2, 3, 2, 102), (63, 3, 2, 103), (256, 2, 3, 104), (1000, 2, 1, 105), (2048, 1, 2, 106)]


def emd_case(n, s, r, seed):
    return gaussian(s, n, seed), uniform(r, n, seed + 1000)


def emd_case_pairs():
    """Every (name, a_i, b_j) of EMD_CASES, each in natural and in reversed point order (the same pair: another summation order)."""
    for n, s, r, seed in EMD_CASES:
        a, b = emd_case(n, s, r, seed)
        for i in range(s):
            for j in range(r):
                yield f"n{n}[{i},{j}]", a[i], b[j]
                yield f"n{n}[{i},{j}]rev", a[i, ::-1], b[j, ::-1]


# End-to-end case (tests/golden/metrics_e2e.npz, tools/gen_golden_metrics.py): S = R = 24 clouds of 512 points, every cloud an
# axis-aligned Gaussian blob with its own three scales in [0.15, 0.9] (distinct shapes: the distance matrices have no near-ties).
E2E = {"S": 24, "R": 24, "n": 512, "seed_sample": 4101, "seed_ref": 4202}


def shape_clouds(count, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    scales = rng.uniform(0.15, 0.9, (count, 1, 3))
    return (scales * rng.standard_normal((count, n, 3))).astype(np.float32)


def e2e_clouds():
    return shape_clouds(E2E["S"], E2E["n"], E2E["seed_sample"]), shape_clouds(E2E["R"], E2E["n"], E2E["seed_ref"])


def chamfer_sum_matrix_ref(a, b):
    ab, ba = chamfer_matrix_ref(a, b)
    return ab + ba


def emd_matrix_ref(a, b):
    return np.array([[emd_approx_ref(p, q) for q in b] for p in a])


def min_relative_gap(m):
    """Smallest (second best - best) / best over the rows of m (inf entries ignored)."""
    s = np.sort(m, axis=1)
    return float(((s[:, 1] - s[:, 0]) / s[:, 0]).min())


def stacked(dxx, dxy, dyy):
    full = np.block([[dxx, dxy], [dxy.T, dyy]]).astype(np.float64)
    np.fill_diagonal(full, np.inf)
    return full


def e2e_min_gap(dxx, dxy, dyy):
    """Smallest relative best-to-second-best gap over the rows and columns of dxy (COV, MMD) and the rows of the stacked 1-NN matrix."""
    return min(min_relative_gap(dxy), min_relative_gap(dxy.T), min_relative_gap(stacked(dxx, dxy, dyy)))
