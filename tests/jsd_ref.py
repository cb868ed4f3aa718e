"""Float64 numpy restatement of the occupancy-grid measures (bdm_amd/metrics.py, csrc/occupancy.hip), shared by test_jsd_host.py and
test_hip_jsd.py.  Written from the definition: a resolution^3 grid over the unit cube whose coordinate i is float32(i / (r - 1) - 0.5)
(arithmetic in double), optionally clipped to the cells whose float32 norm is <= 0.5; every point goes to the nearest kept cell, the
lowest row-major index on ties; hits = points per cell over the whole set, active = clouds per cell; JSD in base 2."""
import numpy as np


def grid_loop(r):
    """The literal triple loop: float32 (r, r, r, 3) and the spacing."""
    grid = np.zeros((r, r, r, 3), dtype=np.float32)
    spacing = 1.0 / float(r - 1)
    for i in range(r):
        for j in range(r):
            for k in range(r):
                grid[i, j, k] = (i * spacing - 0.5, j * spacing - 0.5, k * spacing - 0.5)
    return grid, spacing


_GRIDS = {}


def kept_cells(r, in_sphere=True):
    """(kept, 3) float64 cell centres in row-major order and their flat indices in the full grid."""
    if (r, in_sphere) not in _GRIDS:
        flat = grid_loop(r)[0].reshape(-1, 3)
        if in_sphere:
            norm = np.sqrt(flat[:, 0] * flat[:, 0] + flat[:, 1] * flat[:, 1] + flat[:, 2] * flat[:, 2])   # float32
            keep = np.flatnonzero(norm <= np.float32(0.5))
        else:
            keep = np.arange(len(flat))
        _GRIDS[(r, in_sphere)] = (flat[keep].astype(np.float64), keep)
    return _GRIDS[(r, in_sphere)]


def nearest_kept_cell(points, r, in_sphere=True, chunk=512):
    """points (P, 3) -> (cell, best, margin): index into the kept cells of the nearest one (lowest on ties), its squared distance
    and the gap to the second-best squared distance, all float64 by brute force (margin = inf with a single kept cell)."""
    cells, _ = kept_cells(r, in_sphere)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cell = np.empty(len(pts), dtype=np.int64)
    best = np.empty(len(pts))
    margin = np.full(len(pts), np.inf)
    for p0 in range(0, len(pts), chunk):
        p = pts[p0:p0 + chunk]
        d = (p[:, None, 0] - cells[None, :, 0]) ** 2 + (p[:, None, 1] - cells[None, :, 1]) ** 2 + (p[:, None, 2] - cells[None, :, 2]) ** 2
        c = d.argmin(axis=1)   # the first minimum = the lowest index
        rows = np.arange(len(p))
        cell[p0:p0 + chunk], best[p0:p0 + chunk] = c, d[rows, c]
        if d.shape[1] > 1:
            d[rows, c] = np.inf
            margin[p0:p0 + chunk] = d.min(axis=1) - best[p0:p0 + chunk]
    return cell, best, margin


def occupancy_ref(clouds, r, in_sphere=True, keep=None):
    """clouds (S, N, 3) -> (hits, active, best, margin): int64 counts over the kept cells, and per point (S, N) the squared distance
    to its cell and the margin.  `keep` (S, N) bool leaves points out of the counts."""
    clouds = np.asarray(clouds)
    S, N = clouds.shape[:2]
    K = len(kept_cells(r, in_sphere)[0])
    cell, best, margin = nearest_kept_cell(clouds.reshape(-1, 3), r, in_sphere)
    cell, best, margin = cell.reshape(S, N), best.reshape(S, N), margin.reshape(S, N)
    hits, active = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for s in range(S):
        c = cell[s] if keep is None else cell[s][keep[s]]
        per_cloud = np.bincount(c, minlength=K)
        hits += per_cloud
        active += per_cloud > 0
    return hits, active, best, margin


def entropy_bits(p):
    p = np.asarray(p, dtype=np.float64)
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def jsd_ref(P, Q):
    """JSD in base 2 as the mean of the two Kullback-Leibler divergences from the mixture (not the entropy form the module returns)."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    P, Q = P / P.sum(), Q / Q.sum()
    M = 0.5 * (P + Q)
    kl = lambda a: float((a[a > 0] * np.log2(a[a > 0] / M[a > 0])).sum())
    return 0.5 * kl(P) + 0.5 * kl(Q)


def bernoulli_entropy_mean(active, num_clouds):
    """Mean over the cells of the entropy in nats of Bernoulli(active / num_clouds)."""
    total = 0.0
    for g in np.asarray(active, dtype=np.float64):
        p = g / num_clouds
        for q in (p, 1.0 - p):
            if q > 0:
                total -= q * np.log(q)
    return total / len(active)
