"""TEST INFRASTRUCTURE: CPU restatement of the normal estimator (bdm_amd/csrc/normals.hip, section 10 of bdm_hip.h), the inputs
its tests share, the bounds they hold the kernel to, and the MUTANTS the host test holds against those bounds.

Neighbours: torch float32 elementwise arithmetic in the header's order (dx = x_j - x_i, d2 = (dx*dx + dy*dy) + dz*dz, every
operation a separate rounded tensor op, so nothing is contracted), then a stable sort by (d2, index).  Covariance and
numpy.linalg.eigh in float64 on the float32 points.  Both sign rules restated."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24        # unit roundoff of float32
GAP_MIN = 0.05        # points with (l1 - l0) / l2 below this are left out of the normal comparison (only)
# Bounds.  A float32 numpy restatement (same neighbours, float32 covariance, LAPACK ssyevd) against the
# float64 one on the inputs below shows |n x n_ref| (l1 - l0) / (l2 u) <= 2.42 (the noisy sphere) and curvature errors <= 3.11e-7 l2
# (the torus), measured on the CPU (tests/test_normals_host.py::test_float32_numpy_is_an_eighth_of_the_bounds holds them to
# it); the kernel gets 8 times that for its other summation order and the rounding of its Jacobi rotations.
NORMAL_C = 8 * 2.42
CURV_BOUND = 8 * 3.11e-7


def knn(points, k, ties="earliest", include_self=True):
    """points (N, 3) float32 -> (N, k) int64 indices of the k smallest (d2, j), ascending; -1 rows for non-finite points and
    everywhere when fewer than k points are finite.  ties="latest" and include_self=False are mutants."""
    p = points.float()
    n = p.shape[0]
    finite = torch.isfinite(p).all(dim=1)
    out = torch.full((n, k), -1, dtype=torch.int64)
    if int(finite.sum()) < k + (0 if include_self else 1):
        return out
    for lo in range(0, n, 512):
        q = p[lo:lo + 512]
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = torch.where(finite[None, :], d2, torch.full((), float("nan")))    # NaN sorts behind +inf
        if not include_self:
            d2[torch.arange(q.shape[0]), torch.arange(lo, lo + q.shape[0])] = float("nan")
        if ties == "latest":
            order = (n - 1) - torch.sort(d2.flip(1), dim=1, stable=True).indices[:, :k]
        else:
            order = torch.sort(d2, dim=1, stable=True).indices[:, :k]
        out[lo:lo + 512] = order
    out[~finite] = -1
    return out


def canonical_sign(nrm):
    """orient = 0: the component of largest magnitude positive, lowest axis among equals."""
    ax = np.argmax(np.abs(nrm), axis=1)    # argmax returns the first maximum
    s = np.sign(nrm[np.arange(len(nrm)), ax])
    return nrm * np.where(s == 0, 1.0, s)[:, None]


def estimate(points, k, orient=0, viewpoint=None, idx=None, mutant=None, dtype=np.float64):
    """The restatement for one cloud: dict of idx (N, k) int64, normals (N, 3), curvatures (N, 3) ascending, n_pos (N,) (the
    count rule 1 looks at, for the UNORIENTED eigenvector as LAPACK returned it), flip (N,) bool (rule 1's decision for that
    vector), all float64 (dtype=np.float32: the float32 numpy restatement the bounds are derived from).  Rows of non-finite
    points are NaN.  mutant: None | "no_self" | "k_minus_1" | "about_query" | "largest" | "npos_gt" | "ties_latest"."""
    p32 = points.float()
    if idx is None:
        idx = knn(p32, k - 1 if mutant == "k_minus_1" else k, ties="latest" if mutant == "ties_latest" else "earliest",
                  include_self=mutant != "no_self")
    ok = (idx >= 0).all(dim=1).numpy()
    p = p32.numpy().astype(dtype)
    nb = idx.clamp(min=0).numpy()
    e = p[nb] - p[:, None, :]                                   # (N, k, 3)
    e = np.where(ok[:, None, None], e, 0.0).astype(dtype)
    d = e if mutant == "about_query" else e - e.mean(axis=1, keepdims=True, dtype=dtype)
    cov = (np.einsum("nki,nkj->nij", d, d) / dtype(d.shape[1])).astype(dtype)
    lam, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 2 if mutant == "largest" else 0]
    proj = np.einsum("nki,ni->nk", e, nrm)
    n_pos = (proj > 0).sum(axis=1)
    kk = e.shape[1]
    flip = n_pos > 0.5 * kk if mutant == "npos_gt" else n_pos < 0.5 * kk
    if orient == 0:
        out = canonical_sign(nrm)
    elif orient == 1:
        out = np.where(flip[:, None], -nrm, nrm)
    else:
        vp = np.asarray(viewpoint, dtype=dtype).reshape(3)
        out = np.where((np.einsum("ni,ni->n", nrm, vp[None] - p) < 0)[:, None], -nrm, nrm)
    out = np.where(ok[:, None], out, np.nan)
    lam = np.where(ok[:, None], lam, np.nan)
    return {"idx": idx, "normals": out, "curvatures": lam, "n_pos": n_pos, "flip": flip, "raw": nrm}


def cross_norm(a, b):
    return np.linalg.norm(np.cross(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), axis=-1)


def errors(normals, curvatures, ref):
    """(worst |n x n_ref| (l1 - l0) / (l2 u) over the compared points, worst |l - l_ref| / l2, share of points left out of the
    normal comparison) of float32 results against the float64 restatement `ref` of the same neighbour sets."""
    lam = ref["curvatures"]
    ok = np.isfinite(lam).all(axis=1)
    l0, l1, l2 = lam[ok, 0], lam[ok, 1], lam[ok, 2]
    rel_gap = (l1 - l0) / l2
    keep = rel_gap >= GAP_MIN
    ratio = cross_norm(np.asarray(normals)[ok], ref["normals"][ok]) * rel_gap / U
    curv = np.abs(np.asarray(curvatures, dtype=np.float64)[ok] - lam[ok]) / l2[:, None]
    return float(ratio[keep].max()), float(curv.max()), float(1.0 - keep.mean())


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
def blob(g, n):
    return torch.randn(n, 3, generator=g) * 0.25


def open_blob(g, n, k=3):
    """A blob for k = 3, where a neighbourhood is a triangle and C has rank 2: in a Gaussian blob a fifth of those triangles are
    nearly collinear (l1 < 0.05 l2), exactly the points the normal comparison leaves out.  The points with l1 < 0.1 l2 are drawn
    again (which changes their neighbours' triangles too) until under 1 % are left; a handful of rounds, fixed by the seed."""
    pts = blob(g, n)
    for _ in range(100):
        lam = estimate(pts, k)["curvatures"]
        bad = torch.from_numpy((lam[:, 1] - lam[:, 0]) / lam[:, 2] < 0.1)
        if float(bad.float().mean()) < 0.01:
            break
        pts[bad] = blob(g, int(bad.sum()))
    return pts


def sphere(g, n, radius=0.3, noise=0.0):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    r = radius + (noise * torch.randn(n, 1, generator=g, dtype=torch.float64) if noise else 0.0)
    return (d * r).float()


def torus(g, n, R=0.3, r=0.1):
    u = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    v = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    return torch.stack([(R + r * torch.cos(v)) * torch.cos(u), (R + r * torch.cos(v)) * torch.sin(u), r * torch.sin(v)], dim=1).float()


# name -> (b, n, k, kind, seed): the issue's table
CASES = {
    "b1_n65_k64_blob": (1, 65, 64, "blob", 0),
    "b2_n300_k16_cloud": (2, 300, 16, "cloud", 1),
    "b3_n1025_k3_blob": (3, 1025, 3, "open_blob", 2),
    "b1_n1500_k50_torus": (1, 1500, 50, "torus", 3),
    "b1_n4096_k50_sphere": (1, 4096, 50, "sphere", 4),
}
MAX_LEFT_OUT = {"blob": 0.05, "open_blob": 0.05, "cloud": 0.05, "torus": 0.0, "sphere": 0.0}


@functools.lru_cache(maxsize=None)
def case(name):
    """points (b, n, 3) float32 of a case."""
    from render_ref import _cloud
    b, n, k, kind, seed = CASES[name]
    g = torch.Generator().manual_seed(2000 + seed)
    make = {"blob": lambda: blob(g, n), "open_blob": lambda: open_blob(g, n), "cloud": lambda: _cloud(g, n, 0.03), "torus": lambda: torus(g, n),
            "sphere": lambda: sphere(g, n, noise=0.003)}[kind]
    return torch.stack([make() for _ in range(b)])


@functools.lru_cache(maxsize=None)
def case_ref(name, orient=0):
    """The float64 restatement of every cloud of a case (a list of estimate() dicts); computed once, shared, left unchanged."""
    k = CASES[name][2]
    return [estimate(p, k, orient) for p in case(name)]


@functools.lru_cache(maxsize=None)
def shifted_case():
    """The (2, 300, 16) clouds shifted by (100, -50, 25), rounded to float32: the inputs of the translation test."""
    return (case("b2_n300_k16_cloud") + torch.tensor([100.0, -50.0, 25.0])).float()


@functools.lru_cache(maxsize=None)
def clean_sphere():
    """(1, 1024, 3): the sphere of radius 0.3 without noise, k = 50 (orientation tests, known-surface test)."""
    return sphere(torch.Generator().manual_seed(2100), 1024)[None]


@functools.lru_cache(maxsize=None)
def tie_cloud():
    """(1, 200, 3): points on a 6 x 6 x 6 lattice of pitch 0.05 (many equal distances), 60 of them exact duplicates of others."""
    g = torch.Generator().manual_seed(2101)
    cells = torch.randperm(216, generator=g)[:200]
    pts = torch.stack([cells // 36, (cells // 6) % 6, cells % 6], dim=1).float() * 0.05
    pts[100:130] = pts[0:30]
    pts[170:200] = pts[10:40]
    return pts[None]


@functools.lru_cache(maxsize=None)
def nonfinite_cloud():
    """(1, 300, 3): a blob with 16 points made NaN or infinite in one or all coordinates."""
    g = torch.Generator().manual_seed(2102)
    pts = blob(g, 300)
    sel = torch.randperm(300, generator=g)[:16]
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[nan, 0, 0], [0, nan, 0.1], [0.1, 0, nan], [nan, nan, nan], [inf, 0, 0], [0, -inf, 0], [0, 0.1, inf],
                        [inf, inf, inf], [-inf, nan, 0], [nan, inf, 0], [0.0, 0.0, -inf], [inf, 0.2, nan], [nan, 0.1, 0.1],
                        [0.1, inf, 0.1], [-inf, -inf, -inf], [0.2, nan, inf]])
    pts[sel] = bad
    return pts[None], sel
