"""TEST INFRASTRUCTURE: CPU restatement of the alignment operators (bdm_amd/csrc/align.hip and align_solve.h, section 18 of
bdm_hip.h), the inputs their tests share, and the MUTANTS the host test holds against those inputs.

Partner search: tests/knn_ref.py's knn with k = 1 on the transformed source.  Apply rule: one rounded float32 torch op at a time.
Moments: Python integers (exact at any size).  Solve: align_solve.h's float64 formulas, one operation at a time, in numpy scalars.
The SVD definition (svd_solution) is the independent float64 statement the solve is held against."""
import functools
import math

import numpy as np
import torch

import knn_ref

MUTANTS = ("ties_latest", "no_det_fix", "transposed_R", "scale_from_yvar", "incremental", "batch_stop", "no_zero_stop")
SWEEPS = 10
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
EPS = 1e-9
F64 = np.float64
# Four times the largest gap of R, T, s between the float32-rounded solve and the float64 SVD definition that tools/align_gap.py
# measures over solve_cases(): 5.61e-8 over the random, planar, collinear and single-pair cases, 2.87e-8 over
# the near-reflection cases.  Both are the float32 rounding of entries of magnitude around 1 (half an ulp is 3e-8 below 1, 6e-8 above).
GAP_GENERAL, GAP_NEAR_REFLECTION = 4 * 5.61e-8, 4 * 2.87e-8


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def identity():
    return torch.tensor(IDENTITY, dtype=torch.float32)


def apply(x, tr):
    """x (P, 3) float32, tr (13,) float32 -> s (x @ R) + T by the apply rule: every product and sum a separate rounded op."""
    x, tr = x.float(), tr.float()
    cols = []
    for c in range(3):
        d = (x[:, 0] * tr[c] + x[:, 1] * tr[3 + c]) + x[:, 2] * tr[6 + c]
        cols.append(tr[12] * d + tr[9 + c])
    return torch.stack(cols, dim=1) if x.shape[0] else x.clone()


def partners(xq, y, mutant=None):
    """(P,) int64: the nearest target row of every (transformed) source row, -1 for none."""
    idx, _ = knn_ref.knn(xq, y, 1, "ties_latest" if mutant == "ties_latest" else None)
    return idx[:, 0]


def paired_partners(x, y):
    ok = torch.isfinite(x).all(1) & torch.isfinite(y).all(1)
    return torch.where(ok, torch.arange(x.shape[0]), torch.full((), -1))


def ceil_log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def scale_exp(x, y):
    """The fixed-point exponent e of an entry."""
    rows = [t[torch.isfinite(t).all(1)].abs().reshape(-1) for t in (x, y)]
    vals = torch.cat(rows)
    amax = float(vals.max()) if vals.numel() else 0.0
    field = (int(torch.tensor(amax, dtype=torch.float32).view(torch.int32)) >> 23) & 0xff
    E = max(field, 1) - 127
    nbits = min(24, (62 - ceil_log2(max(x.shape[0], 1))) // 2)
    return nbits - 1 - E


def quantise(t, e):
    """(n, 3) float32 finite rows -> Python integers rint(c 2^e) (round half to even)."""
    return torch.round(t.double() * math.ldexp(1.0, e)).to(torch.int64).tolist()


def moments(x, y, partner, e):
    """The 18 integer moments of the matched pairs: W, Sx (3), Sy (3), Sxy (9, a-major), Sxx, Syy -- Python integers."""
    sel = partner >= 0
    a, g = quantise(x[sel], e), quantise(y[partner[sel]], e)
    m = [len(a)] + [0] * 17
    for p, q in zip(a, g):
        for u in range(3):
            m[1 + u] += p[u]
            m[4 + u] += q[u]
            for w in range(3):
                m[7 + 3 * u + w] += p[u] * q[w]
        m[16] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
        m[17] += q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
    return m


def _rotate(a, v, p, q):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (F64(2.0) * apq)
    t = np.copysign(F64(1.0), theta) / (np.abs(theta) + np.sqrt(theta * theta + F64(1.0)))
    c = F64(1.0) / np.sqrt(t * t + F64(1.0))
    s = t * c
    tau = s / (F64(1.0) + c)
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = F64(0.0)
    for r in range(4):
        if r == p or r == q:
            continue
        arp, arq = a[r][p], a[r][q]
        a[r][p] = a[p][r] = arp - s * (arq + tau * arp)
        a[r][q] = a[q][r] = arq + s * (arp - tau * arq)
    for i in range(4):
        vip, viq = v[i][p], v[i][q]
        v[i][p] = vip - s * (viq + tau * vip)
        v[i][q] = viq + s * (vip - tau * viq)


def central_moments(m, e):
    """Integer moments -> (W, mx, my, M (3 x 3 lists), xvar, yvar) in float64, align_solve.h's order."""
    inv1, inv2, W = F64(math.ldexp(1.0, -e)), F64(math.ldexp(1.0, -2 * e)), F64(float(m[0]))
    f = lambda v: F64(float(v))   # noqa: E731  (int -> float64 rounds to nearest even)
    mx = [(f(m[1 + a]) * inv1) / W for a in range(3)]
    my = [(f(m[4 + a]) * inv1) / W for a in range(3)]
    M = [[(f(m[7 + 3 * a + b]) * inv2) / W - mx[a] * my[b] for b in range(3)] for a in range(3)]
    xvar = (f(m[16]) * inv2) / W - ((mx[0] * mx[0] + mx[1] * mx[1]) + mx[2] * mx[2])
    yvar = (f(m[17]) * inv2) / W - ((my[0] * my[0] + my[1] * my[1]) + my[2] * my[2])
    return W, mx, my, M, xvar, yvar


def horn_rotation(M, sweeps=SWEEPS, return_offdiag=False):
    """M (3 x 3 float64 scalars) -> R (9, row-major): Horn's quaternion through the fixed-sweep Jacobi."""
    n = [[F64(0.0)] * 4 for _ in range(4)]
    n[0][0] = (M[0][0] + M[1][1]) + M[2][2]
    n[1][1] = (M[0][0] - M[1][1]) - M[2][2]
    n[2][2] = (M[1][1] - M[0][0]) - M[2][2]
    n[3][3] = (M[2][2] - M[0][0]) - M[1][1]
    n[0][1] = n[1][0] = M[1][2] - M[2][1]
    n[0][2] = n[2][0] = M[2][0] - M[0][2]
    n[0][3] = n[3][0] = M[0][1] - M[1][0]
    n[1][2] = n[2][1] = M[0][1] + M[1][0]
    n[1][3] = n[3][1] = M[2][0] + M[0][2]
    n[2][3] = n[3][2] = M[1][2] + M[2][1]
    v = [[F64(1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
    with np.errstate(all="ignore"):   # theta^2 may overflow to +inf: t = 0, as in the header
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                _rotate(n, v, p, q)
    best = 0
    for c in (1, 2, 3):
        if n[c][c] > n[best][best]:
            best = c
    qw, qx, qy, qz = v[0][best], v[1][best], v[2][best], v[3][best]
    ln = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    qw, qx, qy, qz = qw / ln, qx / ln, qy / ln, qz / ln
    ww, xx, yy, zz = qw * qw, qx * qx, qy * qy, qz * qz
    xy, xz, yz, wx, wy, wz = qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    two = F64(2.0)
    R = [None] * 9
    R[0], R[3], R[6] = ((ww + xx) - yy) - zz, two * (xy - wz), two * (xz + wy)
    R[1], R[4], R[7] = two * (xy + wz), ((ww - xx) + yy) - zz, two * (yz - wx)
    R[2], R[5], R[8] = two * (xz - wy), two * (yz + wx), ((ww - xx) - yy) + zz
    if return_offdiag:
        off = max(abs(float(n[i][j])) for i in range(4) for j in range(4) if i != j)
        return R, off / max(abs(float(n[best][best])), 1e-300)
    return R


def svd_rotation(M, det_fix=True):
    """The SVD definition in float64 (torch.linalg.svd): R maximising trace(R^T M) over rotations; with det_fix=False over all
    orthogonal matrices (pytorch3d's allow_reflection=True)."""
    Mt = torch.tensor([[float(v) for v in row] for row in M], dtype=torch.float64)
    U, _, Vh = torch.linalg.svd(Mt)
    E = torch.eye(3, dtype=torch.float64)
    if det_fix:
        E[2, 2] = torch.sign(torch.det(U @ Vh)) if float(torch.det(U @ Vh)) != 0.0 else 1.0
    return [F64(v) for v in (U @ E @ Vh).reshape(-1).tolist()]


def solve(m, e, estimate_scale=False, eps=EPS, mutant=None, rotation=None):
    """18 integer moments (m[0] >= 1) -> (R (9), T (3), s, mse) in float64, align_solve.h's order of operations.  rotation:
    a function M -> R replacing Horn's (the SVD definition)."""
    with np.errstate(all="ignore"):
        W, mx, my, M, xvar, yvar = central_moments(m, e)
        if rotation is not None:
            R = rotation(M)
        elif mutant == "no_det_fix":
            R = svd_rotation(M, det_fix=False)
        else:
            R = horn_rotation(M)
        if mutant == "transposed_R":
            R = [R[3 * b + a] for a in range(3) for b in range(3)]
        tr = None
        for a in range(3):
            for b in range(3):
                t = R[3 * a + b] * M[a][b]
                tr = t if tr is None else tr + t
        eps = F64(eps)
        var = yvar if mutant == "scale_from_yvar" else xvar
        s = tr / (var if var > eps else eps) if estimate_scale else F64(1.0)
        T = [my[b] - s * ((mx[0] * R[b] + mx[1] * R[3 + b]) + mx[2] * R[6 + b]) for b in range(3)]
        res = ((s * s) * xvar - (F64(2.0) * s) * tr) + yvar
        mse = res if res > 0.0 else F64(0.0)
    return R, T, s, mse


def to_f32(R, T, s):
    """The 13 float32 of a transform (float64 -> float32 rounds to nearest even)."""
    return torch.tensor([float(v) for v in list(R) + list(T) + [s]], dtype=torch.float64).float()


def corresponding_points_alignment(x, y, estimate_scale=False, eps=EPS, mutant=None):
    """One entry -> (tr (13,) float32, mse float32 tensor scalar, moments, partner)."""
    partner = paired_partners(x, y)
    e = scale_exp(x, y)
    m = moments(x, y, partner, e)
    if m[0] == 0:
        return identity(), torch.tensor(float("nan")), m, partner
    R, T, s, mse = solve(m, e, estimate_scale, eps, mutant)
    return to_f32(R, T, s), torch.tensor(float(mse), dtype=torch.float64).float(), m, partner


class _Entry:
    """The state of one entry of an ICP run."""

    def __init__(self, x, y, start):
        self.x, self.y = x.float(), y.float()
        self.tr = identity() if start is None else start.float().clone()
        self.e = scale_exp(self.x, self.y)
        self.mse = float("nan")
        self.iter, self.done, self.converged = 0, False, False
        self.history = []           # per iteration (tr (13,) float32, mse float64)
        self.cur = self.x           # the `incremental` mutant's moving cloud
        self.passed = False         # the `batch_stop` mutant: this entry's own test holds

    def step(self, max_iterations, thr, estimate_scale, eps, mutant):
        """One iteration and the stopping rule."""
        src = self.cur if mutant == "incremental" else self.x
        partner = partners(apply(src, self.tr if mutant != "incremental" else identity()), self.y, mutant)
        m = moments(src, self.y, partner, self.e)
        if m[0] == 0:
            self.done, self.converged, self.mse = True, False, float("nan")
            return
        R, T, s, mse = solve(m, self.e, estimate_scale, eps, mutant)
        t, prev = self.iter + 1, self.mse
        self.tr, self.mse, self.iter = to_f32(R, T, s), float(mse), t
        if mutant == "incremental":
            self.cur = apply(src, self.tr)
        self.history.append((self.tr, self.mse))
        with np.errstate(all="ignore"):
            rel_ok = t >= 2 and bool((F64(prev) - F64(self.mse)) / F64(prev) <= F64(thr))
        zero = self.mse == 0.0 and mutant != "no_zero_stop"
        if mutant == "batch_stop":
            self.passed = zero or rel_ok
            if t >= max_iterations:
                self.done, self.converged = True, self.passed
            return
        if zero or rel_ok:
            self.done, self.converged = True, True
        elif t >= max_iterations:
            self.done, self.converged = True, False

    def result(self):
        return {"tr": self.tr, "mse": torch.tensor(self.mse, dtype=torch.float64).float(), "converged": self.converged,
                "iterations": self.iter, "xt": apply(self.x, self.tr), "history": self.history}


def icp(x_list, y_list, start=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False, eps=EPS, mutant=None):
    """A batch -> one result dict per entry.  Every entry runs on its own (the `batch_stop` mutant couples them as pytorch3d does)."""
    entries = [_Entry(x, y, None if start is None else start[i]) for i, (x, y) in enumerate(zip(x_list, y_list))]
    if mutant == "batch_stop":
        for _ in range(max_iterations):
            live = [en for en in entries if not en.done]
            if not live:
                break
            for en in live:
                en.step(max_iterations, relative_rmse_thr, estimate_scale, eps, mutant)
            if all(en.passed or en.done for en in entries):
                for en in entries:
                    if not en.done:
                        en.done, en.converged = True, True
    else:
        for en in entries:
            while not en.done:
                en.step(max_iterations, relative_rmse_thr, estimate_scale, eps, mutant)
    return [en.result() for en in entries]


# ---- the inputs the GPU test and the host test share ---------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rotation_matrix(axis, degrees):
    """Rodrigues in float64 -> (3, 3) for the row-vector convention y = x @ R."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = (a / a.norm()).tolist()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    th = math.radians(degrees)
    return (torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)).T


def box(n, seed):
    """A uniform cloud in a 1.0 x 0.6 x 0.3 box around the origin."""
    return ((torch.rand(n, 3, generator=_gen(seed), dtype=torch.float64) - 0.5) * torch.tensor([1.0, 0.6, 0.3], dtype=torch.float64)).float()


def moved(x, degrees, shift, scale=1.0, seed=0, noise=0.0, axis=(1.0, 2.0, 3.0)):
    """A permuted, rotated, scaled and translated copy of x (float64 arithmetic, rounded once)."""
    y = scale * (x.double() @ rotation_matrix(axis, degrees)) + torch.tensor(shift, dtype=torch.float64)
    if noise:
        y = y + noise * torch.randn(y.shape, generator=_gen(seed + 1), dtype=torch.float64)
    return y[torch.randperm(x.shape[0], generator=_gen(seed))].float()


MOMENT_SIZES = ((1, 1), (63, 65), (64, 1024), (257, 1025), (300, 2049), (0, 5), (5, 0))


@functools.lru_cache(maxsize=None)
def moment_case():
    """The ragged batch of the exact-sums test: the sizes of the issue's table; entry 2's target holds every row twice or more (ties:
    the lowest index wins), entries 1 and 4 carry NaN and inf rows on both sides, entry 3 lies around (50, 50, 50) with spread 1."""
    xs, ys = [], []
    for i, (p, r) in enumerate(MOMENT_SIZES):
        shift = 50.0 if i == 3 else 0.0
        x = torch.rand(p, 3, generator=_gen(900 + i)) * 2.0 - 1.0 + shift
        y = torch.rand(r, 3, generator=_gen(950 + i)) * 2.0 - 1.0 + shift
        if i == 2:
            y = y[torch.randint(0, 100, (r,), generator=_gen(990))]
        if i in (1, 4):
            bad = [float("nan"), float("inf"), float("-inf")]
            for k in range(9):
                x[(7 * k + 3) % p, k % 3] = bad[k % 3]
                y[(11 * k + 5) % r, (k + 1) % 3] = bad[(k + 2) % 3]
        xs.append(x), ys.append(y)
    start = torch.stack([to_f32([F64(v) for v in rotation_matrix((1.0, 2.0, 3.0), 4.0 + i).reshape(-1).tolist()],
                                [F64(0.01 * i), F64(-0.02), F64(0.03)], F64(1.0 + 0.01 * i)) for i in range(len(xs))])
    return {"x": xs, "y": ys, "start": start}


@functools.lru_cache(maxsize=None)
def moment_ref(mode, mutant=None):
    """[(moments (18 Python ints), e, partner (P,) int64)] per entry; mode 0 under the case's start transforms, mode 1 paired on the
    entries cut to equal lengths."""
    c = moment_case()
    out = []
    for i, (x, y) in enumerate(zip(c["x"], c["y"])):
        if mode == 1:
            n = min(x.shape[0], y.shape[0])
            x, y = x[:n], y[:n]
            partner = paired_partners(x, y)
        else:
            partner = partners(apply(x, c["start"][i]), y, mutant)
        e = scale_exp(x, y)
        out.append((moments(x, y, partner, e), e, partner))
    return out


def _icp_inputs(name):
    if name in ("rigid", "scale", "init"):
        xs = [box(257, 11), box(512, 12), box(300, 13)]
        sc = 1.1 if name == "scale" else 1.0
        ys = [moved(xs[0], 5.0, (0.02, -0.01, 0.03), seed=21),
              moved(xs[1], 10.0, (0.05, 0.02, -0.04), scale=sc, seed=22),
              moved(box(400, 14), 6.0, (0.01, 0.0, 0.02), seed=23, noise=0.002)]     # another sample of the box: the residual stays
        kw = {"max_iterations": 30, "estimate_scale": name == "scale"}
        init = None
        if name == "init":
            R = rotation_matrix((1.0, 2.0, 3.0), 3.0).reshape(-1).tolist()
            init = torch.stack([to_f32([F64(v) for v in R], [F64(0.01), F64(0.0), F64(-0.01)], F64(1.0))] * 3)
        return {"x": xs, "y": ys, "kw": kw, "init": init}
    if name == "stop":
        a, b = box(200, 31), box(512, 32)
        return {"x": [a, b], "y": [moved(a, 0.0, (0.001, 0.0, 0.0), seed=41), moved(b, 10.0, (0.05, 0.02, -0.04), seed=42)],
                "kw": {"max_iterations": 30}, "init": None}
    if name == "identical":
        lat = (torch.randint(-32, 33, (256, 3), generator=_gen(51)).float() / 64.0)    # dyadic: every moment is exact in float64
        return {"x": [lat], "y": [lat.clone()], "kw": {"max_iterations": 30}, "init": None}
    if name == "capped":
        b = box(300, 61)
        return {"x": [b, torch.zeros(0, 3), box(5, 62)], "y": [moved(b, 10.0, (0.05, 0.02, -0.04), seed=63), box(7, 64), torch.zeros(0, 3)],
                "kw": {"max_iterations": 3}, "init": None}
    raise KeyError(name)


ICP_CASES = ("rigid", "scale", "init", "stop", "identical", "capped")


@functools.lru_cache(maxsize=None)
def icp_case(name):
    return _icp_inputs(name)


@functools.lru_cache(maxsize=None)
def icp_ref(name, mutant=None):
    """The restatement's results for a case, computed once and shared (do not write into them).  With an init transform the start
    cloud is apply(x, init), as bdm_amd.alignment forms it."""
    c = icp_case(name)
    xs = c["x"] if c["init"] is None else [apply(x, c["init"][i]) for i, x in enumerate(c["x"])]
    return icp(xs, c["y"], **c["kw"], mutant=mutant)


@functools.lru_cache(maxsize=None)
def paired_case():
    """Paired sets: two well-conditioned rotated copies with noise (one scaled), a near reflection (the mirror image of a cloud with
    noise: the plain SVD would reflect), a NaN-riddled pair and an empty one."""
    a, b, c = box(300, 71), box(65, 72), box(128, 73)
    ya = (a.double() @ rotation_matrix((3.0, 1.0, 2.0), 40.0) + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
          + 0.01 * torch.randn(300, 3, generator=_gen(74), dtype=torch.float64)).float()
    yb = (1.3 * (b.double() @ rotation_matrix((1.0, 0.0, 1.0), 75.0)) + 0.02 * torch.randn(65, 3, generator=_gen(75), dtype=torch.float64)).float()
    yc = (c * torch.tensor([1.0, 1.0, -1.0]) + 0.01 * torch.randn(128, 3, generator=_gen(76))).float()
    d, yd = box(20, 77), box(20, 78)
    d[3, 1], yd[5, 0], yd[3, 2] = float("nan"), float("inf"), 1.0
    return {"x": [a, b, c, d, torch.zeros(0, 3)], "y": [ya, yb, yc, yd, torch.zeros(0, 3)], "well": (0, 1), "reflection": 2}


@functools.lru_cache(maxsize=None)
def paired_ref(estimate_scale, mutant=None):
    c = paired_case()
    return [corresponding_points_alignment(x, y, estimate_scale, EPS, mutant) for x, y in zip(c["x"], c["y"])]


# ---- the float64 SVD definition and the cases the solve is held against ---------------------------------------------------------------
def _moment_rows(x, y):
    partner = paired_partners(x, y)
    e = scale_exp(x, y)
    return moments(x, y, partner, e), e


@functools.lru_cache(maxsize=None)
def solve_cases():
    """{name: [(moments, e, estimate_scale)]}: what tests/test_align_host.py and tools/align_gap.py compare with the SVD definition."""
    g = _gen(81)
    cases = {"random": [], "planar": [], "collinear": [], "single": [], "near_reflection": []}
    for k in range(12):
        x = (torch.randn(40 + 7 * k, 3, generator=g) * torch.tensor([1.0, 0.7, 0.4])).float()
        y = moved(x, 15.0 + 13.0 * k, (0.3, -0.1, 0.2), scale=1.0 + 0.05 * k, seed=100 + k, noise=0.02)[torch.argsort(torch.randperm(x.shape[0], generator=_gen(100 + k)))]
        cases["random"].append(_moment_rows(x, y) + (k % 2 == 1,))
    for k in range(4):
        x = (torch.randn(50, 3, generator=g) * torch.tensor([1.0, 0.6, 0.0])).float()
        y = (x.double() @ rotation_matrix((1.0, 1.0, 0.5), 20.0 + 30.0 * k) + 0.1).float()
        cases["planar"].append(_moment_rows(x, y) + (False,))
    for k in range(4):
        x = (torch.randn(30, 1, generator=g) * torch.tensor([[1.0, 2.0, -0.5]])).float()
        y = (x.double() @ rotation_matrix((0.0, 1.0, 1.0), 25.0 + 20.0 * k) - 0.2).float()
        cases["collinear"].append(_moment_rows(x, y) + (False,))
    cases["single"].append(_moment_rows(torch.tensor([[0.3, -0.2, 0.9]]), torch.tensor([[1.0, 2.0, 3.0]])) + (False,))
    for k in range(4):
        x = box(100, 90 + k)
        y = (x * torch.tensor([1.0, 1.0, -1.0]) + 0.003 * (k + 1) * torch.randn(100, 3, generator=g)).float()
        cases["near_reflection"].append(_moment_rows(x, y) + (False,))
    return cases


def solve_gap(m, e, estimate_scale, collinear=False):
    """The largest absolute gap of R, T, s between the restatement's float32-rounded outputs and the float64 SVD definition.  A
    collinear cloud leaves the rotation about its line free: there the image of the line's direction takes R's place (the cases' lines
    pass through the origin, so the source mean lies along the direction and T is determined as well)."""
    R, T, s, _ = solve(m, e, estimate_scale)
    Rs, Ts, ss, _ = solve(m, e, estimate_scale, rotation=svd_rotation)
    got = to_f32(R, T, s).double()
    want = torch.tensor([float(v) for v in list(Rs) + list(Ts) + [ss]], dtype=torch.float64)
    if collinear:
        M = central_moments(m, e)[3]
        u = torch.linalg.svd(torch.tensor([[float(v) for v in row] for row in M], dtype=torch.float64))[0][:, 0]
        img = lambda t: u @ t[:9].view(3, 3)   # noqa: E731
        return max(float((img(got) - img(want)).abs().max()), float((got[9:] - want[9:]).abs().max()))
    return float((got - want).abs().max())
