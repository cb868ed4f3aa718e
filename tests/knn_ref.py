"""TEST INFRASTRUCTURE: CPU restatement of the two-set K-nearest-neighbour search and the attribute transfer (bdm_amd/csrc/knn.hip,
section 15 of bdm_hip.h), the inputs its tests share, and the MUTANTS the host test holds against those inputs.

Search: torch elementwise arithmetic in the header's order (dx = r_x - q_x, d2 = (dx*dx + dy*dy) + dz*dz, every operation a separate
rounded tensor op, so nothing is contracted), then a stable sort on d2 alone: among equal d2 the lower index stays first, which is
the (d2, j) order.  This is tests/normals_ref.py's order; that module's knn() is not imported because it is all-or-nothing per cloud
(section 10) where this rule keeps short rows.  Interpolation: sequential sums, one rounded operation at a time.
dtype=torch.float64 evaluates the same formulas in float64."""
import functools

import torch

SEARCH_MUTANTS = ("ties_latest", "k_minus_1", "expanded_square", "accept_nonfinite", "drop_inf", "pad_zero")
INTERP_MUTANTS = ("unnormalised", "no_eps", "descending")
EPS = 1e-8


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def knn(queries, refs, k, mutant=None, dtype=torch.float32):
    """queries (P, 3), refs (R, 3) -> (idx (P, k) int64, d2 (P, k) dtype): the k smallest (d2, j), ascending; a row with fewer
    neighbours ends in idx = -1, d2 = +inf."""
    q, r = queries.to(dtype), refs.to(dtype)
    P, R = q.shape[0], r.shape[0]
    kk = k - 1 if mutant == "k_minus_1" else k
    pad_i, pad_d = (0, 0.0) if mutant == "pad_zero" else (-1, float("inf"))
    idx = torch.full((P, k), pad_i, dtype=torch.int64)
    out = torch.full((P, k), pad_d, dtype=dtype)
    if P == 0 or R == 0 or kk == 0:
        return idx, out
    r_ok, q_ok = torch.isfinite(r).all(dim=1), torch.isfinite(q).all(dim=1)
    nan = torch.full((), float("nan"), dtype=dtype)
    for lo in range(0, P, 512):
        qq = q[lo:lo + 512]
        if mutant == "expanded_square":
            qn = (qq[:, 0] * qq[:, 0] + qq[:, 1] * qq[:, 1]) + qq[:, 2] * qq[:, 2]
            rn = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            dot = (qq[:, None, 0] * r[None, :, 0] + qq[:, None, 1] * r[None, :, 1]) + qq[:, None, 2] * r[None, :, 2]
            d2 = ((qn[:, None] + rn[None, :]) - 2.0 * dot).clamp_min(0.0)
        else:
            dx = r[None, :, 0] - qq[:, None, 0]
            dy = r[None, :, 1] - qq[:, None, 1]
            dz = r[None, :, 2] - qq[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        if mutant != "accept_nonfinite":
            d2 = torch.where(r_ok[None, :], d2, nan)               # nobody's neighbour
        d2 = torch.where(q_ok[lo:lo + 512, None], d2, nan)         # no neighbours
        if mutant == "drop_inf":
            d2 = torch.where(torch.isinf(d2), nan, d2)
        if mutant == "ties_latest":
            s = torch.sort(d2.flip(1), dim=1, stable=True)         # NaN sorts behind +inf
            order, vals = (R - 1) - s.indices, s.values
        else:
            s = torch.sort(d2, dim=1, stable=True)
            order, vals = s.indices, s.values
        m = min(kk, R)
        order, vals = order[:, :m], vals[:, :m]
        absent = torch.isnan(vals)
        idx[lo:lo + 512, :m] = torch.where(absent, torch.full((), pad_i), order)
        out[lo:lo + 512, :m] = torch.where(absent, torch.full((), pad_d, dtype=dtype), vals)
    return idx, out


def interpolate(attr, idx, d2, mode, eps=EPS, fill=float("nan"), mutant=None, dtype=torch.float32):
    """attr (R, c), idx (P, k), d2 (P, k) -> (P, c): mode 0 the first entry that takes part, mode 1 inverse squared distance."""
    a, d = attr.to(dtype), d2.to(dtype)
    P, k = idx.shape
    R, c = a.shape
    part = (idx >= 0) & (idx < R)
    safe = idx.clamp(0, max(R - 1, 0))
    out = torch.full((P, c), fill, dtype=dtype)
    if P == 0:
        return out
    if R == 0:
        return out
    if mode == 0:
        first = part.int().argmax(dim=1)                               # the first True (0 when there is none)
        rows = a[safe[torch.arange(P), first]]
        return torch.where(part.any(dim=1)[:, None], rows, out)
    e = torch.tensor(0.0 if mutant == "no_eps" else eps, dtype=dtype)
    num, den = torch.zeros(P, c, dtype=dtype), torch.zeros(P, dtype=dtype)
    started = torch.zeros(P, dtype=torch.bool)
    for l in (range(k - 1, -1, -1) if mutant == "descending" else range(k)):
        w = 1.0 / (d[:, l] + e)
        wv = w[:, None] * a[safe[:, l]]
        take = part[:, l]
        num = torch.where((take & started)[:, None], num + wv, torch.where(take[:, None], wv, num))
        den = torch.where(take & started, den + w, torch.where(take, w, den))
        started = started | take
    res = num if mutant == "unnormalised" else num / den[:, None]
    return torch.where(started[:, None], res, out)


def knn_batch(q_list, r_list, k, mutant=None, dtype=torch.float32):
    """[(idx, d2)] per entry."""
    return [knn(q, r, k, mutant, dtype) for q, r in zip(q_list, r_list)]


# ---- the inputs the GPU test and the host test share ---------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def cloud(n, seed, shift=(0.0, 0.0, 0.0)):
    return torch.rand(n, 3, generator=_gen(seed)) * 2.0 - 1.0 + torch.tensor(shift)


R_EDGES = (63, 64, 65, 1023, 1024, 1025, 2049)     # the 64-candidate step and the 1024-row LDS tile
P_EDGES = (1, 3, 4, 5, 15, 16, 17, 65)             # four queries per wave, sixteen per workgroup
K_EDGES = (1, 2, 3, 50, 63, 64)


def _edges(k):
    sizes = list(zip(P_EDGES, R_EDGES + (2049,)))
    return {"k": k, "q": [cloud(p, 100 + i) for i, (p, _) in enumerate(sizes)], "r": [cloud(r, 200 + i) for i, (_, r) in enumerate(sizes)]}


def _short(k):
    rs = (0, 1, k - 1, k)
    return {"k": k, "q": [cloud(5, 300 + i) for i in range(4)], "r": [cloud(r, 310 + i) for i, r in enumerate(rs)]}


def _ragged():
    sizes = ((17, 1025), (0, 40), (33, 0), (5, 2))
    return {"k": 3, "q": [cloud(p, 400 + i) for i, (p, _) in enumerate(sizes)], "r": [cloud(r, 410 + i) for i, (_, r) in enumerate(sizes)]}


def _ties():
    """A 4 x 4 x 4 lattice of spacing 0.25 (all coordinates and all squared distances exact in float32), its first 60 points repeated,
    the 124 rows shuffled; queries on the lattice points and on 33 midpoints of lattice edges: every query has ties in d2."""
    g = torch.arange(4, dtype=torch.float32) * 0.25
    lattice = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).reshape(-1, 3)
    refs = torch.cat([lattice, lattice[:60]])[torch.randperm(124, generator=_gen(500))]
    mid = lattice[:33] + torch.tensor([0.125, 0.0, 0.0])
    return {"k": 8, "q": [torch.cat([lattice, mid])], "r": [refs]}


def _nonfinite(k):
    """40 rows in each set, 16 of them with a NaN or an infinity somewhere; reference row 5 lies 3e19 away from everything (a finite
    point: d2 overflows to +inf and it is still a neighbour).  With k = 50 every row is short: 23 near neighbours, then the far one."""
    q, r = cloud(40, 600), cloud(40, 601)
    bad = [float("nan"), float("inf"), float("-inf")]
    for i in range(16):
        q[2 * i + 1, i % 3] = bad[i % 3]
        r[2 * i, (i + 1) % 3] = bad[(i + 2) % 3]
    r[5] = torch.tensor([3e19, 0.0, 0.0])
    return {"k": k, "q": [q], "r": [r]}


def _shifted():
    return {"k": 5, "q": [cloud(33, 700, (100.0, -50.0, 25.0))], "r": [cloud(300, 701, (100.0, -50.0, 25.0))]}


CASES = {**{f"edges_k{k}": functools.partial(_edges, k) for k in K_EDGES}, "short_k3": functools.partial(_short, 3),
         "short_k64": functools.partial(_short, 64), "ragged": _ragged, "ties": _ties, "nonfinite_k50": functools.partial(_nonfinite, 50),
         "nonfinite_k3": functools.partial(_nonfinite, 3), "shifted": _shifted}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_ref(name, mutant=None):
    """[(idx int64, d2 float32)] per entry: computed once and shared (do not write into it)."""
    c = case(name)
    return knn_batch(c["q"], c["r"], c["k"], mutant)


# which case shows each mutant of the search (tests/test_knn_host.py asserts that it does)
MUTANT_CASE = {"ties_latest": "ties", "k_minus_1": "edges_k3", "expanded_square": "shifted", "accept_nonfinite": "nonfinite_k50",
               "drop_inf": "nonfinite_k50", "pad_zero": "short_k3"}

INTERP_C = (1, 3, 4, 16)


@functools.lru_cache(maxsize=None)
def interp_case():
    """One entry of 12 queries against 9 reference rows, k = 4, with hand-made (idx, d2) rows as bdm_knn_points writes them: m = 0
    (row 0), m = 1 (row 1), a coincident point with d2 = 0 (row 2), a +inf entry with idx >= 0 (row 3), the rest m = k from the
    restatement's search; and a second entry of 3 queries against an EMPTY reference set (m = 0 everywhere)."""
    q, r = cloud(12, 800), cloud(9, 801)
    q[2] = r[4]
    idx, d2 = knn(q, r, 4)
    idx[0], d2[0] = -1, float("inf")
    idx[1, 1:], d2[1, 1:] = -1, float("inf")
    d2[3, 3] = float("inf")
    assert float(d2[2, 0]) == 0.0 and int(idx[2, 0]) == 4
    empty_i, empty_d = knn(cloud(3, 802), torch.zeros(0, 3), 4)
    return {"k": 4, "np": [12, 3], "nr": [9, 0], "idx": torch.cat([idx, empty_i]), "d2": torch.cat([d2, empty_d]),
            "attr": {c: torch.rand(9, c, generator=_gen(810 + c)) * 4.0 - 2.0 for c in INTERP_C}}


def interp_ref(c, mode, fill, mutant=None, dtype=torch.float32):
    ic = interp_case()
    out, lo = [], 0
    for n, nr in zip(ic["np"], ic["nr"]):
        attr = ic["attr"][c] if nr else torch.zeros(0, c)
        out.append(interpolate(attr, ic["idx"][lo:lo + n], ic["d2"][lo:lo + n], mode, EPS, fill, mutant, dtype))
        lo += n
    return torch.cat(out)
