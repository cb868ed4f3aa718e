"""The rule of include/bdm_hip.h section 16 (mesh cleaning: vertex adjacency, connected components, Taubin smoothing) in torch on the
CPU, the case table of tests/test_hip_mesh_clean.py and the mutants of tests/test_mesh_clean_host.py.

Adjacency comes from torch.unique of directed keys, labels by iterating the round to its fixed point.  The smoothing is float32 with
one rounding per operation (every operation is formed in float64 and rounded to float32, which is the correctly rounded float32
operation: see _rounded) over a padded neighbour table walked in rank order, so the sums are sequential; dtype=torch.float64 gives
the same formulas in float64."""
import functools

import torch

import surface_ref as S

ADJ_MUTANTS = ("no_dedup", "descending", "accept_repeated", "wrap_index")
COMP_MUTANTS = ("rank_by_size", "face_comp_zero")
SMOOTH_MUTANTS = ("gauss_seidel", "mu_first", "no_eps", "one_minus_f64", "isolated_moved")
EPS = 1e-12
LAMBD, MU = 0.53, -0.34


def bits(t):
    return t.contiguous().view(torch.int32)


def same_floats(a, b):
    """Equal as bits, except that a NaN equals any NaN (which NaN an operation returns is not part of the rule)."""
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb]))


# ---- adjacency ------------------------------------------------------------------------------------------------------------------------
def connected_mask(faces, V, mutant=None):
    """(F,) bool: the connected faces (three indices in [0, V), pairwise different), and the faces with the indices the rule reads."""
    f = faces.long().reshape(-1, 3)
    if mutant == "wrap_index" and V > 0:
        f = f % V
    ok = ((f >= 0) & (f < V)).all(1)
    if mutant != "accept_repeated":
        ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return ok, f


def adjacency(faces, V, mutant=None):
    """One mesh -> (first (V + 1,) int32, nbr int32): the sorted neighbour sets as a CSR."""
    ok, f = connected_mask(faces, V, mutant)
    f = f[ok]
    a = torch.cat([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    c = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    keys = a * max(V, 1) + c
    keys = torch.sort(keys).values if mutant == "no_dedup" else torch.unique(keys)
    src, dst = keys // max(V, 1), keys % max(V, 1)
    if mutant == "descending":
        order = torch.argsort(src * max(V, 1) + (max(V, 1) - 1 - dst))
        src, dst = src[order], dst[order]
    first = torch.zeros(V + 1, dtype=torch.int64)
    first[1:] = torch.cumsum(torch.bincount(src, minlength=V), 0)
    return first.int(), dst.int()


def labels(first, nbr):
    """The fixed point of m_i = min(l_i, l_j for j in N(i)), l'_i = l_{m_i}, from l_i = i -> (labels (V,) int64, rounds that changed a label)."""
    V = first.numel() - 1
    l = torch.arange(V)
    src = torch.repeat_interleave(torch.arange(V), (first[1:] - first[:-1]).long())
    dst = nbr.long()
    rounds = 0
    while True:
        m = l.clone().scatter_reduce_(0, src, l[dst], "amin", include_self=True)
        new = l[m]
        if torch.equal(new, l):
            return l, rounds
        l, rounds = new, rounds + 1


def components(faces, V, mutant=None):
    """One mesh -> dict(first, nbr, vert_comp (V,), face_comp (F,), comp_verts (C,), comp_faces (C,), rounds); int64 but for the CSR."""
    first, nbr = adjacency(faces, V)
    l, rounds = labels(first, nbr)
    roots = torch.unique(l)
    vert_comp = torch.searchsorted(roots, l)
    comp_verts = torch.bincount(vert_comp, minlength=roots.numel())
    if mutant == "rank_by_size":
        order = torch.argsort(-comp_verts, stable=True)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel())
        vert_comp, comp_verts = rank[vert_comp], comp_verts[order]
    ok, f = connected_mask(faces, V)
    face_comp = torch.full((f.shape[0],), 0 if mutant == "face_comp_zero" else -1, dtype=torch.int64)
    face_comp[ok] = vert_comp[f[ok, 0]]
    comp_faces = torch.bincount(vert_comp[f[ok, 0]], minlength=roots.numel())
    return {"first": first, "nbr": nbr, "vert_comp": vert_comp, "face_comp": face_comp, "comp_verts": comp_verts, "comp_faces": comp_faces,
            "rounds": rounds}


# ---- smoothing ------------------------------------------------------------------------------------------------------------------------
def _table(first, nbr):
    """(V, dmax) neighbour indices packed to the left in list order, (V,) degrees."""
    V = first.numel() - 1
    deg = (first[1:] - first[:-1]).long()
    dmax = int(deg.max()) if V else 0
    table = torch.zeros(V, max(dmax, 1), dtype=torch.int64)
    row = torch.repeat_interleave(torch.arange(V), deg)
    col = torch.arange(nbr.numel()) - first[:-1].long()[row]
    table[row, col] = nbr.long()
    return table, deg


def _rounded(fn):
    """A float32 operation as the float64 operation on the same values, rounded once more: for +, -, *, / and sqrt the double rounding is
    innocuous (53 >= 2 * 24 + 2 bits), so the result is the correctly rounded float32 one whatever vector unit torch's float32 kernels
    were built for (an AVX-512 build was seen to differ from exact rational arithmetic in the last bit of a weight).  With float64
    operands it is the plain float64 operation."""
    def op(*args):
        return fn(*[a.double() for a in args]).to(args[0].dtype)
    return op


_add, _sub, _mul, _div, _sqrt = (_rounded(f) for f in (torch.add, torch.sub, torch.mul, torch.div, torch.sqrt))


def _weight(p, q, mode, eps):
    if mode == 1:
        return torch.ones(p.shape[0], dtype=p.dtype)
    d = _sub(p, q)
    d2 = _add(_add(_mul(d[:, 0], d[:, 0]), _mul(d[:, 1], d[:, 1])), _mul(d[:, 2], d[:, 2]))
    den = _add(_sqrt(d2), eps.expand_as(d2))
    return _div(torch.ones_like(den), den)


def half_step(v, first, nbr, f, mode, mutant=None):
    """One half-step with factor f (a tensor of v's dtype holding the float32 value) on one mesh."""
    table, deg = _table(first, nbr)
    eps = torch.tensor(0.0 if mutant == "no_eps" else EPS, dtype=torch.float32).to(v.dtype)
    one = torch.ones((), dtype=v.dtype)
    if mutant == "gauss_seidel":   # in place, vertex after vertex
        v = v.clone()
        for i in range(v.shape[0]):
            if deg[i]:
                v[i] = half_step(v, first, nbr, f, mode)[i]
        return v
    Sm, W = torch.zeros_like(v), torch.zeros(v.shape[0], dtype=v.dtype)
    for k in range(int(deg.max()) if v.shape[0] else 0):
        q = v[table[:, k]]
        w = _weight(v, q, mode, eps)
        wq = _mul(w[:, None].expand_as(q), q)
        on = deg > k
        Sm = torch.where(on[:, None], wq if k == 0 else _add(Sm, wq), Sm)
        W = torch.where(on, w if k == 0 else _add(W, w), W)
    if mutant == "one_minus_f64":
        keep = ((1.0 - f.double()) * v.double()).to(v.dtype)
    else:
        keep = _mul(_sub(one, f).expand_as(v), v)
    new = _add(keep, _mul(f.expand_as(v), _div(Sm, W[:, None].expand_as(Sm))))
    return new if mutant == "isolated_moved" else torch.where((deg > 0)[:, None], new, v)


def taubin(verts, first, nbr, lambd=LAMBD, mu=MU, num_iter=10, mode=0, mutant=None, dtype=torch.float32):
    """num_iter iterations (lambd half-step, then mu half-step) on one mesh -> (V, 3) of `dtype`."""
    v = verts.to(dtype)
    fs = [torch.tensor(lambd, dtype=torch.float32).to(dtype), torch.tensor(mu, dtype=torch.float32).to(dtype)]
    if mutant == "mu_first":
        fs = fs[::-1]
    for _ in range(num_iter):
        for f in fs:
            v = half_step(v, first, nbr, f, mode, mutant)
    return v


def remove_small(verts, faces, min_fraction=0.1, min_faces=1, keep_largest=False):
    """The island removal of one mesh from the rule alone -> (verts, faces int64)."""
    import math
    c = components(faces, verts.shape[0])
    cf = c["comp_faces"]
    if cf.numel() == 0:
        return verts, faces.long()[:0]
    if keep_largest:
        keep = torch.zeros(cf.numel(), dtype=torch.bool)
        keep[int(torch.argmax((cf == cf.max()).int()))] = True
    else:
        keep = cf >= max(min_faces, math.ceil(min_fraction * int(cf.max())))
    vmask = keep[c["vert_comp"]]
    fmask = torch.tensor([fc >= 0 and bool(keep[fc]) for fc in c["face_comp"].tolist()], dtype=torch.bool)
    new = torch.cumsum(vmask.long(), 0) - 1
    return verts[vmask], new[faces.long()[fmask]]


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _coords(V, seed, shift=(0.0, 0.0, 0.0)):
    return torch.rand(V, 3, generator=_gen(seed)) + torch.tensor(shift)


def fan(valence, seed):
    """A closed fan: hub 0 and a rim of `valence` vertices."""
    rim = torch.arange(1, valence + 1)
    return _coords(valence + 1, seed), torch.stack([torch.zeros_like(rim), rim, rim.roll(-1)], 1)


def strip(V, seed):
    """A triangle strip of V vertices under a shuffled numbering: a long diameter with labels that travel far."""
    i = torch.arange(V - 2)
    f = torch.stack([i, i + 1, i + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    perm = torch.randperm(V, generator=_gen(seed))
    return _coords(V, seed + 1), perm[f]


def separate_triangles(n, unused, seed):
    f = torch.arange(3 * n).view(n, 3)
    perm = torch.randperm(3 * n + unused, generator=_gen(seed))
    return _coords(3 * n + unused, seed + 1), perm[f]


def bad_faces(seed):
    """V = 12: good faces mixed with faces that repeat an index and faces with the indices -1 and V."""
    V = 12
    f = torch.tensor([[0, 1, 2], [2, 2, 3], [3, 4, 5], [4, 5, 5], [6, 6, 6], [-1, 7, 8], [7, 8, V], [8, 9, 10], [0, 1, V + 5], [9, 10, 8],
                      [5, 3, 4], [11, -1, -1]])
    return _coords(V, seed), f


def island_cloud():
    """A 1024-point sphere (r = 0.4, noise 0.008) plus 48 points on a sphere of r = 0.06 at x = 0.75."""
    g = _gen(3211)
    p, n = S.sphere(g, 1024, 0.4, noise=0.008)
    q, m = S.sphere(g, 48, 0.06)
    return torch.cat([p, q + torch.tensor([0.75, 0.0, 0.0])]), torch.cat([n, m])


@functools.lru_cache(maxsize=None)
def island_mesh():
    r = S.reconstruct(*island_cloud(), 32, 3)
    return r["verts"], r["faces"].long()


@functools.lru_cache(maxsize=None)
def two_spheres_mesh():
    r = S.reconstruct(*S.two_spheres(_gen(3212), 1024), 32, 3)
    return r["verts"], r["faces"].long()


@functools.lru_cache(maxsize=None)
def clean_sphere_mesh():
    r = S.reconstruct(*S.sphere(_gen(3211), 1024, 0.4), 32, 3)
    return r["verts"], r["faces"].long()


def _small():
    tri = torch.tensor([[0, 1, 2]])
    return {
        "one_vertex": (_coords(1, 10), torch.zeros(0, 3, dtype=torch.int64)),
        "one_triangle": (_coords(3, 11), tri),
        "two_triangles_consistent": (_coords(4, 12), torch.tensor([[0, 1, 2], [2, 1, 3]])),
        "two_triangles_against": (_coords(4, 13), torch.tensor([[0, 1, 2], [1, 2, 3]])),
        "same_face_twice": (_coords(3, 14), torch.tensor([[0, 1, 2], [0, 1, 2]])),
        "fan_70": fan(70, 15),
        "fan_300": fan(300, 16),
        "empty": (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)),
        "strip_255": strip(255, 20), "strip_256": strip(256, 22), "strip_257": strip(257, 24), "strip_1025": strip(1025, 26),
        "triangles_200_unused_10": separate_triangles(200, 10, 30),
        "bad_faces": bad_faces(32),
        "shifted": (_coords(4, 34, (100.0, -50.0, 25.0)), torch.tensor([[0, 1, 2], [2, 1, 3]])),
    }


@functools.lru_cache(maxsize=None)
def batch():
    """The ragged batch of the GPU test, in order: [(name, verts (V, 3) float32, faces (F, 3) int64)]."""
    out = [(k, v.float(), f.long()) for k, (v, f) in _small().items()]
    out.append(("two_spheres", *two_spheres_mesh()))
    out.append(("island", *island_mesh()))
    return out


@functools.lru_cache(maxsize=None)
def batch_components():
    return [components(f, v.shape[0]) for _, v, f in batch()]


@functools.lru_cache(maxsize=None)
def batch_taubin(mode, num_iter, lambd=LAMBD, mu=MU):
    return [taubin(v, c["first"], c["nbr"], lambd, mu, num_iter, mode) for (_, v, _), c in zip(batch(), batch_components())]


def coincident_mesh():
    """Two triangles on a common side whose vertices 1 and 2, neighbours, coincide: w = 1 / 1e-12f."""
    v = _coords(4, 40)
    v[2] = v[1]
    return v, torch.tensor([[0, 1, 2], [2, 1, 3]])


def nan_mesh():
    """fan_70 with the coordinates of rim vertex 5 NaN."""
    v, f = fan(70, 15)
    v = v.clone()
    v[5] = float("nan")
    return v, f


def radial_spread(v):
    r = (v.double() - v.double().mean(0)).norm(dim=1)
    return float(r.std() / r.mean())


def signed_volume(v, f):
    tri = v.double()[f.long()]
    return float((tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum() / 6.0)
