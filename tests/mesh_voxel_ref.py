"""The solid-voxelisation rule of include/bdm_hip.h section 21 restated on the CPU: numpy.float32 for the
snap, integers for everything else.  The integers are numpy int64 so that a mesh of thousands of faces takes a moment, and the
magnitudes that int64 must hold are bounded first with Python's unbounded integers (_assert_bounds).  Nothing here is shared with
bdm_amd/csrc/mesh_voxel.hip.  Named mutants change one clause each; tests/test_mesh_voxel_host.py shows that every one of them is told
apart from the rule by a hand mesh.

The rule in short.  Grid of R cells per axis, origin o, cell size h; a vertex snaps to q_a = rintf(((v_a - o_a) / h) * 256) in float32,
usable when finite with every |q_a| <= 2^19; cell centre i sits at 256 i + 128.  A face with an index out of range, a repeated index
or an unusable vertex is dropped and counted.  Every predicate is evaluated at the centre moved by (eps, eps^2, eps^3): along axis w,
with (u, v) the two other axes in increasing order, a column centre is covered when the three edge functions of the face (wound
positive in (u, v)) are > 0, or == 0 on an edge with dv < 0 or (dv == 0 and du > 0); cell k of a covered column is below the face when
sign~(n . (p_k - a)) sign(n_w) < 0, sign~ of zero being the sign of the first non-zero of (n_x, n_y, n_z); the face flips the parity of
the cells below it.  A cell is inside along an axis when its flips are odd."""
import functools
import math

import numpy as np
import torch

SNAP, HALF = 256, 128
GUARD = 2 ** 19
MAX_R = 512
MODES = {"vote": 0, "x": 1, "y": 2, "z": 3}
MUTANTS = ("render_owns", "tie_not_below", "owns_both", "no_swap", "cyclic_uv", "truncate_snap")
COUNT_KEYS = ("faces_used", "faces_dropped", "occupied_x", "occupied_y", "occupied_z", "occupied", "disagree", "reserved")
UV = {0: (1, 2), 1: (0, 2), 2: (0, 1)}          # the projection plane of the ray along w: the two other axes in increasing order
UV_CYCLIC = {0: (1, 2), 1: (2, 0), 2: (0, 1)}   # the mutant's


def f32(x):
    return np.asarray(x, dtype=np.float32)


def default_frame(verts_np, R):
    """-> (origin float32 (3,), cell float32): the bounding cube of the finite vertices, h = side / R in float32; side 1 where the
    largest extent is zero or not finite (no finite vertex: origin 0)."""
    v = f32(verts_np).reshape(-1, 3)
    fin = np.isfinite(v).all(axis=1) if v.shape[0] else np.zeros(0, dtype=bool)
    if not fin.any():
        return np.zeros(3, dtype=np.float32), np.float32(np.float32(1) / np.float32(R))
    lo, hi = v[fin].min(axis=0), v[fin].max(axis=0)
    with np.errstate(over="ignore"):
        side = np.float32((hi - lo).max())
    if not (side > 0 and np.isfinite(side)):
        side = np.float32(1)
    return lo.astype(np.float32), np.float32(side / np.float32(R))


def pair_frame(verts_a, verts_b, R):
    """The bounding cube of the two meshes of a pair together."""
    return default_frame(np.concatenate([f32(verts_a).reshape(-1, 3), f32(verts_b).reshape(-1, 3)]), R)


def snap(verts_np, origin, cell, mutant=None):
    """-> (q int64 (V, 3), usable bool (V,)): float32, operation by operation; ties to even."""
    v = f32(verts_np).reshape(-1, 3)
    o, h = f32(origin).reshape(1, 3), np.float32(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        p = ((v - o) / h).astype(np.float32) * np.float32(SNAP)
        q = np.trunc(p) if mutant == "truncate_snap" else np.rint(p)
        usable = np.isfinite(v).all(axis=1) & (np.abs(q) <= np.float32(GUARD)).all(axis=1)   # NaN fails the comparison
    return np.where(usable[:, None], q, 0).astype(np.int64), usable


def _assert_bounds(q, R):
    """With Python integers: differences of snapped coordinates and of a centre and a vertex stay within 2^20, hence normal components
    within 2^41 and g within 3 2^61 < 2^63, which is what the int64 arithmetic below needs."""
    top = int(np.abs(q).max()) if q.size else 0
    assert top <= GUARD and 1 <= R <= MAX_R
    diff = max(2 * top, SNAP * (R - 1) + HALF + top)
    assert diff <= 2 ** 20
    normal = 2 * diff * diff
    assert normal <= 2 ** 41
    assert 3 * normal * diff <= 3 * 2 ** 61 < 2 ** 63


def _span(lo, hi, R):
    """Cell centres 256 i + 128 inside [lo, hi], clamped to the grid: first and last index (first > last: none)."""
    first = np.maximum(-((HALF - lo) // SNAP), 0)   # ceil((lo - 128) / 256)
    last = np.minimum((hi - HALF) // SNAP, R - 1)
    return first, last


def _sign(x):
    return (x > 0).astype(np.int64) - (x < 0).astype(np.int64)


def _owned(du, dv, mutant):
    if mutant == "render_owns":
        return (dv > 0) | ((dv == 0) & (du > 0))
    if mutant == "owns_both":
        return np.ones_like(du, dtype=bool)
    return (dv < 0) | ((dv == 0) & (du > 0))


def axis_flips(q, tri, R, w, mutant=None):
    """The flip counts of the used faces `tri` (F, 3 vertex rows) along axis w -> int64 (R, R, R) indexed [ix][iy][iz]: how many faces
    have their highest cell below them exactly here (c - 1 along w)."""
    flips = np.zeros((R, R, R), dtype=np.int64)
    if tri.shape[0] == 0:
        return flips
    u, v = (UV_CYCLIC if mutant == "cyclic_uv" else UV)[w]
    a, b, c = q[tri[:, 0]], q[tri[:, 1]], q[tri[:, 2]]
    area = (b[:, u] - a[:, u]) * (c[:, v] - a[:, v]) - (b[:, v] - a[:, v]) * (c[:, u] - a[:, u])
    keep = area != 0
    if mutant == "no_swap":
        keep &= area > 0
    a, b, c, area = a[keep], b[keep], c[keep], area[keep]
    flip = area < 0
    b2, c2 = np.where(flip[:, None], c, b), np.where(flip[:, None], b, c)   # wound positive in (u, v)
    n = np.cross(b - a, c - a)                                            # the face's own order (the product below does not depend on it)
    u0, u1 = _span(np.minimum(a[:, u], np.minimum(b[:, u], c[:, u])), np.maximum(a[:, u], np.maximum(b[:, u], c[:, u])), R)
    v0, v1 = _span(np.minimum(a[:, v], np.minimum(b[:, v], c[:, v])), np.maximum(a[:, v], np.maximum(b[:, v], c[:, v])), R)
    nu, nv = np.maximum(u1 - u0 + 1, 0), np.maximum(v1 - v0 + 1, 0)
    count = nu * nv
    face = np.repeat(np.arange(a.shape[0]), count)                         # one row per (face, column of its box)
    if face.size == 0:
        return flips
    within = np.arange(face.size) - np.repeat(np.cumsum(count) - count, count)
    iu, iv = u0[face] + within % nu[face], v0[face] + within // nu[face]
    pu, pv = SNAP * iu + HALF, SNAP * iv + HALF
    A, B, C, N = a[face], b2[face], c2[face], n[face]
    covered = np.ones(face.size, dtype=bool)
    for s, e in ((B, C), (C, A), (A, B)):
        du, dv = e[:, u] - s[:, u], e[:, v] - s[:, v]
        edge = du * (pv - s[:, v]) - dv * (pu - s[:, u])
        covered &= (edge > 0) | ((edge == 0) & _owned(du, dv, mutant))
    iu, iv, A, N = iu[covered], iv[covered], A[covered], N[covered]
    pu, pv = pu[covered], pv[covered]
    # g(k) = g0 + 256 n_w k; below(k) <=> G(k) = sign(n_w) g(k) < 0, or == 0 with a negative tie
    g0 = N[:, u] * (pu - A[:, u]) + N[:, v] * (pv - A[:, v]) + N[:, w] * (HALF - A[:, w])
    sw = _sign(N[:, w])
    first = np.where(N[:, 0] != 0, N[:, 0], np.where(N[:, 1] != 0, N[:, 1], N[:, 2]))
    tie_below = (_sign(first) * sw < 0) if mutant != "tie_not_below" else np.zeros(sw.shape, dtype=bool)
    G0, D = sw * g0, SNAP * np.abs(N[:, w])
    cells = np.where(tie_below, (-G0) // D + 1, -(G0 // D))               # floor division: the cells with G < 0, or <= 0
    cells = np.clip(cells, 0, R)

    def below(k):
        G = G0 + D * k
        return (G < 0) | ((G == 0) & tie_below)
    assert bool((below(cells - 1) | (cells == 0)).all()) and not bool((below(cells) & (cells < R)).any()), "below is not monotone"
    hit = cells > 0
    idx = [None, None, None]
    idx[u], idx[v], idx[w] = iu[hit], iv[hit], cells[hit] - 1
    np.add.at(flips, tuple(idx), 1)
    return flips


def used_faces(faces_np, V, usable):
    """-> (the rows of the used faces (F', 3) int64, the number dropped)."""
    f = np.asarray(faces_np, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f, 0
    ok = ((f >= 0) & (f < V)).all(axis=1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    ok[ok] &= usable[f[ok]].all(axis=1)
    return f[ok], int((~ok).sum())


def voxelize(verts, faces, R, origin=None, cell=None, mode="vote", mutant=None):
    """One mesh -> dict(occupancy bool (R, R, R) indexed [ix][iy][iz], axes uint8 (bits 0..2: inside along x, y, z), inside: the three
    bool grids, counts: the eight numbers of COUNT_KEYS, info: the same by name, origin, cell)."""
    assert mode in MODES and 1 <= R <= MAX_R
    vn = f32(torch.as_tensor(verts).float().reshape(-1, 3).numpy())
    if origin is None or cell is None:
        assert origin is None and cell is None
        origin, cell = default_frame(vn, R)
    origin, cell = f32(origin).reshape(3), np.float32(cell)
    assert cell > 0 and np.isfinite(cell)
    q, usable = snap(vn, origin, cell, mutant)
    _assert_bounds(q, R)
    tri, dropped = used_faces(torch.as_tensor(faces).reshape(-1, 3).numpy(), vn.shape[0], usable)
    inside = []
    for w in range(3):
        flips = axis_flips(q, tri, R, w, mutant)
        suffix = np.flip(np.cumsum(np.flip(flips, axis=w), axis=w), axis=w)   # flips at or above the cell
        inside.append((suffix & 1).astype(bool))
    votes = inside[0].astype(np.int64) + inside[1] + inside[2]
    occ = votes >= 2 if mode == "vote" else inside[MODES[mode] - 1]
    axes = (inside[0].astype(np.uint8) | (inside[1].astype(np.uint8) << 1) | (inside[2].astype(np.uint8) << 2))
    disagree = int(((votes != 0) & (votes != 3)).sum())
    counts = [int(tri.shape[0]), dropped, int(inside[0].sum()), int(inside[1].sum()), int(inside[2].sum()), int(occ.sum()), disagree, 0]
    return {"occupancy": torch.from_numpy(np.ascontiguousarray(occ)), "axes": torch.from_numpy(np.ascontiguousarray(axes)),
            "inside": [torch.from_numpy(np.ascontiguousarray(g)) for g in inside], "counts": counts, "info": dict(zip(COUNT_KEYS, counts)),
            "origin": origin, "cell": cell}


def iou(a, b):
    """Two bool grids of one shape -> (iou float (nan for an empty union), intersection, union): exact integers."""
    a, b = torch.as_tensor(a).bool(), torch.as_tensor(b).bool()
    assert a.shape == b.shape
    inter, union = int((a & b).sum()), int((a | b).sum())
    return (inter / union if union else float("nan")), inter, union


def odd_degree_edges(faces, V):
    """The number of undirected edges that an odd number of the connected faces share (0: every ray crosses the surface an even
    number of times wherever the faces are)."""
    f = torch.as_tensor(faces).reshape(-1, 3).long().numpy()
    if f.shape[0] == 0:
        return 0
    ok = ((f >= 0) & (f < V)).all(axis=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = f[ok]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n & 1).sum())


# ---- hand-built meshes ----------------------------------------------------------------------------------------------------------------
BOX_F = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]
OCTA_F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]


def _v(rows):
    return torch.tensor(rows, dtype=torch.float64).float().reshape(-1, 3)


def _f(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def box(lo, hi):
    """The axis-aligned box lo .. hi (two corners), twelve outward faces; vertex index = x + 2 y + 4 z."""
    return _v([(x, y, z) for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])]), _f(BOX_F)


def lattice_box(lo=(1, 2, 1), hi=(6, 5, 7)):
    """A box whose faces pass exactly through cell centres, in the frame origin 0, cell 1: corner i means the centre of cell i.  Under
    the rule it is the cells lo <= i < hi (low-inclusive, high-exclusive); with equal extents on two axes the face diagonals pass
    through centres too."""
    return box([c + 0.5 for c in lo], [c + 0.5 for c in hi])


def octahedron(centre=(3.5, 3.5, 3.5), radius=3.0):
    """Vertices on cell centres (frame origin 0, cell 1): +-x, +-y, +-z; outward faces."""
    c = torch.tensor(centre, dtype=torch.float64)
    rows = [c + radius * torch.tensor(d, dtype=torch.float64) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    return torch.stack(rows).float(), _f(OCTA_F)


def uv_sphere(stacks=24, slices=48, radius=0.4, centre=(0.013, -0.021, 0.034)):
    """2 slices + 2 slices (stacks - 2) faces: 2208 at the defaults."""
    rows = [(0.0, 0.0, radius)]
    for i in range(1, stacks):
        th = math.pi * i / stacks
        for j in range(slices):
            ph = 2 * math.pi * j / slices
            rows.append((radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)))
    rows.append((0.0, 0.0, -radius))
    south, faces = len(rows) - 1, []

    def ring(i, j):
        return 1 + (i - 1) * slices + j % slices
    for j in range(slices):
        faces.append((0, ring(1, j), ring(1, j + 1)))
        faces.append((south, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
        for i in range(1, stacks - 1):
            faces.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            faces.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return (_v(rows).double() + torch.tensor(centre, dtype=torch.float64)).float(), _f(faces)


def reversed_every_other(faces):
    f = torch.as_tensor(faces).clone()
    f[1::2] = f[1::2][:, [0, 2, 1]]
    return f


SURFACE_CLOUDS = {"sphere": (2048, 16, 3), "torus": (4096, 16, 3), "ellipsoid": (2048, 16, 3), "two_spheres": (4096, 24, 3),
                  "open_sphere": (512, 32, 2)}


@functools.lru_cache(maxsize=None)
def surface_mesh(name):
    """The surface-nets meshes of surface_ref.reconstruct: name -> (verts, faces); points, resolution and support of SURFACE_CLOUDS.  The
    first four are closed; "open_sphere" (512 points at resolution 32) has holes."""
    import surface_ref as S
    n, R, s = SURFACE_CLOUDS[name]
    g = torch.Generator().manual_seed(2500 + sorted(SURFACE_CLOUDS).index(name))
    p, nr = {"sphere": S.sphere, "torus": S.torus, "ellipsoid": S.ellipsoid, "two_spheres": S.two_spheres, "open_sphere": S.sphere}[name](g, n)
    m = S.reconstruct(p, nr, R, s)
    return m["verts"].float(), m["faces"].long()


def hand_meshes():
    """name -> (verts, faces, origin or None, cell or None): a given frame, or the mesh's own bounding cube."""
    nan, inf = float("nan"), float("inf")
    lv, lf = lattice_box()
    cv, cf = lattice_box((1, 1, 1), (6, 6, 6))
    ov, of = octahedron()
    sv, sf = uv_sphere()
    tv, tf = box((0.3, 0.2, 0.1), (5.1, 6.3, 7.2))
    bad = torch.cat([tf, _f([(0, 0, 1), (0, 1, 8), (-1, 2, 3)])])
    nf = torch.cat([tv, _v([(nan, 0, 0), (1, inf, 2)])])
    far = torch.cat([tv, _v([(2048.0, 1, 1), (2048.00390625, 1, 1)])])   # q = 2^19 and 2^19 + 1 in the frame origin 0, cell 1
    return {
        "lattice_box": (lv, lf, (0, 0, 0), 1.0),
        "lattice_cube": (cv, cf, (0, 0, 0), 1.0),
        "octahedron": (ov, of, (0, 0, 0), 1.0),
        "uv_sphere": (sv, sf, None, None),
        "uv_sphere_mixed_winding": (sv, reversed_every_other(sf), None, None),
        "tilted_box": (tv @ _rot().T, tf, None, None),
        "bad_indices": (tv, bad, (0, 0, 0), 1.0),
        "nonfinite": (nf, torch.cat([tf, _f([(0, 1, 8), (2, 9, 3)])]), (0, 0, 0), 1.0),
        "beyond_guard": (far, torch.cat([tf, _f([(0, 1, 8), (0, 1, 9)])]), (0, 0, 0), 1.0),
        "above_and_below": (_v([(1, 1, 100), (6, 1, 100), (1, 6, 100), (1, 1, -100), (6, 1, -100), (1, 6, -100)]), _f([(0, 1, 2), (3, 4, 5)]),
                            (0, 0, 0), 1.0),
        "open_box": (tv, tf[:10], None, None),
        "big_triangle": (_v([(-3, -2, 0.1), (40, -1, 3.3), (-2, 41, 6.9)]), _f([(0, 1, 2)]), (0, 0, 0), 1.0),
        "no_faces": (tv, _f([]), None, None),
        "empty": (torch.zeros(0, 3), _f([]), None, None),
    }


def _rot():
    a, b = 0.37, 0.81
    rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], dtype=torch.float64)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float64)
    return (rz @ rx).float()


@functools.lru_cache(maxsize=None)
def batch():
    """Every mesh of the tables as one ragged batch: a tuple of (name, verts, faces, origin or None, cell or None).  A hand mesh with a
    frame keeps it at every R (cells beyond R are simply outside the grid); the others take their own bounding cube."""
    rows = [(k, *v) for k, v in hand_meshes().items()]
    rows += [(k, *surface_mesh(k), None, None) for k in SURFACE_CLOUDS]
    return tuple(rows)


def frame_of(row, R):
    """(origin float32 (3,), cell float32) of a row of batch() at resolution R."""
    _, v, _, origin, cell = row
    if origin is None:
        return default_frame(v.numpy(), R)
    return f32(origin), np.float32(cell)


# ---- binvox, written by hand for the reader's tests --------------------------------------------------------------------------------------
def binvox_bytes(voxels, translate=(0.0, 0.0, 0.0), scale=1.0):
    """The file of a (D, D, D) bool grid indexed [x][y][z]: linear index x D^2 + z D + y, runs of at most 255."""
    vox = np.asarray(voxels, dtype=bool)
    D = vox.shape[0]
    flat = vox.transpose(0, 2, 1).reshape(-1)
    head = f"#binvox 1\ndim {D} {D} {D}\ntranslate {translate[0]} {translate[1]} {translate[2]}\nscale {scale}\ndata\n".encode("ascii")
    body, i = bytearray(), 0
    while i < flat.size:
        j = i
        while j < flat.size and flat[j] == flat[i] and j - i < 255:
            j += 1
        body += bytes((int(flat[i]), j - i))
        i = j
    return head + bytes(body)
