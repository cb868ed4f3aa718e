"""The vertex-clustering rule of include/bdm_hip.h section 20 restated on the CPU in plain Python: dictionaries
and Python integers for everything combinatorial, numpy.float32 for the two float32 operations of the key (and of the cell size), and
mesh_fill_ref's fixed-point mean (Python floats, one numpy float32 rounding).  Nothing here is shared with
bdm_amd/csrc/mesh_decimate.hip.  Named mutants change one clause each; tests/test_mesh_decimate_host.py shows that every one of them
is told apart from the rule by at least one mesh of the table below."""
import functools
from fractions import Fraction

import numpy as np
import torch

import mesh_fill_ref as MF
from mesh_fill_ref import bits, same_floats  # noqa: F401  (the tests compare with them)

MUTANTS = ("leader_largest", "order_by_key", "anchor_origin", "mean_singletons", "mean_f32", "oriented_duplicates", "keep_highest",
           "keep_collapsed")
COLLAPSED, DUPLICATE, BAD = -1, -2, -3
MAX_CELL = 2 ** 21 - 1
INFO_KEYS = ("new_vertices", "new_faces", "collapsed_faces", "duplicate_faces", "bad_faces", "nonfinite_vertices", "largest_cluster",
             "merged_vertices")


def bounds(vn):
    """(finite mask, lo, hi): lo / hi float32 (3,) over the finite vertices, None without one."""
    fin = np.isfinite(vn).all(axis=1) if vn.shape[0] else np.zeros(0, dtype=bool)
    if not fin.any():
        return fin, None, None
    return fin, vn[fin].min(axis=0), vn[fin].max(axis=0)


def cell_size(vn, voxel_size=None, resolution=None):
    """Rule 2 -> numpy.float32."""
    assert (voxel_size is None) != (resolution is None)
    if voxel_size is not None:
        return np.float32(voxel_size)
    _, lo, hi = bounds(vn)
    h = np.float32(0)
    if lo is not None:
        with np.errstate(over="ignore"):
            ext = max(np.float32(hi[a] - lo[a]) for a in range(3))   # float32 - float32 -> float32
            h = np.float32(ext / np.float32(resolution))
    return h if h > 0 and np.isfinite(h) else np.float32(1)


def cell(c, lo, h):
    """Rule 3 for one coordinate -> Python int."""
    with np.errstate(over="ignore"):
        q = np.float32(np.float32(np.float32(c) - np.float32(lo)) / h)
    return int(np.floor(q)) if q < 2 ** 21 else MAX_CELL


def _mean(col, e, mutant):
    if mutant == "mean_f32":
        acc = np.float32(0)
        for c in col:
            acc = np.float32(acc + c)
        return np.float32(acc / np.float32(len(col)))
    return MF.fixed_mean(col, e)


def decimate(verts, faces, voxel_size=None, resolution=None, contraction="average", attrs=None, mutant=None):
    """One mesh (verts (V, 3) float32, faces (F, 3) integer, attrs (V, C) float32 or None) -> dict(verts, faces, attrs, vert_map (V,),
    face_map (F,), info, h, clusters: the member lists in new-vertex order)."""
    assert contraction in ("average", "first")
    verts = torch.as_tensor(verts).float().reshape(-1, 3)
    faces_t = torch.as_tensor(faces).reshape(-1, 3)
    V = verts.shape[0]
    attrs = torch.zeros(V, 0) if attrs is None else torch.as_tensor(attrs).float()
    vn, an = verts.numpy(), attrs.numpy()
    fin, lo, hi = bounds(vn)
    h = cell_size(vn, voxel_size, resolution)
    if mutant == "anchor_origin":
        lo = np.zeros(3, dtype=np.float32)
    members = {}   # key -> member indices, ascending
    for v in range(V):
        key = tuple(cell(vn[v, a], lo[a], h) for a in (2, 1, 0)) if fin[v] else ("nonfinite", v)   # (kz, ky, kx) orders as the packed key
        members.setdefault(key, []).append(v)
    leader = (lambda m: max(m)) if mutant == "leader_largest" else (lambda m: min(m))   # noqa: E731
    if mutant == "order_by_key":
        order = sorted(members, key=lambda k: (isinstance(k[0], str), k))
    else:
        order = sorted(members, key=lambda k: leader(members[k]))
    clusters = [members[k] for k in order]
    vert_map = [0] * V
    for new, m in enumerate(clusters):
        for v in m:
            vert_map[v] = new
    ev, ea = MF.scale_exp(vn), MF.scale_exp(an)
    out_v, out_a = np.empty((len(clusters), 3), dtype=np.float32), np.empty((len(clusters), an.shape[1]), dtype=np.float32)
    for new, m in enumerate(clusters):
        lead = leader(m)
        through_mean = len(m) > 1 or (mutant == "mean_singletons" and fin[lead])
        if contraction == "first" or not through_mean:
            out_v[new], out_a[new] = vn[lead], an[lead]   # bit for bit
            continue
        for d in range(3):
            out_v[new, d] = _mean(vn[m, d], ev, mutant)
        for d in range(an.shape[1]):
            col = an[m, d]
            out_a[new, d] = _mean(col, ea, mutant) if np.isfinite(col).all() else np.nan
    face_map, keys, chosen = [], {}, {}   # keys: old index -> the key of a face that is judged; chosen: key -> the old index that stays
    rows = [tuple(int(i) for i in f) for f in faces_t.tolist()]
    for i, f in enumerate(rows):
        if not MF.connected(f, V):
            face_map.append(BAD)
            continue
        nf = tuple(vert_map[x] for x in f)
        if len(set(nf)) < 3:
            face_map.append(None if mutant == "keep_collapsed" else COLLAPSED)
            continue
        if mutant == "oriented_duplicates":
            at = nf.index(min(nf))
            keys[i] = nf[at:] + nf[:at]
        else:
            keys[i] = tuple(sorted(nf))
        chosen[keys[i]] = i if mutant == "keep_highest" else chosen.get(keys[i], i)
        face_map.append(None if chosen[keys[i]] == i else DUPLICATE)
    for i, key in keys.items():   # keep_highest: the earlier ones lose
        if chosen[key] != i:
            face_map[i] = DUPLICATE
    kept = [(i, tuple(vert_map[x] for x in rows[i])) for i in range(len(rows)) if face_map[i] is None]
    for new, (i, _) in enumerate(kept):
        face_map[i] = new
    sizes = [len(m) for m in clusters]
    info = dict(zip(INFO_KEYS, (len(clusters), len(kept), face_map.count(COLLAPSED), face_map.count(DUPLICATE), face_map.count(BAD),
                                int((~fin).sum()), max(sizes, default=0), sum(s for s in sizes if s > 1))))
    return {"verts": torch.from_numpy(out_v), "attrs": torch.from_numpy(out_a),
            "faces": torch.tensor([nf for _, nf in kept], dtype=faces_t.dtype).reshape(-1, 3),
            "vert_map": torch.tensor(vert_map, dtype=torch.int64), "face_map": torch.tensor(face_map, dtype=torch.int64), "info": info,
            "h": h, "clusters": clusters}


def spread_bound(h, lo, hi, a):
    """two finite vertices of one cell differ along axis a by less than this, as an exact rational, provided no
    quotient of the mesh clamps."""
    h, ext = Fraction(float(h)), Fraction(float(hi[a])) - Fraction(float(lo[a]))
    return h * (1 + Fraction(1, 2 ** 22)) + Fraction(1, 2 ** 22) * (1 + Fraction(1, 2 ** 21)) * ext


# ---- hand-built meshes ----------------------------------------------------------------------------------------------------------------
CUBE_V = [(x, y, z) for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)]   # vertex index = x + 2 y + 4 z
CUBE_F = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]


def _v(rows):
    return torch.tensor(rows, dtype=torch.float64).float().reshape(-1, 3)


def _f(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def hand_meshes():
    """name -> (verts, faces, kwargs of decimate): the table of the issue."""
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(2024)
    quad = [(0, 0), (1, 0), (1, 1), (0, 1)]
    sheets = _v([(x, y, 0.0) for x, y in quad] + [(x, y, 0.1) for x, y in quad])
    blob = torch.rand(60, 3, generator=g, dtype=torch.float64).float() * 0.5 + 100.0   # amax near 100: E = 6
    blob[7] = torch.tensor([3.0e-6, 99.0, 104.0])                                       # alone in its cell, low bits below 2^-33
    crowd = torch.rand(40, 3, generator=g, dtype=torch.float64).float()                # 40 random members in one cell
    return {
        "cube_r1": (_v(CUBE_V), _f(CUBE_F), dict(resolution=1)),            # k = 0 or 1 = R on every axis: eight cells
        "cube_r2": (_v(CUBE_V), _f(CUBE_F), dict(resolution=2)),
        "cube_one_cell": (_v(CUBE_V), _f(CUBE_F), dict(voxel_size=2.0)),    # one vertex, no face, 12 collapsed
        "two_triangles": (_v([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, 1, 0.1)]), _f([(0, 1, 2), (1, 0, 3)]), dict(voxel_size=0.5)),
        "parallel_quads": (sheets, _f([(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6)]), dict(voxel_size=0.6)),
        "vertex_at_hi": (_v([(0, 0, 0), (0.5, 0, 0), (1.0, 0, 0), (0.75, 0.1, 0)]), _f([(0, 1, 3), (1, 2, 3)]), dict(resolution=2)),
        "coincident": (_v([(0.3, -2.0, 7.0)] * 3), _f([(0, 1, 2)]), dict(resolution=8)),
        "clamped": (_v([(0, 0, 0), (1, 0, 0), (3, 0, 0), (0, 1, 0)]), _f([(0, 1, 3), (1, 2, 3)]), dict(voxel_size=1e-7)),
        "nonfinite": (_v([(0, 0, 0), (nan, 0, 0), (1, 0, 0), (1, inf, 0), (0.01, 0, 0), (nan, 0, 0), (1, 1, 0)]),
                      _f([(0, 1, 2), (4, 5, 2), (0, 2, 6), (4, 2, 6), (3, 2, 6)]), dict(resolution=4)),
        "all_nonfinite": (_v([(nan, 0, 0), (0, inf, 0), (0, 0, -inf)]), _f([(0, 1, 2)]), dict(resolution=4)),
        "bad_indices": (_v(CUBE_V), _f(CUBE_F[:4] + [(0, 0, 1), (0, 1, 8), (-1, 2, 3), (5, 6, 5)]), dict(voxel_size=0.75)),
        "no_faces": (torch.rand(9, 3, generator=g), _f([]), dict(resolution=2)),
        "empty": (torch.zeros(0, 3), _f([]), dict(resolution=4)),
        "interleaved": (_v([(0.9, 0.9, 0.9), (0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (0.8, 0.9, 0.9), (0.1, 0.9, 0.1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]),
                        _f([(0, 1, 4), (3, 4, 2), (4, 1, 0)]), dict(resolution=2)),
        "shifted": (blob, torch.randint(0, 60, (80, 3), generator=g), dict(voxel_size=0.125)),
        "crowd": (crowd, torch.randint(0, 40, (30, 3), generator=g), dict(voxel_size=4.0)),
    }


@functools.lru_cache(maxsize=None)
def surface_mesh(name):
    v, f = MF.surface_mesh(name)
    return v, f


SURFACE_MESHES = ("sphere600", "torus1500")


def attrs_for(V, seed):
    """(V, 5) float32: three uint8 colour channels as floats, two float channels; the last one holds NaNs at every seventh vertex."""
    u8, fl = MF.colors_for(V, seed)
    a = torch.cat([u8.float(), fl], dim=1)
    a[::7, 4] = float("nan")
    return a


@functools.lru_cache(maxsize=None)
def batch():
    """Every mesh of the tables as one ragged batch: a tuple of (name, verts, faces, attrs (V, 5), voxel_size); the voxel size is used by
    the runs that give one per mesh (the hand mesh's own, or the cell of its resolution; the surface meshes: 0.07)."""
    rows = []
    for i, (name, (v, f, kw)) in enumerate(hand_meshes().items()):
        h = kw["voxel_size"] if "voxel_size" in kw else float(cell_size(v.numpy(), resolution=kw["resolution"]))
        rows.append((name, v, f, attrs_for(v.shape[0], i), h))
    for i, name in enumerate(SURFACE_MESHES):
        v, f = surface_mesh(name)
        rows.append((name, v, f, attrs_for(v.shape[0], 100 + i), 0.07))
    return tuple(rows)


# ---- large meshes with a closed form --------------------------------------------------------------------------------------------------
def grid_triangles(n, unused, seed, merge):
    """mesh_fill_ref.separate_triangles' n triangles under its shuffled numbering, every face four times (as it is, rotated, reversed,
    rotated and reversed), on coordinates of this function's own: with merge = False vertex j sits alone at the corner of cell j of a
    64 x 64 x many grid of unit cells; with merge = True the three vertices of triangle t share cell t and every unused vertex has a
    cell of its own.  voxel_size = 1.  -> (verts, faces (4 n, 3), expected): the integer entries of decimate()'s dict in closed form,
    for sizes at which its Python loops are too slow (tests/test_mesh_decimate_host.py holds this against decimate())."""
    _, tri = MF.separate_triangles(n, unused, seed)
    V = 3 * n + unused
    faces = torch.cat([tri, tri[:, [1, 2, 0]], tri[:, [2, 1, 0]], tri[:, [0, 2, 1]]])
    cell_of = torch.arange(V)
    offset = torch.zeros(V, dtype=torch.float64)
    if merge:
        used = torch.zeros(V, dtype=torch.bool)
        used[tri.flatten()] = True
        cell_of[tri.flatten()] = torch.arange(n).repeat_interleave(3)
        cell_of[~used] = n + torch.arange(unused)
        offset[tri.flatten()] = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64).repeat(n)
        offset[~used] = 0.5   # lo is 0.25 along x: every vertex of cell c then has floor(x - 0.25) = c
    verts = torch.stack([(cell_of % 64).double() + offset, ((cell_of // 64) % 64).double(), (cell_of // 4096).double()], dim=1).float()
    if not merge:
        expected = {"vert_map": torch.arange(V), "face_map": torch.cat([torch.arange(n), torch.full((3 * n,), DUPLICATE)]), "faces": tri,
                    "info": dict(zip(INFO_KEYS, (V, n, 0, 3 * n, 0, 0, 1, 0)))}
        return verts, faces, expected
    lead = torch.full((n + unused,), V, dtype=torch.int64).scatter_reduce(0, cell_of, torch.arange(V), reduce="amin")   # per cell
    rank = torch.empty_like(lead)
    rank[lead.argsort()] = torch.arange(n + unused)
    expected = {"vert_map": rank[cell_of], "face_map": torch.full((4 * n,), COLLAPSED), "faces": tri[:0],
                "info": dict(zip(INFO_KEYS, (n + unused, 0, 4 * n, 0, 0, 0, 3, 3 * n))), "cell_of": cell_of}
    return verts, faces, expected
