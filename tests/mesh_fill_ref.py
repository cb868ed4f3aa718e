"""The hole-filling rule of include/bdm_hip.h section 19 restated on the CPU in plain Python: integers for
everything combinatorial, Python's float (float64) and one numpy float32 rounding for the fixed-point mean.  Nothing here is shared
with bdm_amd/csrc/mesh_fill.hip.  Named mutants change one clause each; tests/test_mesh_fill_host.py shows that every one of them is
told apart from the rule by at least one case of the table below."""
import functools
import math

import numpy as np
import torch

import surface_ref as S

MUTANTS = ("wrong_winding", "succ_per_vertex", "fill_pinched", "label_largest", "faces_loop_order", "mean_f32")
FILLED, TOO_LARGE, PINCHED, NONFINITE = 1, 2, 4, 8
INFO_KEYS = ("boundary_edges", "loops", "filled_loops", "too_large_loops", "pinched_loops", "nonfinite_loops", "blocked_edges", "new_vertices",
             "new_faces")


def connected(face, V):
    a, b, c = face
    return all(0 <= i < V for i in face) and a != b and b != c and a != c


def boundary(faces, V, mutant=None):
    """One mesh -> dict(loop: per half-edge the label, -1 not on the boundary, -2 blocked; labels: ascending; succ: {h: h'};
    cycle: {label: its half-edges from the label on}; src: {h: source vertex})."""
    faces = [tuple(int(i) for i in f) for f in torch.as_tensor(faces).reshape(-1, 3).tolist()]
    half = {}   # (a, x) -> the half-edges a -> x
    ends = {}
    for f, face in enumerate(faces):
        if not connected(face, V):
            continue
        for k in range(3):
            a, x = face[k], face[(k + 1) % 3]
            half.setdefault((a, x), []).append(3 * f + k)
            ends[3 * f + k] = (a, x)

    def kind(a, x):
        out, inn = len(half.get((a, x), ())), len(half.get((x, a), ()))
        return "boundary" if (out, inn) == (1, 0) else "interior" if (out, inn) == (1, 1) else "irregular"

    bnd = sorted(h for h, (a, x) in ends.items() if kind(a, x) == "boundary")
    succ = {}
    for h in bnd:
        f, k = divmod(h, 3)
        a, x, cur = faces[f][(k + 1) % 3], faces[f][(k + 2) % 3], 3 * f + (k + 1) % 3
        if mutant == "succ_per_vertex":   # any boundary half-edge out of the target vertex: the smallest
            out = [g for g in bnd if ends[g][0] == a]
            succ[h] = out[0] if out else None
            continue
        while True:
            what = kind(a, x)
            if what == "boundary":
                succ[h] = cur
                break
            if what == "irregular":
                succ[h] = None
                break
            g = half[(x, a)][0]   # the face (x, a, y) across the edge
            f, k = divmod(g, 3)
            x, cur = faces[f][(k + 2) % 3], 3 * f + (k + 1) % 3
    loop = [-1] * (3 * len(faces))
    cycle = {}
    for h in bnd:
        if loop[h] != -1:
            continue
        path, seen, t = [], set(), h
        while t is not None and t not in seen and loop[t] == -1:
            seen.add(t), path.append(t)
            t = succ[t]
        if t is not None and t in seen:   # a cycle closes inside this path; what leads into it (only a mutant's succ does) is blocked
            start = path.index(t)
            members = path[start:]
            label = max(members) if mutant == "label_largest" else min(members)
            at = members.index(label)
            cycle[label] = members[at:] + members[:at]
            for g in members:
                loop[g] = label
            for g in path[:start]:
                loop[g] = -2
        else:   # ended blocked, or ran into something already settled, which (succ being injective on what is not blocked) is blocked
            for g in path:
                loop[g] = -2
    return {"loop": loop, "labels": sorted(cycle), "succ": succ, "cycle": cycle, "src": {h: ends[h][0] for h in bnd}, "faces": faces,
            "boundary": bnd}


def scale_exp(values):
    """e of rule 5 from the finite entries of a float32 array."""
    a = np.abs(np.asarray(values, dtype=np.float32).reshape(-1))
    a = a[np.isfinite(a)]
    amax = np.float32(a.max()) if a.size else np.float32(0)
    field = (int(amax.view(np.uint32)) >> 23) & 0xFF
    return 39 - (max(field, 1) - 127)


def fixed_mean(column, e):
    """The fixed-point mean of finite float32 values."""
    total = sum(round(float(c) * 2.0 ** e) for c in column)   # round: to nearest even, exact integer
    return np.float32((float(total) * 2.0 ** -e) / float(len(column)))


def mean_bound(values, exact_mean):
    """Rule 5's derived bound on |fixed_mean - exact mean| for a mesh whose coordinates are `values`."""
    E = 39 - scale_exp(values)
    return 2.0 ** (E - 40) * (1 + 2.0 ** -23) + (2.0 ** -24 + 2.0 ** -51) * abs(exact_mean)


def _mean_rows(rows, e, mutant):
    rows = np.asarray(rows, dtype=np.float32)
    out = np.empty(rows.shape[1], dtype=np.float32)
    for d in range(rows.shape[1]):
        col = rows[:, d]
        if not np.isfinite(col).all():
            out[d] = np.nan
        elif mutant == "mean_f32":
            acc = np.float32(0)
            for c in col:
                acc = np.float32(acc + c)
            out[d] = np.float32(acc / np.float32(len(col)))
        else:
            out[d] = fixed_mean(col, e)
    return out


def fill(verts, faces, max_hole_edges=32, attrs=None, mutant=None):
    """One mesh (verts (V, 3) float32, faces (F, 3) integer, attrs (V, C) float32 or None) -> dict(verts, faces, attrs, halfedge_loop
    (F, 3), loop_sizes, loop_flags (per loop, ascending label), labels, info)."""
    verts = torch.as_tensor(verts).float().reshape(-1, 3)
    faces_t = torch.as_tensor(faces).reshape(-1, 3)
    V, F = verts.shape[0], faces_t.shape[0]
    attrs = torch.zeros(V, 0) if attrs is None else torch.as_tensor(attrs).float()
    b = boundary(faces_t, V, mutant)
    vn = verts.numpy()
    sizes, flags = [], []
    for label in b["labels"]:
        members = b["cycle"][label]
        src = [b["src"][h] for h in members]
        fl = (TOO_LARGE if len(members) > max_hole_edges else 0) | (PINCHED if len(set(src)) < len(src) else 0)
        fl |= 0 if np.isfinite(vn[src]).all() else NONFINITE
        if mutant == "fill_pinched":
            fl &= ~PINCHED
        sizes.append(len(members)), flags.append(fl or FILLED)
    filled = [label for label, fl in zip(b["labels"], flags) if fl == FILLED]
    new_index = {label: V + r for r, label in enumerate(filled)}
    ev, ea = scale_exp(vn), scale_exp(attrs.numpy())
    new_v = [_mean_rows(vn[[b["src"][h] for h in b["cycle"][label]]], ev, mutant) for label in filled]
    new_a = [_mean_rows(attrs.numpy()[[b["src"][h] for h in b["cycle"][label]]], ea, mutant) for label in filled]
    if mutant == "faces_loop_order":
        order = [h for label in filled for h in b["cycle"][label]]
    else:
        order = [h for h in b["boundary"] if b["loop"][h] in new_index]
    new_f = []
    for h in order:
        f, k = divmod(h, 3)
        a, x = b["faces"][f][k], b["faces"][f][(k + 1) % 3]
        c = new_index[b["loop"][h]]
        new_f.append((a, x, c) if mutant == "wrong_winding" else (x, a, c))
    out_v = torch.cat([verts, torch.from_numpy(np.stack(new_v))]) if new_v else verts.clone()
    out_a = torch.cat([attrs, torch.from_numpy(np.stack(new_a).reshape(len(new_a), attrs.shape[1]))]) if new_a else attrs.clone()
    out_f = torch.cat([faces_t, torch.tensor(new_f, dtype=faces_t.dtype)]) if new_f else faces_t.clone()
    blocked = sum(1 for x in b["loop"] if x == -2)
    info = dict(zip(INFO_KEYS, (len(b["boundary"]), len(sizes), len(filled), sum(1 for x in flags if x & TOO_LARGE),
                                sum(1 for x in flags if x & PINCHED), sum(1 for x in flags if x & NONFINITE), blocked, len(filled), len(new_f))))
    return {"verts": out_v, "faces": out_f, "attrs": out_a, "halfedge_loop": torch.tensor(b["loop"], dtype=torch.int64).reshape(F, 3),
            "loop_sizes": torch.tensor(sizes, dtype=torch.int64), "loop_flags": torch.tensor(flags, dtype=torch.int64), "labels": b["labels"],
            "info": info}


def uint8_mean(column):
    """The correctly rounded (half to even) mean of uint8 values, in integers."""
    total, n = sum(int(c) for c in column), len(column)
    q, r = divmod(total, n)
    return min(255, q + (1 if 2 * r > n or (2 * r == n and q % 2 == 1) else 0))


# ---- hand-built meshes ----------------------------------------------------------------------------------------------------------------
OCTA = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1), (5, 2, 1), (5, 3, 2), (5, 4, 3), (5, 1, 4)]   # apex 0, equator 1..4, nadir 5


def _coords(V, seed, scale=1.0, shift=(0.0, 0.0, 0.0)):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(V, 3, generator=g, dtype=torch.float64) - 0.5) * scale + torch.tensor(shift, dtype=torch.float64)).float()


def _faces(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def hand_meshes():
    """name -> (verts, faces, max_hole_edges): the table of the issue."""
    octa = lambda drop: [f for i, f in enumerate(OCTA) if i not in drop]   # noqa: E731
    return {
        "tetra_open": (_coords(4, 1), _faces([(0, 1, 2), (0, 3, 1), (1, 3, 2)]), 32),
        "two_triangles_one_vertex": (_coords(5, 2), _faces([(0, 1, 2), (0, 3, 4)]), 32),
        "fin": (_coords(5, 3), _faces([(0, 1, 2), (1, 0, 3), (0, 1, 4)]), 32),
        "same_winding": (_coords(4, 4), _faces([(0, 1, 2), (0, 1, 3)]), 32),
        "octa_pinched": (_coords(6, 5), _faces(octa({0, 2})), 32),               # two faces that share only the apex
        "octa_bad_faces": (_coords(6, 6), _faces(octa({0}) + [(0, 0, 1), (0, 1, 9)]), 32),
        "octa_too_large": (_coords(6, 7), _faces(octa({0, 1})), 3),             # two adjacent faces: one loop of 4
        "empty": (torch.zeros(0, 3), _faces([]), 32),
        "no_faces": (_coords(7, 8), _faces([]), 32),
        "octa_closed": (_coords(6, 9), _faces(OCTA), 32),                        # a mesh whose boundary list is empty
        "octa_scaled_1e3": (_coords(6, 10, 2e3), _faces(octa({3})), 32),
        "octa_scaled_1e-3": (_coords(6, 11, 2e-3), _faces(octa({5})), 32),
        "octa_shifted": (_coords(6, 12, 1.0, (100.0, -50.0, 25.0)), _faces(octa({6})), 32),
    }


def nonfinite_meshes():
    """An open octahedron whose hole touches a NaN vertex (not filled), and one whose NaN vertex is away from the hole (filled)."""
    v = _coords(6, 13)
    v[1, 2] = float("nan")
    w = _coords(6, 14)
    w[5, 0] = float("inf")
    faces = _faces([f for i, f in enumerate(OCTA) if i != 0])
    return {"nan_on_rim": (v, faces, 32), "inf_off_rim": (w, faces, 32)}


def fan(valence, seed):
    """A closed fan: hub 0 and a rim of `valence` vertices, the rim its one boundary loop.  The hub has 2 * valence records."""
    rim = torch.arange(1, valence + 1)
    return _coords(valence + 1, seed), torch.stack([torch.zeros_like(rim), rim, rim.roll(-1)], 1)


def fan_meshes():
    """name -> (verts, faces, max_hole_edges): hubs of 32 records (the longest segment the kernel sorts by insertion), of 34 (the
    shortest it heap-sorts) and of 140.  At a cap of 64 the rims of the first two are filled and the third is too large."""
    return {f"fan_{n}": (*fan(n, 40 + n), 64) for n in (16, 17, 70)}


def separate_triangles(n, unused, seed):
    """n triangles without a common vertex under a shuffled numbering, and `unused` vertices that no face names."""
    perm = torch.randperm(3 * n + unused, generator=torch.Generator().manual_seed(seed))
    return _coords(3 * n + unused, seed + 1), perm[torch.arange(3 * n).view(n, 3)]


def separate_triangles_filled(faces, V):
    """What fill() gives on separate_triangles at any cap >= 3, in closed form, for sizes at which its loop over the half-edges is
    too slow: triangle f is one loop of the half-edges 3f, 3f + 1, 3f + 2, labelled 3f and filled; its new vertex is V + f and its
    new faces, in half-edge order, are (v_{k+1}, v_k, V + f).  -> the integer entries of fill()'s dict; the new vertex rows are
    fixed_mean over the three vertices of the triangle (tests/test_mesh_fill_host.py holds this against fill())."""
    faces = torch.as_tensor(faces).long().reshape(-1, 3)
    n = faces.shape[0]
    label = 3 * torch.arange(n)
    new_f = torch.stack([faces[:, [1, 2, 0]], faces, (V + torch.arange(n))[:, None].expand(n, 3)], dim=2).reshape(3 * n, 3)
    return {"faces": torch.cat([faces, new_f]), "halfedge_loop": label[:, None].expand(n, 3).contiguous(), "labels": label.tolist(),
            "loop_sizes": torch.full((n,), 3), "loop_flags": torch.full((n,), FILLED), "info": dict(zip(INFO_KEYS, (3 * n, n, n, 0, 0, 0, 0, n, 3 * n)))}


@functools.lru_cache(maxsize=None)
def surface_mesh(name):
    """The surface_ref meshes of the issue's second table -> (verts, faces)."""
    if name == "sphere600":
        p, n = S.sphere(torch.Generator().manual_seed(2), 600)
        R, s = 32, 2
    elif name == "torus1500":
        p, n = S.torus(torch.Generator().manual_seed(3201), 1500)
        R, s = 32, 2
    elif name == "lattice32":
        p, n = S.lattice_plane(32)
        R, s = 32, 3
    else:
        raise KeyError(name)
    m = S.reconstruct(p, n, R, s)
    return m["verts"].float(), m["faces"].long()


SURFACE_MESHES = ("sphere600", "torus1500", "lattice32")


def colors_for(V, seed):
    """(uint8 (V, 3), float32 (V, 2)) attribute rows."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, 256, (V, 3), generator=g, dtype=torch.uint8), torch.randn(V, 2, generator=g) * 3.0


@functools.lru_cache(maxsize=None)
def batch():
    """Every mesh of the tables as one ragged batch: a tuple of (name, verts, faces, max_hole_edges); the surface meshes at cap 64."""
    rows = [(k, *v) for k, v in {**hand_meshes(), **nonfinite_meshes()}.items()]
    rows += [(k, *surface_mesh(k), 64) for k in SURFACE_MESHES]
    rows += [(k, *v) for k, v in fan_meshes().items()]
    return tuple(rows)


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def same_floats(a, b):
    """Bitwise equal, a NaN equal to any NaN."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape:
        return False
    nan = torch.isnan(a) & torch.isnan(b)
    return bool((nan | (bits(a) == bits(b))).all())
