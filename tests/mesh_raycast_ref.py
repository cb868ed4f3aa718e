"""The ray rule of include/bdm_hip.h section 24 restated on the CPU in numpy.float32 (float64 only where the rule
says so): the exhaustive loop over the used faces, a radix tree over (Morton key, position) with skip links built by recursion, and
the stackless walk over it.  Nothing here is shared with bdm_amd/csrc.  Named mutants change one clause each;
tests/test_mesh_raycast_host.py shows that the table below tells every one of them apart from the rule, and that the walk equals the
exhaustive loop on it (the pruning theorem).

The rule in short.  A ray (o, d, tmin, tmax) is invalid when o, d or tmin is not finite, d == 0, tmax is NaN or tmin > tmax.  A face
with an index out of range, a repeated index or a non-finite vertex is dropped.  Triangle test: Woop, Benthin and Wald's shear and scale
along the dominant axis of d, three float32 edge functions, all three again in float64 when one is zero, rejected on mixed signs or a
zero determinant, t = the scaled-z sum over the determinant.  Face interval: per axis tn, tf = (lo - o) / d, (hi - o) / d ordered by the
sign of d, as (bound - o) * (1 / d), widened by factors 1 -+ 2^-16 away from the interval, a NaN ignored; the face is accepted when
max(tmin, tn's) <= t <= min(tmax, tf's) and t is finite.  closest: the minimum t, the lowest face on ties; any; count."""
import functools
import math

import numpy as np
import torch

import mesh_voxel_ref as VR

F = np.float32
SHRINK, GROW = F(1 - 2.0 ** -16), F(1 + 2.0 ** -16)
THIRD = F(1.0 / 3.0)
MODES = {"closest": 0, "any": 1, "count": 2}
MUTANTS = ("prune_ge", "highest_on_ties", "no_f64", "no_interval", "unwidened")
COUNT_KEYS = ("rays_valid", "rays_invalid", "rays_hit", "faces_used", "faces_dropped")
INF = F(np.inf)


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


# ---- faces and rays -------------------------------------------------------------------------------------------------------------------
def used_faces(verts, faces):
    """-> (index inside the mesh of every used face (n,), its corners (n, 3, 3) float32, the number dropped)."""
    v = f32(torch.as_tensor(verts).float().reshape(-1, 3).numpy())
    f = np.asarray(torch.as_tensor(faces).reshape(-1, 3).long().numpy(), dtype=np.int64)
    if f.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3, 3), dtype=np.float32), 0
    ok = ((f >= 0) & (f < v.shape[0])).all(axis=1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    ok[ok] &= np.isfinite(v[f[ok]]).all(axis=(1, 2))
    idx = np.nonzero(ok)[0]
    return idx, v[f[idx]].reshape(-1, 3, 3), int((~ok).sum())


class Ray:
    """The set-up of one ray (rule 1 and the constants of rules 3 and 4)."""

    def __init__(self, row):
        r = f32(row).reshape(8)
        self.o, self.d, self.tmin, self.tmax = r[0:3], r[3:6], r[6], r[7]
        self.valid = bool(np.isfinite(r[:7]).all() and (self.d != 0).any() and not np.isnan(self.tmax) and self.tmin <= self.tmax)
        with np.errstate(all="ignore"):
            self.inv = (F(1) / self.d).astype(np.float32)
            self.neg = np.signbit(self.d)
            a = np.abs(self.d)
            kz = 0
            if a[1] > a[kz]:
                kz = 1
            if a[2] > a[kz]:
                kz = 2
            kx, ky = (kz + 1) % 3, (kz + 2) % 3
            if self.d[kz] < 0:
                kx, ky = ky, kx
            self.kx, self.ky, self.kz = kx, ky, kz
            self.sx, self.sy, self.sz = F(self.d[kx] / self.d[kz]), F(self.d[ky] / self.d[kz]), F(F(1) / self.d[kz])


def interval(q, lo, hi, mutant=None):
    """Rule 4 for boxes lo, hi (..., 3) -> (near, far) float32 (...): the ray's tmin and tmax folded in."""
    shrink, grow = (F(1), F(1)) if mutant == "unwidened" else (SHRINK, GROW)
    with np.errstate(all="ignore"):
        a = ((lo - q.o).astype(np.float32) * q.inv).astype(np.float32)
        b = ((hi - q.o).astype(np.float32) * q.inv).astype(np.float32)
        tn, tf = np.where(q.neg, b, a), np.where(q.neg, a, b)
        tn = np.where(tn >= 0, tn * shrink, tn * grow).astype(np.float32)
        tf = np.where(tf >= 0, tf * grow, tf * shrink).astype(np.float32)
        near = np.fmax(np.fmax(np.fmax(q.tmin, tn[..., 0]), tn[..., 1]), tn[..., 2])
        far = np.fmin(np.fmin(np.fmin(q.tmax, tf[..., 0]), tf[..., 1]), tf[..., 2])
    return near.astype(np.float32), far.astype(np.float32)


def face_hits(q, tri, mutant=None):
    """Rules 3 and 4 for every used face (n, 3, 3) -> (accepted bool, t, b1, b2, back), each (n,)."""
    n = tri.shape[0]
    with np.errstate(all="ignore"):
        if mutant == "no_interval":
            near, far = np.full(n, q.tmin, dtype=np.float32), np.full(n, q.tmax, dtype=np.float32)
        else:
            near, far = interval(q, tri.min(axis=1), tri.max(axis=1), mutant)
        p = (tri - q.o).astype(np.float32)                                     # (n, corner, axis)
        pz = p[:, :, q.kz]
        X = (p[:, :, q.kx] - (q.sx * pz).astype(np.float32)).astype(np.float32)
        Y = (p[:, :, q.ky] - (q.sy * pz).astype(np.float32)).astype(np.float32)
        Z = (q.sz * pz).astype(np.float32)
        Ax, Bx, Cx, Ay, By, Cy = X[:, 0], X[:, 1], X[:, 2], Y[:, 0], Y[:, 1], Y[:, 2]

        def edge(a, b, c, d, ty):
            a, b, c, d = (x.astype(ty) for x in (a, b, c, d))
            return ((a * b).astype(ty) - (c * d).astype(ty)).astype(ty)
        U, V, W = edge(Cx, By, Cy, Bx, np.float32), edge(Ax, Cy, Ay, Cx, np.float32), edge(Bx, Ay, By, Ax, np.float32)
        Ud, Vd, Wd = U.astype(np.float64), V.astype(np.float64), W.astype(np.float64)
        again = (U == 0) | (V == 0) | (W == 0)
        if mutant != "no_f64":
            Ud = np.where(again, edge(Cx, By, Cy, Bx, np.float64), Ud)
            Vd = np.where(again, edge(Ax, Cy, Ay, Cx, np.float64), Vd)
            Wd = np.where(again, edge(Bx, Ay, By, Ax, np.float64), Wd)
            U, V, W = Ud.astype(np.float32), Vd.astype(np.float32), Wd.astype(np.float32)
        mixed = ((Ud < 0) | (Vd < 0) | (Wd < 0)) & ((Ud > 0) | (Vd > 0) | (Wd > 0))
        det = ((U + V).astype(np.float32) + W).astype(np.float32)
        T = (((U * Z[:, 0]).astype(np.float32) + (V * Z[:, 1]).astype(np.float32)).astype(np.float32) + (W * Z[:, 2]).astype(np.float32)).astype(np.float32)
        t = (T / det).astype(np.float32)
        ok = ~mixed & (det != 0) & (near <= t) & (t <= far) & np.isfinite(t)
        b1, b2 = (V / det).astype(np.float32), (W / det).astype(np.float32)
    return ok, t, b1, b2, det < 0


def _answer(idx, ok, t, mutant):
    """The position of the closest accepted face: the minimum t, the lowest (mutant: highest) face index on ties; None without one."""
    best = None
    for k in np.nonzero(ok)[0]:
        if best is None or t[k] < t[best] or (t[k] == t[best] and ((idx[k] > idx[best]) if mutant == "highest_on_ties" else (idx[k] < idx[best]))):
            best = k
    return best


def _empty_out(R):
    return {"t": np.full(R, np.inf, dtype=np.float32), "face": np.full(R, -1, dtype=np.int32), "bary": np.zeros((R, 2), dtype=np.float32),
            "back": np.zeros(R, dtype=np.uint8), "occluded": np.zeros(R, dtype=np.uint8), "crossings": np.zeros(R, dtype=np.int32)}


def _store(out, i, idx, best, ok, t, b1, b2, back):
    out["occluded"][i], out["crossings"][i] = int(ok.any()), int(ok.sum())
    if best is not None:
        out["t"][i], out["face"][i], out["bary"][i], out["back"][i] = t[best], idx[best], (b1[best], b2[best]), int(back[best])


def exhaustive(verts, faces, rays, mutant=None):
    """One mesh, rays (R, 8) -> dict of the six per-ray outputs and counts (5)."""
    idx, tri, dropped = used_faces(verts, faces)
    rays = f32(rays).reshape(-1, 8)
    out, nvalid, nhit = _empty_out(rays.shape[0]), 0, 0
    for i, row in enumerate(rays):
        q = Ray(row)
        if not q.valid:
            continue
        nvalid += 1
        ok, t, b1, b2, back = face_hits(q, tri, mutant)
        best = _answer(idx, ok, t, mutant)
        _store(out, i, idx, best, ok, t, b1, b2, back)
        nhit += int(ok.any())
    out["counts"] = [nvalid, rays.shape[0] - nvalid, nhit, int(idx.shape[0]), dropped]
    return out


# ---- the hierarchy --------------------------------------------------------------------------------------------------------------------
def _spread(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_keys(verts, tri):
    """The 30-bit codes of the centroids ((a + b) + c) * (1 / 3) of the used faces in the box of the mesh's finite vertices."""
    v = f32(torch.as_tensor(verts).float().reshape(-1, 3).numpy())
    fin = v[np.isfinite(v).all(axis=1)]
    if tri.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    with np.errstate(all="ignore"):
        c = (((tri[:, 0] + tri[:, 1]).astype(np.float32) + tri[:, 2]).astype(np.float32) * THIRD).astype(np.float32)
        ext = (hi - lo).astype(np.float32)
        s = np.where((ext > 0) & np.isfinite(ext), F(1024) / ext, F(0)).astype(np.float32)
        cell = np.fmin(np.fmax(((c - lo).astype(np.float32) * s).astype(np.float32), F(0)), F(1023)).astype(np.int64)
    return (_spread(cell[:, 0]) << 2) | (_spread(cell[:, 1]) << 1) | _spread(cell[:, 2])


def build(verts, faces):
    """The tree of one mesh in the layout of the device buffer: n used faces, nodes 0 .. n - 2 internal (link = left child), nodes
    n - 1 .. 2 n - 2 leaves (link = the face), skip = the node after the subtree or -1; lo, hi (2 n - 1, 3) float32."""
    idx, tri, dropped = used_faces(verts, faces)
    n = idx.shape[0]
    keys = morton_keys(verts, tri)
    order = np.argsort(keys, kind="stable")
    aug = [(int(keys[k]) << 32) | pos for pos, k in enumerate(order)]   # (key, position): all different
    N = max(2 * n - 1, 0)
    tree = {"n": n, "dropped": dropped, "lo": np.zeros((N, 3), dtype=np.float32), "hi": np.zeros((N, 3), dtype=np.float32),
            "link": np.full(N, -1, dtype=np.int64), "skip": np.full(N, -1, dtype=np.int64)}
    if n == 0:
        return tree
    work = [(0 if n > 1 else n - 1, 0, n - 1, -1)]   # node, first, last, skip
    post = []
    while work:
        node, first, last, skip = work.pop()
        tree["skip"][node] = skip
        if first == last:
            k = order[first]
            tree["link"][node], tree["lo"][node], tree["hi"][node] = idx[k], tri[k].min(axis=0), tri[k].max(axis=0)
            continue
        top = (aug[first] ^ aug[last]).bit_length()            # the highest differing bit
        split = max(g for g in range(first, last) if (aug[first] ^ aug[g]).bit_length() < top)
        lc = split if split > first else n - 1 + split
        rc = split + 1 if split + 1 < last else n - 1 + split + 1
        tree["link"][node] = lc
        post.append((node, lc, rc))
        work.append((lc, first, split, rc))
        work.append((rc, split + 1, last, skip))
    for node, lc, rc in reversed(post):                        # children before parents
        tree["lo"][node], tree["hi"][node] = np.minimum(tree["lo"][lc], tree["lo"][rc]), np.maximum(tree["hi"][lc], tree["hi"][rc])
    return tree


def check_tree(tree, verts, faces):
    """The invariants of a tree in the device layout, from a restatement or read back from the device: every used face is in exactly
    one leaf, a leaf's box is the bitwise min / max of its face, an internal box that of the leaves below it, and a depth-first walk
    by link and skip visits every node once and ends.  -> the depth."""
    idx, tri, dropped = used_faces(verts, faces)
    n = tree["n"]
    assert n == idx.shape[0] and tree["dropped"] == dropped
    if n == 0:
        return 0
    where = {int(f): k for k, f in enumerate(idx)}
    link, skip, lo, hi = tree["link"], tree["skip"], tree["lo"], tree["hi"]
    assert sorted(int(x) for x in link[n - 1:2 * n - 1]) == sorted(where), "the leaves are not the used faces, each once"
    for node in range(n - 1, 2 * n - 1):
        k = where[int(link[node])]
        assert lo[node].tobytes() == tri[k].min(axis=0).tobytes() and hi[node].tobytes() == tri[k].max(axis=0).tobytes(), node
    seen, node = [], 0
    while node >= 0:
        assert 0 <= node < 2 * n - 1 and len(seen) < 2 * n - 1, "the walk leaves the mesh or does not end"
        seen.append(node)
        node = int(link[node]) if node < n - 1 else int(skip[node])
    assert sorted(seen) == list(range(2 * n - 1)), "the walk does not visit every node once"
    at = {v: k for k, v in enumerate(seen)}   # the subtree of a node = the nodes visited from it until its skip
    for node in range(n - 1):
        end = at[int(skip[node])] if skip[node] >= 0 else len(seen)
        leaves = [v for v in seen[at[node]:end] if v >= n - 1]
        assert leaves, node
        blo, bhi = np.min(lo[leaves], axis=0), np.max(hi[leaves], axis=0)
        assert lo[node].tobytes() == blo.tobytes() and hi[node].tobytes() == bhi.tobytes(), f"the box of node {node}"
    height, todo = 0, [(0, 1)]                # a node's children are link and the node after link's subtree
    while todo:
        x, d = todo.pop()
        height = max(height, d)
        if x < n - 1:
            todo.append((int(link[x]), d + 1))
            todo.append((int(skip[int(link[x])]), d + 1))
    return height


def walk(tree, q, ok, t, idx_of_face, mode, mutant=None):
    """The stackless walk of one valid ray over a tree; ok, t: the face rule's verdicts by used-face position; idx_of_face: face index
    -> that position.  -> (the positions of the accepted faces it met, in order, the best one, the number of steps)."""
    n = tree["n"]
    met, best, steps = [], None, 0
    node = 0 if n > 0 else -1
    while node >= 0:
        steps += 1
        assert steps <= 2 * n, "the walk exceeds the cap"
        if node >= n - 1:
            k = idx_of_face[int(tree["link"][node])]
            if ok[k]:
                met.append(k)
                if best is None or t[k] < t[best] or (t[k] == t[best] and k < best):   # positions ascend with the face index
                    best = k
                if mode == "any":
                    break
            node = int(tree["skip"][node])
        else:
            near, far = interval(q, tree["lo"][node], tree["hi"][node], "unwidened" if mutant == "unwidened" else None)
            enter = bool(near <= far)
            if mode == "closest" and best is not None:
                enter = enter and not (near >= t[best] if mutant == "prune_ge" else near > t[best])
            node = int(tree["link"][node] if enter else tree["skip"][node])
    return met, best, steps


def tree_cast(verts, faces, rays, mutant=None, tree=None):
    """The same outputs as exhaustive(), by the walk, mode by mode; also "steps", the longest walk."""
    idx, tri, dropped = used_faces(verts, faces)
    tree = build(verts, faces) if tree is None else tree
    pos = {int(f): k for k, f in enumerate(idx)}
    rays = f32(rays).reshape(-1, 8)
    out, nvalid, nhit, longest = _empty_out(rays.shape[0]), 0, 0, 0
    for i, row in enumerate(rays):
        q = Ray(row)
        if not q.valid:
            continue
        nvalid += 1
        ok, t, b1, b2, back = face_hits(q, tri, mutant)
        _, best, s0 = walk(tree, q, ok, t, pos, "closest", mutant)
        met1, _, s1 = walk(tree, q, ok, t, pos, "any", mutant)
        met2, _, s2 = walk(tree, q, ok, t, pos, "count", mutant)
        longest = max(longest, s0, s1, s2)
        if best is not None:
            out["t"][i], out["face"][i], out["bary"][i], out["back"][i] = t[best], idx[best], (b1[best], b2[best]), int(back[best])
        out["occluded"][i], out["crossings"][i] = int(bool(met1)), len(met2)
        nhit += int(bool(met2))
    out["counts"] = [nvalid, rays.shape[0] - nvalid, nhit, int(idx.shape[0]), dropped]
    out["steps"] = longest
    return out


OUTPUTS = ("t", "face", "bary", "back", "occluded", "crossings")


def same(a, b):
    """Two results agree bit for bit (NaN never appears in an output)."""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in OUTPUTS) and list(a["counts"]) == list(b["counts"])


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _rays(o, d, tmin=0.0, tmax=np.inf):
    o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
    n = max(o.shape[0], d.shape[0])
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
    return r


def random_rays(verts, count, seed):
    """Philox-seeded: origins in a shell around the box of the finite vertices (a few inside it), aimed at points of the box."""
    g = np.random.Generator(np.random.Philox(seed))
    v = f32(torch.as_tensor(verts).float().reshape(-1, 3).numpy())
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = (v.min(axis=0), v.max(axis=0)) if v.shape[0] else (np.zeros(3), np.ones(3))
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    u = g.normal(size=(count, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = np.where(g.random(count) < 0.2, 0.3, 2.5)[:, None]
    o = c + u * radius * np.linalg.norm(h)
    target = c + (g.random((count, 3)) * 2 - 1) * h
    r = _rays(o, target - o)
    r[: count // 4, 7] = 1.0          # segments that end at the target
    r[count // 4: count // 3, 6] = 0.5
    return r


def aimed_rays(points):
    """Rays whose line passes exactly through each point: small integer directions, origins 4 directions back (exact in float32 for
    the half-integer coordinates of lattice_box and octahedron)."""
    dirs = f32([(0, 0, -1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1), (-1, 2, 3), (1, -1, 0)])
    p = f32(points).reshape(-1, 1, 3)
    o = (p - 4 * dirs[None]).reshape(-1, 3)
    return _rays(o, np.broadcast_to(dirs[None], (p.shape[0], dirs.shape[0], 3)).reshape(-1, 3))


def _edge_midpoints(verts, faces):
    v, f = verts.numpy().astype(np.float64), faces.numpy()
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    return (v[e[:, 0]] + v[e[:, 1]]) / 2


def pinned(verts, faces, rays):
    """For every ray that hits: the same ray with tmin == tmax == its t (on the hit) and with both one float above it (off it)."""
    ref = exhaustive(verts, faces, rays)
    hit = ref["face"] >= 0
    on, off = rays[hit].copy(), rays[hit].copy()
    on[:, 6] = on[:, 7] = ref["t"][hit]
    off[:, 6] = off[:, 7] = np.nextafter(ref["t"][hit], INF)
    return np.concatenate([on, off])


def special_rays():
    nan, inf = np.nan, np.inf
    rows = [
        (0, 0, 0, 0, 0, 0, 0, inf), (0, 0, 0, 0, 0, -0.0, 0, inf),            # d == 0
        (nan, 0, 0, 0, 0, 1, 0, inf), (0, inf, 0, 0, 0, 1, 0, inf), (0, 0, 0, nan, 0, 1, 0, inf), (0, 0, 0, 0, -inf, 1, 0, inf),
        (0, 0, 0, 0, 0, 1, nan, inf), (0, 0, 0, 0, 0, 1, -inf, inf), (0, 0, 0, 0, 0, 1, 0, nan), (0, 0, 0, 0, 0, 1, 2, 1),
        (0, 0, 0, 0, 0, 1, inf, inf), (4, 4, -3, 0, 0, 1, 0, -inf),
        (4, 4, -3, 0, 0, 1, -inf + 0, 5), (4, 4, -3, 0, 0, 1, 0, inf), (4, 4, -3, 0, 0, 1, -100, 100), (4, 4, 30, 0, 0, -1, 0, inf),
        (4, 4, 4, 0.3, -0.2, 1, 0, inf), (4, 4, 4, -1, 0, 0, 0, inf), (4, 4, 4, 1e-30, 1, 0, 0, inf), (4, 4, 4, 0, -0.0, 1, -50, 50),
        (4, 4, -3, 0, 0, 1e-42, 0, inf), (4, 4, -3, 0, 0, 1e30, 0, inf),
    ]
    return f32(rows)


def box_plane_rays():
    """lattice_box spans (1.5, 2.5, 1.5) .. (6.5, 5.5, 7.5): rays lying in its planes, along its edges, grazing its faces."""
    return np.concatenate([
        _rays([(0, 2.5, 3), (0, 4, 1.5), (1.5, 0, 3), (6.5, 9, 7.5), (0, 2.5, 1.5), (1.5, 2.5, -2)], [(1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1)]),
        _rays([(0, 2.5, 3), (0, 2.5, 0)], [(1, 0, 0.25), (1, 0, 1)]),                       # in the plane y = 2.5, oblique
        _rays([(0, 2.5000002, 3), (0, 2.4999998, 3), (0, 4, 7.4999995)], [(1, 0, 0)] * 3),  # grazing: one float inside and outside
        _rays([(0, 0, 0), (-1, 2, 1)], [(1.5, 2.5, 1.5), (2.5, 0.5, 0.5)]),                 # through a corner, oblique
    ])


@functools.lru_cache(maxsize=None)
def surface_torus():
    """The surface-nets mesh of surface_ref.reconstruct for 4096 points of a torus at 32^3, support 3: 1504 vertices, 3008 faces, closed,
    irregular: crowded Morton cells, an unbalanced tree, a dozen workgroups in the build."""
    import surface_ref as S
    p, nr = S.torus(torch.Generator().manual_seed(2600), 4096)
    m = S.reconstruct(p, nr, 32, 3)
    return m["verts"].float(), m["faces"].long()


@functools.lru_cache(maxsize=None)
def hand_meshes():
    """name -> (verts, faces), in the order of the batch."""
    nan = float("nan")
    sv, sf = VR.uv_sphere(8, 16, radius=3.0, centre=(4.0, 4.0, 4.0))
    tri_v, tri_f = VR._v([(1, 1, 2), (7, 2, 2.5), (3, 8, 3)]), VR._f([(0, 1, 2)])
    bv, bf = VR.box((0.3, 0.2, 0.1), (5.1, 6.3, 7.2))
    bad_v = torch.cat([bv, VR._v([(nan, 0, 0), (1, 2, 3)])])
    bad_f = torch.cat([bf[:5], VR._f([(0, 1, 8), (0, 0, 1), (3, 3, 3), (0, 1, 12), (-1, 2, 3)]), bf[5:], VR._f([(0, 1, 9)])])
    e = 2.0 ** -13
    return {
        "no_faces": (sv, VR._f([])),
        "one_face": (sv, sf[:1]),
        "two_faces": (sv, sf[40:42]),
        "three_faces": (sv, sf[:3]),
        "faces64": (sv, sf[:64]),
        "faces65": (sv, sf[:65]),
        "eight_copies": (tri_v, tri_f.repeat(8, 1)),
        "empty": (torch.zeros(0, 3), VR._f([])),
        "box": (bv, bf),
        "octahedron": VR.octahedron(),
        "lattice_box": VR.lattice_box(),
        "uv_sphere": VR.uv_sphere(24, 48),
        "surface": surface_torus(),
        "bad": (bad_v, bad_f),
        "sliver_edge": (VR._v([(-1, 1, 0), (-1, -(1 - e), 0), (1 + e, 1, 0)]), VR._f([(0, 1, 2)])),
        "wide_flat": (VR._v([(1, -1e6, -1e6), (1, 1e6, -1e6), (1, 0, 1e6)]), VR._f([(0, 1, 2)])),
    }


@functools.lru_cache(maxsize=None)
def batch():
    """The table: a tuple of (name, verts, faces, rays (R, 8) float32), one ragged batch with the empty mesh in the middle.  0, 1 and
    65 rays occur; the other counts follow from the cases."""
    m = hand_meshes()
    rows = []
    for k, (name, (v, f)) in enumerate(m.items()):
        if name == "no_faces":
            rays = random_rays(v, 1, 10)
        elif name == "one_face":
            rays = np.zeros((0, 8), dtype=np.float32)
        elif name in ("two_faces", "faces64", "faces65"):
            rays = np.concatenate([random_rays(v, 45, 20 + k), aimed_rays(v.numpy()[f.numpy()[:2].reshape(-1)][:3])[:20]])   # 65 rays
        elif name == "eight_copies":
            base = _rays([(3, 3, -1), (3, 3, 9), (1, 1, 0), (20, 20, 0)], [(0.1, 0.2, 1), (0, 0, -1), (0, 0, 1), (0, 0, 1)])
            rays = np.concatenate([base, pinned(v, f, base), random_rays(v, 24, 31)])
        elif name == "empty":
            rays = np.concatenate([special_rays()[:3], random_rays(VR._v([(0, 0, 0), (1, 1, 1)]), 4, 32)])
        elif name in ("lattice_box", "octahedron"):
            aim = aimed_rays(np.concatenate([v.numpy().astype(np.float64), _edge_midpoints(v, f)]))
            inside = _rays([(4, 4, 4)] * 6, [(1, 0, 0), (0, -1, 0), (0.3, 0.2, 1), (1, 1, 1), (-2, 1, 0.5), (0, 0, -1)])
            extra = box_plane_rays() if name == "lattice_box" else np.zeros((0, 8), dtype=np.float32)
            base = np.concatenate([aim, inside, extra])
            rays = np.concatenate([base, pinned(v, f, base), special_rays(), random_rays(v, 60, 40 + k)])
        elif name == "sliver_edge":
            rays = _rays([(0, 0, -1), (0, 0.5, -1), (0, 0, 1)], [(0, 0, 1), (0, 0, 1), (0, 0, -1)])
        elif name == "wide_flat":
            rays = _rays([(0, 0.3, 0.2), (0, 0.3, 0.2), (0, 50, -20)], [(0.9, 0.5, 1), (1, 0.5, 0.25), (0.5, 0.2, 1)])
        elif name == "box":
            rays = np.concatenate([random_rays(v, 200, 50), _rays([(2, 3, 4)] * 3, [(1, 0, 0), (0.2, 1, 0.1), (-1, -1, -1)])])
        else:
            rays = random_rays(v, {"uv_sphere": 120, "surface": 300}.get(name, 40), 60 + k)
        rows.append((name, v, f, f32(rays)))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def references():
    """The exhaustive restatement of every row of batch(), computed once."""
    return tuple(exhaustive(v, f, rays) for _, v, f, rays in batch())


@functools.lru_cache(maxsize=None)
def trees():
    return tuple(build(v, f) for _, v, f, _ in batch())


# ---- the Python surface, restated -------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n):
    """n unit vectors in float64, rounded once to float32."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)
