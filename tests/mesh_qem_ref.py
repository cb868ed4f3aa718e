"""The quadric edge-collapse rule of include/bdm_hip.h section 23 restated on the CPU in plain Python: lists,
dictionaries and Python integers for everything combinatorial, Python floats (IEEE float64, one operation at a time, in the order the
header writes them, no library sums) for everything that decides, one numpy.float32 rounding per stored coordinate and per key.
Nothing here is shared with bdm_amd/csrc/mesh_qem.hip.  Named mutants change one clause each; tests/test_mesh_qem_host.py shows
that every one of them is told apart from the rule by at least one mesh of the generators below."""
import functools
import math

import numpy as np
import torch

import mesh_fill_ref as MF
from mesh_fill_ref import bits, same_floats  # noqa: F401  (the tests compare with them)

MUTANTS = ("one_hop", "no_link", "no_flip", "quadric_order", "b_survives", "no_boundary_quadric", "cost_before_clamp")
COLLAPSED, BAD = -1, -3
INVALID = (1 << 64) - 1
REASONS = ("nonmanifold", "locked", "cost", "link", "boundary", "valence", "flip")
STOPS = ("running", "target", "no_edge", "max_rounds")
INFO_KEYS = ("stop", "rounds", "collapses", "faces_in", "faces_out", "vertices_in", "vertices_out", "locked_vertices", "bad_faces",
             "max_cost_bits", "selected", "candidates") + tuple("rejected_" + r for r in REASONS) + ("target",)
INF = float("inf")


def f32(x):
    """One rounding to float32, back as a Python float."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


def f32_bits(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return int(np.float32(x).view(np.uint32))


def finite(x):
    return abs(x) < INF   # False for NaN


# ---- float64 pieces, in the header's order ----------------------------------------------------------------------------------------------
def normal(p0, p1, p2):
    ax, ay, az = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    bx, by, bz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def plane_quadric(n, d, s):
    x, y, z = n
    return [(x * x) * s, (x * y) * s, (x * z) * s, (x * d) * s, (y * y) * s, (y * z) * s, (y * d) * s, (z * z) * s, (z * d) * s, (d * d) * s]


def face_term(p0, p1, p2):
    """(quadric, normal, area) of a face, None when its float64 normal is zero or not finite."""
    n = normal(p0, p1, p2)
    l2 = dot3(n, n)
    if not (l2 > 0.0 and l2 < INF):
        return None
    area = 0.5 * math.sqrt(l2)
    d = -dot3(n, p0)
    return plane_quadric(n, d, area / l2), n, area


def boundary_term(p, q, n, area, weight):
    """The plane through the edge p -> q perpendicular to the face of normal n."""
    ex, ey, ez = q[0] - p[0], q[1] - p[1], q[2] - p[2]
    m = (ey * n[2] - ez * n[1], ez * n[0] - ex * n[2], ex * n[1] - ey * n[0])
    l2 = dot3(m, m)
    if not (l2 > 0.0 and l2 < INF):
        return None
    d = -dot3(m, p)
    return plane_quadric(m, d, (weight * area) / l2)


def error(q, v):
    x, y, z = v
    a = ((q[0] * x) * x + (q[4] * y) * y) + (q[7] * z) * z
    b = ((q[1] * x) * y + (q[2] * x) * z) + (q[5] * y) * z
    c = (q[3] * x + q[6] * y) + q[8] * z
    return ((a + 2.0 * b) + 2.0 * c) + q[9]


def clamp(e):
    return e if e > 0.0 else (0.0 if e == e else e)


def target_and_cost(q, pa, pb, mutant=None):
    """Rule 2 -> (target (float64 triple), cost)."""
    c00 = q[4] * q[7] - q[5] * q[5]
    c01 = q[1] * q[7] - q[5] * q[2]
    c02 = q[1] * q[5] - q[4] * q[2]
    det = (q[0] * c00 - q[1] * c01) + q[2] * c02
    tr = (q[0] + q[4]) + q[7]
    mid = ((pa[0] + pb[0]) * 0.5, (pa[1] + pb[1]) * 0.5, (pa[2] + pb[2]) * 0.5)
    dx, dy, dz = pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]
    len2 = (dx * dx + dy * dy) + dz * dz
    if abs(det) > 2.0 ** -40 * ((tr * tr) * tr):
        r0, r1, r2 = -q[3], -q[6], -q[8]
        m0 = r1 * q[7] - q[5] * r2
        m1 = r1 * q[5] - q[4] * r2
        m2 = q[1] * r2 - r1 * q[2]
        x = ((r0 * c00 - q[1] * m0) + q[2] * m1) / det
        y = ((q[0] * m0 - r0 * c01) + q[2] * m2) / det
        z = ((r0 * c02 - q[0] * m1) - q[1] * m2) / det
        ox, oy, oz = x - mid[0], y - mid[1], z - mid[2]
        if (ox * ox + oy * oy) + oz * oz <= len2:
            return (x, y, z), clamp(error(q, (x, y, z)))
    best, cost = pa, error(q, pa)
    if mutant != "cost_before_clamp":
        cost = clamp(cost)
    for cand in (pb, mid):
        c = error(q, cand)
        if mutant != "cost_before_clamp":
            c = clamp(c)
        if c < cost:
            best, cost = cand, c
    return best, clamp(cost)


# ---- state ------------------------------------------------------------------------------------------------------------------------------
class State:
    """One mesh between rounds."""

    def __init__(self, verts, faces, target, boundary_weight=1.0, maximum_error=INF, max_rounds=256, mutant=None):
        verts = torch.as_tensor(verts).float().reshape(-1, 3)
        self.V, self.mutant = verts.shape[0], mutant
        self.pos = [[float(c) for c in row] for row in verts.tolist()]
        rows = [tuple(int(i) for i in f) for f in torch.as_tensor(faces).reshape(-1, 3).tolist()]
        self.F = len(rows)
        self.target, self.weight, self.maximum_error, self.max_rounds = int(target), float(boundary_weight), float(maximum_error), int(max_rounds)
        self.locked = [not all(finite(c) for c in p) for p in self.pos]
        self.faces, self.fcode = [], []
        for f in rows:
            ok = MF.connected(f, self.V)
            self.faces.append(list(f) if ok else [-1, -1, -1])
            self.fcode.append(0 if ok else BAD)
            if not ok:
                for i in f:
                    if 0 <= i < self.V:
                        self.locked[i] = True
        self.vlive, self.parent = [True] * self.V, list(range(self.V))
        self.live_faces, self.live_verts = self.fcode.count(0), self.V
        self.rounds = self.collapses = self.max_cost_bits = self.selected = self.candidates = 0
        self.rejected = dict.fromkeys(REASONS, 0)
        seg = self.incidence()
        self.Q = [self.vertex_quadric(seg, v) for v in range(self.V)]
        self.stop = 1 if self.live_faces <= self.target else 0
        self.last = {}

    def incidence(self):
        """Per vertex the ascending records neighbour << 32 | half-edge << 1 | direction (0: the half-edge leaves the vertex)."""
        seg = [[] for _ in range(self.V)]
        for f, idx in enumerate(self.faces):
            if idx[0] < 0:
                continue
            for c in range(3):
                v, nxt, prv = idx[c], idx[(c + 1) % 3], idx[(c + 2) % 3]
                seg[v].append(nxt << 32 | (3 * f + c) << 1)
                seg[v].append(prv << 32 | (3 * f + (c + 2) % 3) << 1 | 1)
        for s in seg:
            s.sort()
        return seg

    @staticmethod
    def runs(s):
        """[(neighbour, out, in, lowest half-edge)] of a sorted segment."""
        out = []
        for r in s:
            n, he, d = r >> 32, (r & 0xFFFFFFFF) >> 1, r & 1
            if out and out[-1][0] == n:
                o = out[-1]
                out[-1] = (n, o[1] + (1 - d), o[2] + d, min(o[3], he))
            else:
                out.append((n, 1 - d, d, he))
        return out

    def corner_faces(self, s):
        """(face, corner of the vertex) once per face around the vertex of segment s."""
        return [(((r & 0xFFFFFFFF) >> 1) // 3, ((r & 0xFFFFFFFF) >> 1) % 3) for r in s if not r & 1]

    def vertex_quadric(self, seg, v):
        q = [0.0] * 10
        edge = {n: o + i for n, o, i, _ in self.runs(seg[v])}
        terms = []
        for f, c in sorted(self.corner_faces(seg[v])):
            idx = self.faces[f]
            p = [self.pos[i] for i in idx]
            t = face_term(*p)
            if t is None:
                continue
            terms.append(t[0])
            if self.mutant == "no_boundary_quadric":
                continue
            for e in (c, (c + 2) % 3):   # the half-edge that leaves v, then the one that arrives
                a, b = idx[e], idx[(e + 1) % 3]
                if edge[b if a == v else a] == 1:
                    bt = boundary_term(self.pos[a], self.pos[b], t[1], t[2], self.weight)
                    if bt is not None:
                        terms.append(bt)
        if self.mutant == "quadric_order":
            terms.reverse()
        for t in terms:
            q = [x + y for x, y in zip(q, t)]
        return q

    # ---- one round ----------------------------------------------------------------------------------------------------------------------
    def evaluate(self, seg, info, h, lo, hi, out, inn):
        """Rules 1 - 3 for the edge of id h -> (key, target as float32 values, reason or None)."""
        if not ((out, inn) in ((1, 1), (1, 0), (0, 1))) or info[lo][2] or info[hi][2]:
            return INVALID, None, "nonmanifold"
        if self.locked[lo] or self.locked[hi]:
            return INVALID, None, "locked"
        q = [x + y for x, y in zip(self.Q[lo], self.Q[hi])]
        tgt, cost = target_and_cost(q, self.pos[lo], self.pos[hi], self.mutant)
        fc = f32(cost)
        if not (cost <= self.maximum_error and fc < INF):
            return INVALID, None, "cost"
        t32 = [f32(c) for c in tgt]
        interior = out + inn == 2
        nl, nh = [r[0] for r in self.runs(seg[lo])], [r[0] for r in self.runs(seg[hi])]
        common = len(set(nl) & set(nh))
        if self.mutant != "no_link" and common != (2 if interior else 1):
            return INVALID, None, "link"
        if interior and info[lo][1] and info[hi][1]:
            return INVALID, None, "boundary"
        for r in seg[lo]:
            if r >> 32 == hi:
                idx = self.faces[((r & 0xFFFFFFFF) >> 1) // 3]
                c = [i for i in idx if i != lo and i != hi][0]
                if info[c][0] < (3 if info[c][1] else 4):
                    return INVALID, None, "valence"
        if self.mutant != "no_flip":
            for v, other in ((lo, hi), (hi, lo)):
                for f, c in self.corner_faces(seg[v]):
                    idx = self.faces[f]
                    if other in idx:
                        continue
                    p = [self.pos[i] for i in idx]
                    old = normal(*p)
                    p[c] = t32
                    if not dot3(normal(*p), old) > 0.0:
                        return INVALID, None, "flip"
        return f32_bits(cost) << 32 | h, t32, None

    def round(self):
        """One round; the trace of it (keys, selected half-edges) stays in self.last."""
        seg = self.incidence()
        info = []   # (neighbours, on the boundary, at an irregular edge)
        for v in range(self.V):
            rs = self.runs(seg[v])
            info.append((len(rs), any(o + i == 1 for _, o, i, _ in rs), any((o, i) not in ((1, 1), (1, 0), (0, 1)) for _, o, i, _ in rs)))
        keys, targets, ends = {}, {}, {}
        self.rejected, self.candidates = dict.fromkeys(REASONS, 0), 0
        for v in range(self.V):
            for n, o, i, h in self.runs(seg[v]):
                if v < n:
                    key, t32, why = self.evaluate(seg, info, h, v, n, o, i)
                    keys[h], targets[h], ends[h] = key, t32, (v, n)
                    self.candidates += 1
                    if why:
                        self.rejected[why] += 1
        m1 = [min([keys[h] for _, _, _, h in self.runs(seg[v])], default=INVALID) for v in range(self.V)]
        if self.mutant == "one_hop":
            m2 = m1
        else:
            m2 = [min([m1[v]] + [m1[n] for n, *_ in self.runs(seg[v])]) for v in range(self.V)]
        chosen = sorted(h for h, k in keys.items() if k != INVALID and k == m2[ends[h][0]] and k == m2[ends[h][1]])
        for h in chosen:
            lo, hi = ends[h]
            if self.mutant == "b_survives":
                lo, hi = hi, lo
            self.pos[lo] = list(targets[h])
            self.Q[lo] = [x + y for x, y in zip(self.Q[lo], self.Q[hi])]
            self.vlive[hi], self.parent[hi] = False, lo
            self.live_verts -= 1
            for f, c in self.corner_faces(seg[hi]):
                if lo in self.faces[f]:
                    self.faces[f] = [-1, -1, -1]
                    self.live_faces -= 1
                else:
                    self.faces[f][c] = lo
            self.max_cost_bits = max(self.max_cost_bits, keys[h] >> 32)
        self.collapses += len(chosen)
        self.selected = len(chosen)
        self.rounds += 1
        if self.live_faces <= self.target:
            self.stop = 1
        elif not chosen:
            self.stop = 2
        elif self.rounds >= self.max_rounds:
            self.stop = 3
        self.last = {"keys": keys, "selected": chosen, "ends": ends, "m1": m1, "m2": m2}

    def run(self, rounds=None):
        """Up to `rounds` rounds (all that are left without it) -> still running?"""
        done = 0
        while self.stop == 0 and (rounds is None or done < rounds):
            self.round()
            done += 1
        return self.stop == 0

    # ---- the output ---------------------------------------------------------------------------------------------------------------------
    def info(self):
        out = dict(stop=self.stop, rounds=self.rounds, collapses=self.collapses, faces_in=self.F, faces_out=self.live_faces, vertices_in=self.V,
                   vertices_out=self.live_verts, locked_vertices=sum(self.locked), bad_faces=self.fcode.count(BAD),
                   max_cost_bits=self.max_cost_bits, selected=self.selected, candidates=self.candidates)
        out.update({"rejected_" + r: self.rejected[r] for r in REASONS})
        out["target"] = self.target
        return out

    def finish(self, attrs=None):
        """-> dict(verts, faces, attrs, vert_map, face_map, info, members)."""
        root = []
        for v in range(self.V):
            while self.parent[v] != v:
                v = self.parent[v]
            root.append(v)
        alive = [v for v in range(self.V) if self.vlive[v]]
        new = {v: i for i, v in enumerate(alive)}
        vert_map = [new[r] for r in root]
        face_map, kept = [], []
        for f, idx in enumerate(self.faces):
            if idx[0] < 0:
                face_map.append(BAD if self.fcode[f] == BAD else COLLAPSED)
            else:
                face_map.append(len(kept))
                kept.append([new[i] for i in idx])
        members = [[] for _ in alive]
        for v, m in enumerate(vert_map):
            members[m].append(v)
        an = (torch.zeros(self.V, 0) if attrs is None else torch.as_tensor(attrs).float()).numpy()
        ea = MF.scale_exp(an)
        out_a = np.empty((len(alive), an.shape[1]), dtype=np.float32)
        for i, m in enumerate(members):
            for d in range(an.shape[1]):
                col = an[m, d]
                out_a[i, d] = col[0] if len(m) == 1 else (MF.fixed_mean(col, ea) if np.isfinite(col).all() else np.nan)
        return {"verts": torch.tensor([self.pos[v] for v in alive], dtype=torch.float64).float().reshape(-1, 3),
                "faces": torch.tensor(kept, dtype=torch.int64).reshape(-1, 3), "attrs": torch.from_numpy(out_a),
                "vert_map": torch.tensor(vert_map, dtype=torch.int64), "face_map": torch.tensor(face_map, dtype=torch.int64),
                "info": self.info(), "members": members}

    def quadrics(self):
        return torch.tensor(self.Q, dtype=torch.float64).reshape(-1, 10)


def decimate(verts, faces, target, boundary_weight=1.0, maximum_error=INF, max_rounds=256, attrs=None, mutant=None, chunk=None):
    """One mesh through init, the rounds (in calls of `chunk`) and finish."""
    s = State(verts, faces, target, boundary_weight, maximum_error, max_rounds, mutant)
    while s.run(chunk):
        pass
    return s.finish(attrs)


# ---- what the tests measure -------------------------------------------------------------------------------------------------------------
def topology(faces):
    """dict(open_edges, inconsistent_edges, multi_edges, euler, duplicate_faces, loops) of a face list over the vertices it uses."""
    rows = [tuple(int(i) for i in f) for f in torch.as_tensor(faces).reshape(-1, 3).tolist()]
    half = {}
    for f in rows:
        for c in range(3):
            half[(f[c], f[(c + 1) % 3])] = half.get((f[c], f[(c + 1) % 3]), 0) + 1
    edges = {(min(a, b), max(a, b)) for a, b in half}
    count = {e: (half.get(e, 0), half.get((e[1], e[0]), 0)) for e in edges}
    used = {i for f in rows for i in f}
    nxt = {a: b for (a, b), n in half.items() if half.get((b, a), 0) == 0}   # boundary half-edges; simple loops only
    loops, seen = 0, set()
    for a in nxt:
        if a not in seen:
            loops += 1
            while a in nxt and a not in seen:
                seen.add(a)
                a = nxt[a]
    return dict(open_edges=sum(o + i == 1 for o, i in count.values()), multi_edges=sum(o + i > 2 for o, i in count.values()),
                inconsistent_edges=sum(o + i == 2 and o != i for o, i in count.values()), euler=len(used) - len(edges) + len(rows),
                duplicate_faces=len(rows) - len({tuple(sorted(f)) for f in rows}), loops=loops)


def signed_volume(verts, faces):
    v = torch.as_tensor(verts).double()
    f = torch.as_tensor(faces).long().reshape(-1, 3)
    return float((v[f[:, 0]] * torch.cross(v[f[:, 1]], v[f[:, 2]], dim=1)).sum() / 6.0)


# ---- generators -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [tuple(c / math.sqrt(1 + t * t) for c in p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = [(x + y) / 2 for x, y in zip(v[a], v[b])]
                n = math.sqrt(sum(c * c for c in p))
                v.append(tuple(c / n for c in p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return torch.tensor(v, dtype=torch.float64).float(), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def torus(nu=16, nv=8, R=1.0, r=0.4):
    v, f = [], []
    for i in range(nu):
        for j in range(nv):
            a, b = 2 * math.pi * i / nu, 2 * math.pi * j / nv
            v.append(((R + r * math.cos(b)) * math.cos(a), (R + r * math.cos(b)) * math.sin(a), r * math.sin(b)))
    for i in range(nu):
        for j in range(nv):
            p, q, s, t = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(p, q, s), (p, s, t)]
    return torch.tensor(v, dtype=torch.float64).float(), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def grid(n=9):
    """An open flat n x n sheet in the plane z = 0.25."""
    v = [(i / (n - 1), j / (n - 1), 0.25) for i in range(n) for j in range(n)]
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            p, q, s, t = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            f += [(p, q, s), (p, s, t)]
    return torch.tensor(v, dtype=torch.float64).float(), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def tilted(n=9):
    """The flat sheet in a plane of no special direction: every quadric error is rounding noise around zero, of either sign."""
    v, f = grid(n)
    nrm = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    nrm = nrm / nrm.norm()
    u = torch.tensor([1.0, 0.2, 0.0], dtype=torch.float64)
    u = u - (u @ nrm) * nrm
    u = u / u.norm()
    w = torch.linalg.cross(nrm, u)
    d = v.double()
    return (d[:, :1] * u + d[:, 1:2] * w + 0.37 * nrm).float(), f


def hand_meshes():
    tet_v = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    tet_f = [(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)]
    two_v = tet_v + [(-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)]
    two_f = tet_f + [(0, 4, 5), (0, 6, 4), (0, 5, 6), (4, 6, 5)]
    fin_v = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1.0, 0.0), (0.5, -1.0, 0.2), (0.5, 0.1, 1.0)]
    fin_f = [(0, 1, 2), (1, 0, 3), (0, 1, 4)]
    fan_v = [(0.0, 0.0, 0.3)] + [(math.cos(2 * math.pi * k / 40), math.sin(2 * math.pi * k / 40), 0.02 * (k % 3)) for k in range(40)]
    fan_f = [(0, 1 + k, 1 + (k + 1) % 40) for k in range(40)]
    octa_v = [(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)]
    t = lambda v, f: (torch.tensor(v, dtype=torch.float64).float(), torch.tensor(f, dtype=torch.int64))   # noqa: E731
    return {"tetrahedron": t(tet_v, tet_f), "two_tetrahedra": t(two_v, two_f), "fin": t(fin_v, fin_f), "fan40": t(fan_v, fan_f),
            "octahedron": t(octa_v, MF.OCTA)}


def attrs_for(V, seed, C=3):
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(V, C, generator=g) * 2.0
