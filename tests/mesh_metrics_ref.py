"""CPU restatement of bdm_hip.h section 14 (mesh metrics: surface samples and point-to-face distance) -- TEST INFRASTRUCTURE.

Written against the header's text, not against csrc/mesh_metrics.hip: torch float32 elementwise operations, one rounding each (eager
torch fuses nothing; division is IEEE on the host, the square root goes through _sqrt), int64 sums, torch.searchsorted for the face pick and
oracle.ref_rng.philox4x32_10 for the random words.  `dtype=torch.float64` evaluates the same formulas in float64 on the same
(float32) inputs: the yardstick of tests/test_mesh_metrics_host.py and tools/mesh_metrics_gap.py.

Also here: the case table both test files share, and the mutants (deliberately wrong variants of the rule) that the host test
requires the cases to tell apart from the rule."""
import functools
import math

import numpy as np
import torch

from oracle import ref_rng

TILE = 256           # faces per LDS tile of mm_dist_kernel (MM_TILE)
THREADS = 256        # workgroup of every kernel of the file (MM_THREADS)
SCAN_SPAN = THREADS * THREADS   # faces whose workgroup sums one pass of mm_scan_kernel covers
MESH_PURPOSE = 5     # bdm_amd.rng.MESH
SEED = 2024

# mutant -> what it gets wrong.  DIST_MUTANTS change bdm_point_mesh_distance, SAMPLE_MUTANTS bdm_mesh_sample_points.
DIST_MUTANTS = {"no_inside_test": "plane distance taken without the inside test", "strict_inside": "s_i > 0 instead of s_i >= 0",
                "highest_on_ties": "the highest face index wins among equal distances", "invalid_not_skipped": "faces with nn == 0 take part"}
SAMPLE_MUTANTS = {"c_ge_t": "the first face with C_i >= t", "no_sqrt": "barycentrics from u1 instead of sqrt(u1)",
                  "q_truncated": "q truncated instead of rounded to nearest even"}
# Equivalent mutant, kept for the record: dropping the shortcut `t = 0 when l2 == 0`.  A valid face has nn > 0, and l2_i == 0 with nn > 0
# needs an edge whose squared length underflows (|e| < 3e-23) next to one longer than 1e15 |e|; there the quotient h / 0 is +-inf or
# NaN, the clamp turns it into 0 or 1, and c = a + t e differs from a by less than 3e-23: d moves only where it is itself below
# 1e-45.  No test input can tell the two apart, so this mutant is exempt from the "every mutant is told apart" assertion.
EQUIVALENT_MUTANTS = {"no_l2_shortcut": "t = h / l2 also when l2 == 0"}


def _sqrt(x):
    """Correctly rounded square root.  torch.sqrt's vectorised float32 path is NOT (measured: 748 of 100 000 uniform values in [0, 3)
    come out one ulp off on an AVX-512 host, and the set differs between hosts); the float64 square root rounded to float32 is (53
    bits are more than 2 x 24 + 2, so the second rounding cannot move the result)."""
    return torch.from_numpy(np.sqrt(x.double().numpy())).to(x.dtype)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)


def face_quantities(verts, faces, dtype=torch.float32, mutant=None):
    """v (F, 3, 3), e (F, 3, 3) with e[:, i] = v_{i+1} - v_i, l2 (F, 3), n (F, 3), nn (F), valid (F) of one mesh."""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    faces = faces.long().reshape(F, 3)
    inrange = ((faces >= 0) & (faces < V)).all(dim=1)
    if V == 0:
        z = torch.zeros(F, 3, 3, dtype=dtype)
        return {"v": z, "e": z, "l2": z[:, :, 0], "n": z[:, 0], "nn": z[:, 0, 0], "valid": torch.zeros(F, dtype=torch.bool)}
    v = verts.to(dtype)[faces.clamp(0, V - 1)]
    finite = torch.isfinite(v).all(dim=2).all(dim=1)
    e = torch.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], dim=1)
    g = v[:, 2] - v[:, 0]
    n = _cross(e[:, 0], g)
    nn = _dot(n, n)
    valid = inrange & finite
    if mutant != "invalid_not_skipped":
        valid = valid & (nn > 0) & (nn < math.inf)
    return {"v": v, "e": e, "l2": _dot(e, e), "n": n, "nn": nn, "valid": valid}


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
def philox_words(key, count, draw, purpose=MESH_PURPOSE, first=0):
    """(count, 4) uint32: the words of counters (j, 0, draw, purpose), j = first .. first + count - 1 < 2^32."""
    ctr = np.zeros((count, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(first, first + count, dtype=np.uint64) & 0xFFFFFFFF
    ctr[:, 2], ctr[:, 3] = draw, purpose
    return ref_rng.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))


def face_weights(verts, faces, mutant=None):
    """(q (F) int64, inclusive prefix C (F) int64, a (F) float32, face quantities)."""
    fq = face_quantities(verts, faces)
    a = torch.where(fq["valid"], _sqrt(fq["nn"]), torch.zeros(()))
    if a.numel() == 0 or not bool(fq["valid"].any()):
        q = torch.zeros(a.shape, dtype=torch.int64)
        return q, q.clone(), a, fq
    x = (a / a.max()) * torch.tensor(1073741824.0)
    q = (torch.trunc(x) if mutant == "q_truncated" else torch.round(x)).to(torch.int64)   # torch.round: half to even
    q = torch.where(fq["valid"], q, torch.zeros((), dtype=torch.int64))
    return q, torch.cumsum(q, 0), a, fq


def sample_mesh(verts, faces, S, key, draw=0, purpose=MESH_PURPOSE, mutant=None, first=0):
    """One mesh -> points (S, 3) float32, face_idx (S) int32, normals (S, 3) float32: samples first .. first + S - 1."""
    q, C, a, fq = face_weights(verts, faces, mutant)
    c_last = int(C[-1]) if C.numel() else 0
    if c_last == 0:
        return torch.zeros(S, 3), torch.full((S,), -1, dtype=torch.int32), torch.zeros(S, 3)
    w = philox_words(int(key), S, draw, purpose, first)
    t = torch.tensor([(((int(w0) << 32) | int(w1)) * c_last) >> 64 for w0, w1 in zip(w[:, 0], w[:, 1])], dtype=torch.int64)
    idx = torch.searchsorted(C, t, right=(mutant != "c_ge_t"))   # right=True: the first i with C_i > t
    scale = torch.tensor(2.0 ** -24)
    u1 = torch.from_numpy((w[:, 2] >> 8).astype(np.float32)) * scale
    u2 = torch.from_numpy((w[:, 3] >> 8).astype(np.float32)) * scale
    su = u1 if mutant == "no_sqrt" else _sqrt(u1)
    one = torch.tensor(1.0)
    b0, b1, b2 = (one - su)[:, None], (su * (one - u2))[:, None], (su * u2)[:, None]
    v = fq["v"][idx]
    points = (b0 * v[:, 0] + b1 * v[:, 1]) + b2 * v[:, 2]
    normals = fq["n"][idx] / a[idx][:, None]
    return points, idx.to(torch.int32), normals


def sample_batch(verts_list, faces_list, S, keys, draw=0, purpose=MESH_PURPOSE, mutant=None):
    """-> {"points" (B, S, 3), "face_idx" (B, S) int32, "normals" (B, S, 3)}"""
    rows = [sample_mesh(v, f, S, k, draw, purpose, mutant) for v, f, k in zip(verts_list, faces_list, keys)]
    return {"points": torch.stack([r[0] for r in rows]), "face_idx": torch.stack([r[1] for r in rows]),
            "normals": torch.stack([r[2] for r in rows])}


# ---- distance ------------------------------------------------------------------------------------------------------------------------
def pair_sqdist(fq, x, mutant=None):
    """(P, F): the rule's d for every (point, face) of one mesh, +inf where the face is invalid or d is NaN.  x (P, 3) in fq's dtype."""
    v, e, l2, n, nn = fq["v"], fq["e"], fq["l2"], fq["n"], fq["nn"]
    dtype = x.dtype
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    d_e, inside = None, None
    for i in range(3):
        a, ei = v[None, :, i], e[None, :, i]
        r = x[:, None, :] - a
        h = _dot(ei, r)
        t = h / l2[None, :, i]
        if mutant != "no_l2_shortcut":
            t = torch.where(l2[None, :, i] == 0, zero, t)
        t = torch.where(t > 0, t, zero)
        t = torch.where(t < 1, t, one)
        c = a + t[..., None] * ei
        w = x[:, None, :] - c
        d = _dot(w, w)
        d_e = d if d_e is None else torch.where(d < d_e, d, d_e)
        s = _dot(n[None], _cross(ei, r))
        ok = (s > 0) if mutant == "strict_inside" else (s >= 0)
        inside = ok if inside is None else inside & ok
    if mutant == "no_inside_test":
        inside = torch.ones_like(inside)
    k = _dot(n[None], x[:, None, :] - v[None, :, 0])
    d_p = (k * k) / nn[None]
    d = torch.where(inside & (d_p < d_e), d_p, d_e)
    d = torch.where(fq["valid"][None], d, torch.full((), math.inf, dtype=dtype))
    return torch.where(torch.isnan(d), torch.full((), math.inf, dtype=dtype), d)


def distance_mesh(verts, faces, points, mutant=None, dtype=torch.float32, chunk=2048):
    """One mesh -> sqdist (P) in `dtype`, face_idx (P) int32."""
    P, F = int(points.shape[0]), int(faces.shape[0])
    x = points.to(dtype)
    best = torch.full((P,), math.inf, dtype=dtype)
    idx = torch.full((P,), -1, dtype=torch.int64)
    highest = mutant == "highest_on_ties"
    for lo in range(0, F, chunk):
        fq = face_quantities(verts, faces[lo:lo + chunk], dtype, mutant)
        d = pair_sqdist(fq, x, mutant)
        dmin = d.min(dim=1).values
        ar = torch.arange(lo, lo + d.shape[1])[None]
        eq = d == dmin[:, None]
        pick = torch.where(eq, ar, torch.full((), -1)).max(dim=1).values if highest else torch.where(eq, ar, torch.full((), 1 << 40)).min(dim=1).values
        take = ((dmin <= best) if highest else (dmin < best)) & (dmin < math.inf)
        best, idx = torch.where(take, dmin, best), torch.where(take, pick, idx)
    bad = ~torch.isfinite(x).all(dim=1)
    best = torch.where(bad, torch.full((), math.inf, dtype=dtype), best)
    idx = torch.where(bad | (best == math.inf), torch.full((), -1), idx)
    return best, idx.to(torch.int32)


def distance_batch(verts_list, faces_list, points, mutant=None, dtype=torch.float32):
    """points (B, P, 3) -> {"sqdist" (B, P), "face_idx" (B, P) int32}"""
    rows = [distance_mesh(v, f, p, mutant, dtype) for v, f, p in zip(verts_list, faces_list, points)]
    return {"sqdist": torch.stack([r[0] for r in rows]), "face_idx": torch.stack([r[1] for r in rows])}


def morton_order(points, bits=10):
    """(B, P) int32: the points of every cloud in Morton order of their coordinates quantised to `bits` bits per axis over the cloud's
    bounding box (non-finite coordinates quantise to 0); ties in ascending index (a stable sort)."""
    p = torch.nan_to_num(points.double(), nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = p.min(dim=1, keepdim=True).values, p.max(dim=1, keepdim=True).values
    cell = ((p - lo) / (hi - lo).clamp_min(1e-30) * ((1 << bits) - 1)).long().clamp(0, (1 << bits) - 1)
    code = torch.zeros(cell.shape[:2], dtype=torch.int64)
    for b in range(bits):
        for axis in range(3):
            code |= ((cell[..., axis] >> b) & 1) << (3 * b + axis)
    return torch.sort(code, dim=1, stable=True).indices.to(torch.int32)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def box_mesh(sx=1.0, sy=1.0, sz=1.0, centre=(0.0, 0.0, 0.0)):
    """Axis-aligned box with sides (sx, sy, sz): 8 vertices, 12 faces wound outwards."""
    c = torch.tensor([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=torch.float32) - 0.5   # vertex 4x + 2y + z
    verts = c * torch.tensor([sx, sy, sz]) + torch.tensor(centre)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x, +x, -y, +y, -z, +z
    faces = [t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))]
    return verts, torch.tensor(faces, dtype=torch.int64)


def icosphere(level=1, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """Subdivided icosahedron: 20 * 4^level faces wound outwards, vertices on the sphere (to float32 rounding)."""
    g = (1 + 5 ** 0.5) / 2
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
             (-g, 0, 1)]
    verts = [tuple(np.array(v) / np.linalg.norm(v)) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
             (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, out = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (np.array(verts[a]) + np.array(verts[b])) / 2
                verts.append(tuple(m / np.linalg.norm(m)))
                cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    v = torch.tensor(np.array(verts) * radius + np.array(centre), dtype=torch.float32)
    return v, torch.tensor(faces, dtype=torch.int64)


def soup(F, seed, size=0.25, centre=(0.0, 0.0, 0.0)):
    """F separate random triangles of extent `size` in a unit cube around `centre` (3 F vertices)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(F, 1, 3, generator=g) - 0.5
    verts = (base + (torch.rand(F, 3, 3, generator=g) - 0.5) * size).reshape(3 * F, 3) + torch.tensor(centre)
    return verts.contiguous(), torch.arange(3 * F, dtype=torch.int64).reshape(F, 3)


def cloud(P, seed, centre=(0.0, 0.0, 0.0), spread=1.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) - 0.5) * spread + torch.tensor(centre)


def degenerate_mesh():
    """A soup of 40 valid faces with invalid ones among them: repeated vertices, collinear vertices, NaN and inf vertices, indices out
    of range (negative and >= V).  The collinear faces lie right next to query points of the "degenerate" case."""
    verts, faces = soup(40, 7, size=0.3)
    extra = torch.tensor([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3],          # 120 .. 122: collinear
                          [math.nan, 0.0, 0.0], [0.0, math.inf, 0.0], [0.0, 0.0, -math.inf],   # 123 .. 125
                          [0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0]])          # 126 .. 128: collinear on the x axis
    verts = torch.cat([verts, extra])
    bad = torch.tensor([[120, 121, 122], [5, 5, 9], [11, 12, 11], [3, 123, 4], [124, 6, 7], [8, 9, 125], [0, 1, 129], [-1, 2, 3],
                        [126, 127, 128], [13, 14, 2 ** 31 - 1], [20, 20, 20]], dtype=torch.int64)
    order = torch.cat([bad[:4], faces[:15], bad[4:8], faces[15:], bad[8:]])
    return verts, order


def tiny_faces_mesh(F=SCAN_SPAN + 300):
    """F - 1 small right triangles whose doubled area is 1.6 * 2^-30 of the one big face that comes LAST: q = 2 each (1 if truncated),
    so C_i = 2 (i + 1) over the small faces, and a sample whose t falls among them tells `C_i > t` from `C_i >= t`.  More faces than
    one pass of the scan kernel covers."""
    n = F - 1
    leg = math.sqrt(1.6) * 2.0 ** -15
    i = torch.arange(n)
    base = torch.stack([(i % 256).float() * 2.0 ** -9, (i // 256).float() * 2.0 ** -9, torch.full((n,), 0.5)], dim=1)
    tri = torch.stack([base, base + torch.tensor([leg, 0.0, 0.0]), base + torch.tensor([0.0, leg, 0.0])], dim=1)
    verts = torch.cat([tri.reshape(3 * n, 3), torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])]).float()
    return verts.contiguous(), torch.arange(3 * F, dtype=torch.int64).reshape(F, 3)


def special_points_case():
    """Points exactly on vertices, on edge midpoints, on faces and on symmetry planes, with the faces that tie there.
    faces 0, 1: two coplanar triangles mirrored in x = 0 (sharing the edge on the y axis); faces 2, 3: a triangle and its mirror image
    in z = 0 -- both far from 0, 1; faces 4, 5: the same triangle twice; face 6: a 3-4-5-scaled triangle whose nn is not a power of two."""
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0],                      # 0 .. 3
                          [5, 0, 0.5], [6, 0, 0.25], [5, 1, 0.75], [5, 0, -0.5], [6, 0, -0.25], [5, 1, -0.75],   # 4 .. 9
                          [0, 5, 0], [1, 5, 0], [0, 6, 0],                                  # 10 .. 12
                          [-5, 0, 0], [-2, 0, 0], [-5, 3, 0]], dtype=torch.float32)        # 13 .. 15
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 9, 8], [10, 11, 12], [10, 11, 12], [13, 14, 15]], dtype=torch.int64)
    pts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 0, 0.5],                        # on vertices
           [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0],             # on edge midpoints
           [0.25, 0.25, 0], [-0.25, 0.5, 0], [0.25, 5.25, 0],                   # on faces
           [0, 0.5, 0.7], [0, 0.25, -0.3], [0, 2.0, 0.1], [0, -1.0, 0.0],       # x = 0: between faces 0 and 1
           [5.25, 0.25, 0], [5.5, 0.5, 0], [4.0, 0.3, 0], [7.0, -1.0, 0],       # z = 0: between faces 2 and 3
           [0.3, 5.3, 0.4], [2.0, 5.0, 0.3], [-1.0, 7.0, -0.2]]                 # the doubled face
    # above the edge v13 -> v14 of face 6 (s_0 == 0 exactly; the projection falls on the edge): d_p and d_e round differently
    pts += [[-5 + 0.37 * k, 0, 0.1 + 0.13 * k] for k in range(1, 8)]
    return verts, faces, torch.tensor(pts, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def dist_case(name):
    """-> {"verts": [..], "faces": [..], "points": (B, P, 3)}"""
    if name.startswith("soup_"):   # soup_f<F>_p<P>
        F, P = int(name.split("_")[1][1:]), int(name.split("_")[2][1:])
        v, f = soup(F, 100 + F)
        return {"verts": [v], "faces": [f], "points": cloud(P, 200 + P)[None]}
    if name == "batch3":
        far = (100.0, -50.0, 25.0)
        v0, f0 = icosphere(1, 0.5)
        v1, f1 = soup(300, 11, centre=far)
        v2, f2 = torch.rand(4, 3, generator=torch.Generator().manual_seed(3)), torch.zeros(0, 3, dtype=torch.int64)
        pts = torch.stack([cloud(65, 21), cloud(65, 22, centre=far), cloud(65, 23)])
        return {"verts": [v0, v1, v2], "faces": [f0, f1, f2], "points": pts}
    if name == "degenerate":
        v, f = degenerate_mesh()
        pts = cloud(120, 31)
        pts[5], pts[17, 1], pts[40, 2], pts[41] = math.nan, math.inf, -math.inf, torch.tensor([math.nan, math.inf, 0.0])
        near = torch.tensor([[0.15, 0.15, 0.15], [0.2, 0.2, 0.21], [0.6, 0.001, 0.0], [0.3, 0.0, 0.0], [0.75, 0.0, 0.001]])
        return {"verts": [v], "faces": [f], "points": torch.cat([pts, near])[None]}
    if name == "special":
        v, f, pts = special_points_case()
        return {"verts": [v], "faces": [f], "points": pts[None]}
    if name == "no_valid_face":
        v, _ = soup(4, 5)
        return {"verts": [v], "faces": [torch.tensor([[0, 0, 1], [2, 3, 99]])], "points": cloud(9, 41)[None]}
    raise KeyError(name)


# F one below, at and one above the face tile and across two tiles; P = 1, 63, 65 and one above the workgroup
DIST_CASES = [f"soup_f{TILE - 1}_p1", f"soup_f{TILE}_p63", f"soup_f{TILE + 1}_p65", f"soup_f{2 * TILE + 1}_p{THREADS + 1}", "batch3",
              "degenerate", "special", "no_valid_face"]


@functools.lru_cache(maxsize=None)
def dist_ref(name, mutant=None):
    c = dist_case(name)
    return distance_batch(c["verts"], c["faces"], c["points"], mutant)


def sample_keys(count, first_index=0, seed=SEED):
    return [ref_rng.shape_key(seed, first_index + m) for m in range(count)]


TINY_DRAW = 7   # the draw of the "tiny" case: chosen so that samples land among the small faces (asserted by the host test)


@functools.lru_cache(maxsize=None)
def sample_case(name):
    """-> {"verts", "faces", "S", "keys", "draw"}"""
    if name in ("ico_s1", "ico_s3", "ico_s4097"):
        v, f = icosphere(2, 0.7, (0.1, -0.2, 0.3))
        return {"verts": [v], "faces": [f], "S": int(name.split("_s")[1]), "keys": sample_keys(1), "draw": 0}
    if name == "batch3":
        c = dist_case("batch3")
        return {"verts": c["verts"], "faces": c["faces"], "S": 130, "keys": sample_keys(3, 7), "draw": 3}
    if name == "degenerate":
        v, f = degenerate_mesh()
        return {"verts": [v], "faces": [f], "S": 300, "keys": sample_keys(1, 2), "draw": 1}
    if name == "box":
        v, f = box_mesh(1.0, 2.0, 3.0)
        return {"verts": [v], "faces": [f], "S": 257, "keys": sample_keys(1, 4), "draw": 0}
    if name == "tiny":
        v, f = tiny_faces_mesh()
        return {"verts": [v], "faces": [f], "S": 4097, "keys": sample_keys(1, 5), "draw": TINY_DRAW}
    if name == "no_valid_face":
        c = dist_case("no_valid_face")
        return {"verts": c["verts"], "faces": c["faces"], "S": 5, "keys": sample_keys(1), "draw": 0}
    raise KeyError(name)


SAMPLE_CASES = ["ico_s1", "ico_s3", "ico_s4097", "batch3", "degenerate", "box", "tiny", "no_valid_face"]


@functools.lru_cache(maxsize=None)
def sample_ref(name, mutant=None):
    c = sample_case(name)
    return sample_batch(c["verts"], c["faces"], c["S"], c["keys"], c["draw"], mutant=mutant)


# measured by tools/mesh_metrics_gap.py (pair_gap below): case -> (worst absolute, worst relative) float32-vs-float64 gap per pair;
# tests/test_mesh_metrics_host.py asserts GAP_MARGIN times these.  The absolute figure follows the scale of the case: coordinates
# around 100 in batch3, squared distances around 100 in "special".
GAP = {
    "soup_f255_p1": (1.014e-07, 5.066e-07),
    "soup_f256_p63": (4.080e-07, 3.544e-06),
    "soup_f257_p65": (2.587e-07, 1.946e-06),
    "soup_f513_p257": (3.971e-07, 1.939e-05),
    "batch3": (8.855e-06, 3.077e-04),
    "degenerate": (2.696e-07, 6.088e-07),
    "special": (1.080e-05, 1.463e-07),
}
GAP_MARGIN = 2.0
UNIT_GAP_ABS = GAP_MARGIN * max(GAP[k][0] for k in GAP if k.startswith("soup_"))   # shapes inside a unit cube around the origin


REL_FLOOR = 1e-6


def pair_gap(name):
    """(worst absolute gap, worst gap relative to the float64 value where that is >= REL_FLOOR, pairs) between the float32 rule and the float64
    evaluation of the same formulas over the (finite point, valid face) pairs of a distance case"""
    c = dist_case(name)
    worst_abs = worst_rel = 0.0
    pairs = 0
    for verts, faces, pts in zip(c["verts"], c["faces"], c["points"]):
        pts = pts[torch.isfinite(pts).all(dim=1)]
        if faces.shape[0] == 0 or pts.shape[0] == 0:
            continue
        d32 = pair_sqdist(face_quantities(verts, faces), pts)
        fq64 = face_quantities(verts, faces, torch.float64)
        fq64["valid"] = face_quantities(verts, faces)["valid"]   # the float32 rule decides which faces take part
        d64 = pair_sqdist(fq64, pts.double())
        ok = torch.isfinite(d32) & torch.isfinite(d64)
        if not bool(ok.any()):
            continue
        gap = (d32.double() - d64).abs()[ok]
        worst_abs = max(worst_abs, float(gap.max()))
        big = d64[ok] >= REL_FLOOR
        if bool(big.any()):
            worst_rel = max(worst_rel, float((gap[big] / d64[ok][big]).max()))
        pairs += int(ok.sum())
    return worst_abs, worst_rel, pairs



def bits(t):
    """float32 tensors as their bit patterns (so that -0.0 != 0.0 and NaN == NaN), others unchanged"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
