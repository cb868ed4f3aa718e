"""TEST INFRASTRUCTURE: CPU restatement of the mesher (bdm_amd/csrc/surface.hip, section 12 of bdm_hip.h: fixed-point IMLS grid
and surface nets), its MUTANTS, the clouds its tests share with their analytic outward normals, and the case table of the GPU test.

Steps 1 - 3: torch float32 elementwise arithmetic in the header's order, every operation a separate rounded tensor op (nothing is
contracted; torch's CPU division is correctly rounded).  Step 4: int64 sums, stored as int32.  Steps 5, 6: integer masks and
torch.nonzero for the ascending orders; the vertex positions again in float32, operation by operation."""
import functools
import itertools
import math

import torch

MUTANTS = ("window_shifted", "su_le", "truncate", "no_clamp", "defined_any_weight", "never_reversed", "skip_dropped", "axis_major_edges")
FIX = 4096

# the 12 edges of a cell in the header's order: corner a in lexicographic (dx, dy, dz), then axis 0, 1, 2 with a[axis] == 0
EDGES = [(a, axis) for a in itertools.product((0, 1), repeat=3) for axis in range(3) if a[axis] == 0]
EDGES_AXIS_MAJOR = sorted(EDGES, key=lambda e: (e[1], e[0]))   # the mutant's order


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def threshold(min_weight):
    return max(1, int(torch.round(f32(min_weight) * f32(float(FIX)))))


def grid_of(points, normals, R, s, mutant=None):
    """Steps 1 - 4 of one cloud -> dict(SW, SU (R, R, R) int32, valid, live, c (3,), inv)."""
    p, nr = points.float(), normals.float()
    SW, SU = torch.zeros(R ** 3, dtype=torch.int64), torch.zeros(R ** 3, dtype=torch.int64)
    ok = torch.isfinite(p).all(dim=1) & torch.isfinite(nr).all(dim=1)
    out = {"valid": int(ok.sum()), "live": False, "c": None, "inv": None}
    if out["valid"]:
        pv, nv = p[ok], nr[ok]
        lo, hi = pv.amin(dim=0), pv.amax(dim=0)
        out["live"] = not bool((lo == hi).all())
    if out["live"]:
        c = f32(0.5) * (lo + hi)
        half = (f32(0.5) * (hi - lo)).amax()
        inv = f32(float(R - 1 - 2 * (s + 1))) / (f32(2.0) * half)
        mid = f32((R - 1) / 2)
        q = (pv - c) * inv + mid
        keep = ((q >= 0) & (q <= R - 1)).all(dim=1)
        q, nv = q[keep], nv[keep]
        base = torch.floor(q).long()
        s2, lim = f32(float(s * s)), float(FIX * s)
        offsets = range(-s, s) if mutant == "window_shifted" else range(-s + 1, s + 1)
        for o in itertools.product(offsets, repeat=3):
            g = base + torch.tensor(o)
            inside = ((g >= 0) & (g <= R - 1)).all(dim=1)
            d = g.float() - q
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            t = s2 - d2
            w = t / s2
            w3 = (w * w) * w
            a = (nv[:, 0] * dx + nv[:, 1] * dy) + nv[:, 2] * dz
            u = w3 * a
            rnd = torch.trunc if mutant == "truncate" else torch.round   # torch.round: half to even
            W = rnd(w3 * f32(float(FIX)))
            U = rnd(u * f32(float(FIX)))
            U = torch.where(torch.isnan(U), torch.zeros_like(U), U.clamp(-2.0 ** 40, 2.0 ** 40) if mutant == "no_clamp" else U.clamp(-lim, lim))
            hit = inside & (t > 0)
            lin = ((g[:, 0] * R + g[:, 1]) * R + g[:, 2])[hit]
            SW.index_add_(0, lin, W[hit].long())
            SU.index_add_(0, lin, U[hit].long())
        out["c"], out["inv"] = c, inv
    out["SW"], out["SU"] = SW.view(R, R, R).int(), SU.view(R, R, R).int()
    return out


def mesh_of(grid, R, thr, mutant=None):
    """Steps 5, 6 from the grid -> dict(verts (V, 3) float32, faces (F, 3) int32, skipped)."""
    SW, SU = grid["SW"], grid["SU"]
    defined = (SW > 0) if mutant == "defined_any_weight" else (SW >= thr)
    neg = (SU <= 0) if mutant == "su_le" else (SU < 0)
    f = SU.float() / SW.float()
    m = R - 1
    all_def, n_neg = torch.ones(m, m, m, dtype=torch.bool), torch.zeros(m, m, m, dtype=torch.int64)
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        all_def &= defined[dx:dx + m, dy:dy + m, dz:dz + m]
        n_neg += neg[dx:dx + m, dy:dy + m, dz:dz + m]
    active = torch.zeros(R, R, R, dtype=torch.bool)            # indexed by the cell's lowest corner, as the kernel's map
    active[:m, :m, :m] = all_def & (n_neg >= 1) & (n_neg <= 7)
    cells = torch.nonzero(active.flatten())[:, 0]               # ascending (i R + j) R + k: the order of (i (R-1) + j)(R-1) + k
    ids = torch.full((R ** 3,), -1, dtype=torch.int64)
    ids[cells] = torch.arange(cells.numel())
    verts = torch.zeros(cells.numel(), 3, dtype=torch.float32)
    if cells.numel():
        ci = torch.stack([cells // (R * R), (cells // R) % R, cells % R], dim=1)
        total, count = torch.zeros(cells.numel(), 3, dtype=torch.float32), torch.zeros(cells.numel(), dtype=torch.float32)
        for a, axis in (EDGES_AXIS_MAJOR if mutant == "axis_major_edges" else EDGES):
            e = tuple(a[x] + (x == axis) for x in range(3))
            ia, ie = (ci[:, 0] + a[0], ci[:, 1] + a[1], ci[:, 2] + a[2]), (ci[:, 0] + e[0], ci[:, 1] + e[1], ci[:, 2] + e[2])
            cross = neg[ia] != neg[ie]
            tt = f[ia] / (f[ia] - f[ie])
            point = torch.stack([tt if x == axis else torch.full_like(tt, float(a[x])) for x in range(3)], dim=1)
            total = torch.where(cross[:, None], total + point, total)
            count = count + cross.float()
        pos = ci.float() + total / count[:, None]
        verts = (pos - f32((R - 1) / 2)) / grid["inv"] + grid["c"]
    idx = torch.arange(R)
    coord = [idx.view(R, 1, 1).expand(R, R, R), idx.view(1, R, 1).expand(R, R, R), idx.view(1, 1, R).expand(R, R, R)]
    stride = (R * R, R, 1)
    faces, skipped = [], 0
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        place = (coord[axis] <= R - 2) & (coord[u] >= 1) & (coord[u] <= R - 2) & (coord[v] >= 1) & (coord[v] <= R - 2)
        up = lambda x: torch.roll(x, -1, dims=axis)             # the value at g + e_axis (the wrap is masked by `place`)
        cand = place & defined & up(defined) & (neg != up(neg))
        a11 = active
        a10, a01 = torch.roll(active, 1, dims=v), torch.roll(active, 1, dims=u)
        a00 = torch.roll(a10, 1, dims=u)
        all4 = a00 & a10 & a11 & a01
        skipped += int((cand & ~all4).sum())
        emit = cand if mutant == "skip_dropped" else cand & all4
        g = torch.nonzero(emit.flatten())[:, 0]                 # ascending linear order of the lower node
        c00, c10, c11, c01 = ids[g - stride[u] - stride[v]], ids[g - stride[v]], ids[g], ids[g - stride[u]]
        keep = neg.flatten()[g] if mutant != "never_reversed" else torch.ones_like(g, dtype=torch.bool)
        quad = torch.where(keep[:, None], torch.stack([c00, c10, c11, c01], dim=1), torch.stack([c01, c11, c10, c00], dim=1))
        faces.append(torch.stack([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], dim=1).reshape(-1, 3))
    return {"verts": verts, "faces": torch.cat(faces).int(), "skipped": skipped}


def reconstruct(points, normals, R, s, min_weight=0.0, mutant=None):
    """One cloud -> dict(SW, SU, counts [V, F, skipped, valid], verts, faces)."""
    grid = grid_of(points, normals, R, s, mutant)
    mesh = mesh_of(grid, R, threshold(min_weight), mutant)
    return {"SW": grid["SW"], "SU": grid["SU"], "verts": mesh["verts"], "faces": mesh["faces"],
            "counts": [mesh["verts"].shape[0], mesh["faces"].shape[0], mesh["skipped"], grid["valid"]]}


def reconstruct_batch(points, normals, R, s, min_weight=0.0, mutant=None):
    return [reconstruct(p, n, R, s, min_weight, mutant) for p, n in zip(points, normals)]


def default_resolution(n):
    return min(256, max(16, 8 * round(math.sqrt(n / 4) / 8)))


# ---- clouds with analytic outward normals: (points (n, 3), normals (n, 3)) float32 ----------------------------------------------------
def _unit(g, n):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=1)


def sphere(g, n, r=0.4, noise=0.0):
    d = _unit(g, n)
    p = d * r
    if noise:
        p = p + noise * torch.randn(n, 3, generator=g, dtype=torch.float64)
    return p.float(), d.float()


def ellipsoid(g, n, axes=(0.5, 0.3, 0.2), centre=(0.0, 0.0, 0.0)):
    d = _unit(g, n)
    ax = torch.tensor(axes, dtype=torch.float64)
    nrm = torch.nn.functional.normalize(d / ax, dim=1)
    return (d * ax + torch.tensor(centre, dtype=torch.float64)).float(), nrm.float()


def torus(g, n, R=0.35, r=0.12):
    """Rejection-sampled uniformly in area."""
    out_t, out_p = [], []
    while sum(t.numel() for t in out_t) < n:
        th, ph, w = (torch.rand(2 * n, generator=g, dtype=torch.float64) for _ in range(3))
        th, ph = 2 * math.pi * th, 2 * math.pi * ph
        ok = w < (R + r * torch.cos(ph)) / (R + r)
        out_t.append(th[ok]), out_p.append(ph[ok])
    th, ph = torch.cat(out_t)[:n], torch.cat(out_p)[:n]
    ring = torch.stack([torch.cos(th), torch.sin(th), torch.zeros_like(th)], dim=1)
    nrm = ring * torch.cos(ph)[:, None] + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) * torch.sin(ph)[:, None]
    return (ring * R + nrm * r).float(), nrm.float()


def cube(g, n, side=0.8):
    face = torch.randint(0, 6, (n,), generator=g)
    uv = (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * side
    axis, sign = face // 2, (face % 2).double() * 2 - 1
    p, nrm = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64)
    for a in range(3):
        m = axis == a
        p[m, a], nrm[m, a] = sign[m] * side / 2, sign[m]
        p[m, (a + 1) % 3], p[m, (a + 2) % 3] = uv[m, 0], uv[m, 1]
    return p.float(), nrm.float()


def two_spheres(g, n, r=0.2, gap=0.6):
    pa, na = sphere(g, n // 2, r)
    pb, nb = sphere(g, n - n // 2, r)
    shift = torch.tensor([gap / 2, 0.0, 0.0])
    return torch.cat([pa - shift, pb + shift]), torch.cat([na, nb])


def lattice_plane(m=32):
    """m x m points on the plane z = 0.25, normals +z: an open surface with zero extent on one axis."""
    x = torch.linspace(-0.5, 0.5, m)
    p = torch.stack([x.view(m, 1).expand(m, m), x.view(1, m).expand(m, m), torch.full((m, m), 0.25)], dim=-1).reshape(-1, 3)
    return p.float(), torch.tensor([0.0, 0.0, 1.0]).expand(m * m, 3).contiguous()


def on_nodes(R=16, s=2):
    """Points exactly on grid nodes: integer coordinates spanning [0, R - 1 - 2 (s + 1)] give inv = 1 and q = p + s + 1.  A pair with
    opposite normals at (4, 4, 4) leaves SU = 0 with SW > 0 around it; a point two nodes above, whose long normal makes U clamp, turns
    the nodes between negative: cells with corners of SU = 0 and SU < 0 only (the >= 0 side of rule 4).  A short wall of on-node
    points beside them gives ordinary cells."""
    span = R - 1 - 2 * (s + 1)
    pts = [(0, 0, 0), (span, span, span), (4, 4, 4), (4, 4, 4), (4, 4, 6)]
    nrm = [(0, 0, -1), (0, 0, 1), (0, 0, 1), (0, 0, -1), (0, 0, 50)]
    for x in range(0, span + 1):
        for y in range(0, 3):
            pts.append((x, y, 2)), nrm.append((0, 0, 1))
    return torch.tensor(pts, dtype=torch.float32), torch.tensor(nrm, dtype=torch.float32)


def with_nonfinite(points, normals, g, bad_points=16, bad_normals=24):
    """Copies with `bad_points` rows of NaN / inf coordinates and `bad_normals` other rows of NaN normals."""
    p, nr = points.clone(), normals.clone()
    rows = torch.randperm(p.shape[0], generator=g)[:bad_points + bad_normals]
    for e, i in enumerate(rows[:bad_points].tolist()):
        p[i, e % 3] = (float("nan"), float("inf"), float("-inf"))[e % 3]
    nr[rows[bad_points:], 1] = float("nan")
    return p, nr


# ---- the GPU case table: name -> (points (b, n, 3), normals (b, n, 3), R, s, min_weight) ----------------------------------------------
def _stack(clouds):
    return torch.stack([c[0] for c in clouds]), torch.stack([c[1] for c in clouds])


def _torus_case(R, s, min_weight=0.0):
    return lambda: (*_stack([torus(torch.Generator().manual_seed(3201), 1500)]), R, s, min_weight)


def _case_b1_n65():
    return (*_stack([sphere(torch.Generator().manual_seed(3200), 65)]), 16, 2, 0.0)


def _case_ellipsoids():
    g = torch.Generator().manual_seed(3202)
    return (*_stack([ellipsoid(g, 1025), ellipsoid(g, 1025, (0.3, 0.45, 0.25), (100.0, -50.0, 25.0)), ellipsoid(g, 1025, (0.2, 0.2, 0.5))]), 32, 3, 0.0)


def _case_nonfinite():
    g = torch.Generator().manual_seed(3203)
    return (*_stack([with_nonfinite(*sphere(g, 300), g), with_nonfinite(*ellipsoid(g, 300), g)]), 16, 3, 0.0)


def _case_all_equal():
    return torch.full((1, 40, 3), 0.125), torch.tensor([0.0, 0.0, 1.0]).expand(1, 40, 3).contiguous(), 16, 2, 0.0


def _case_lattice():
    return (*_stack([lattice_plane(32)]), 32, 3, 0.0)


def _case_on_nodes():
    return (*_stack([on_nodes(16, 2)]), 16, 2, 0.0)


CASES = {"b1_n65_R16_s2": _case_b1_n65, "b3_n1025_ellipsoids_R32_s3": _case_ellipsoids, "b2_n300_nonfinite_R16_s3": _case_nonfinite,
         "b1_n40_all_equal": _case_all_equal, "lattice_plane_R32_s3": _case_lattice, "on_nodes_pair_R16_s2": _case_on_nodes,
         "torus_R48_s2_min_weight": _torus_case(48, 2, 0.05)}
CASES.update({f"torus_R{R}_s{s}": _torus_case(R, s) for R in (16, 32, 48) for s in (2, 3, 4)})
# the inputs on which every mutant is asserted to change an output (tests/test_surface_host.py): the small ones
MUTANT_CASES = ("b1_n65_R16_s2", "on_nodes_pair_R16_s2", "lattice_plane_R32_s3", "torus_R48_s2_min_weight", "torus_R16_s2")
LARGE_CASE = ("b1_n16384_torus_R128_s4", lambda: (*_stack([torus(torch.Generator().manual_seed(3204), 16384)]), 128, 4, 0.0))
FINE_CASE = ("b1_n4096_sphere_R256_s2", lambda: (*_stack([sphere(torch.Generator().manual_seed(3205), 4096)]), 256, 2, 0.0))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_ref(name, mutant=None):
    pts, nrm, R, s, mw = case_inputs(name)
    return reconstruct_batch(pts, nrm, R, s, mw, mutant)


def same_mesh(a, b):
    """Bit equality of two results of `reconstruct` (verts compared as bits: equal floats, no NaN expected)."""
    return (torch.equal(a["SW"], b["SW"]) and torch.equal(a["SU"], b["SU"]) and list(a["counts"]) == list(b["counts"]) and
            torch.equal(a["verts"].view(torch.int32), b["verts"].view(torch.int32)) and torch.equal(a["faces"], b["faces"]))
