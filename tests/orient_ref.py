"""TEST INFRASTRUCTURE: CPU restatement of the visibility-voting orientation (bdm_amd/csrc/orient.hip, section 11 of bdm_hip.h),
its MUTANTS, the clouds its tests share with their true outward normals, and the case table of the GPU test.

Projection: torch float32 elementwise arithmetic in the header's order, every operation a separate rounded tensor op (nothing is
contracted; torch's CPU division and sqrt are correctly rounded).  Z-buffer, votes and the Jacobi fallback are integer."""
import functools
import math

import numpy as np
import torch

import normals_ref as R

MUTANTS = ("no_eps", "splat0", "depth_reversed", "lt", "gauss_seidel", "self_not_skipped")
DEFAULTS = dict(num_views=32, resolution=128, splat=2, depth_tolerance_px=2.0, fallback_k=8, fallback_rounds=8)


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def floor_clamp(x, hi):
    """clamp(floor(x), 0, hi) as int64; NaN -> 0."""
    f = torch.floor(x)
    return torch.where(f >= 0, torch.minimum(f, f32(float(hi))), torch.zeros_like(f)).long()


def sgn(x):
    """+1, -1, 0 (zero or NaN) as int64."""
    return (x > 0).long() - (x < 0).long()


def eps_of(depth_tolerance_px, resolution):
    return int(round(depth_tolerance_px * 65536 / resolution))


def vote(points, normals, views, r, splat, eps, mutant=None):
    """Votes of one cloud: dict of votes (n,), seen (n,) int32 and the counts the input checks look at: clipped (splats cut at
    the image border), ties (pixels whose nearest key two or more points share), zero_dots (visible pairs with sigma = 0)."""
    p, nr, views = points.float(), normals.float(), views.float()
    n = p.shape[0]
    votes, seen = torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)
    stats = {"clipped": 0, "ties": 0, "zero_dots": 0}
    finite = torch.isfinite(p).all(dim=1)
    if mutant == "no_eps":
        eps = 0
    if mutant == "splat0":
        splat = 0
    if int(finite.sum()) == 0:
        return {"votes": votes.int(), "seen": seen.int(), **stats}
    pf = p[finite]
    c = f32(0.5) * (pf.amin(dim=0) + pf.amax(dim=0))
    q = pf - c
    rho = dot(q[:, 0], q[:, 1], q[:, 2], q[:, 0], q[:, 1], q[:, 2]).amax()
    if not bool(rho > 0):
        return {"votes": votes.int(), "seen": seen.int(), **stats}
    h = f32(1.02) * torch.sqrt(rho)
    half_r, one, big = f32(0.5 * r), f32(1.0), 1 << 40
    where = torch.nonzero(finite)[:, 0]
    nf = nr[finite]
    for u, w, d in views:
        a, b, t = (dot(q[:, 0], q[:, 1], q[:, 2], e[0], e[1], e[2]) for e in (u, w, d))
        X = floor_clamp((a / h + one) * half_r, r - 1)
        Y = floor_clamp((b / h + one) * half_r, r - 1)
        depth = (one + t / h) if mutant == "depth_reversed" else (one - t / h)
        Z = floor_clamp(depth * f32(32768.0), 65535)
        zb = torch.full((r * r,), big, dtype=torch.int64)
        hits = []
        for ox in range(-splat, splat + 1):
            for oy in range(-splat, splat + 1):
                x, y = X + ox, Y + oy
                inside = (x >= 0) & (x < r) & (y >= 0) & (y < r)
                stats["clipped"] += int((~inside).sum())
                hits.append(((x * r + y)[inside], Z[inside]))
        pix, key = torch.cat([hh[0] for hh in hits]), torch.cat([hh[1] for hh in hits])
        zb.scatter_reduce_(0, pix, key, "amin")
        nearest = torch.zeros(r * r, dtype=torch.int64).scatter_add_(0, pix, (key == zb[pix]).long())
        stats["ties"] += int((nearest >= 2).sum())
        own = zb[X * r + Y]
        visible = (Z < own + eps) if mutant == "lt" else (Z <= own + eps)
        sigma = sgn(dot(nf[:, 0], nf[:, 1], nf[:, 2], d[0], d[1], d[2]))
        stats["zero_dots"] += int((visible & (sigma == 0)).sum())
        votes[where] += visible.long() * sigma
        seen[where] += visible.long()
    return {"votes": votes.int(), "seen": seen.int(), **stats}


def fallback(s, normals, knn_idx, kg, rounds, mutant=None):
    """The Jacobi rounds on the state s (n,) int64 -> (s, decided_round (n,): 0 = by its votes, r >= 1 = in fallback round r,
    -1 = still undecided, rounds run).  gauss_seidel (in place, ascending index) and self_not_skipped are mutants."""
    nr = normals.float()
    n, k = knn_idx.shape
    i_of = torch.arange(n)[:, None]
    ok = (knn_idx >= 0) & (knn_idx < n)
    if mutant != "self_not_skipped":
        ok = ok & (knn_idx != i_of)
    window = ok & (torch.cumsum(ok.long(), dim=1) <= kg)
    nb = knn_idx.clamp(0, n - 1)
    sd = sgn(dot(nr[:, None, 0], nr[:, None, 1], nr[:, None, 2], nr[nb][..., 0], nr[nb][..., 1], nr[nb][..., 2])) * window.long()
    s = s.clone()
    decided = torch.where(s != 0, 0, -1)
    ran = 0
    for rnd in range(1, rounds + 1):
        ran = rnd
        if mutant == "gauss_seidel":
            new = s.clone()
            for i in torch.nonzero(s == 0)[:, 0].tolist():
                new[i] = int(sgn((new[nb[i]] * sd[i]).sum()))
        else:
            new = torch.where(s == 0, sgn((s[nb] * sd).sum(dim=1)), s)
        changed = new != s
        decided[changed] = rnd
        s = new
        if not bool(changed.any()):
            break
    return s, decided, ran


def orient(points, normals, knn_idx, views, r, splat, eps, kg, rounds, mutant=None):
    """The whole rule for one cloud (points, normals (n, 3) float32; knn_idx (n, k) int64): dict of normals_out (n, 3) float32,
    votes, seen (n,) int32, undecided (int), s (n,) the final state, s_vote (n,) the state after voting, decided_round (n,),
    rounds_run, and vote()'s counts."""
    v = vote(points, normals, views, r, splat, eps, mutant)
    s_vote = sgn(v["votes"])
    s, decided, ran = fallback(s_vote, normals, knn_idx, kg, rounds, mutant)
    bits = normals.float().contiguous().view(torch.int32)
    out = torch.where((s < 0)[:, None], bits ^ torch.tensor(-2 ** 31, dtype=torch.int32), bits).view(torch.float32)
    return {**v, "normals_out": out, "undecided": int((s == 0).sum()), "s": s, "s_vote": s_vote, "decided_round": decided,
            "rounds_run": ran}


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN normals stay NaN and must keep their bits)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def wrong_share(oriented, truth, estimated=None, well=0.7):
    """(wrong, counted): oriented normals with a non-positive dot product with the true outward normal, among the points whose
    estimated normal has |n . n_true| > well (all finite points when well is None)."""
    o, t = np.asarray(oriented, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    d = np.einsum("ni,ni->n", o, t)
    keep = np.isfinite(d) if well is None else np.abs(np.einsum("ni,ni->n", np.asarray(o if estimated is None else estimated, dtype=np.float64), t)) > well
    return int((d[keep] <= 0).sum()), int(keep.sum())


# ---- clouds with their true outward normals ---------------------------------------------------------------------------------------
def sphere(g, n, radius=0.3, centre=(0.0, 0.0, 0.0)):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    return (d * radius + torch.tensor(centre, dtype=torch.float64)).float(), d.float()


def torus(g, n, R_=0.3, r_=0.1):
    u = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    v = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    pts = torch.stack([(R_ + r_ * torch.cos(v)) * torch.cos(u), (R_ + r_ * torch.cos(v)) * torch.sin(u), r_ * torch.sin(v)], dim=1)
    nrm = torch.stack([torch.cos(v) * torch.cos(u), torch.cos(v) * torch.sin(u), torch.sin(v)], dim=1)
    return pts.float(), nrm.float()


def two_spheres(g, n, gap=1.0):
    a, na = sphere(g, n // 2, centre=(-0.5 * gap, 0.0, 0.0))
    b, nb = sphere(g, n - n // 2, centre=(0.5 * gap, 0.0, 0.0))
    return torch.cat([a, b]), torch.cat([na, nb])


def ellipsoid(g, n, axes, centre=(0.0, 0.0, 0.0)):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    ax = torch.tensor(axes, dtype=torch.float64)
    nrm = d / ax
    return (d * ax + torch.tensor(centre, dtype=torch.float64)).float(), (nrm / nrm.norm(dim=1, keepdim=True)).float()


def box(g, n, size, centre=(0.0, 0.0, 0.0), skip=()):
    """n points uniform on the surface of an axis-aligned box (faces chosen by area), faces named in `skip` ("+z", "-x", ...) left
    out; -> (points, outward face normals)."""
    size = torch.tensor(size, dtype=torch.float64)
    faces = [(ax, sg) for ax in range(3) for sg in (-1.0, 1.0) if ("+" if sg > 0 else "-") + "xyz"[ax] not in skip]
    area = torch.tensor([float(size[(ax + 1) % 3] * size[(ax + 2) % 3]) for ax, _ in faces], dtype=torch.float64)
    which = torch.multinomial(area / area.sum(), n, replacement=True, generator=g)
    pts = (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * size
    nrm = torch.zeros(n, 3, dtype=torch.float64)
    for f, (ax, sg) in enumerate(faces):
        m = which == f
        pts[m, ax] = sg * 0.5 * size[ax]
        nrm[m, ax] = sg
    return (pts + torch.tensor(centre, dtype=torch.float64)).float(), nrm.float()


def slab(g, n, thickness=0.05):
    return box(g, n, (1.0, 0.6, thickness))


def table(g, n, top=0.04, leg=0.06, height=0.18, length=0.7, width=0.45):
    """A slab on four legs (boxes whose top faces, hidden under the slab, are left out); the points are shared by surface area.
    The extents are chosen by two arguments, at 4000 points and k = 16.  The neighbourhood radius sqrt(k A / (pi n)) = 0.034 of
    the total area A = 0.89 stays below the top's thickness 0.04: the neighbourhoods of the top's two large faces do not reach
    each other, so there the neighbour-majority rule is the coin flip the feature is for, not a systematic inward pull.  And
    those two faces (2 x 0.7 x 0.45 = 0.63) are 70 % of A: a coin flip on them leaves more than 30 % of the signs on either
    side whatever the rule does on the legs, whose 0.06-wide faces every neighbourhood wraps around (a low table)."""
    parts = [((length, width, top), (0.0, 0.0, 0.0), ())]
    for sx in (-1, 1):
        for sy in (-1, 1):
            parts.append(((leg, leg, height), (sx * (0.5 * length - 0.5 * leg - 0.02), sy * (0.5 * width - 0.5 * leg - 0.02), -0.5 * top - 0.5 * height), ("+z",)))
    areas = []
    for size, _, skip in parts:
        a = 2 * (size[0] * size[1] + size[1] * size[2] + size[0] * size[2]) - (size[0] * size[1] if skip else 0.0)
        areas.append(a)
    counts = [int(round(n * a / sum(areas))) for a in areas]
    counts[0] += n - sum(counts)
    made = [box(g, cnt, size, centre, skip) for cnt, (size, centre, skip) in zip(counts, parts)]
    return torch.cat([m[0] for m in made]), torch.cat([m[1] for m in made])


def lattice_plane(side=32, duplicates=60):
    """side x side points of the plane z = 0 at dyadic coordinates (multiples of 1/side: every projection is exact) plus
    `duplicates` exact copies of some of them, with normals (0, 0, 1); AXIS_VIEWS look at it along +x, -x, +y, -y and +z: points
    on pixel borders, equal depth keys (all of them along z), and dot(n, d) == 0 in the four views along x and y."""
    ii, jj = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    pts = torch.stack([ii.flatten() / side - 0.5 + 0.5 / side, jj.flatten() / side - 0.5 + 0.5 / side, torch.zeros(side * side)], dim=1).float()
    pts = torch.cat([pts, pts[7:7 + 17 * duplicates:17]])
    nrm = torch.zeros_like(pts)
    nrm[:, 2] = 1.0
    return pts, nrm


AXIS_VIEWS = torch.tensor([[[0, 1, 0], [0, 0, 1], [1, 0, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                           [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]],
                           [[1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float32)


def default_views(num_views=32):
    from bdm_amd.normals import fibonacci_views
    return fibonacci_views(num_views)


def estimated(points, k, orient=0):
    """(normals (n, 3) float32, knn_idx (n, k) int64) of the float64 PCA restatement, rounded to float32."""
    est = R.estimate(points, k, orient)
    return torch.from_numpy(est["normals"]).float(), est["idx"]


# ---- the GPU test's case table: name -> (cloud maker, k, parameters) -------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(3000 + seed)


def _ellipsoids():
    g = _gen(1)
    specs = [((0.3, 0.2, 0.1), (0.0, 0.0, 0.0)), ((3.0, 1.0, 2.0), (100.0, -50.0, 25.0)), ((0.02, 0.05, 0.03), (-1.0, 2.0, 0.5))]
    return torch.stack([ellipsoid(g, 1025, ax, ce)[0] for ax, ce in specs])


def _nonfinite():
    g = _gen(2)
    pts = torch.stack([torus(g, 300)[0], sphere(g, 300)[0]])
    bad = R.nonfinite_cloud()[0][0][R.nonfinite_cloud()[1]]
    pts[0, torch.randperm(300, generator=g)[:16]] = bad
    pts[1, torch.randperm(300, generator=g)[:16]] = bad.flip(0)
    return pts


CASES = {   # name -> (points maker -> (b, n, 3), k, overrides of DEFAULTS, explicit views or None)
    "b1_n65_k8": (lambda: sphere(_gen(0), 65)[0][None], 8, {}, None),
    "b3_n1025_ellipsoids": (_ellipsoids, 16, {}, None),
    "b2_n300_nonfinite": (_nonfinite, 16, {}, None),
    "b1_n1024_slab": (lambda: slab(_gen(3), 1024)[0][None], 16, {}, None),
    "b1_n1500_torus": (lambda: torus(_gen(4), 1500)[0][None], 16, {}, None),
    "lattice_axis_views": (lambda: lattice_plane()[0][None], 16, dict(resolution=64, depth_tolerance_px=0.0), AXIS_VIEWS),
    "degenerate_all_equal": (lambda: torch.full((1, 40, 3), 0.25), 16, {}, None),
    "b1_n4000_table": (lambda: table(_gen(6), 4000)[0][None], 16, {}, None),
}
# the largest supported configuration size: its normals and neighbour lists come from the GPU estimator (the CPU restatement of the
# neighbour search would take minutes), so only the GPU test builds it
LARGE_CASE = ("b1_n16384_torus", lambda: torus(_gen(5), 16384)[0][None], 16, DEFAULTS)
for _res in (32, 128):
    for _splat in (0, 2):
        for _views in (1, 32):
            for _rounds in (0, 8):
                CASES[f"torus_r{_res}_s{_splat}_v{_views}_f{_rounds}"] = (
                    lambda: torus(_gen(4), 1500)[0][None], 16, dict(resolution=_res, splat=_splat, num_views=_views, fallback_rounds=_rounds), None)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(points (b, n, 3), normals (b, n, 3) float32, knn_idx (b, n, k) int64, views (v, 3, 3), params dict) of a case.  The
    normals are the float64 PCA restatement's with the canonical sign, rounded to float32; in the lattice case they are (0, 0, 1),
    in the degenerate case (all points equal) as well; in
    the non-finite case 8 further rows of finite points are made NaN."""
    make, k, over, views = CASES[name]
    pts = make()
    par = {**DEFAULTS, **over}
    if views is None:
        views = default_views(par["num_views"])
    nrm, idx = [], []
    for c in range(pts.shape[0]):
        if name == "lattice_axis_views":
            nc, ic = lattice_plane()[1], R.knn(pts[c], k)
        elif name == "degenerate_all_equal":
            nc, ic = torch.tensor([0.0, 0.0, 1.0]).expand(pts.shape[1], 3).clone(), R.knn(pts[c], k)
        else:
            nc, ic = estimated(pts[c], k)
        if name == "b2_n300_nonfinite":
            nc[torch.nonzero(torch.isfinite(nc).all(dim=1))[5:45:5, 0]] = float("nan")
        nrm.append(nc)
        idx.append(ic)
    return pts, torch.stack(nrm), torch.stack(idx), views, par


@functools.lru_cache(maxsize=None)
def case_ref(name, mutant=None):
    """The restatement of every cloud of a case (a list of orient() dicts); computed once, shared, left unchanged."""
    return orient_batch(*case_inputs(name), mutant=mutant)


def orient_batch(pts, nrm, idx, views, par, mutant=None):
    eps = eps_of(par["depth_tolerance_px"], par["resolution"])
    return [orient(pts[c], nrm[c], idx[c], views, par["resolution"], par["splat"], eps, par["fallback_k"], par["fallback_rounds"], mutant)
            for c in range(pts.shape[0])]
