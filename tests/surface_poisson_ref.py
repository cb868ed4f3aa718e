"""TEST INFRASTRUCTURE: CPU restatement of the Poisson mesher (bdm_amd/csrc/surface_poisson.hip, section 22 of bdm_hip.h: splat of
the oriented normals, integer divergence, a fixed schedule of multigrid V-cycles, the level through the samples, the hand-over to the
surface nets of section 12), its MUTANTS and the case table of the GPU test.

Every float32 step is a separate rounded torch op in the header's order (nothing is contracted); sums whose order could matter are
int64.  `dtype=torch.float64` runs the same solve in double precision for the convergence study; only float32 is the rule."""
import functools
import itertools

import torch

import surface_ref as S

MUTANTS = ("ghost_node", "constant_prolongation", "restriction_reversed", "truncate", "border_kept", "iso_nearest", "coarsest_one_fewer",
           "checkerboards_kept")
FIX = 4096
ACCEPTED = (16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256)
PRE, POST, COARSEST, TAIL_SIDE = 2, 2, 32, 20      # sweeps before / after the coarse correction, on the coarsest level; LDS tail
DEFAULT_CYCLES = 12
SU_LIMIT = 2 ** 23
SEPARATE_PASSES = 2                                # passes that take checkerboard grid faces out of SU (step 6)


def sides(R):
    """The sides of the levels: halved while even and above 4."""
    out = [R]
    while out[-1] % 2 == 0 and out[-1] > 4:
        out.append(out[-1] // 2)
    return out


def accepted(R):
    return R % 8 == 0 and 16 <= R <= 256 and sides(R)[-1] <= 8


def nearest_accepted(R):
    return min(ACCEPTED, key=lambda a: (abs(a - R), a))


def launches(R, cycles):
    """Kernel launches and memsets of one bdm_surface_poisson_grid call: frame, memset, splat, divergence; per cycle six per global
    level and one for the LDS tail (the whole solve is one launch when level 0 is in the tail); maximum, samples, level, hand-over;
    the passes over the checkerboard faces; the four of the mark stage."""
    glob = sum(1 for m in sides(R) if m > TAIL_SIDE)
    return 4 + (cycles * (6 * glob + 1) if glob else 1) + 4 + SEPARATE_PASSES + 4


def _t(x, dtype=torch.float32):
    return torch.tensor(x, dtype=dtype)


# ---- steps 1 - 3: frame, splat, divergence ----------------------------------------------------------------------------------------------
def splat_of(points, normals, R, s, mutant=None):
    """-> dict(W, Vx, Vy, Vz (R, R, R) int32, D (R, R, R) int32, valid, live, c, inv, q (the samples' grid coordinates))."""
    p, nr = points.float(), normals.float()
    grids = [torch.zeros(R ** 3, dtype=torch.int64) for _ in range(4)]
    ok = torch.isfinite(p).all(dim=1) & torch.isfinite(nr).all(dim=1)
    out = {"valid": int(ok.sum()), "live": False, "c": None, "inv": None, "q": torch.zeros(0, 3)}
    if out["valid"]:
        pv, nv = p[ok], nr[ok]
        lo, hi = pv.amin(dim=0), pv.amax(dim=0)
        out["live"] = not bool((lo == hi).all())
    if out["live"]:
        c = _t(0.5) * (lo + hi)
        half = (_t(0.5) * (hi - lo)).amax()
        inv = _t(float(R - 1 - 2 * (s + 3))) / (_t(2.0) * half)
        q = (pv - c) * inv + _t((R - 1) / 2)
        keep = ((q >= 0) & (q <= R - 1)).all(dim=1)
        q, nv = q[keep], nv[keep]
        base = torch.floor(q).long()
        s2 = _t(float(s * s))
        rnd = torch.trunc if mutant == "truncate" else torch.round   # torch.round: half to even
        for o in itertools.product(range(-s + 1, s + 1), repeat=3):
            g = base + torch.tensor(o)
            inside = ((g >= 0) & (g <= R - 1)).all(dim=1)
            d = g.float() - q
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            t = s2 - ((dx * dx + dy * dy) + dz * dz)
            w = t / s2
            w3 = (w * w) * w
            hit = inside & (t > 0)
            lin = ((g[:, 0] * R + g[:, 1]) * R + g[:, 2])[hit]
            grids[0].index_add_(0, lin, rnd(w3 * _t(float(FIX)))[hit].long())
            for a in range(3):
                v = rnd((w3 * nv[:, a]) * _t(float(FIX)))
                v = torch.where(torch.isnan(v), torch.zeros_like(v), v.clamp(-float(FIX), float(FIX)))
                grids[1 + a].index_add_(0, lin, v[hit].long())
        out["c"], out["inv"], out["q"] = c, inv, q
    n = points.shape[0]
    assert n * FIX < 2 ** 31 and 6 * n * FIX < 2 ** 31                      # the header's bound, in Python integers
    assert all(int(g.abs().max()) <= n * FIX for g in grids)
    V = [g.view(R, R, R) for g in grids[1:]]
    D = torch.zeros(R, R, R, dtype=torch.int64)
    for a in range(3):
        pad = torch.nn.functional.pad(V[a].movedim(a, 2), (1, 1)).movedim(2, a)   # zero outside the grid
        D += pad.narrow(a, 2, R) - pad.narrow(a, 0, R)
    assert int(D.abs().max()) < 2 ** 31
    out["W"], out["Vx"], out["Vy"], out["Vz"] = (g.view(R, R, R).int() for g in grids)
    out["D"] = D.int()
    return out


# ---- step 4: the solve ------------------------------------------------------------------------------------------------------------------
def _ghosted(x, dim, mutant):
    """x with one ghost layer on both ends of `dim`: minus the edge value (the boundary is on the cell face)."""
    lo, hi = x.narrow(dim, 0, 1), x.narrow(dim, x.shape[dim] - 1, 1)
    if mutant == "ghost_node":
        return torch.cat([torch.zeros_like(lo), x, torch.zeros_like(hi)], dim=dim)
    return torch.cat([-lo, x, -hi], dim=dim)


def _stencil(phi, mutant):
    """(S - 6 phi): S = ((xm + xp) + (ym + yp)) + (zm + zp)."""
    m = phi.shape[0]
    pairs = []
    for dim in range(3):
        g = _ghosted(phi, dim, mutant)
        pairs.append(g.narrow(dim, 0, m) + g.narrow(dim, 2, m))
    return ((pairs[0] + pairs[1]) + pairs[2]) - _t(6.0, phi.dtype) * phi


def sweep(phi, f, h2, mutant=None):
    return phi + ((_stencil(phi, mutant) - _t(h2, phi.dtype) * f) * _t(1.0 / 7.0, torch.float32).to(phi.dtype))


def residual(phi, f, h2, mutant=None):
    return f - _stencil(phi, mutant) * _t(1.0 / h2, phi.dtype)


def restrict(res, mutant=None):
    order = list(itertools.product((0, 1), repeat=3))
    if mutant == "restriction_reversed":
        order = order[::-1]
    total = None
    for a, b, c in order:
        child = res[a::2, b::2, c::2]
        total = child if total is None else total + child
    return total * _t(0.125, res.dtype)


def prolong(e, mutant=None):
    """Trilinear, along z, then y, then x: child 2 K + a takes 0.75 e[K] + 0.25 e[K - 1 + 2 a], ghosts as in the stencil."""
    if mutant == "constant_prolongation":
        return e.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)
    near, far = _t(0.75, e.dtype), _t(0.25, e.dtype)
    for dim in (2, 1, 0):
        m = e.shape[dim]
        g = _ghosted(e, dim, mutant)
        low = near * e + far * g.narrow(dim, 0, m)
        high = near * e + far * g.narrow(dim, 2, m)
        shape = list(e.shape)
        shape[dim] = 2 * m
        e = torch.stack([low, high], dim=dim + 1).reshape(shape)
    return e


def _vcycle(phi, f, level, last, mutant):
    h2 = float(4 ** level)
    if level == last:
        phi = torch.zeros_like(f)
        for _ in range(COARSEST - 1 if mutant == "coarsest_one_fewer" else COARSEST):
            phi = sweep(phi, f, h2, mutant)
        return phi
    if phi is None:
        phi = torch.zeros_like(f)
    for _ in range(PRE):
        phi = sweep(phi, f, h2, mutant)
    e = _vcycle(None, restrict(residual(phi, f, h2, mutant), mutant), level + 1, last, mutant)
    phi = phi + prolong(e, mutant)
    for _ in range(POST):
        phi = sweep(phi, f, h2, mutant)
    return phi


def solve(D, cycles, mutant=None, dtype=torch.float32, history=None):
    """phi after `cycles` V-cycles from zero; history, a list, receives the residual's 2-norm over the right-hand side's per cycle."""
    f = D.to(dtype)
    R = f.shape[0]
    last = len(sides(R)) - 1
    phi = torch.zeros_like(f)
    for _ in range(cycles):
        phi = _vcycle(phi, f, 0, last, mutant)
        if history is not None:
            history.append(float(residual(phi.double(), f.double(), 1.0).norm() / f.double().norm().clamp_min(1e-300)))
    return phi


# ---- steps 5 - 7: level, hand-over, density ---------------------------------------------------------------------------------------------
def _lerp(a, b, t):
    return a + t * (b - a)


def sample(phi, q, mutant=None):
    """phi at the grid coordinates q (m, 3), trilinear along z, then y, then x."""
    R = phi.shape[0]
    if mutant == "iso_nearest":
        g = torch.round(q).long().clamp(0, R - 1)
        return phi[g[:, 0], g[:, 1], g[:, 2]]
    base = torch.floor(q).long().clamp(max=R - 2)
    t = q - base.float()
    i, j, k = base[:, 0], base[:, 1], base[:, 2]
    cx = []
    for dx in (0, 1):
        cy = [_lerp(phi[i + dx, j + dy, k], phi[i + dx, j + dy, k + 1], t[:, 2]) for dy in (0, 1)]
        cx.append(_lerp(cy[0], cy[1], t[:, 1]))
    return _lerp(cx[0], cx[1], t[:, 0])


def level_of(phi, q, mutant=None):
    """-> (iso, scale) float32 tensors; (0, 0) when there is nothing to cut."""
    M = phi.abs().max()
    if q.shape[0] == 0 or float(M) == 0.0:
        return _t(0.0), _t(0.0)
    scale = _t(float(2 ** 22)) / M
    qs = scale * _t(256.0)
    total = int(torch.round(sample(phi, q, mutant) * qs).long().sum())
    assert abs(total) < 2 ** 62
    iso = (torch.tensor(total, dtype=torch.int64).float() / _t(float(q.shape[0]))) / qs
    return iso, scale


def checkerboards(SU):
    """-> (mask of the negative nodes that lie on a grid face whose two diagonals differ in sign: this node and the one across the face
    negative, the two others not; the number of such faces)."""
    R = SU.shape[0]
    neg = SU < 0
    hit, faces = torch.zeros(R, R, R, dtype=torch.bool), 0
    for u, v in ((0, 1), (0, 2), (1, 2)):
        sl = lambda du, dv: tuple(slice(d, R - 1 + d) if ax in (u, v) else slice(None) for ax, d in ((0, du if u == 0 else 0),
                                  (1, du if u == 1 else (dv if v == 1 else 0)), (2, dv if v == 2 else 0)))
        n00, n10, n01, n11 = neg[sl(0, 0)], neg[sl(1, 0)], neg[sl(0, 1)], neg[sl(1, 1)]
        a, b = n00 & n11 & ~n10 & ~n01, n10 & n01 & ~n00 & ~n11
        faces += int(a.sum()) + int(b.sum())
        hit[sl(0, 0)] |= a
        hit[sl(1, 1)] |= a
        hit[sl(1, 0)] |= b
        hit[sl(0, 1)] |= b
    return hit, faces


def separate(SU, passes=SEPARATE_PASSES):
    """`passes` times: every node of `checkerboards`, judged on the grid before the pass, becomes 1.  -> (SU, checkerboard faces left)."""
    for _ in range(passes):
        hit, _ = checkerboards(SU)
        SU = torch.where(hit, torch.ones_like(SU), SU)
    return SU, checkerboards(SU)[1]


def hand_over(phi, iso, scale, mutant=None):
    """-> (SW, SU, border_raised)."""
    R = phi.shape[0]
    if float(scale) == 0.0:
        return torch.zeros(R, R, R, dtype=torch.int32), torch.zeros(R, R, R, dtype=torch.int32), 0
    SU = torch.round((phi - iso) * scale).clamp(-float(SU_LIMIT), float(SU_LIMIT)).int()
    border = torch.ones(R, R, R, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    low = border & (SU < 1)
    raised = int(low.sum())
    if mutant != "border_kept":
        SU = torch.where(low, torch.ones_like(SU), SU)
    if mutant != "checkerboards_kept":
        SU = separate(SU)[0]
    return torch.full((R, R, R), FIX, dtype=torch.int32), SU, raised


def active_cells(SW, SU):
    """Ascending linear indices (i R + j) R + k of the active cells: the order of the vertices."""
    R = SU.shape[0]
    m = R - 1
    neg, defined = SU < 0, SW >= 1
    n_neg, all_def = torch.zeros(m, m, m, dtype=torch.int64), torch.ones(m, m, m, dtype=torch.bool)
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        n_neg += neg[dx:dx + m, dy:dy + m, dz:dz + m]
        all_def &= defined[dx:dx + m, dy:dy + m, dz:dz + m]
    active = torch.zeros(R, R, R, dtype=torch.bool)
    active[:m, :m, :m] = all_def & (n_neg >= 1) & (n_neg <= 7)
    return torch.nonzero(active.flatten())[:, 0]


def density_of(W, SW, SU):
    R = W.shape[0]
    m = R - 1
    total = torch.zeros(R, R, R, dtype=torch.int64)
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        total[:m, :m, :m] += W[dx:dx + m, dy:dy + m, dz:dz + m]
    return total.flatten()[active_cells(SW, SU)].float() * _t(1.0 / (8 * FIX))


def mesh_from_field(phi, splat, R, mutant=None, iso_scale=None):
    """Steps 5 - 7 on a given field (the forced-border test hands in its own)."""
    iso, scale = level_of(phi, splat["q"], mutant) if iso_scale is None else iso_scale
    SW, SU, raised = hand_over(phi, iso, scale, mutant)
    grid = {"SW": SW, "SU": SU, "inv": splat["inv"], "c": splat["c"]}
    mesh = S.mesh_of(grid, R, 1)
    return {"phi": phi, "iso": iso, "scale": scale, "SW": SW, "SU": SU, "border_raised": raised, "verts": mesh["verts"], "faces": mesh["faces"],
            "density": density_of(splat["W"], SW, SU), "counts": [mesh["verts"].shape[0], mesh["faces"].shape[0], mesh["skipped"], splat["valid"]]}


def reconstruct(points, normals, R, s, cycles=DEFAULT_CYCLES, mutant=None):
    """One cloud -> dict(W, Vx, Vy, Vz, D, phi, iso, scale, SW, SU, border_raised, counts [V, F, skipped, valid], verts, faces, density)."""
    if not accepted(R):
        raise ValueError(f"resolution={R} is not accepted; the nearest is {nearest_accepted(R)}")
    splat = splat_of(points, normals, R, s, mutant)
    phi = solve(splat["D"], cycles, mutant) if splat["live"] else torch.zeros(R, R, R)
    out = mesh_from_field(phi, splat, R, mutant)
    out.update({k: splat[k] for k in ("W", "Vx", "Vy", "Vz", "D")})
    return out


def reconstruct_batch(points, normals, R, s, cycles=DEFAULT_CYCLES, mutant=None):
    return [reconstruct(p, n, R, s, cycles, mutant) for p, n in zip(points, normals)]


KEYS_INT = ("W", "Vx", "Vy", "Vz", "D", "SW", "SU", "faces")
KEYS_BITS = ("phi", "iso", "scale", "verts", "density")


def differences(a, b):
    """The names of the outputs on which two results differ (floats compared as bits)."""
    out = [k for k in KEYS_INT if not torch.equal(a[k], b[k])]
    out += [k for k in KEYS_BITS if not torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32))]
    if list(a["counts"]) != list(b["counts"]):
        out.append("counts")
    if a["border_raised"] != b["border_raised"]:
        out.append("border_raised")
    return out


# ---- the clouds of the closure table and the GPU case table -------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


CLOSURE = {"sphere_512_R32_s2": (lambda: S.sphere(_gen(3300), 512), 32, 2), "sphere_600_R32_s2": (lambda: S.sphere(_gen(3301), 600), 32, 2),
           "sphere_1024_R32_s3": (lambda: S.sphere(_gen(3302), 1024), 32, 3), "torus_1500_R32_s3": (lambda: S.torus(_gen(3201), 1500), 32, 3),
           "torus_1500_R48_s2": (lambda: S.torus(_gen(3201), 1500), 48, 2), "sphere_4096_R64_s3": (lambda: S.sphere(_gen(3303), 4096), 64, 3)}


@functools.lru_cache(maxsize=None)
def closure_inputs(name):
    make, R, s = CLOSURE[name]
    return (*make(), R, s)


def _one(cloud):
    return cloud[0][None], cloud[1][None]


def _case_ellipsoids():
    pts, nrm, _, _, _ = S.case_inputs("b3_n1025_ellipsoids_R32_s3")
    return pts, nrm, 32, 3, 4


def _case_nonfinite():
    pts, nrm, _, _, _ = S.case_inputs("b2_n300_nonfinite_R16_s3")
    return pts, nrm, 16, 3, 2


# name -> (points (b, n, 3), normals (b, n, 3), R, s, cycles)
CASES = {"b1_n65_R16_s2_c3": lambda: (*_one(S.sphere(_gen(3200), 65)), 16, 2, 3),
         "b1_n257_R24_s2_c3": lambda: (*_one(S.sphere(_gen(3304), 257)), 24, 2, 3),
         "b3_n1025_ellipsoids_R32_s3_c4": _case_ellipsoids,
         "b2_n300_nonfinite_R16_s3_c2": _case_nonfinite,
         "b1_n40_all_equal_R16_s2_c1": lambda: (*S.case_inputs("b1_n40_all_equal")[:2], 16, 2, 1),
         "lattice_plane_R32_s3_c4": lambda: (*_one(S.lattice_plane(32)), 32, 3, 4),
         "sphere_512_R32_s2_default": lambda: (*_one(closure_inputs("sphere_512_R32_s2")[:2]), 32, 2, DEFAULT_CYCLES),
         "torus_R48_s2_c3": lambda: (*_one(S.torus(_gen(3201), 1500)), 48, 2, 3),
         "torus_R48_s3_c3": lambda: (*_one(S.torus(_gen(3201), 1500)), 48, 3, 3),
         "torus_R48_s4_c3": lambda: (*_one(S.torus(_gen(3201), 1500)), 48, 4, 3),
         "torus_R40_s3_c3": lambda: (*_one(S.torus(_gen(3201), 1500)), 40, 3, 3),
         "sphere_4096_R64_s3_default": lambda: (*_one(closure_inputs("sphere_4096_R64_s3")[:2]), 64, 3, DEFAULT_CYCLES)}
LARGE_CASE = ("b1_n16384_torus_R128_s4_c2", lambda: (*_one(S.torus(_gen(3204), 16384)), 128, 4, 2))
# the input of the GPU table on which each mutant is asserted to change an output (tests/test_surface_poisson_host.py)
MUTANT_CASES = {"ghost_node": "b1_n65_R16_s2_c3", "constant_prolongation": "b1_n257_R24_s2_c3", "restriction_reversed": "torus_R40_s3_c3",
                "truncate": "b2_n300_nonfinite_R16_s3_c2", "border_kept": "lattice_plane_R32_s3_c4", "iso_nearest": "b1_n65_R16_s2_c3",
                "coarsest_one_fewer": "torus_R48_s2_c3", "checkerboards_kept": "torus_R48_s3_c3"}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_ref(name, mutant=None):
    pts, nrm, R, s, cycles = case_inputs(name)
    return reconstruct_batch(pts, nrm, R, s, cycles, mutant)
