"""TEST INFRASTRUCTURE: CPU restatement of the mesh renderer (bdm_amd/csrc/mesh_render.hip; the rule is the text of
include/bdm_hip.h section 13), the inputs its tests share and the GPU case table.

Brute force over every face's bounding box, taken one pixel WIDER than the face on every side (so the box arithmetic of the kernel is
not restated): all (face, pixel) pairs of a mesh are laid out in one long vector and everything is elementwise on it -- torch int64
for the coverage, float32 for the rest, one rounding per operation (CPU torch neither fuses nor reorders elementwise operations;
its float32 division is correctly rounded, its int64 -> float32 conversion rounds to nearest even).  The winner of a pixel is the
minimum of (bits of z) << 32 | face index, by scatter_reduce.  `render` also returns the number of covering fragments per pixel.

MUTANTS are deliberate misreadings of the rule; tests/test_mesh_render_host.py asserts that each changes an output on at least one
input of the GPU case table, so that the equalities of tests/test_hip_mesh_render.py are not vacuous."""
import functools
import math

import torch

MUTANTS = ("own_never", "own_always", "tie_high_index", "no_swap_back", "screen_linear_z", "truncate", "centre_at_corner", "cull_reversed")
SNAP, GUARD = 256, float(2 ** 22)
EMPTY_KEY = torch.iinfo(torch.int64).max


def project(verts, cam, H, W, ortho, mutant=None):
    """SX, SY (int64), zv (float32), usable (bool) per vertex."""
    verts, c = verts.float(), cam.float()
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    xv = x * c[0] + y * c[3] + z * c[6] + c[9]
    yv = x * c[1] + y * c[4] + z * c[7] + c[10]
    zv = x * c[2] + y * c[5] + z * c[8] + c[11]
    if ortho:
        u, v = c[12] * xv + c[14], c[13] * yv + c[15]
    else:
        u, v = c[12] * xv / zv + c[14], c[13] * yv / zv + c[15]
    px = ((1.0 - u) * torch.tensor(0.5 * W, dtype=torch.float32)) * float(SNAP)
    py = ((1.0 - v) * torch.tensor(0.5 * H, dtype=torch.float32)) * float(SNAP)
    assert px.dtype == torch.float32 and zv.dtype == torch.float32
    usable = torch.isfinite(zv) & (zv > 0) & (px.abs() <= GUARD) & (py.abs() <= GUARD)
    snap = torch.trunc if mutant == "truncate" else torch.round        # torch.round rounds half to even
    zero = torch.zeros_like(px)
    return snap(torch.where(usable, px, zero)).long(), snap(torch.where(usable, py, zero)).long(), zv, usable


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(dx, dy, mutant):
    if mutant == "own_never":
        return torch.zeros_like(dx, dtype=torch.bool)
    if mutant == "own_always":
        return torch.ones_like(dx, dtype=torch.bool)
    return (dy > 0) | ((dy == 0) & (dx > 0))


def render(verts, faces, cam, H, W, ortho=False, cull=False, vert_features=None, face_features=None, background=None, mutant=None):
    """One mesh -> {"pix_to_face" (H, W) int32, "zbuf" (H, W), "bary" (H, W, 3), "count" (H, W) int64 fragments per pixel,
    "image" (H, W, C) or None (made iff background is given)}."""
    assert mutant is None or mutant in MUTANTS
    assert vert_features is None or face_features is None
    V, F = verts.shape[0], faces.shape[0]
    pix_to_face = torch.full((H * W,), -1, dtype=torch.int32)
    zbuf = torch.full((H * W,), -1.0)
    bary = torch.full((H * W, 3), -1.0)
    count = torch.zeros(H * W, dtype=torch.int64)
    won = torch.zeros(0, dtype=torch.int64)
    if V and F:
        SX, SY, zv, usable = project(verts, cam, H, W, ortho, mutant)
        faces = faces.long()
        in_range = ((faces >= 0) & (faces < V)).all(1)
        fc = faces.clamp(0, V - 1)
        live = in_range & usable[fc].all(1)
        X, Y, Z = SX[fc], SY[fc], zv[fc]                                       # (F, 3)
        A = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
        live &= A != 0
        if cull:
            live &= (A > 0) if mutant == "cull_reversed" else (A < 0)
        swapped = A < 0
        order = torch.where(swapped[:, None], torch.tensor([[0, 2, 1]]), torch.tensor([[0, 1, 2]]))
        X, Y, Z, A = X.gather(1, order), Y.gather(1, order), Z.gather(1, order), A.abs()
        # one pixel wider than the face on every side, clamped to the image
        xa = (torch.div(X.min(1).values, SNAP, rounding_mode="floor") - 1).clamp(0, W - 1)
        xb = (torch.div(X.max(1).values, SNAP, rounding_mode="floor") + 1).clamp(0, W - 1)
        ya = (torch.div(Y.min(1).values, SNAP, rounding_mode="floor") - 1).clamp(0, H - 1)
        yb = (torch.div(Y.max(1).values, SNAP, rounding_mode="floor") + 1).clamp(0, H - 1)
        live &= (X.max(1).values >= -SNAP) & (X.min(1).values <= SNAP * (W + 1)) & (Y.max(1).values >= -SNAP) & (Y.min(1).values <= SNAP * (H + 1))
        ids = torch.nonzero(live)[:, 0]
        bw = (xb - xa + 1)[ids]
        sizes = bw * (yb - ya + 1)[ids]
        start = torch.cumsum(sizes, 0) - sizes
        slot = torch.repeat_interleave(torch.arange(ids.numel()), sizes)
        local = torch.arange(int(sizes.sum())) - start[slot]
        f = ids[slot]
        xi, yi = xa[f] + local % bw[slot], ya[f] + torch.div(local, bw[slot], rounding_mode="floor")
        half = 0 if mutant == "centre_at_corner" else SNAP // 2
        px, py = SNAP * xi + half, SNAP * yi + half
        x0, x1, x2, y0, y1, y2 = X[f, 0], X[f, 1], X[f, 2], Y[f, 0], Y[f, 1], Y[f, 2]
        E = [_edge(x1, y1, x2, y2, px, py), _edge(x2, y2, x0, y0, px, py), _edge(x0, y0, x1, y1, px, py)]
        own = [_owns(x2 - x1, y2 - y1, mutant), _owns(x0 - x2, y0 - y2, mutant), _owns(x1 - x0, y1 - y0, mutant)]
        covered = torch.ones_like(f, dtype=torch.bool)
        for e, o in zip(E, own):
            covered &= (e > 0) | ((e == 0) & o)
        area = A[f].to(torch.float32)
        w = [e.to(torch.float32) / area for e in E]
        zf = [Z[f, 0], Z[f, 1], Z[f, 2]]
        if ortho or mutant == "screen_linear_z":
            z = w[0] * zf[0] + w[1] * zf[1] + w[2] * zf[2]
            bc = w
        else:
            t = [w[i] / zf[i] for i in range(3)]
            s = t[0] + t[1] + t[2]
            z = 1.0 / s
            bc = [t[i] / s for i in range(3)]
        assert z.dtype == torch.float32
        keep = covered & torch.isfinite(z) & (z > 0)
        f, xi, yi, z, bc = f[keep], xi[keep], yi[keep], z[keep], [b[keep] for b in bc]
        pix = yi * W + xi
        count = torch.bincount(pix, minlength=H * W)
        low = (F - 1 - f) if mutant == "tie_high_index" else f
        key = (z.view(torch.int32).long() << 32) | low
        best = torch.full((H * W,), EMPTY_KEY, dtype=torch.int64).scatter_reduce(0, pix, key, "amin", include_self=True)
        win = key == best[pix]                                                 # one fragment per (face, pixel): the winner is unique
        f, pix, z, bc = f[win], pix[win], z[win], [b[win] for b in bc]
        assert pix.unique().numel() == pix.numel()
        if mutant != "no_swap_back":
            sw = swapped[f]
            bc = [bc[0], torch.where(sw, bc[2], bc[1]), torch.where(sw, bc[1], bc[2])]
        pix_to_face[pix] = f.int()
        zbuf[pix] = z
        bary[pix] = torch.stack(bc, 1)
        won = pix
    out = {"pix_to_face": pix_to_face.view(H, W), "zbuf": zbuf.view(H, W), "bary": bary.view(H, W, 3), "count": count.view(H, W), "image": None}
    if background is not None:
        bg = torch.as_tensor(background, dtype=torch.float32).reshape(-1)
        image = bg.expand(H * W, -1).clone()
        if won.numel():
            fw = pix_to_face[won].long()
            if vert_features is not None:
                b, ft = bary[won], vert_features.float()[faces[fw]]            # (n, 3), (n, 3, C): the face's own vertex order
                image[won] = b[:, 0:1] * ft[:, 0] + b[:, 1:2] * ft[:, 1] + b[:, 2:3] * ft[:, 2]
            elif face_features is not None:
                image[won] = face_features.float()[fw]
            else:
                image[won] = 0.0
        out["image"] = image.view(H, W, -1)
    return out


def render_batch(verts_list, faces_list, cams, H, W, ortho=False, cull=False, vert_features=None, face_features=None, background=None,
                 mutant=None):
    """A batch, mesh by mesh -> the dict of `render` with a leading batch axis; the packed feature arrays are split per mesh."""
    nv, nf = [v.shape[0] for v in verts_list], [f.shape[0] for f in faces_list]
    vf = [None] * len(nv) if vert_features is None else torch.split(vert_features, nv)
    ff = [None] * len(nf) if face_features is None else torch.split(face_features, nf)
    outs = [render(v, f, c, H, W, ortho, cull, a, b, background, mutant) for v, f, c, a, b in zip(verts_list, faces_list, cams, vf, ff)]
    return {k: (None if outs[0][k] is None else torch.stack([o[k] for o in outs])) for k in outs[0]}


def same(a, b, keys=("pix_to_face", "zbuf", "bary", "image")):
    """Bit equality of two result dicts (floats compared as int32 patterns)."""
    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(bits(a[k]), bits(b[k]))) for k in keys)


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(level=3, radius=0.4):
    """(verts (V, 3) float32, faces (F, 3) int64), F = 20 * 4^level (1280 at level 3), closed, every face wound outwards."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [tuple(c / math.sqrt(1 + t * t) for c in p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, new = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = [(verts[a][i] + verts[b][i]) / 2 for i in range(3)]
                n = math.sqrt(sum(c * c for c in m))
                verts.append(tuple(c / n for c in m))
                cache[key] = len(verts) - 1
            return cache[key]
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            new += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = new
    V, F = torch.tensor(verts, dtype=torch.float64), torch.tensor(faces, dtype=torch.int64)
    tri = V[F]
    outward = (torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1) * tri.mean(1)).sum(1) > 0
    F = torch.where(outward[:, None], F, F[:, [0, 2, 1]])
    return (V * radius).float(), F


def ortho_pixel_camera():
    """Identity rotation, T = (0, 0, 2), focal 1, orthographic: ndc = world xy, so the world point (1 - (2 i + 1) / W, 1 - (2 j + 1) / H)
    lands exactly on the centre of pixel (j, i) when W and H are powers of two."""
    from bdm_amd.cameras import OrthographicCameras
    return OrthographicCameras(focal_length=1.0, T=torch.tensor([[0.0, 0.0, 2.0]]))


def on_centres(ij, H, W, z=0.0):
    """World points on the centres of the pixels (column i, row j) given as an (n, 2) integer tensor, for ortho_pixel_camera()."""
    ij = torch.as_tensor(ij, dtype=torch.float32)
    return torch.stack([1.0 - (2.0 * ij[:, 0] + 1.0) / W, 1.0 - (2.0 * ij[:, 1] + 1.0) / H, torch.full((ij.shape[0],), float(z))], 1)


def lattice(m=6, step=3, first=1, H=32, W=32, seed=0):
    """An m x m lattice of vertices on pixel centres `step` apart, every cell split along a diagonal that alternates with the cell's
    parity, every face wound at random -> (verts, faces, (first pixel, last pixel) of the lattice)."""
    g = torch.Generator().manual_seed(seed)
    ij = torch.tensor([[first + step * i, first + step * j] for j in range(m) for i in range(m)])
    faces = []
    for j in range(m - 1):
        for i in range(m - 1):
            a, b, c, d = j * m + i, j * m + i + 1, (j + 1) * m + i + 1, (j + 1) * m + i
            faces += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    faces = torch.tensor(faces)
    flip = torch.rand(faces.shape[0], generator=g) < 0.5
    faces = torch.where(flip[:, None], faces[:, [0, 2, 1]], faces)
    return on_centres(ij, H, W), faces, (first, first + step * (m - 1))


def fan(H=16, W=16, seed=1):
    """Eight faces around the centre of pixel (8, 8), rim vertices on pixel centres, wound at random."""
    g = torch.Generator().manual_seed(seed)
    rim = [(13, 8), (12, 12), (8, 13), (4, 12), (3, 8), (4, 4), (8, 3), (12, 4)]
    verts = on_centres(torch.tensor([(8, 8)] + rim), H, W)
    faces = torch.tensor([(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)])
    flip = torch.rand(8, generator=g) < 0.5
    return verts, torch.where(flip[:, None], faces[:, [0, 2, 1]], faces)


def view_to_world(xv, cam):
    R, T = cam[:9].view(3, 3), cam[9:12]
    return (xv - T) @ R.t()


# ---- the GPU case table --------------------------------------------------------------------------------------------------------------
# every case: {"verts": [..], "faces": [..] (int64, local), "cams": packed (B, 16), "camera": the camera object, "ortho", "cull", "H", "W"}
def _persp(n=1, first=0):
    from bdm_amd.cameras import join_cameras, r2n2_camera
    return join_cameras([r2n2_camera(30.0 + 70.0 * (first + i), 27.0 - 9.0 * i, 1.4 + 0.1 * i) for i in range(n)])


def _ortho(n=1, first=0):
    from bdm_amd.cameras import OrthographicCameras, look_at_view_transform
    R, T = look_at_view_transform(dist=10.0, elev=30, azim=[40.0 + 95.0 * (first + i) for i in range(n)])
    return OrthographicCameras(focal_length=1.6, R=R, T=T)


def _case(verts, faces, camera, H, W, cull=False):
    return {"verts": [v.float().contiguous() for v in verts], "faces": [f.long().contiguous() for f in faces], "cams": camera.packed(),
            "camera": camera, "ortho": bool(camera.orthographic), "cull": cull, "H": H, "W": W}


def _one_triangle():
    cam = _persp()
    v = view_to_world(torch.tensor([[0.3, 0.25, 1.2], [-0.35, 0.1, 1.6], [0.05, -0.3, 1.3]]), cam.packed()[0])
    return _case([v], [torch.tensor([[0, 1, 2]])], cam, 16, 16)


def _big_quad():
    """A tilted quad far larger than the 64 x 64 image: both boxes are clamped, both faces take the large-face path."""
    cam = _persp()
    v = view_to_world(torch.tensor([[9.0, 7.0, 2.5], [-8.0, 6.5, 1.5], [-9.0, -7.2, 1.1], [8.5, -8.0, 3.0]]), cam.packed()[0])
    return _case([v], [torch.tensor([[0, 1, 2], [0, 3, 2]])], cam, 64, 64)


def _pile():
    """3000 sub-pixel faces around the centre of ONE pixel, each with vertices of its own at its own depth (one address takes every
    atomic), then 3000 faces that share three vertices (equal depth everywhere: the index decides), 32 x 32, orthographic."""
    cam = ortho_pixel_camera()
    g = torch.Generator().manual_seed(5)
    n = 3000
    centre = on_centres(torch.tensor([[14, 12]]), 32, 32)[0]
    tri = torch.tensor([[0.012, 0.008, 0.0], [-0.011, 0.009, 0.0], [0.001, -0.013, 0.0]])    # a pixel is 1 / 16 wide in these units
    depth = torch.rand(n, generator=g) * 0.5
    small = (centre + tri)[None].repeat(n, 1, 1)
    small[:, :, 2] = depth[:, None] + torch.tensor([0.0, 0.01, 0.02])
    shared = torch.tensor([[0.31, 0.42, 0.9], [-0.23, 0.35, 0.9], [0.04, -0.38, 0.9]])
    verts = torch.cat([small.reshape(-1, 3), shared])
    faces = torch.cat([torch.arange(3 * n).view(n, 3), torch.tensor([[3 * n, 3 * n + 1, 3 * n + 2]]).repeat(n, 1)])
    faces[n + 1::2] = faces[n + 1::2][:, [0, 2, 1]]                       # every other coincident face wound the other way
    return _case([verts], [faces], cam, 32, 32)


def _sphere(H, W, ortho, cull):
    v, f = icosphere(3)
    return _case([v + torch.tensor([0.03, -0.02, 0.01])], [f], _ortho() if ortho else _persp(), H, W, cull)


def _batch3():
    """Three meshes of different sizes under three cameras; the middle one has vertices and no face."""
    v3, f3 = icosphere(3)
    v1, f1 = icosphere(1, 0.3)
    return _case([v3, v1[:7], v1 + torch.tensor([0.1, 0.0, -0.05])], [f3, torch.zeros(0, 3, dtype=torch.int64), f1], _persp(3), 24, 40)


def _degenerate(ortho):
    """An icosphere with vertices made NaN, infinite, behind the camera, in the camera plane and beyond the 2^22 guard, faces with a
    repeated vertex, collinear faces and faces with indices -1, V and 2^30."""
    cam = _ortho() if ortho else _persp()
    v, f = icosphere(2)
    v, f = v.clone(), f.clone()
    g = torch.Generator().manual_seed(11)
    sel = torch.randperm(v.shape[0], generator=g)[:10]
    nan, inf = float("nan"), float("inf")
    v[sel[0]], v[sel[1]], v[sel[2]] = torch.tensor([nan, 0.0, 0.0]), torch.tensor([0.1, inf, 0.0]), torch.tensor([0.0, 0.1, -inf])
    view = torch.tensor([[0.01, 0.02, -1.0], [0.3, -0.2, 0.0], [0.02, 0.01, -1e-3], [3e4, 0.0, 1.0], [0.0, -3e4, 1.0], [1e-3, 1e-3, 1e-30],
                         [1e20, 1e20, 1.0]])
    v[sel[3:]] = view_to_world(view, cam.packed()[0])
    V = v.shape[0]
    extra = torch.tensor([[0, 0, 5], [3, 7, 7], [-1, 2, 3], [1, V, 4], [2, 3, 2 ** 30], [4, 4, 4]])
    line = torch.tensor([[0.2, 0.2, 0.0], [0.0, 0.0, 0.0], [-0.2, -0.2, 0.0]])          # three collinear vertices -> A == 0 when snapped alike
    v = torch.cat([v, line])
    f = torch.cat([f[:100], extra, torch.tensor([[V, V + 1, V + 2]]), f[100:]])
    return _case([v], [f], cam, 32, 32)


def _clipped():
    """Faces partly and wholly outside the image: a sphere pushed over the image's corner, a second one far outside."""
    v, f = icosphere(2, 0.35)
    cam = _persp()
    far = v + view_to_world(torch.tensor([[3.0, 3.0, 0.0]]), cam.packed()[0]) - view_to_world(torch.zeros(1, 3), cam.packed()[0])
    shift = view_to_world(torch.tensor([[0.45, 0.5, 0.0]]), cam.packed()[0]) - view_to_world(torch.zeros(1, 3), cam.packed()[0])
    return _case([torch.cat([v + shift, far])], [torch.cat([f, f + v.shape[0]])], cam, 24, 40)


def _on_centres():
    """The lattice and the fan of the host tests, vertices exactly on pixel centres: centres ON edges and ON shared vertices."""
    (lv, lf, _), (fv, ff) = lattice(), fan(32, 32)
    cam = ortho_pixel_camera()
    from bdm_amd.cameras import join_cameras
    return _case([lv, fv], [lf, ff], join_cameras([cam, cam]), 32, 32)


CASES = {"one_triangle_16": _one_triangle, "on_centres_32": _on_centres,"big_quad_64": _big_quad, "pile_32": _pile, "batch3_24x40": _batch3,
         "degenerate_persp_32": lambda: _degenerate(False), "degenerate_ortho_32": lambda: _degenerate(True), "clipped_24x40": _clipped}
for _H, _W in ((64, 64), (24, 40)):
    for _ortho_flag in (False, True):
        for _cull in (False, True):
            CASES[f"sphere_{_H}x{_W}_{'ortho' if _ortho_flag else 'persp'}_cull{int(_cull)}"] = functools.partial(_sphere, _H, _W, _ortho_flag, _cull)
FEATURE_CASE = "sphere_24x40_persp_cull0"
BACKGROUND = (0.78431373, 0.5, 0.25, 0.125)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_ref(name, mutant=None):
    """The restatement's fragments of a case (no image), computed once and shared."""
    c = case(name)
    return render_batch(c["verts"], c["faces"], c["cams"], c["H"], c["W"], c["ortho"], c["cull"], mutant=mutant)


def case_features(name, channels, per):
    """Packed features in [0, 1] for a case: per = "vert" or "face"."""
    c = case(name)
    rows = sum((v if per == "vert" else f).shape[0] for v, f in zip(c["verts"], c["faces"]))
    return torch.rand(rows, channels, generator=torch.Generator().manual_seed(100 + channels))
