"""The ray rule of include/bdm_hip.h section 24 on the CPU alone (tests/mesh_raycast_ref.py): the walk over the tree equals the
exhaustive loop on every case of the GPU table (the pruning theorem of DESIGN.md section 28), every named mutant changes an output
on that table, the tree's invariants hold, the argument checks of bdm_amd/mesh_raycast.py raise before anything is launched, and
camera_rays agrees with the rasteriser's restatement.  No GPU is needed."""
import functools

import numpy as np
import pytest
import torch

import mesh_raycast_ref as R
import mesh_render_ref as RR
import mesh_voxel_ref as VR


@functools.lru_cache(maxsize=None)
def _walked():
    return tuple(R.tree_cast(v, f, rays, tree=tree) for (_, v, f, rays), tree in zip(R.batch(), R.trees()))


def test_the_table_holds_what_the_issue_lists():
    rows = R.batch()
    names = [n for n, *_ in rows]
    assert [f.shape[0] for _, _, f, _ in rows][:6] == [0, 1, 2, 3, 64, 65] and names[len(names) // 2 - 1] == "empty"
    assert {0, 1, 65} <= {rays.shape[0] for *_, rays in rows}
    refs = R.references()
    total = np.sum([r["counts"] for r in refs], axis=0)
    assert total[1] >= 20 and total[2] > 1000 and total[4] == 5                 # invalid rays, rays that hit, dropped faces
    assert max(int(r["crossings"].max()) for r, (*_, rays) in zip(refs, rows) if rays.shape[0]) >= 7   # a ray through a vertex of six faces
    lat = refs[names.index("lattice_box")]
    rays = rows[names.index("lattice_box")][3]
    pinned = (rays[:, 6] == rays[:, 7]) & np.isfinite(rays[:, 6])
    assert (lat["face"][pinned] >= 0).sum() > 50 and (lat["face"][pinned] < 0).sum() > 50   # tmin == tmax on a hit and off it
    assert np.isinf(rays[:, 7]).sum() > 100 and (lat["back"] == 1).sum() > 10   # tmax = inf; origins inside hit backs


def test_the_walk_equals_the_exhaustive_loop_on_every_case():
    for (name, *_), ref, got in zip(R.batch(), R.references(), _walked()):
        assert R.same(ref, got), name


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_an_output_of_the_table(mutant):
    changed = []
    for (name, v, f, rays), ref, tree in zip(R.batch(), R.references(), R.trees()):
        if f.shape[0] > 100:
            continue   # the small meshes tell every mutant apart
        got = R.tree_cast(v, f, rays, mutant=mutant, tree=tree) if mutant == "prune_ge" else R.exhaustive(v, f, rays, mutant=mutant)
        if not R.same(ref, got):
            changed.append(name)
    assert changed, mutant
    expected = {"no_f64": "sliver_edge", "no_interval": "wide_flat", "prune_ge": "lattice_box", "highest_on_ties": "eight_copies", "unwidened": "box"}
    assert expected[mutant] in changed


def test_the_trees_keep_their_invariants_and_every_walk_ends_within_the_cap():
    for (name, v, f, _), tree, got in zip(R.batch(), R.trees(), _walked()):
        depth = R.check_tree(tree, v, f)
        n = tree["n"]
        assert got["steps"] <= max(2 * n - 1, 0), name                           # walk() asserts the cap of 2 n itself
        assert depth <= 2 * max(int(np.ceil(np.log2(max(n, 1)))), 1) + 2, (name, depth, n)
    eight = R.trees()[[n for n, *_ in R.batch()].index("eight_copies")]
    assert eight["n"] == 8 and R.check_tree(eight, *R.hand_meshes()["eight_copies"]) == 4   # all keys equal: split by position


def test_a_closed_mesh_does_not_leak():
    """Random rays from outside a closed mesh cross an even number of faces, the interval condition changes no answer, and a ray from
    inside a star-shaped mesh always hits: the widened face interval rejects no hit that the edge functions accept."""
    for name in ("uv_sphere", "surface", "octahedron"):
        v, f = R.hand_meshes()[name]
        rays = R.random_rays(v, 200, 7)
        rays[:, 6], rays[:, 7] = 0.0, np.inf
        out = R.exhaustive(v, f, rays)
        no_interval = R.exhaustive(v, f, rays, mutant="no_interval")
        assert R.same(out, no_interval), name                                    # the interval changes nothing on a generic mesh
        vn = np.asarray(v.numpy(), dtype=np.float64)
        c, half = (vn.min(axis=0) + vn.max(axis=0)) / 2, np.linalg.norm(vn.max(axis=0) - vn.min(axis=0)) / 2
        outside = np.linalg.norm(rays[:, 0:3] - c, axis=1) > 1.5 * half          # the shell of random_rays, not its inner fifth
        assert outside.sum() > 100 and (out["crossings"][outside] % 2 == 0).all() and (out["crossings"][outside] > 0).sum() > 50, name
        if name != "surface":                                                    # the torus is not star-shaped: its centre is in the hole
            inside = R._rays(np.broadcast_to(vn.mean(axis=0), (200, 3)), rays[:, 3:6])
            assert (R.exhaustive(v, f, inside)["face"] >= 0).all(), name


# ---- the Python surface: argument checks ----------------------------------------------------------------------------------------------
def test_malformed_arguments_raise_before_anything_is_launched():
    from bdm_amd import mesh_raycast as MR
    from bdm_amd.cameras import PerspectiveCameras
    v, f = VR.octahedron()
    meshes = ([v], [f])
    o, d = [torch.zeros(4, 3)], [torch.ones(4, 3)]
    for fn in (MR.cast_rays, MR.test_occlusions, MR.count_intersections):
        with pytest.raises(ValueError):
            fn(([v], [f.float()]), o, d)
        with pytest.raises(ValueError):
            fn(([], []), [], [])
        with pytest.raises(ValueError):
            fn(meshes, o + o, d + d)
        with pytest.raises(ValueError):
            fn(meshes, [torch.zeros(4, 2)], d)
        with pytest.raises(ValueError):
            fn(meshes, o, [torch.ones(5, 3)])
        with pytest.raises(ValueError):
            fn(meshes, torch.zeros(2, 4, 3), torch.zeros(2, 4, 3))
        with pytest.raises(ValueError):
            fn(meshes, o, torch.ones(1, 4, 3))
        with pytest.raises(TypeError):
            fn(meshes, "rays", d)
        with pytest.raises(TypeError):
            fn(meshes, [np.zeros((4, 3))], d)
        with pytest.raises(TypeError):
            fn(meshes, [torch.zeros(4, 3, dtype=torch.int64)], [torch.ones(4, 3, dtype=torch.int64)])
        with pytest.raises(ValueError):
            fn(meshes, o, d, tmin=2.0, tmax=1.0)
        with pytest.raises(ValueError):
            fn(meshes, o, d, tmin=float("nan"))
        with pytest.raises(ValueError):
            fn(meshes, o, d, tmax=[torch.zeros(3)])
        for kw in (dict(tmin=float("nan"), tmax=[torch.ones(4)]), dict(tmin=[torch.zeros(4)], tmax=float("nan")), dict(tmin=float("-inf")),
                   dict(tmin=float("inf"), tmax=[torch.ones(4)]), dict(tmin=[torch.zeros(4)], tmax=float("-inf"))):
            with pytest.raises(ValueError):   # a scalar bound is judged on its own
                fn(meshes, o, d, **kw)
        with pytest.raises(TypeError):
            fn(meshes, o, d, tmin="0")
        with pytest.raises(TypeError):
            fn(meshes, o, d, exhaustive=1)
        with pytest.raises(RuntimeError):   # well-formed host tensors: refused, there is no CPU path
            fn(meshes, o, d)
    with pytest.raises(ValueError):
        MR.build_bvh("mesh")
    with pytest.raises(ValueError):
        MR.build_bvh(([], []))
    cams = PerspectiveCameras()
    with pytest.raises(TypeError):
        MR.camera_rays("camera", 8)
    with pytest.raises(TypeError):
        MR.camera_rays(cams, 8.0)
    with pytest.raises(ValueError):
        MR.camera_rays(cams, (0, 8))
    for kw in (dict(), dict(eyes=torch.zeros(1, 3), directions=torch.zeros(1, 3))):
        with pytest.raises(ValueError):
            MR.points_visible(meshes, [v], **kw)
    with pytest.raises(ValueError):
        MR.points_visible(meshes, [v, v], eyes=torch.zeros(1, 3))
    with pytest.raises(ValueError):
        MR.points_visible(meshes, [v], eyes=torch.zeros(2, 3))
    with pytest.raises(TypeError):
        MR.points_visible(meshes, [v], eyes=[[0, 0, 0]])
    with pytest.raises(ValueError):
        MR.points_visible(meshes, [v[:, :2]], eyes=torch.zeros(1, 3))
    with pytest.raises(ValueError):
        MR.points_visible(meshes, [v], eyes=torch.zeros(1, 3), offset=-1.0)
    for kw in (dict(num_samples=0), dict(num_samples=2.5), dict(max_distance=0.0), dict(max_distance=-1), dict(directions=torch.zeros(4, 2)),
               dict(directions=torch.full((4, 3), float("nan"))), dict(offset=float("inf"))):
        with pytest.raises(ValueError):
            MR.vertex_ambient_occlusion(meshes, **kw)
    with pytest.raises(TypeError):
        MR.vertex_ambient_occlusion(meshes, directions=[[0, 0, 1]])
    assert torch.equal(MR.fibonacci_sphere(32), torch.from_numpy(R.fibonacci_sphere(32)))
    assert float((MR.fibonacci_sphere(32).double().norm(dim=1) - 1).abs().max()) < 1e-6


# ---- camera rays against the rasteriser's restatement ------------------------------------------------------------------------------------
def _near_an_edge(verts, faces, cam, H, W, ortho, units=1.0):
    """(H, W) bool: the pixel centre lies within `units` / 256 of a pixel of a projected (snapped) edge of a face, inside or outside it."""
    SX, SY, zv, usable = RR.project(verts, cam, H, W, ortho)
    assert bool(usable.all())
    X, Y = SX[faces].double(), SY[faces].double()                               # (F, 3)
    px = (RR.SNAP * torch.arange(W) + RR.SNAP // 2).double()[None, None, :]
    py = (RR.SNAP * torch.arange(H) + RR.SNAP // 2).double()[None, :, None]
    near = torch.zeros(H, W, dtype=torch.bool)
    dist = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        ax, ay, bx, by = X[:, a, None, None], Y[:, a, None, None], X[:, b, None, None], Y[:, b, None, None]
        length = ((bx - ax) ** 2 + (by - ay) ** 2).sqrt().clamp_min(1e-9)
        dist.append(((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / length)  # signed distance to the edge's line
    d = torch.stack(dist)                                                      # (3, F, H, W)
    sign = torch.sign(d.sum(dim=0).sum(dim=(1, 2), keepdim=True))               # the face's winding on screen
    d = d * sign
    inside_ish = (d >= -units).all(dim=0)                                       # within the face grown by `units`
    on_rim = inside_ish & (d.abs() <= units).any(dim=0)
    return on_rim.any(dim=0)


def test_camera_rays_name_the_faces_the_rasteriser_names():
    """uv_sphere under the perspective camera of the render tests (r2n2_camera(30, 27, 1.4)) at 48 x 48: the closest hit of every pixel
    ray, by the restatement, names the face of mesh_render_ref.render at every pixel whose centre is not within the snapping distance
    (1 / 256 of a pixel) of a projected edge of any face, front or back; those left out are at most 5 % of the covered pixels.  The
    same under the orthographic camera of the render tests at 64 x 64 (at 48 x 48 that camera leaves out 6.1 %: more edges per pixel)."""
    from bdm_amd import mesh_raycast as MR
    v, f = VR.uv_sphere(24, 48)
    for camera, H, W in ((RR._persp(), 48, 48), (RR._ortho(), 64, 64)):
        ortho = bool(camera.orthographic)
        want = RR.render(v, f, camera.packed()[0], H, W, ortho=ortho)["pix_to_face"]
        o, d = MR.camera_rays(camera, (H, W))
        assert o.shape == (1, H * W, 3) and d.dtype == torch.float32
        got = R.exhaustive(v, f, R._rays(o[0].numpy(), d[0].numpy()))
        face = torch.from_numpy(got["face"]).view(H, W)
        skip = _near_an_edge(v, f, camera.packed()[0], H, W, ortho)
        covered = want >= 0
        assert int(covered.sum()) > 300
        share = float((skip & covered).sum()) / float(covered.sum())
        print(f"ortho={ortho}: {int(covered.sum())} covered pixels, {share:.2%} within the snapping distance of an edge")
        assert share <= 0.05
        assert torch.equal(face[~skip], want[~skip]), f"ortho={ortho}: {int((face != want)[~skip].sum())} pixels differ"


def test_the_unasserted_band_of_points_visible_is_below_thirty_percent_and_the_rest_holds():
    """The vertices of uv_sphere seen from an eye at five radii: those with n . u >= 0.2 are visible, those with n . u <= -0.2 hidden
    (u the unit vector to the eye), by the restatement; the band in between holds at most 30 % of the vertices."""
    from bdm_amd.cameras import Meshes
    v, f = VR.uv_sphere(24, 48)
    centre, radius = torch.tensor([0.013, -0.021, 0.034]), 0.4
    eye = centre + 5 * radius * torch.tensor([0.6, 0.48, 0.64])
    n = Meshes([v], [f]).verts_normals_packed()
    to_eye = eye[None] - v
    u = to_eye / to_eye.norm(dim=1, keepdim=True)
    c = (n * u).sum(dim=1)
    band = (c.abs() < 0.2)
    assert float(band.sum()) / v.shape[0] <= 0.30
    diag = float((v.max(dim=0).values - v.min(dim=0).values).norm())
    o = v + (1e-4 * diag) * u
    hidden = torch.from_numpy(R.exhaustive(v, f, R._rays(o.numpy(), (eye[None] - o).numpy(), 0.0, 1.0))["occluded"]).bool()
    assert not bool(hidden[c >= 0.2].any()) and bool(hidden[c <= -0.2].all())
    assert int((c >= 0.2).sum()) > 300 and int((c <= -0.2).sum()) > 300
