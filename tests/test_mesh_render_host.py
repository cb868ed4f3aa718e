"""The rule of the mesh renderer (include/bdm_hip.h section 13) examined on the CPU restatement tests/mesh_render_ref.py, and the host
side of the feature (Meshes, the argument checks, main_render.render_tree): no GPU."""
import math

import numpy as np
import pytest
import torch

import mesh_render_ref as M


def _frag(verts, faces, cam, H, W, ortho, cull=False, mutant=None):
    return M.render(verts, faces, cam.packed()[0], H, W, ortho, cull, mutant=mutant)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_lattice_on_pixel_centres_covers_every_interior_pixel_once():
    """Vertices ON pixel centres, so centres lie on edges, on both kinds of diagonal and on vertices shared by 4 to 8 faces; the
    faces are wound at random, so both branches of the swap take part."""
    verts, faces, (lo, hi) = M.lattice()
    out = _frag(verts, faces, M.ortho_pixel_camera(), 32, 32, True)
    count = out["count"]
    inside = torch.zeros(32, 32, dtype=torch.bool)
    inside[lo + 1:hi, lo + 1:hi] = True
    outside = torch.ones(32, 32, dtype=torch.bool)
    outside[lo:hi + 1, lo:hi + 1] = False
    assert bool((count[inside] == 1).all()), count
    assert bool((count[outside] == 0).all()) and int(count.max()) == 1
    # the border of the lattice belongs to it where its edge owns the boundary: exactly two of the four sides, one corner
    assert int(count.sum()) == (hi - lo) ** 2
    never = _frag(verts, faces, M.ortho_pixel_camera(), 32, 32, True, mutant="own_never")["count"]
    always = _frag(verts, faces, M.ortho_pixel_camera(), 32, 32, True, mutant="own_always")["count"]
    assert int(never[inside].min()) == 0 and int(never.max()) == 1 and int(always[inside].min()) == 1 and int(always[inside].max()) >= 4
    assert bool((never <= count).all()) and bool((always >= count).all())


def test_fan_around_a_pixel_centre_gives_the_centre_to_one_face():
    verts, faces = M.fan()
    out = _frag(verts, faces, M.ortho_pixel_camera(), 16, 16, True)
    count = out["count"]
    assert int(count.max()) == 1 and int(count[8, 8]) == 1
    rim = np.array([(13, 8), (12, 12), (8, 13), (4, 12), (3, 8), (4, 4), (8, 3), (12, 4)], dtype=np.float64)
    for yi in range(16):
        for xi in range(16):   # strictly inside the (convex) octagon, float64
            d = np.roll(rim, -1, axis=0) - rim
            cross = d[:, 0] * (yi - rim[:, 1]) - d[:, 1] * (xi - rim[:, 0])
            if (cross > 0).all() or (cross < 0).all():
                assert int(count[yi, xi]) == 1, (yi, xi)
            elif ((cross > 0).any() and (cross < 0).any()):
                assert int(count[yi, xi]) == 0, (yi, xi)
    for xi, yi in ((9, 8), (10, 10), (8, 11), (6, 6)):   # centres on spokes
        assert int(count[yi, xi]) == 1
    assert int(_frag(verts, faces, M.ortho_pixel_camera(), 16, 16, True, mutant="own_always")["count"][8, 8]) == 8
    assert int(_frag(verts, faces, M.ortho_pixel_camera(), 16, 16, True, mutant="own_never")["count"][8, 8]) == 0


@pytest.mark.parametrize("ortho", [False, True])
def test_closed_sphere_from_outside_does_not_change_under_culling(ortho):
    v, f = M.icosphere(3)
    cam = M._ortho() if ortho else M._persp()
    plain, culled = _frag(v, f, cam, 48, 48, ortho), _frag(v, f, cam, 48, 48, ortho, cull=True)
    assert int((plain["pix_to_face"] >= 0).sum()) > 300 and M.same(plain, culled, ("pix_to_face", "zbuf", "bary"))
    assert int(plain["count"].max()) == 2 and int(culled["count"].max()) == 1      # front and back without culling
    inside_out = _frag(v, f[:, [0, 2, 1]], cam, 48, 48, ortho, cull=True)           # wound inwards: the far side is what faces the camera
    assert bool(((inside_out["pix_to_face"] >= 0) == (plain["pix_to_face"] >= 0)).all())
    hit = plain["pix_to_face"] >= 0
    assert bool((inside_out["zbuf"][hit] > plain["zbuf"][hit]).all())


@pytest.mark.parametrize("ortho", [False, True])
def test_front_faces_are_those_whose_float64_normal_points_to_the_camera(ortho):
    """The sign of the rule, pinned: A < 0 in snapped screen coordinates <=> (v1 - v0) x (v2 - v0) . (towards the viewer) > 0."""
    v, f = M.icosphere(3)
    cam = M._ortho() if ortho else M._persp()
    SX, SY, _, usable = M.project(v, cam.packed()[0], 224, 224, ortho)
    assert bool(usable.all())
    X, Y = SX[f], SY[f]
    A = M._edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    tri = v.double()[f]
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    R, T = cam.R[0].double(), cam.T[0].double()
    to_viewer = (-R[:, 2]).expand_as(normal) if ortho else (-(T @ R.t()) - tri.mean(1))
    cos = (normal * to_viewer).sum(1) / (normal.norm(dim=1) * to_viewer.norm(dim=1))
    clear = cos.abs() > 0.02                                                         # not edge-on: the snapping cannot flip these
    assert int(clear.sum()) > 1200 and int((A[clear] < 0).sum()) > 300 and int((A[clear] > 0).sum()) > 300
    assert bool(((A < 0) == (cos > 0))[clear].all())


def test_silhouette_of_an_orthographic_sphere():
    """The covered area lies between the discs of radius r - 1 and r + 1 pixels (the polyhedron is inscribed: its sagitta at level 3 is
    below a tenth of a pixel here)."""
    v, f = M.icosphere(3, 0.4)
    cam = M._ortho()
    out = _frag(v, f, cam, 64, 64, True)
    r = 0.4 * 1.6 * 32
    area = int((out["pix_to_face"] >= 0).sum())
    print(f"silhouette: {area} pixels, pi r^2 = {math.pi * r * r:.1f}")
    assert math.pi * (r - 1) ** 2 <= area <= math.pi * (r + 1) ** 2


# ---- depth ------------------------------------------------------------------------------------------------------------------------------
def _quad_on_centres(z_of_corner, H=32, W=32, focal=2.0):
    """A quad under a perspective camera at the origin looking along +z whose corners project ONTO the centres of the pixels (4, 5),
    (27, 6), (26, 28), (3, 27): view x = ndc z / focal."""
    from bdm_amd.cameras import PerspectiveCameras
    ij = torch.tensor([[4, 5], [27, 6], [26, 28], [3, 27]], dtype=torch.float64)
    z = torch.tensor(z_of_corner, dtype=torch.float64)
    ndc = torch.stack([1.0 - (2.0 * ij[:, 0] + 1.0) / W, 1.0 - (2.0 * ij[:, 1] + 1.0) / H], 1)
    verts = torch.cat([ndc * z[:, None] / focal, z[:, None]], 1)
    return verts, torch.tensor([[0, 1, 2], [0, 2, 3]]), PerspectiveCameras(focal_length=focal)


def test_depth_of_a_plane_facing_the_camera_is_constant_to_2_ulp():
    verts, faces, cam = _quad_on_centres([1.75] * 4)
    out = _frag(verts.float(), faces, cam, 32, 32, False)
    z = out["zbuf"][out["pix_to_face"] >= 0]
    assert z.numel() > 400
    ulp = float(np.spacing(np.float32(1.75)))
    spread = float(z.max() - z.min()) / ulp
    off = float((z.double() - 1.75).abs().max()) / ulp
    print(f"frontal plane: {z.numel()} pixels, spread {spread:.2f} ulp, largest distance from 1.75 {off:.2f} ulp")
    assert off <= 2.0 and spread <= 2.0


def test_depth_under_perspective_is_perspective_correct_and_the_screen_linear_mutant_is_not():
    """A plane tilted in depth (1.0 .. 3.0 over 23 pixels): the rule's depth is the plane's own depth along the ray of the pixel centre.
    Bound 1e-3: the corners are snapped to 1 / 256 pixel (at most 1 / 512 pixel off) and the depth changes by at most 0.2 per pixel
    here, so the snapping moves it by at most 4e-4; the float32 roundings are below 1e-6.  Interpolating depth linearly on the
    screen is wrong by tenths.  (On a plane FACING the camera the screen-linear depth is constant as well -- sum w_i z = z -- so the
    mutant can only show on a tilted one.)"""
    z_corner = [1.0, 3.0, 3.0, 1.0]
    verts, faces, cam = _quad_on_centres(z_corner)
    # the four corners are coplanar? corners 0, 1, 2 define the plane; keep the quad planar by solving corner 3's depth on it
    n = torch.linalg.cross(verts[1] - verts[0], verts[2] - verts[0], dim=0)
    d = float((n * verts[0]).sum())
    ray3 = verts[3] / verts[3, 2]
    verts[3] = ray3 * d / float((n * ray3).sum())
    out = _frag(verts.float(), faces, cam, 32, 32, False)
    lin = _frag(verts.float(), faces, cam, 32, 32, False, mutant="screen_linear_z")
    hit = out["pix_to_face"] >= 0
    assert bool((hit == (lin["pix_to_face"] >= 0)).all()) and int(hit.sum()) > 400
    yi, xi = torch.nonzero(hit, as_tuple=True)
    ray = torch.stack([(1.0 - (2.0 * xi.double() + 1.0) / 32) / 2.0, (1.0 - (2.0 * yi.double() + 1.0) / 32) / 2.0, torch.ones(xi.numel(), dtype=torch.float64)], 1)
    want = d / (ray * n).sum(1)
    err = float((out["zbuf"][hit].double() - want).abs().max())
    err_lin = float((lin["zbuf"][hit].double() - want).abs().max())
    print(f"tilted plane: rule {err:.2e}, screen-linear mutant {err_lin:.2e}")
    assert err <= 1e-3 and err_lin > 0.1
    b = out["bary"][hit].double()
    assert float((b.sum(1) - 1.0).abs().max()) < 1e-6 and float(b.min()) >= 0.0


def test_barycentrics_follow_the_faces_own_vertex_order():
    """The same triangle wound both ways: vertex k of each face gets the same weight at every pixel (bit for bit: the swap puts the
    same numbers through the same operations), which the mutant without the swap back does not give."""
    c = M.case("one_triangle_16")
    v, cam = c["verts"][0], c["cams"][0]
    a = M.render(v, torch.tensor([[0, 1, 2]]), cam, 16, 16)
    b = M.render(v, torch.tensor([[0, 2, 1]]), cam, 16, 16)
    assert int((a["pix_to_face"] >= 0).sum()) > 10 and torch.equal(a["zbuf"], b["zbuf"])
    assert torch.equal(a["bary"][..., [0, 2, 1]], b["bary"])
    tri = v.double()
    hit = a["pix_to_face"] >= 0
    point = (a["bary"][hit].double()[:, :, None] * tri[None]).sum(1)                 # the surface point the weights name
    _, _, zv, _ = M.project(point.float(), cam, 16, 16, False)
    assert float((zv - a["zbuf"][hit]).abs().max()) < 1e-5
    bad = M.render(v, torch.tensor([[0, 1, 2]]), cam, 16, 16, mutant="no_swap_back")
    bad2 = M.render(v, torch.tensor([[0, 2, 1]]), cam, 16, 16, mutant="no_swap_back")
    assert not (torch.equal(a["bary"], bad["bary"]) and torch.equal(b["bary"], bad2["bary"]))


def test_equal_depths_go_to_the_lower_face_index():
    c = M.case("pile_32")
    out = M.case_ref("pile_32")
    p2f = out["pix_to_face"][0]
    assert int(out["count"][0].max()) >= 3000
    shared = p2f >= 3000
    assert int(shared.sum()) > 50 and bool((p2f[shared] == 3000).all())            # 3000 coincident faces: the first wins every pixel
    assert int(out["count"][0][12, 14]) == 6000 and 0 <= int(p2f[12, 14]) < 3000     # the pile's pixel: the nearest sub-pixel face
    depth = c["verts"][0][:9000, 2].view(3000, 3)
    assert int(p2f[12, 14]) in torch.topk(-depth.mean(1), 5).indices.tolist()


# ---- the mutants and the case table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_changes_an_output_on_a_gpu_case(mutant):
    """The GPU test compares the kernel with the restatement on exactly these inputs: a misreading of the rule that changed nothing on
    them would pass it."""
    changed = [name for name in M.CASES if not M.same(M.case_ref(name), M.case_ref(name, mutant), ("pix_to_face", "zbuf", "bary"))]
    print(f"{mutant}: changes {len(changed)} of {len(M.CASES)} cases: {changed}")
    assert changed


def test_cases_hold_what_they_are_there_for():
    quad = M.case_ref("big_quad_64")
    assert bool((quad["pix_to_face"] >= 0).all()) and set(quad["pix_to_face"].unique().tolist()) == {0, 1}
    deg = [M.case_ref("degenerate_persp_32"), M.case_ref("degenerate_ortho_32")]
    assert all(100 < int((d["pix_to_face"] >= 0).sum()) < 32 * 32 for d in deg)
    clipped = M.case_ref("clipped_24x40")["pix_to_face"][0]
    assert bool((clipped[0, :5] >= 0).any() or (clipped[:5, 0] >= 0).any()) and int((clipped >= 0).sum()) > 20 and int(clipped.max()) < 320
    batch = M.case_ref("batch3_24x40")
    assert bool((batch["pix_to_face"][1] == -1).all()) and int((batch["pix_to_face"][0] >= 0).sum()) > 50 and int((batch["pix_to_face"][2] >= 0).sum()) > 20
    for name in M.CASES:
        if name.startswith("sphere"):
            assert M.case(name)["faces"][0].shape[0] == 1280 and int((M.case_ref(name)["pix_to_face"] >= 0).sum()) > 100


def test_images_of_the_restatement():
    c = M.case(M.FEATURE_CASE)
    frag = M.case_ref(M.FEATURE_CASE)
    hit = frag["pix_to_face"][0] >= 0
    vf, ff = M.case_features(M.FEATURE_CASE, 3, "vert"), M.case_features(M.FEATURE_CASE, 3, "face")
    args = (c["verts"], c["faces"], c["cams"], c["H"], c["W"], c["ortho"], c["cull"])
    smooth = M.render_batch(*args, vert_features=vf, background=M.BACKGROUND[:3])["image"][0]
    flat = M.render_batch(*args, face_features=ff, background=M.BACKGROUND[:3])["image"][0]
    bare = M.render_batch(*args, background=M.BACKGROUND[:3])["image"][0]
    bg = torch.tensor(M.BACKGROUND[:3])
    assert torch.equal(smooth[~hit], bg.expand(int((~hit).sum()), 3)) and torch.equal(bare, torch.where(hit[..., None], torch.zeros(3), bg))
    assert torch.equal(flat[hit], ff[frag["pix_to_face"][0][hit].long()])
    tri = vf.double()[c["faces"][0][frag["pix_to_face"][0][hit].long()]]
    want = (frag["bary"][0][hit].double()[:, :, None] * tri).sum(1)
    assert float((smooth[hit].double() - want).abs().max()) < 4 * 2.0 ** -24          # three products, two sums, values in [0, 1]


# ---- Meshes ---------------------------------------------------------------------------------------------------------------------------
def test_meshes_container_and_vertex_normals():
    from bdm_amd.cameras import Meshes
    v3, f3 = M.icosphere(3, 0.4)
    v1, f1 = M.icosphere(1, 0.3)
    meshes = Meshes([v3, v1, torch.zeros(0, 3)], [f3, f1, torch.zeros(0, 3, dtype=torch.int64)])
    assert len(meshes) == 3 and meshes.verts_list()[1] is v1 and meshes.faces_list()[0] is f3
    assert meshes.verts_packed().shape == (v3.shape[0] + v1.shape[0], 3) and torch.equal(meshes.verts_packed()[v3.shape[0]:], v1)
    assert meshes.mesh_to_verts_packed_first_idx().tolist() == [0, v3.shape[0], v3.shape[0] + v1.shape[0]]
    assert meshes.mesh_to_faces_packed_first_idx().tolist() == [0, 1280, 1360]
    packed = meshes.faces_packed()
    assert packed.dtype == torch.int64 and torch.equal(packed[:1280], f3) and torch.equal(packed[1280:], f1 + v3.shape[0])
    normals = meshes.verts_normals_packed()
    assert normals.shape == meshes.verts_packed().shape
    assert float((normals.double().norm(dim=1) - 1.0).abs().max()) < 1e-5
    # float64, the sum written out face by face
    verts64 = meshes.verts_packed().double()
    tri = verts64[packed]
    fn = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    acc = torch.zeros_like(verts64)
    for row, n in zip(packed.tolist(), fn):
        for k in row:
            acc[k] += n
    want = acc / acc.norm(dim=1, keepdim=True)
    assert float((normals.double() - want).abs().max()) < 1e-5
    sphere = meshes.verts_packed()[:v3.shape[0]].double()
    radial = sphere / sphere.norm(dim=1, keepdim=True)          # on a sphere the vertex normal is the radius, up to the squared angle
    assert float((normals[:v3.shape[0]].double() - radial).abs().max()) < 2e-2   # a face subtends (about 0.16 rad here: 0.013)
    assert float((meshes.faces_normals_packed().double().norm(dim=1) - 1.0).abs().max()) < 1e-5
    assert len(Meshes([], [])) == 0 and Meshes([], []).verts_packed().shape == (0, 3)
    for bad in (lambda: Meshes(v3, f3), lambda: Meshes([v3], [f3, f1]), lambda: Meshes([v3[:, :2]], [f3]), lambda: Meshes([v3], [f3.float()]),
                lambda: Meshes([v3.long()], [f3]), lambda: Meshes([v3], [f3[:, :2]])):
        with pytest.raises(ValueError):
            bad()


def test_argument_errors_come_before_any_launch():
    """Host tensors everywhere: a ValueError means the check ran before the library was asked for anything."""
    from bdm_amd.cameras import Meshes, PerspectiveCameras
    from bdm_amd.render import rasterize_meshes, render_mesh_batch, visualize_mesh_batch
    v, f = M.icosphere(1)
    one, two = Meshes([v], [f]), Meshes([v, v], [f, f])
    cam = PerspectiveCameras(focal_length=2.0, T=torch.tensor([[0.0, 0.0, 2.0]]))
    with pytest.raises(ValueError, match="cameras for"):
        rasterize_meshes(cam, two)
    with pytest.raises(ValueError, match="Meshes"):
        rasterize_meshes(cam, v)
    for size in (0, 4097, (16, 0), (5000, 16)):
        with pytest.raises(ValueError, match="image size"):
            rasterize_meshes(cam, one, image_size=size)
    with pytest.raises(ValueError, match="shading"):
        render_mesh_batch(cam, one, shading="phong")
    with pytest.raises(ValueError, match="vert_colors"):
        render_mesh_batch(cam, one, shading="flat", vert_colors=torch.zeros(v.shape[0], 3))
    with pytest.raises(ValueError, match="features"):
        render_mesh_batch(cam, one, shading="none", vert_colors=torch.zeros(v.shape[0] + 1, 3))
    with pytest.raises(ValueError, match="features"):
        render_mesh_batch(cam, one, shading="none", vert_colors=torch.zeros(v.shape[0], 3), background_color=(0.0, 0.0))
    with pytest.raises(ValueError, match="background"):
        render_mesh_batch(cam, one, shading="none", background_color=(0.0,) * 5)
    with pytest.raises(ValueError, match="ambient"):
        render_mesh_batch(cam, one, ambient=1.5)
    with pytest.raises(ValueError, match="divide 360"):
        visualize_mesh_batch(one, num_frames=7)
    with pytest.raises(ValueError, match="no mesh"):
        visualize_mesh_batch(Meshes([], []))
    from bdm_amd.render import _render_meshes
    with pytest.raises(ValueError, match="exclusive"):
        _render_meshes(cam, one, 16, vert_features=torch.zeros(v.shape[0], 3), face_features=torch.zeros(f.shape[0], 3), background=(0.0,) * 3)


# ---- main_render.py -------------------------------------------------------------------------------------------------------------------
def test_config_keys():
    from bdm_amd.config import ProjectConfig, parse_overrides
    import main_render as MR
    cfg = ProjectConfig()
    assert cfg.run.render_mesh_subdir == "pred_mesh" and cfg.run.render_mesh_shading == "smooth"
    cfg = parse_overrides(["run.render_mesh_subdir=meshes", "run.render_mesh_shading=flat"])
    assert cfg.run.render_mesh_subdir == "meshes" and cfg.run.render_mesh_shading == "flat"
    assert MR.KINDS == ("gt", "pred", "colored")
    with pytest.raises(ValueError, match="render_mesh_shading"):
        MR.parse_args(["dataset=synthetic", "run.render_sample_dir=/x", "run.render_mesh_shading=phong"])


def test_render_tree_draws_the_mesh_tree_only_where_it_exists(tmp_path):
    import main_render as MR
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    from PIL import Image
    cfg = MR.parse_args(["dataset=synthetic", f"run.render_sample_dir={tmp_path}", "dataloader.batch_size=3", "dataset.num_shapes=5",
                         "run.render_num_frames=2"])
    g = np.random.Generator(np.random.PCG64(0))
    for stem in ("synthetic_000000", "synthetic_000003"):
        save_pointcloud_ply(g.standard_normal((20, 3)), tmp_path / "pred" / "chair" / f"{stem}.ply")
    loader = SyntheticShapes(range(5), 3, image_size=32, num_points=8)
    cams = {i: c for batch in loader for i, c in zip(batch.frame_number, batch.camera)}
    cloud_stub = lambda cameras, points, colors: torch.zeros(len(cameras), 4, 6, 3)   # noqa: E731
    orbit_stub = lambda points, colors, path, n: [path.with_name(f"{path.stem}-{f}.png") for f in range(n)]   # noqa: E731
    calls, orbits = [], []

    def mesh_stub(cameras, verts, faces):   # image = (shape index recovered from the camera, vertex count, face count) / 255
        calls.append([(tuple(v.shape), tuple(f.shape), f.dtype) for v, f in zip(verts, faces)])
        out = torch.zeros(len(cameras), 4, 6, 3)
        for r, cam in enumerate(cameras):
            shape = [i for i, c in cams.items() if torch.equal(c.T, cam.T) and torch.equal(c.R, cam.R)]
            assert len(shape) == 1
            out[r] = torch.tensor([shape[0] + 0.5, verts[r].shape[0] + 0.5, faces[r].shape[0] + 0.5]) / 255.0
        return out

    def mesh_orbit_stub(verts, faces, path, n):
        orbits.append((path.name, tuple(verts.shape), tuple(faces.shape), n))
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(n)]

    # no mesh tree: the files written and the list returned are those of the call without the two new arguments
    before = MR.render_tree(cfg, loader, cloud_stub, orbit_stub)
    again = MR.render_tree(cfg, loader, cloud_stub, orbit_stub, mesh_fn=mesh_stub, mesh_orbit_fn=mesh_orbit_stub)
    assert again == before and not calls and not orbits and not (tmp_path / "renders" / "mesh").exists()
    assert sorted(p.name for p in (tmp_path / "renders").iterdir()) == ["pred"]

    meshes = {"synthetic_000000": (5, 4), "synthetic_000001-0": (6, 3), "synthetic_000001-1": (7, 2), "synthetic_000003": (9, 8)}
    for stem, (nv, nf) in meshes.items():
        save_mesh_ply(g.standard_normal((nv, 3)), g.integers(0, nv, size=(nf, 3)), tmp_path / "pred_mesh" / "chair" / f"{stem}.ply")
    save_pointcloud_ply(g.standard_normal((11, 3)), tmp_path / "pred_mesh" / "chair" / "synthetic_000002.ply")        # a cloud: no face element
    save_mesh_ply(g.standard_normal((4, 3)), g.integers(0, 4, size=(2, 3)), tmp_path / "pred_mesh" / "chair" / "synthetic_000001-x.ply")
    with pytest.raises(ValueError, match="mesh_fn"):
        MR.render_tree(cfg, loader, cloud_stub, orbit_stub)
    written = MR.render_tree(cfg, loader, cloud_stub, orbit_stub, mesh_fn=mesh_stub, mesh_orbit_fn=mesh_orbit_stub)
    new = [p for p in written if p not in before]
    assert [p for p in written if p in before] == before
    pngs = [p for p in new if p.parent.parent.name == "mesh"]
    assert sorted(p.stem for p in pngs) == sorted(meshes) and all(p.parent == tmp_path / "renders" / "mesh" / "chair" and p.exists() for p in pngs)
    assert sorted(p.name for p in new if p.parent.parent.name == "mesh_orbit") == sorted(f"{s}-{f}.png" for s in meshes for f in range(2))
    assert len(new) == 4 + 8
    # first batch (entries 0, 1, 2): three meshes in one call; second batch: entry 3
    assert calls == [[((5, 3), (4, 3), torch.int64), ((6, 3), (3, 3), torch.int64), ((7, 3), (2, 3), torch.int64)], [((9, 3), (8, 3), torch.int64)]]
    for stem, (nv, nf) in meshes.items():
        px = np.asarray(Image.open(tmp_path / "renders" / "mesh" / "chair" / f"{stem}.png"))
        assert px.shape == (4, 6, 3) and px[0, 0].tolist() == [int(stem[10:16]), nv, nf]
    assert sorted(orbits) == sorted((f"{s}.png", (nv, 3), (nf, 3), 2) for s, (nv, nf) in meshes.items())
    cfg.run.render_num_frames = 1
    orbits.clear()
    got = MR.render_tree(cfg, loader, cloud_stub, None, mesh_fn=mesh_stub, mesh_orbit_fn=mesh_orbit_stub)
    cfg.run.render_mesh_subdir = "absent"
    plain = MR.render_tree(cfg, loader, cloud_stub, None)
    assert plain == [p for p in before if p.parent.parent.name != "orbit"] and len(got) == len(plain) + 4 and not orbits
