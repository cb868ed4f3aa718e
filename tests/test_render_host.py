"""Host side of the renderer (no GPU): look_at_view_transform and OrthographicCameras, the make_grid restatement, the main_render.py
directory walk, and the sanity of the CPU restatement (tests/render_ref.py) the GPU tests compare against: its mutants must fall
outside the image bound at the inputs the GPU tests use."""
import numpy as np
import pytest
import torch

import render_ref as R


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def test_look_at_view_transform_properties():
    from bdm_amd.cameras import OrthographicCameras, PerspectiveCameras, look_at_view_transform
    dist = 10.0
    Rm, T = look_at_view_transform(dist=dist, elev=30, azim=list(range(0, 360, 30)))
    assert Rm.shape == (12, 3, 3) and T.shape == (12, 3)
    eye = torch.eye(3).expand(12, 3, 3)
    assert torch.allclose(Rm @ Rm.transpose(1, 2), eye, atol=1e-6) and torch.allclose(torch.linalg.det(Rm), torch.ones(12), atol=1e-6)
    centre = -torch.bmm(T[:, None, :], Rm.transpose(1, 2))[:, 0]                       # C = -T R^T
    assert torch.allclose(centre.norm(dim=1), torch.full((12,), dist), atol=1e-5)
    assert torch.allclose(centre[0], dist * torch.tensor([0.0, 0.5, 3 ** 0.5 / 2]), atol=1e-5)         # azim 0: on the +Z side, above
    assert torch.allclose(centre[3], dist * torch.tensor([3 ** 0.5 / 2, 0.5, 0.0]), atol=1e-5)         # azim 90: on the +X side
    for cls, ortho in ((PerspectiveCameras, False), (OrthographicCameras, True)):
        cams = cls(focal_length=0.7, R=Rm, T=T)
        assert cams.orthographic is ortho and cams.packed().shape == (12, 16) and len(cams) == 12
        assert type(cams.clone()) is cls and type(cams.to("cpu")) is cls
        for i in range(12):
            u, v, d = R.project(torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), cams.packed()[i], ortho)
            assert abs(float(u[0])) < 1e-6 and abs(float(v[0])) < 1e-6 and abs(float(d[0]) - dist) < 1e-5   # origin -> image centre
            assert float(v[1]) > float(v[0]) + 1e-3 and abs(float(u[1])) < 1e-6                              # world +Y is image-up
    # scalars, radians, broadcasting; straight down the up axis (pytorch3d's replacement of the vanishing x axis)
    R1, T1 = look_at_view_transform(2.0, np.pi / 6, 0.0, degrees=False)
    R2, T2 = look_at_view_transform(2.0, 30.0, 0.0)
    assert R1.shape == (1, 3, 3) and torch.allclose(R1, R2, atol=1e-6) and torch.allclose(T1, T2, atol=1e-6)
    R3, T3 = look_at_view_transform(3.0, 90.0, 0.0)
    assert torch.allclose(R3[0] @ R3[0].t(), torch.eye(3), atol=1e-5) and torch.allclose(T3, torch.tensor([[0.0, 0.0, 3.0]]), atol=1e-5)


def test_join_cameras_keeps_the_camera_type():
    from bdm_amd.cameras import OrthographicCameras, PerspectiveCameras, join_cameras, r2n2_camera
    a = join_cameras([r2n2_camera(10, 20, 1.5), r2n2_camera(50, 25, 1.6)])
    assert type(a) is PerspectiveCameras and len(a) == 2
    b = join_cameras([OrthographicCameras(focal_length=0.25), OrthographicCameras(focal_length=0.5)])
    assert type(b) is OrthographicCameras and b.focal_length.tolist() == [[0.25, 0.25], [0.5, 0.5]]


# ---- make_grid -----------------------------------------------------------------------------------------------------------------------
def test_make_grid_small_cases():
    from bdm_amd.render import make_grid
    x = torch.arange(3 * 2 * 1 * 2, dtype=torch.float32).reshape(3, 2, 1, 2) + 10   # three 1 x 2 images of two channels
    g = make_grid(x, nrow=2, padding=1, pad_value=-1.0)
    P = -1.0
    want0 = [[P, P, P, P, P, P, P], [P, 10, 11, P, 14, 15, P], [P, P, P, P, P, P, P], [P, 18, 19, P, P, P, P], [P, P, P, P, P, P, P]]
    assert g.shape == (2, 5, 7) and g[0].tolist() == want0
    assert g[1, 1].tolist() == [P, 12, 13, P, 16, 17, P]
    assert torch.equal(make_grid(x[:1], nrow=1, pad_value=1.0), x[0])                 # one image: returned as it is, no border
    one = make_grid(torch.full((2, 1, 1, 1), 0.5), nrow=1, padding=2, pad_value=1.0)  # single channel -> three; nrow 1 -> a column
    assert one.shape == (3, 8, 5) and one[:, 2, 2].tolist() == [0.5] * 3 and one[:, 5, 2].tolist() == [0.5] * 3
    assert float(one.sum()) == 3 * (8 * 5 - 2) * 1.0 + 3 * 2 * 0.5
    for B, nrow in ((4, 2), (5, 2), (2, 1), (7, 3), (1, 1)):                           # against the independent numpy restatement
        y = torch.rand(B, 3, 4, 5, generator=torch.Generator().manual_seed(B))
        assert np.array_equal(make_grid(y, nrow=nrow, pad_value=1).numpy(), R.make_grid(y.numpy(), nrow))


# ---- the restatement's own sanity ----------------------------------------------------------------------------------------------------
def test_fragments_against_a_per_pixel_loop():
    """The vectorised restatement against the plainest statement of the rule, pixel by pixel, on a tiny input with ties."""
    pts, packed, _, _ = R.tie_case()
    H = W = 12
    radius, k = 0.2, 3
    idx, zbuf, dists, count = R.fragments(pts[0], packed[0], H, W, radius, k)
    u, v, d = R.project(pts[0], packed[0])
    r2 = R.radius2(radius)
    for yi in range(H):
        for xi in range(W):
            xf, yf = 1.0 - (2.0 * torch.tensor(float(xi)) + 1.0) / W, 1.0 - (2.0 * torch.tensor(float(yi)) + 1.0) / H
            dx, dy = xf - u, yf - v
            d2 = dx * dx + dy * dy
            cand = sorted((float(d[i]), i) for i in range(pts.shape[1]) if bool(d2[i] < r2) and bool(d[i] >= 0))
            assert int(count[yi, xi]) == len(cand)
            want = [c[1] for c in cand[:k]] + [-1] * (k - min(k, len(cand)))
            assert idx[yi, xi].tolist() == want
            for j, i in enumerate(want):
                assert float(dists[yi, xi, j]) == (float(d2[i]) if i >= 0 else -1.0) and float(zbuf[yi, xi, j]) == (2.0 if i >= 0 else -1.0)
    assert int((count > k).sum()) > 0 and int((count == 0).sum()) > 0


def test_windowless_restatement_agrees_with_the_conditioning_rasteriser():
    """k = 1 of the renderer's rule is the conditioning rule: slot 0 equals oracle.ref_sampler.rasterize_bruteforce."""
    from oracle.ref_sampler import rasterize_bruteforce
    pts, packed, _, _ = R.case("n300_32_k1")
    idx = R.case_fragments("n300_32_k1")[0]
    assert torch.equal(idx[0, :, :, 0], rasterize_bruteforce(pts[0], packed[0], 32, 32, 0.05))


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_have_every_pixel_class(name):
    B, N, H, W, radius, k, ortho, _, _ = R.CASES[name]
    count = R.case_fragments(name)[3]
    assert int((count > k).sum()) > 0 and int((count == 0).sum()) > 0
    assert k == 1 or int(((count >= 1) & (count < k)).sum()) > 0       # (no such pixel exists for k = 1)


IMAGE_INPUTS = [("b2_n300_32_k4", 0), ("tie", 0), ("one_pixel", 0)]   # what tests/test_hip_render.py composites


def _frag_input(name, b):
    if name == "tie":
        pts, packed, _, feats = R.tie_case()
        return pts[b], packed[b], feats[b], 32, 32, 0.05, 4, False
    if name == "one_pixel":
        pts, packed, _, feats = R.one_pixel_case()
        return pts[b], packed[b], feats[b], 32, 32, 0.02, 4, False
    B, N, H, W, radius, k, ortho, _, _ = R.CASES[name]
    pts, packed, _, feats = R.case(name)
    return pts[b], packed[b], feats[b], H, W, radius, k, ortho


@pytest.mark.parametrize("compositor", ["norm_weighted", "alpha"])
def test_mutants_fall_outside_the_image_bound(compositor):
    """Each mutant of the restatement must differ from it by more than the bound the GPU image test asserts, at that test's own
    inputs -- otherwise the GPU test could not tell the mutant from the rule."""
    bg = (0.78431373, 0.5, 0.25)
    pts, cam, feats, H, W, radius, k, ortho = _frag_input("b2_n300_32_k4", 0)
    idx, zbuf, dists, count = R.fragments(pts, cam, H, W, radius, k, ortho)
    bound = R.image_bound(k, compositor)
    true = R.composite(idx, dists, feats[:, :3], bg, radius, compositor)
    assert float(true.min()) >= 0.0 and float(true.max()) <= 1.0 + 1e-12
    mutants = ["linear_weight", "any_empty", "drop_slot"] + (["no_norm"] if compositor == "norm_weighted" else [])
    for m in mutants:
        diff = float((R.composite(idx, dists, feats[:, :3], bg, radius, compositor, mutant=m) - true).abs().max())
        assert diff > 100 * bound, (m, diff, bound)
    # ties by LATEST index: visible where all depths are equal (the tie input)
    pts, cam, feats, H, W, radius, k, ortho = _frag_input("tie", 0)
    idx, _, dists, count = R.fragments(pts, cam, H, W, radius, k)
    idx2, _, dists2, _ = R.fragments(pts, cam, H, W, radius, k, ties="latest")
    assert not torch.equal(idx, idx2) and int((count > k).sum()) > 0
    true = R.composite(idx, dists, feats[:, :3], bg, radius, compositor)
    diff = float((R.composite(idx2, dists2, feats[:, :3], bg, radius, compositor) - true).abs().max())
    assert diff > 100 * R.image_bound(k, compositor), diff


def test_float32_composite_of_the_restatement_meets_the_bound():
    """The bound is not vacuous on the CPU either: the same sums in float32, slot by slot, stay inside it."""
    for name, b in IMAGE_INPUTS:
        pts, cam, feats, H, W, radius, k, ortho = _frag_input(name, b)
        idx, _, dists, _ = R.fragments(pts, cam, H, W, radius, k, ortho)
        used, r2 = idx >= 0, R.radius2(radius)
        w = torch.where(used, 1.0 - dists / r2, torch.zeros(()))
        f = feats[idx.clamp(min=0)]
        num, den, alpha, trans = torch.zeros(H, W, 4), torch.zeros(H, W), torch.zeros(H, W, 4), torch.ones(H, W)
        for j in range(k):
            num = num + (w[..., j, None] * f[..., j, :])
            den = den + w[..., j]
            alpha = alpha + (w[..., j] * trans)[..., None] * f[..., j, :]
            trans = trans * (1.0 - w[..., j])
        got = {"norm_weighted": num / den.clamp(min=1e-4)[..., None], "alpha": alpha}
        for comp in got:
            want = R.composite(idx, dists, feats, (0.0,) * 4, radius, comp)
            err = float((got[comp].double() - want)[used[..., 0]].abs().max())
            assert err <= R.image_bound(k, comp), (name, comp, err)


# ---- main_render.py ------------------------------------------------------------------------------------------------------------------
def test_config_keys():
    from bdm_amd.config import ProjectConfig, parse_overrides
    cfg = ProjectConfig()
    assert cfg.run.render_sample_dir is None and cfg.run.render_num_frames == 1
    cfg = parse_overrides(["run.render_sample_dir=/x/y", "run.render_num_frames=4"])
    assert cfg.run.render_sample_dir == "/x/y" and cfg.run.render_num_frames == 4


def test_main_render_arguments_and_directory_walk(tmp_path):
    """gt / pred for entries 0, 1 (two samples) and 3 (another point count) of five, colored for entry 0 only: every cloud found is
    rendered with ITS entry's camera and written under renders/<kind>/; the orbit takes each prediction once, coloured where a
    coloured copy exists."""
    import main_render as MR
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_pointcloud_ply, save_pointcloud_ply_rgb
    from PIL import Image
    with pytest.raises(ValueError, match="render_sample_dir"):
        MR.parse_args(["dataset=synthetic"])
    with pytest.raises(ValueError, match="divide 360"):
        MR.parse_args(["dataset=synthetic", f"run.render_sample_dir={tmp_path}", "run.render_num_frames=7"])
    cfg = MR.parse_args(["dataset=synthetic", f"run.render_sample_dir={tmp_path}", "dataloader.batch_size=3", "dataset.num_shapes=5",
                         "run.render_num_frames=2"])
    g = np.random.Generator(np.random.PCG64(0))
    stems = {"synthetic_000000": 20, "synthetic_000001-0": 20, "synthetic_000001-1": 20, "synthetic_000003": 33}
    for stem, n in stems.items():
        save_pointcloud_ply(g.standard_normal((n, 3)), tmp_path / "pred" / "chair" / f"{stem}.ply")
        save_pointcloud_ply(g.standard_normal((n, 3)), tmp_path / "gt" / "chair" / f"{stem}.ply")
    save_pointcloud_ply(g.standard_normal((5, 3)), tmp_path / "pred" / "chair" / "synthetic_000001-x.ply")   # not a sample index
    save_pointcloud_ply_rgb(g.standard_normal((20, 3)), np.full((20, 3), 51 / 255.0), tmp_path / "colored" / "chair" / "synthetic_000000.ply")
    loader = SyntheticShapes(range(5), 3, image_size=32, num_points=8)
    cams = {i: c for batch in loader for i, c in zip(batch.frame_number, batch.camera)}
    calls, orbits = [], []

    def stub(cameras, points, colors):   # image = (shape index recovered from the camera, point count, first colour) / 255
        calls.append((len(cameras), tuple(points.shape), None if colors is None else tuple(colors.shape)))
        out = torch.zeros(len(cameras), 4, 6, 3)
        for r, cam in enumerate(cameras):
            shape = [i for i, c in cams.items() if torch.equal(c.T, cam.T) and torch.equal(c.R, cam.R)]
            assert len(shape) == 1
            out[r, :, :, 0] = (shape[0] + 0.5) / 255.0
            out[r, :, :, 1] = (points.shape[1] + 0.5) / 255.0
            out[r, :, :, 2] = 0.0 if colors is None else (float(colors[r, 0, 0]) * 255.0 + 0.5) / 255.0
        return out

    def orbit_stub(points, colors, path, num_frames):
        orbits.append((path.name, tuple(points.shape), colors is not None, num_frames))
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(num_frames)]

    written = MR.render_tree(cfg, loader, stub, orbit_stub)
    want = [("gt", s) for s in stems] + [("pred", s) for s in stems] + [("colored", "synthetic_000000")]
    pngs = [p for p in written if p.parent.parent.name != "orbit"]
    assert sorted((p.parent.parent.name, p.stem) for p in pngs) == sorted(want)
    assert all(p.parent.name == "chair" and p.parent.parent.parent == tmp_path / "renders" and p.exists() for p in pngs)
    assert sorted(p.name for p in (tmp_path / "renders" / "pred" / "chair").iterdir()) == sorted(f"{s}.png" for s in stems)
    # first batch (entries 0, 1, 2): colored (1 cloud), gt and pred (3 clouds of 20 points each); second batch: entry 3, gt and pred
    assert sorted(calls, key=str) == sorted([(1, (1, 20, 3), (1, 20, 3)), (3, (3, 20, 3), None), (3, (3, 20, 3), None),
                                             (1, (1, 33, 3), None), (1, (1, 33, 3), None)], key=str)
    for kind, stem in want:
        px = np.asarray(Image.open(tmp_path / "renders" / kind / "chair" / f"{stem}.png"))
        assert px.shape == (4, 6, 3)
        assert px[0, 0].tolist() == [int(stem[10:16]), stems[stem], 51 if kind == "colored" else 0]
    assert sorted(orbits) == sorted([("synthetic_000000.png", (1, 20, 3), True, 2), ("synthetic_000001-0.png", (1, 20, 3), False, 2),
                                     ("synthetic_000001-1.png", (1, 20, 3), False, 2), ("synthetic_000003.png", (1, 33, 3), False, 2)])
    assert sorted(p.name for p in written if p.parent.parent.name == "orbit") == sorted(
        f"{s}-{f}.png" for s in stems for f in range(2))
    # run.render_num_frames = 1 (the default): no orbit
    cfg.run.render_num_frames = 1
    orbits.clear()
    MR.render_tree(cfg, loader, stub, orbit_stub)
    assert not orbits
