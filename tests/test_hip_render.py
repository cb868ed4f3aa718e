"""bdm_render_points (csrc/render.hip) and bdm_amd/render.py on the GPU against the CPU restatement tests/render_ref.py: the
fragments bit for bit, the images inside the derived bounds (render_ref.image_bound), the invariances with torch.equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = (0.78431373, 0.5, 0.25, 0.125)


def _gpu(cams, pts, H, W, radius, k, feats=None, bg=None, compositor=None, fragments=True):
    """One kernel call through bdm_amd.render._render, results on the host."""
    from bdm_amd.render import _render
    frag, image = _render(cams.to("cuda"), pts.cuda(), (H, W), radius, k, None if feats is None else feats.cuda(), bg, compositor, fragments)
    torch.cuda.synchronize()
    return (None if frag is None else tuple(t.cpu() for t in frag)), (None if image is None else image.cpu())


def _assert_fragments(got, want, what):
    for name, g, w in zip(("idx", "zbuf", "dists"), got, want[:3]):
        bad = (g != w) & ~((g != g) & (w != w))
        assert torch.equal(g, w), f"{what}: {name} differs at {int(bad.sum())} of {g.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"


@pytest.mark.parametrize("name", list(R.CASES))
def test_fragments_equal_the_restatement(hip, name):
    B, N, H, W, radius, k, ortho, _, _ = R.CASES[name]
    pts, packed, cams, _ = R.case(name)
    want = R.case_fragments(name)
    count = want[3]
    assert int((count > k).sum()) > 0 and int((count == 0).sum()) > 0 and (k == 1 or int(((count >= 1) & (count < k)).sum()) > 0)
    assert cams.orthographic is ortho
    got, _ = _gpu(cams, pts, H, W, radius, k)
    assert got[0].dtype == torch.int64 and got[0].shape == (B, H, W, k)
    _assert_fragments(got, want, name)
    from bdm_amd.render import rasterize_points
    frag = rasterize_points(cams.to("cuda"), pts.cuda(), (H, W), radius, k)
    assert torch.equal(frag.idx.cpu(), want[0]) and torch.equal(frag.zbuf.cpu(), want[1]) and torch.equal(frag.dists.cpu(), want[2])


def test_ties_follow_the_point_index(hip):
    pts, packed, cams, _ = R.tie_case()
    want = R.fragments(pts[0], packed[0], 32, 32, 0.05, 4)
    assert int((want[3] > 4).sum()) > 0 and bool((want[1][want[0] >= 0] == 2.0).all())   # one depth; lists longer than k exist
    dup = want[0][(want[0][..., 0] >= 0) & (want[0][..., 1] >= 100)]                    # (duplicates 100.. of 0..29 share every pixel)
    assert dup.numel() > 0
    got, _ = _gpu(cams, pts, 32, 32, 0.05, 4)
    _assert_fragments(tuple(g[0] for g in got), want, "ties")
    assert not torch.equal(got[0][0], R.fragments(pts[0], packed[0], 32, 32, 0.05, 4, ties="latest")[0])


def test_long_list_and_degenerate_projections(hip):
    """3000 points in ONE pixel (every chunk of the tile's stream is full of survivors) with behind-camera, NaN, z -> 0+ and
    far-outside points among them, and the same kinds mixed into a general cloud: equal to the restatement, and BDM_OK (an error
    would have raised): the counterpart of test_rasterizer_survives_degenerate_projections."""
    pts, packed, cams, _ = R.one_pixel_case()
    for k in (4, 16):
        want = R.fragments(pts[0], packed[0], 32, 32, 0.02, k)
        assert int((want[3] > 0).sum()) == 1 and int(want[3].max()) > 2900      # one pixel holds (almost) every point
        got, _ = _gpu(cams, pts, 32, 32, 0.02, k)
        _assert_fragments(tuple(g[0] for g in got), want, f"one pixel k={k}")
    assert 0.0 < float(got[1][got[0] >= 0].min()) < 1e-29                       # the candidate at z = 1e-30 leads its pixel
    B, N, H, W, radius, k, ortho, _, _ = R.CASES["b2_n300_32_k4"]
    pts, packed, cams, _ = R.case("b2_n300_32_k4")
    bad = torch.stack([R.with_degenerates(pts[b], packed[b], torch.Generator().manual_seed(5 + b)) for b in range(B)])
    assert int(torch.isnan(bad).sum()) == 2 * 6
    want = [R.fragments(bad[b], packed[b], H, W, radius, k) for b in range(B)]
    got, _ = _gpu(cams, bad, H, W, radius, k)
    for b in range(B):
        _assert_fragments(tuple(g[b] for g in got), want[b], f"degenerates, shape {b}")


def _image_inputs():
    out = []
    for name in ("b2_n300_32_k4", "ortho_b2_n300_32_k4", "n200_24x40_k16"):
        B, N, H, W, radius, k, ortho, _, _ = R.CASES[name]
        pts, packed, cams, feats = R.case(name)
        out.append((name, pts, packed, cams, feats, H, W, radius, k, ortho))
    pts, packed, cams, feats = R.tie_case()
    out.append(("tie", pts, packed, cams, feats, 32, 32, 0.05, 4, False))
    pts, packed, cams, feats = R.one_pixel_case()
    out.append(("one_pixel", pts, packed, cams, feats, 32, 32, 0.02, 4, False))
    return out


@pytest.mark.parametrize("compositor", ["norm_weighted", "alpha"])
@pytest.mark.parametrize("channels", [3, 4])
def test_image_against_the_float64_composite(hip, compositor, channels):
    """Elementwise |image - float64 composite of the kernel's own fragments| <= render_ref.image_bound(k, compositor) =
    (2k + 3) 2^-24 for BOTH compositors, features in [0, 1].  Derivation (render_ref.image_bound): the terms are non-negative and
    the exact result is <= 1, so relative errors of the terms bound the absolute error of the sum.  norm_weighted: one product and
    <= k - 1 additions per numerator term, k - 1 additions in the denominator, one division: 2k roundings.  alpha: term j is
    f (w_j T_j) with T_j = prod_{i<j} fl(1 - w_i): j subtractions, j - 1 rounded products (T starts at 1), two more products,
    <= k - j additions: k + j + 1 <= 2k roundings.  + 3 u for second-order terms.  The weights 1 - d2 / r^2 are taken in float32 on
    both sides from bit-identical d2 (asserted first), with one correctly rounded division and one subtraction."""
    bg = BG[:channels]
    for name, pts, packed, cams, feats, H, W, radius, k, ortho in _image_inputs():
        f = feats[..., :channels].contiguous()
        frag, image = _gpu(cams, pts, H, W, radius, k, f, bg, compositor)
        bound = R.image_bound(k, compositor)
        for b in range(pts.shape[0]):
            want_frag = R.fragments(pts[b], packed[b], H, W, radius, k, ortho) if name in ("tie", "one_pixel") else tuple(
                t[b] for t in R.case_fragments(name))
            _assert_fragments(tuple(g[b] for g in frag), want_frag, name)
            want = R.composite(frag[0][b], frag[2][b], f[b], bg, radius, compositor)
            err = (image[b].double() - want).abs()
            print(f"{name}[{b}] {compositor} c={channels}: max err {float(err.max()):.3e} bound {bound:.3e}")
            assert float(err.max()) <= bound, (name, b, float(err.max()), bound)
            empty = frag[0][b][..., 0] < 0
            assert torch.equal(image[b][empty], torch.tensor(bg).expand(int(empty.sum()), channels))   # background unchanged


def test_image_without_features_is_black_on_background(hip):
    B, N, H, W, radius, k, ortho, _, _ = R.CASES["b2_n300_32_k4"]
    pts, packed, cams, _ = R.case("b2_n300_32_k4")
    idx = R.case_fragments("b2_n300_32_k4")[0]
    for compositor in ("norm_weighted", "alpha"):
        _, image = _gpu(cams, pts, H, W, radius, k, None, BG[:3], compositor, fragments=False)
        want = torch.where((idx[..., 0] < 0)[..., None], torch.tensor(BG[:3]), torch.zeros(3))
        assert torch.equal(image, want)
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.render import render_pointcloud_batch_pytorch3d
    img = render_pointcloud_batch_pytorch3d(cams.to("cuda"), Pointclouds(pts.cuda()), image_size=32, radius=radius, points_per_pixel=k,
                                            background_color=BG[:3]).cpu()
    assert torch.equal(img, want)
    with pytest.raises(ValueError):
        render_pointcloud_batch_pytorch3d(cams.to("cuda"), Pointclouds(pts.cuda()), compositor="softmax")


def test_invariances(hip):
    name = "b2_n300_32_k4"
    B, N, H, W, radius, k, ortho, _, _ = R.CASES[name]
    pts, packed, cams, feats = R.case(name)
    f = feats[..., :3].contiguous()
    from bdm_amd.cameras import PerspectiveCameras
    for compositor in ("norm_weighted", "alpha"):
        frag, image = _gpu(cams, pts, H, W, radius, k, f, BG[:3], compositor)
        # image-only call == call that also stores the fragments
        none, only = _gpu(cams, pts, H, W, radius, k, f, BG[:3], compositor, fragments=False)
        assert none is None and torch.equal(only, image)
        # each shape of the batch == the same shape alone
        for b in range(B):
            one = PerspectiveCameras(cams.focal_length[b:b + 1], cams.principal_point[b:b + 1], cams.R[b:b + 1], cams.T[b:b + 1])
            fr1, im1 = _gpu(one, pts[b:b + 1], H, W, radius, k, f[b:b + 1], BG[:3], compositor)
            assert torch.equal(im1[0], image[b]) and all(torch.equal(a[0], c[b]) for a, c in zip(fr1, frag))
        # a permuted cloud (features alike): same image, idx maps through the permutation; the input has no equal depths
        for b in range(B):
            depth = R.project(pts[b], packed[b])[2]
            assert depth.unique().numel() == N
        perm = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(9 + b)) for b in range(B)])
        p_pts = torch.stack([pts[b][perm[b]] for b in range(B)])
        p_f = torch.stack([f[b][perm[b]] for b in range(B)])
        fr2, im2 = _gpu(cams, p_pts, H, W, radius, k, p_f, BG[:3], compositor)
        assert torch.equal(im2, image)
        for b in range(B):
            mapped = torch.where(fr2[0][b] >= 0, perm[b][fr2[0][b].clamp(min=0)], torch.full((), -1))
            assert torch.equal(mapped, frag[0][b]) and torch.equal(fr2[1][b], frag[1][b]) and torch.equal(fr2[2][b], frag[2][b])


def test_limits_return_an_error_and_launch_nothing(hip):
    from bdm_amd import _lib as L
    from bdm_amd import ops
    B, N, H, W = 1, 64, 32, 32
    pts = torch.rand(B, N, 3, device="cuda")
    cam = R.tie_case()[1].cuda()
    ws = ops.workspace(L.lib().bdm_render_workspace_bytes(B, N, H, W, L.c_float(0.05)), "cuda", "render")
    for k, c, radius, what in ((17, 3, 0.05, "points per pixel"), (0, 3, 0.05, "points per pixel"), (4, 5, 0.05, "channels"),
                               (4, 0, 0.05, "channels"), (4, 3, 0.51, "radius")):
        idx = torch.full((B, H, W, max(k, 1)), -7, dtype=torch.int32, device="cuda")
        image = torch.full((B, H, W, max(c, 1)), -7.0, device="cuda")
        bg = torch.zeros(8, device="cuda")
        rc = L.lib().bdm_render_points(B, N, H, W, k, c, L.c_float(radius), 0, 0, L.ptr(pts), L.ptr(cam), None, L.ptr(bg), L.ptr(idx),
                                       None, None, L.ptr(image), L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        assert rc != 0 and what in L.lib().bdm_last_error().decode()
        assert bool((idx == -7).all()) and bool((image == -7.0).all())          # nothing ran
    with pytest.raises(L.BdmHipError):
        from bdm_amd.render import rasterize_points
        rasterize_points(R.tie_case()[2].to("cuda"), pts, 32, 0.05, 17)
    # radius of exactly 8 pixel pitches is accepted; an empty batch is a no-op
    assert L.lib().bdm_render_points(B, N, H, W, 4, 3, L.c_float(0.5), 0, 0, L.ptr(pts), L.ptr(cam), None, L.ptr(bg), None, None, None,
                                     L.ptr(torch.empty(B, H, W, 3, device="cuda")), L.ptr(ws), L.stream()) == 0
    assert L.lib().bdm_render_points(0, N, H, W, 4, 3, L.c_float(0.05), 0, 0, None, None, None, None, None, None, None, None, None,
                                     L.stream()) == 0
    torch.cuda.synchronize()


def test_orbit_frames_and_grid(hip, tmp_path):
    """visualize_pointcloud_batch_pytorch3d with the orbiting orthographic cameras: frame f of shape b equals the restatement's
    render from look_at_view_transform(10, 30, azim_f) within the norm_weighted bound; the frames are tiled and written as
    <stem>-<f>.png."""
    from bdm_amd.cameras import OrthographicCameras, Pointclouds, look_at_view_transform
    from bdm_amd.render import visualize_pointcloud_batch_pytorch3d
    from PIL import Image
    g = torch.Generator().manual_seed(3)
    pts, feats = torch.randn(2, 400, 3, generator=g) * 0.8, torch.rand(2, 400, 3, generator=g)
    grids = visualize_pointcloud_batch_pytorch3d(Pointclouds(pts.cuda(), feats.cuda()), output_file_image=str(tmp_path / "o" / "x.png"),
                                                 num_frames=3)
    assert grids.shape == (3, 3, 2 * 226 + 2, 226 + 2)                # nrow = int(sqrt(2)) = 1: a column of two
    assert sorted(os.listdir(tmp_path / "o")) == ["x-0.png", "x-1.png", "x-2.png"]
    Rm, T = look_at_view_transform(10.0, 30, [0, 120, 240])
    for f in (0, 2):
        cam = OrthographicCameras(focal_length=0.25, R=Rm[f:f + 1], T=T[f:f + 1]).packed()[0]
        for b in range(2):
            idx, _, dists, _ = R.fragments(pts[b], cam, 224, 224, 0.01, 10, ortho=True)
            want = R.composite(idx, dists, feats[b], (0.78431373,) * 3, 0.01, "norm_weighted")
            got = grids[f][:, 2 + b * 226:2 + b * 226 + 224, 2:226].permute(1, 2, 0)
            assert float((got.double() - want).abs().max()) <= R.image_bound(10, "norm_weighted")
            assert int((idx[..., 0] >= 0).sum()) > 100
        png = np.asarray(Image.open(tmp_path / "o" / f"x-{f}.png"))
        assert np.array_equal(png, (grids[f].numpy() * 255.0).astype(np.uint8).transpose(1, 2, 0))
    one = visualize_pointcloud_batch_pytorch3d(Pointclouds(pts.cuda(), None), output_file_image=str(tmp_path / "single.png"))
    assert one.shape == (1, 3, 454, 228) and (tmp_path / "single.png").exists()


def test_command_line_renders_the_sample_tree(hip, tmp_path):
    """`main.py run.job=sample` on two tiny synthetic shapes, a hand-coloured copy of one prediction, then main_render.py, each in a
    fresh child process: renders/{gt,pred,colored,orbit} exist and every PNG is within one level per byte of the restatement's."""
    from bdm_amd.cameras import OrthographicCameras, look_at_view_transform
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply_rgb
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["dataset=synthetic", "dataset.max_points=1024", "dataset.num_shapes=2", "dataloader.batch_size=2"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "run.job=sample", f"run.save_dir={tmp_path}", "run.name=render_cli",
                          "run.num_inference_steps=25", "run.diffusion_scheduler=ddpm"] + common, capture_output=True, text=True, env=env,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    root = sorted((tmp_path / "render_cli").iterdir())[0] / "sample"
    names = [f"synthetic_{j:06d}" for j in range(2)]
    pred0 = load_pointcloud_ply(root / "pred" / "chair" / f"{names[0]}.ply")
    colours = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=pred0.shape) / 255.0
    save_pointcloud_ply_rgb(pred0, colours, root / "colored" / "chair" / f"{names[0]}.ply")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "main_render.py"), f"run.render_sample_dir={root}", "run.render_num_frames=2"]
                         + common, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    for kind in ("gt", "pred"):
        assert sorted(os.listdir(root / "renders" / kind / "chair")) == [f"{n}.png" for n in names]
    assert os.listdir(root / "renders" / "colored" / "chair") == [f"{names[0]}.png"]
    assert sorted(os.listdir(root / "renders" / "orbit" / "chair")) == [f"{n}-{f}.png" for n in names for f in range(2)]
    batch = next(iter(SyntheticShapes(range(2), 2, seed=42, image_size=224, num_points=1024)))
    bg = (0.78431373,) * 3

    def check(png, pts, cam, feats, ortho=False, min_cover=0):
        idx, _, dists, _ = R.fragments(torch.from_numpy(pts), cam, 224, 224, 0.01, 10, ortho)
        want = R.composite(idx, dists, feats, bg, 0.01, "norm_weighted")
        want = (want.float().numpy() * 255.0).astype(np.uint8)
        got = np.asarray(Image.open(png))
        assert got.shape == (224, 224, 3) and int((idx[..., 0] >= 0).sum()) >= min_cover
        assert int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) <= 1, png

    for j, name in enumerate(names):
        cam = batch.camera[j].packed()[0]
        for kind in ("gt", "pred"):
            check(root / "renders" / kind / "chair" / f"{name}.png", load_pointcloud_ply(root / kind / "chair" / f"{name}.ply"), cam, None,
                  min_cover=50 if kind == "gt" else 0)   # (the ground truth is known to face the camera; a random-weight prediction is not)
    pts, col = load_pointcloud_ply(root / "colored" / "chair" / f"{names[0]}.ply", with_colors=True)
    check(root / "renders" / "colored" / "chair" / f"{names[0]}.png", pts, batch.camera[0].packed()[0], torch.from_numpy(col))
    Rm, T = look_at_view_transform(10.0, 30, [0, 180])
    ocam = OrthographicCameras(focal_length=0.25, R=Rm[1:2], T=T[1:2]).packed()[0]
    check(root / "renders" / "orbit" / "chair" / f"{names[0]}-1.png", pts, ocam, torch.from_numpy(col), ortho=True)
    check(root / "renders" / "orbit" / "chair" / f"{names[1]}-1.png", load_pointcloud_ply(root / "pred" / "chair" / f"{names[1]}.ply"), ocam,
          None, ortho=True)
