"""Host checks of the normal estimator's pieces (no GPU): the CPU restatement tests/normals_ref.py against known surfaces, its
MUTANTS against the bounds the GPU test holds the kernel to (tests/test_hip_normals.py), the float32 numpy restatement those
bounds are derived from, PLY I/O with normals, shade_by_normals, the command line's parsing and file walk, main_render's new key."""
import json

import numpy as np
import pytest
import torch

import normals_ref as R


# ---- the restatement against known surfaces ------------------------------------------------------------------------------------------
def test_plane_gives_the_plane_normal_and_zero_l0():
    g = torch.Generator().manual_seed(5)
    uv = torch.rand(400, 2, generator=g, dtype=torch.float64) - 0.5
    a, b = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64), torch.tensor([-2.0, 1.0, 0.0], dtype=torch.float64)
    n = torch.linalg.cross(a, b)
    n = (n / n.norm()).numpy()
    pts = (uv[:, :1] * a / a.norm() + uv[:, 1:] * b / b.norm()).float()
    ref = R.estimate(pts, 20)
    assert float(R.cross_norm(ref["normals"], n[None]).max()) < 1e-5      # float32 points: off the plane by 2^-24 of their size
    assert float((ref["curvatures"][:, 0] / ref["curvatures"][:, 2]).max()) < 1e-12
    assert bool((ref["curvatures"][:, 0] <= ref["curvatures"][:, 1]).all() and (ref["curvatures"][:, 1] <= ref["curvatures"][:, 2]).all())


def test_sphere_normals_are_radial_and_rule_1_points_inward():
    pts = R.clean_sphere()[0]
    ref = R.estimate(pts, 50, orient=1)
    radial = (pts.double() / pts.double().norm(dim=1, keepdim=True)).numpy()
    angle = np.degrees(np.arcsin(np.clip(R.cross_norm(ref["normals"], radial), 0.0, 1.0)))
    assert float(angle.max()) <= 7.0, float(angle.max())                  # what 1024 points on the sphere allow at k = 50
    assert bool((np.einsum("ni,ni->n", ref["normals"], radial) < 0).all())  # every neighbour lies on the concave side
    assert int(np.abs(ref["n_pos"] - 25).min()) >= 13                     # |n_pos - k/2| >= k/4: the GPU test compares every decision
    vp = np.array([0.0, 0.0, 5.0])
    out = R.estimate(pts, 50, orient=2, viewpoint=vp)["normals"]
    assert bool((np.einsum("ni,ni->n", out, vp[None] - pts.double().numpy()) >= 0).all())
    canon = R.estimate(pts, 50, orient=0)["normals"]
    big = np.abs(canon).argmax(axis=1)
    assert bool((canon[np.arange(len(canon)), big] > 0).all())


def test_nonfinite_points_are_nobodys_neighbours():
    pts, sel = R.nonfinite_cloud()
    ref = R.estimate(pts[0], 16)
    bad = torch.zeros(300, dtype=torch.bool)
    bad[sel] = True
    assert bool((ref["idx"][bad] == -1).all()) and bool(np.isnan(ref["normals"][bad.numpy()]).all())
    assert not bool(torch.isin(ref["idx"][~bad], sel).any()) and bool(np.isfinite(ref["normals"][~bad.numpy()]).all())
    few = pts[0, :40].clone()
    few[10:] = float("nan")                                                # 10 finite points, k = 16
    assert bool((R.knn(few, 16) == -1).all())


# ---- the bounds: where they come from, and that they have teeth ----------------------------------------------------------------------
INPUTS = list(R.CASES) + ["shifted"]


def _clouds(name):
    return (R.shifted_case(), 16, "cloud") if name == "shifted" else (R.case(name), R.CASES[name][2], R.CASES[name][3])


@pytest.mark.parametrize("name", INPUTS)
def test_float32_numpy_is_an_eighth_of_the_bounds(name):
    """The derivation of NORMAL_C and CURV_BOUND: float32 covariance + LAPACK float32 eigh on the float64 restatement's
    neighbours was measured at an eighth of what the kernel is allowed (normals_ref.py); asserted here at a quarter, since
    another BLAS sums in another order.  The share of points left out of the normal comparison meets the condition on every
    input (that figure is float64 alone)."""
    pts, k, kind = _clouds(name)
    for cloud in pts:
        ref = R.estimate(cloud, k)
        f32 = R.estimate(cloud, k, idx=ref["idx"], dtype=np.float32)
        ratio, curv, left_out = R.errors(f32["normals"], f32["curvatures"], ref)
        assert ratio <= R.NORMAL_C / 4 and curv <= R.CURV_BOUND / 4, (ratio, curv)
        assert left_out <= R.MAX_LEFT_OUT[kind], left_out


@pytest.mark.parametrize("mutant", ["no_self", "k_minus_1", "about_query", "largest"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_value_mutants_lie_far_outside_the_bounds(name, mutant):
    k = R.CASES[name][2]
    cloud = R.case(name)[0]
    ref = R.case_ref(name)[0]
    mut = R.estimate(cloud, k, mutant=mutant)
    ratio, curv, _ = R.errors(mut["normals"], mut["curvatures"], ref)
    assert ratio > 1000 * R.NORMAL_C or curv > 1000 * R.CURV_BOUND, (ratio, curv)
    if mutant == "no_self":
        assert bool((mut["idx"] != ref["idx"]).any(dim=1).all())


def test_tie_mutant_changes_the_indices_of_the_tie_cloud():
    pts = R.tie_cloud()[0]
    assert len(torch.unique(pts, dim=0)) <= 140                            # 60 exact duplicates
    want, late = R.knn(pts, 16), R.knn(pts, 16, ties="latest")
    assert int((want != late).any(dim=1).sum()) > 100
    d = (pts[:, None, :] - pts[None, :, :]).pow(2).sum(-1)
    kth = torch.gather(d, 1, want[:, 15:16])
    assert int(((d == kth).sum(dim=1) > 1).sum()) > 100                    # equal distances straddle the k-th slot


def test_sign_mutant_flips_every_sphere_normal():
    pts = R.clean_sphere()[0]
    ref, mut = R.estimate(pts, 50, orient=1), R.estimate(pts, 50, orient=1, mutant="npos_gt")
    assert bool((ref["flip"] != mut["flip"]).all())
    assert bool((np.einsum("ni,ni->n", ref["normals"], mut["normals"]) < -0.999).all())


# ---- I/O ---------------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_with_normals_and_the_old_call_forms(tmp_path):
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply, save_pointcloud_ply_normals, save_pointcloud_ply_rgb
    rng = np.random.Generator(np.random.PCG64(3))
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    nrm = rng.standard_normal((37, 3)).astype(np.float32)
    save_pointcloud_ply_normals(pts, nrm, tmp_path / "a" / "n.ply")
    raw = (tmp_path / "a" / "n.ply").read_bytes()
    head = raw[:raw.index(b"end_header\n")].decode().split("\n")
    assert head[1] == "format binary_little_endian 1.0" and [l.split()[1:] for l in head if l.startswith("property")] == [
        ["float", c] for c in ("x", "y", "z", "nx", "ny", "nz")]
    p2, n2 = load_pointcloud_ply(tmp_path / "a" / "n.ply", with_normals=True)
    assert np.array_equal(p2, pts) and np.array_equal(n2, nrm) and n2.dtype == np.float32
    plain = load_pointcloud_ply(tmp_path / "a" / "n.ply")                  # old form on the new file: points alone
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, pts)
    with pytest.raises(ValueError):
        save_pointcloud_ply_normals(pts, nrm[:5], tmp_path / "bad.ply")
    # the old call forms return what they returned
    col = rng.integers(0, 256, size=(37, 3)) / 255.0
    save_pointcloud_ply(pts, tmp_path / "p.ply")
    save_pointcloud_ply(pts, tmp_path / "p_ascii.ply", binary=False)
    save_pointcloud_ply_rgb(pts, col, tmp_path / "c.ply")
    assert np.array_equal(load_pointcloud_ply(tmp_path / "p.ply"), pts)
    assert np.array_equal(load_pointcloud_ply(tmp_path / "p_ascii.ply"), pts)
    out = load_pointcloud_ply(tmp_path / "c.ply", with_colors=True)
    assert isinstance(out, tuple) and len(out) == 2 and np.array_equal(out[0], pts) and np.array_equal(out[1], col.astype(np.float32))
    assert np.array_equal(load_pointcloud_ply(tmp_path / "c.ply", True)[1], col.astype(np.float32))   # positional, as callers pass it
    with pytest.raises(ValueError):
        load_pointcloud_ply(tmp_path / "p.ply", with_normals=True)
    with pytest.raises(ValueError):
        load_pointcloud_ply(tmp_path / "p.ply", with_colors=True)


# ---- shading ---------------------------------------------------------------------------------------------------------------------
def test_shade_by_normals_against_a_hand_computation():
    from bdm_amd.cameras import OrthographicCameras, PerspectiveCameras, look_at_view_transform
    from bdm_amd.render import shade_by_normals
    g = torch.Generator().manual_seed(9)
    pts = torch.randn(2, 5, 3, generator=g) * 0.3
    nrm = torch.randn(2, 5, 3, generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    Rm, T = look_at_view_transform(dist=2.0, elev=[20.0, -35.0], azim=[40.0, 200.0])
    albedo, ambient = (0.9, 0.6, 0.3), 0.25
    for ortho in (False, True):
        cams = (OrthographicCameras if ortho else PerspectiveCameras)(focal_length=1.5, R=Rm, T=T)
        got = shade_by_normals(pts, nrm, cams, ambient=ambient, albedo=albedo)
        assert got.shape == (2, 5, 3)
        for b in range(2):
            Rb, Tb = Rm[b].double().numpy(), T[b].double().numpy()         # X_view = X_world R + T
            centre = -Tb @ Rb.T
            assert np.allclose(centre @ Rb + Tb, 0.0, atol=1e-6)
            for i in range(5):
                p, n = pts[b, i].double().numpy(), nrm[b, i].double().numpy()
                v = Rb[:, 2] if ortho else (centre - p) / np.linalg.norm(centre - p)
                want = np.array(albedo) * (ambient + (1 - ambient) * abs(float(n @ v)))
                assert np.allclose(got[b, i].numpy(), want, atol=2e-6), (ortho, b, i)
        assert torch.equal(shade_by_normals(pts, -nrm, cams, ambient=ambient, albedo=albedo), got)       # two-sided
    default = shade_by_normals(pts, nrm, [PerspectiveCameras(R=Rm[b:b + 1], T=T[b:b + 1]) for b in range(2)])   # a list of single cameras
    assert float(default.min()) >= 0.8 * 0.3 - 1e-6 and float(default.max()) <= 0.8 + 1e-6
    with pytest.raises(ValueError):
        shade_by_normals(pts, nrm, PerspectiveCameras(R=Rm[:1], T=T[:1]))


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_normals_cli_arguments():
    from bdm_amd.normals import parse_args
    a = parse_args(["--in_dir", "i", "--out_dir", "o"])
    assert (a.in_dir, a.out_dir, a.neighborhood_size, a.no_disambiguate, a.batch_size) == ("i", "o", 50, False, 16)
    a = parse_args(["--in_dir", "i", "--out_dir", "o", "--neighborhood-size", "12", "--no-disambiguate", "--batch-size", "3"])
    assert (a.neighborhood_size, a.no_disambiguate, a.batch_size) == (12, True, 3)
    for bad in (["--in_dir", "i"], ["--in_dir", "i", "--out_dir", "o", "--neighborhood-size", "2"],
                ["--in_dir", "i", "--out_dir", "o", "--neighborhood-size", "65"], ["--in_dir", "i", "--out_dir", "o", "--batch-size", "0"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_normals_cli_walks_the_tree_with_a_fake_estimator(tmp_path):
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply
    from bdm_amd.normals import process_tree
    rng = np.random.Generator(np.random.PCG64(4))
    clouds = {"a/x.ply": 30, "a/y.ply": 30, "b/c/z.ply": 30, "b/w.ply": 20, "top.ply": 30}
    pts = {rel: rng.standard_normal((n, 3)).astype(np.float32) for rel, n in clouds.items()}
    for rel, p in pts.items():
        save_pointcloud_ply(p, tmp_path / "in" / rel)
    (tmp_path / "in" / "notes.txt").write_text("not a cloud")
    calls = []

    def fake(points):
        calls.append(tuple(points.shape))
        assert points.dtype == torch.float32 and not points.is_cuda
        nrm = points / points.norm(dim=-1, keepdim=True)
        curv = torch.tensor([1.0, 2.0, 5.0]).expand(*points.shape[:2], 3).clone()
        curv[0, 0] = float("nan")                                          # a non-finite row is left out of the mean
        return nrm, curv

    res = process_tree(tmp_path / "in", tmp_path / "out", fake, batch_size=3)
    assert calls == [(1, 20, 3), (3, 30, 3), (1, 30, 3)]                   # equal point counts share a call, batch_size at most
    assert res["files"] == 5 and res["points"] == 140 and abs(res["mean_surface_variation"] - 0.125) < 1e-12
    assert json.loads(json.dumps(res)) == res
    written = sorted(str(p.relative_to(tmp_path / "out")) for p in (tmp_path / "out").rglob("*") if p.is_file())
    assert written == sorted(clouds)
    for rel, p in pts.items():
        p2, n2 = load_pointcloud_ply(tmp_path / "out" / rel, with_normals=True)
        assert np.array_equal(p2, p) and np.allclose(n2, p / np.linalg.norm(p, axis=1, keepdims=True), atol=1e-6)


def test_python_layer_refuses_bad_sizes_and_host_tensors():
    from bdm_amd import _lib
    from bdm_amd.normals import estimate_pointcloud_normals, knn_self
    pts = torch.zeros(1, 50, 3)
    with pytest.raises(ValueError, match="strictly smaller than the number of points"):
        estimate_pointcloud_normals(pts)                                    # N = 50 = the default neighbourhood
    for k in (2, 65):
        with pytest.raises(ValueError, match="outside 3..64"):
            estimate_pointcloud_normals(torch.zeros(1, 100, 3), neighborhood_size=k)
    with pytest.raises(ValueError):
        knn_self(torch.zeros(50, 3), 8)
    with pytest.raises(_lib.BdmHipError, match="CPU tensor"):
        estimate_pointcloud_normals(torch.zeros(1, 100, 3), neighborhood_size=8)


def test_main_render_accepts_none_and_normals_only(tmp_path):
    import main_render
    base = [f"run.render_sample_dir={tmp_path}"]
    cfg = main_render.parse_args(base)
    assert cfg.run.render_shading == "none" and cfg.run.render_normals_k == 50
    cfg = main_render.parse_args(base + ["run.render_shading=normals", "run.render_normals_k=16"])
    assert cfg.run.render_shading == "normals" and cfg.run.render_normals_k == 16
    assert main_render.parse_args(base + ["run.render_shading=none"]).run.render_shading == "none"
    for bad in ("phong", "Normals", ""):
        with pytest.raises(ValueError):
            main_render.parse_args(base + [f"run.render_shading={bad}"])


def test_render_tree_shades_the_uncoloured_kinds_only(tmp_path):
    """render_tree with fakes: at `normals` gt and pred get shade_fn's colours (one call per batch group), `colored` keeps its own;
    at `none`, and for a config object without the key, nothing is shaded."""
    import types

    import main_render
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_pointcloud_ply, save_pointcloud_ply_rgb
    rng = np.random.Generator(np.random.PCG64(6))
    for j in range(2):
        for kind in ("gt", "pred"):
            save_pointcloud_ply(rng.standard_normal((40, 3)).astype(np.float32), tmp_path / kind / "chair" / f"synthetic_{j:06d}.ply")
    save_pointcloud_ply_rgb(rng.standard_normal((40, 3)).astype(np.float32), np.full((40, 3), 1.0), tmp_path / "colored" / "chair" / "synthetic_000000.ply")

    def run(shading):
        seen, shaded = [], []
        run_cfg = types.SimpleNamespace(render_sample_dir=str(tmp_path), num_sample_batches=None, render_num_frames=1)
        if shading is not None:
            run_cfg.render_shading = shading

        def render_fn(cameras, points, colors):
            seen.append((points.shape[0], None if colors is None else float(colors.mean())))
            return torch.zeros(points.shape[0], 4, 4, 3)

        def shade_fn(cameras, points):
            shaded.append((len(cameras), tuple(points.shape)))
            return torch.full_like(points, 0.25)

        main_render.render_tree(types.SimpleNamespace(run=run_cfg), SyntheticShapes(range(2), 2, num_points=40), render_fn,
                                shade_fn=shade_fn)
        return seen, shaded

    assert run("normals") == ([(1, 1.0), (2, 0.25), (2, 0.25)], [(2, (2, 40, 3)), (2, (2, 40, 3))])
    assert run("none") == ([(1, 1.0), (2, None), (2, None)], [])
    assert run(None) == run("none")
    with pytest.raises(ValueError):
        run("phong")
