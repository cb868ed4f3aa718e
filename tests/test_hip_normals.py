"""bdm_estimate_normals (csrc/normals.hip) and bdm_amd/normals.py on the GPU against the CPU restatement tests/normals_ref.py:
the neighbour indices bit for bit, curvatures and normals inside the bounds derived there (8 x what a float32 numpy restatement
shows against float64), the sign rules, the invariances with torch.equal, the error paths, and the feature end to end.

Measured on an MI355X: worst |n x n_ref| (l1 - l0) / (l2 u) = 2.85 (bound 19.4), worst curvature error
3.51e-7 l2 (bound 2.49e-6); every figure is printed by _assert_within_bounds and listed in the run's parity lines."""
import json
import os

import numpy as np
import pytest
import torch

import helpers
import normals_ref as R

pytestmark = pytest.mark.gpu
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5


def _guarded(shape, dtype):
    """A device buffer of `shape` with PAD sentinel elements on either side, everything sentinel-filled: (whole, view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n].view(*shape)


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _call(pts, k, orient=0, viewpoints=None, idx=True, curv=True, n=None, check_guards=True):
    """One bdm_estimate_normals call on guarded outputs -> (rc, idx int64 or None, normals, curvatures or None) on the host, and
    the guarded buffers when check_guards=False (error paths look at the bodies as well)."""
    from bdm_amd import _lib as L
    b, n_pts = pts.shape[0], pts.shape[1] if n is None else n
    dev = pts.cuda().contiguous()
    vp = None if viewpoints is None else torch.as_tensor(viewpoints, dtype=torch.float32).reshape(-1, 3).expand(b, 3).contiguous().cuda()
    wi, vi = _guarded((b, n_pts, k), torch.int32) if idx else (None, None)
    wn, vn = _guarded((b, n_pts, 3), torch.float32)
    wc, vc = _guarded((b, n_pts, 3), torch.float32) if curv else (None, None)
    rc = L.lib().bdm_estimate_normals(b, n_pts, k, orient, L.ptr(dev), L.ptr(vp), L.ptr(vi), L.ptr(vn), L.ptr(vc), None, L.stream())
    torch.cuda.synchronize()
    if not check_guards:
        return rc, [w for w in (wi, wn, wc) if w is not None]
    for w in (wi, wn, wc):
        assert w is None or _untouched(w), "sentinel bytes around an output were overwritten"
    return rc, (None if vi is None else vi.cpu().long()), vn.cpu(), (None if vc is None else vc.cpu())


def _assert_within_bounds(name, kind, normals, curvatures, ref):
    ratio, curv, left_out = R.errors(normals.numpy(), curvatures.numpy(), ref)
    print(f"{name}: |n x n_ref| gap / u = {ratio:.2f} (bound {R.NORMAL_C:.1f}), curvature error = {curv:.3g} l2 "
          f"(bound {R.CURV_BOUND:.3g}), left out {left_out:.4f}")
    helpers.parity(f"normals {name} |n x ref| gap/u", ratio, R.NORMAL_C)
    helpers.parity(f"normals {name} curvature / l2", curv, R.CURV_BOUND)
    assert left_out <= R.MAX_LEFT_OUT[kind], left_out
    assert curv <= R.CURV_BOUND, curv
    assert ratio <= R.NORMAL_C, ratio
    unit = np.abs(np.linalg.norm(normals.double().numpy(), axis=1) - 1.0)
    assert float(np.nanmax(unit)) < 1e-6


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_against_the_restatement(hip, name):
    b, n, k, kind, _ = R.CASES[name]
    pts, refs = R.case(name), R.case_ref(name)
    rc, idx, normals, curv = _call(pts, k)
    assert rc == 0
    for c in range(b):
        bad = (idx[c] != refs[c]["idx"]).any(dim=1)
        assert torch.equal(idx[c], refs[c]["idx"]), f"{name}[{c}]: {int(bad.sum())} of {n} rows differ, first {torch.nonzero(bad)[:3].tolist()}"
        _assert_within_bounds(f"{name}[{c}]", kind, normals[c], curv[c], refs[c])
        assert bool((curv[c][:, 0] <= curv[c][:, 1]).all() and (curv[c][:, 1] <= curv[c][:, 2]).all())
        canon = normals[c].numpy()                                          # orient = 0: the canonical sign
        assert bool((canon[np.arange(n), np.abs(canon).argmax(axis=1)] > 0).all())


def test_ties_follow_the_point_index(hip):
    pts = R.tie_cloud()
    want = R.knn(pts[0], 16)
    rc, idx, normals, curv = _call(pts, 16)
    assert rc == 0 and torch.equal(idx[0], want)
    assert not torch.equal(idx[0], R.knn(pts[0], 16, ties="latest"))
    assert bool(torch.isfinite(normals).all() and torch.isfinite(curv).all())


def test_nonfinite_points(hip):
    pts, sel = R.nonfinite_cloud()
    ref = R.estimate(pts[0], 16)
    rc, idx, normals, curv = _call(pts, 16)
    assert rc == 0 and torch.equal(idx[0], ref["idx"])
    assert bool((idx[0][sel] == -1).all() and torch.isnan(normals[0][sel]).all() and torch.isnan(curv[0][sel]).all())
    keep = torch.ones(300, dtype=torch.bool)
    keep[sel] = False
    assert bool(torch.isfinite(normals[0][keep]).all() and torch.isfinite(curv[0][keep]).all())
    _assert_within_bounds("nonfinite", "blob", normals[0], curv[0], ref)
    few = pts[:, :40].clone()
    few[0, 10:] = float("nan")                                              # 10 finite points of 40, k = 16
    rc, idx, normals, curv = _call(few, 16)
    assert rc == 0 and bool((idx == -1).all() and torch.isnan(normals).all() and torch.isnan(curv).all())


def test_translation(hip):
    """A kernel that forms raw second moments loses the digits the shift takes; differences about the mean do not."""
    pts = R.shifted_case()
    rc, idx, normals, curv = _call(pts, 16)
    assert rc == 0
    for c in range(2):
        ref = R.estimate(pts[c], 16)
        assert torch.equal(idx[c], ref["idx"])
        _assert_within_bounds(f"shifted[{c}]", "cloud", normals[c], curv[c], ref)


def test_orientation_rules(hip):
    pts = R.clean_sphere()
    p64 = pts[0].double().numpy()
    ref = R.estimate(pts[0], 50, orient=1)
    assert int(np.abs(ref["n_pos"] - 25).min()) >= 13                      # no decision is close: none is left out
    rc, _, normals, _ = _call(pts, 50, orient=1)
    assert rc == 0
    agree = np.einsum("ni,ni->n", normals[0].double().numpy(), ref["normals"])
    assert bool((agree > 0.999).all()), int((agree <= 0.999).sum())         # every flip decision equals the restatement's
    assert bool((np.einsum("ni,ni->n", normals[0].double().numpy(), p64) < 0).all())   # inward on a sphere
    for vp in ((0.0, 0.0, 5.0), (0.1, -0.05, 0.02)):                         # outside and inside the sphere
        rc, _, out, _ = _call(pts, 50, orient=2, viewpoints=vp)
        assert rc == 0
        to_vp = np.asarray(vp)[None] - p64
        clear = np.abs(np.einsum("ni,ni->n", ref["raw"], to_vp)) > 1e-6
        assert clear.mean() > 0.99
        assert bool((np.einsum("ni,ni->n", out[0].double().numpy(), to_vp)[clear] >= 0).all())
        assert float(R.cross_norm(out[0].numpy(), ref["normals"]).max()) < 1e-4
    two = torch.cat([pts, pts])                                             # one viewpoint per cloud
    rc, _, out, _ = _call(two, 50, orient=2, viewpoints=torch.tensor([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]]))
    side = out[0].abs()[:, 2] > 0.1                                         # 5 |n_z| decides the sign there
    assert rc == 0 and bool((out[0][side][:, 2] * out[1][side][:, 2] < 0).all()) and torch.equal(out[0].abs(), out[1].abs())


def test_determinism_and_optional_outputs(hip):
    name = "b3_n1025_k3_blob"
    pts, k = R.case(name), 3
    rc, idx, normals, curv = _call(pts, k, orient=1)
    assert rc == 0
    again = _call(pts, k, orient=1)
    assert torch.equal(again[1], idx) and torch.equal(again[2], normals) and torch.equal(again[3], curv)
    for c in range(3):
        _, i1, n1, c1 = _call(pts[c:c + 1], k, orient=1)
        assert torch.equal(i1[0], idx[c]) and torch.equal(n1[0], normals[c]) and torch.equal(c1[0], curv[c])
    _, none_idx, n2, c2 = _call(pts, k, orient=1, idx=False)
    assert none_idx is None and torch.equal(n2, normals) and torch.equal(c2, curv)
    _, i3, n3, none_curv = _call(pts, k, orient=1, curv=False)
    assert none_curv is None and torch.equal(i3, idx) and torch.equal(n3, normals)
    _, _, n4, _ = _call(pts, k, orient=1, idx=False, curv=False)
    assert torch.equal(n4, normals)
    pts16 = R.case("b2_n300_k16_cloud")                                     # another k, another batch size
    _, i5, n5, c5 = _call(pts16, 16)
    _, i6, n6, c6 = _call(pts16[1:], 16)
    assert torch.equal(i6[0], i5[1]) and torch.equal(n6[0], n5[1]) and torch.equal(c6[0], c5[1])


def test_error_paths_launch_nothing(hip):
    from bdm_amd import _lib as L
    pts = R.case("b2_n300_k16_cloud")
    vp = (0.0, 0.0, 5.0)
    for what, kw in {"k = 2": dict(k=2), "k = 65": dict(k=65), "n = k": dict(k=16, n=16), "orient = 3": dict(k=16, orient=3),
                     "viewpoints at orient 0": dict(k=16, orient=0, viewpoints=vp), "viewpoints at orient 1": dict(k=16, orient=1, viewpoints=vp),
                     "no viewpoints at orient 2": dict(k=16, orient=2)}.items():
        rc, buffers = _call(pts, check_guards=False, **kw)
        assert rc == 1, what
        assert all(_untouched(w, body=True) for w in buffers), what
        assert L.lib().bdm_last_error()
    assert L.lib().bdm_estimate_normals(0, 300, 16, 0, None, None, None, None, None, None, L.stream()) == 0   # b = 0: nothing to do
    assert L.lib().bdm_estimate_normals_workspace_bytes(16, 4096, 50) >= 0
    from bdm_amd.normals import estimate_pointcloud_normals
    with pytest.raises(ValueError, match="strictly smaller than the number of points"):
        estimate_pointcloud_normals(pts[:, :50].cuda())
    with pytest.raises(ValueError, match="outside 3..64"):
        estimate_pointcloud_normals(pts.cuda(), neighborhood_size=65)
    with pytest.raises(ValueError, match="outside 3..64"):
        estimate_pointcloud_normals(pts.cuda(), neighborhood_size=2)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_public_api(hip):
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.normals import estimate_pointcloud_normals, knn_self
    pts = R.clean_sphere()
    ref = R.estimate(pts[0], 50, orient=1)
    out = estimate_pointcloud_normals(Pointclouds(pts.cuda()))               # pytorch3d's defaults: k = 50, rule 1
    assert out.shape == (1, 1024, 3) and out.is_cuda
    assert bool((np.einsum("ni,ni->n", out[0].cpu().double().numpy(), ref["normals"]) > 0.999).all())
    n2, curv = estimate_pointcloud_normals(pts.cuda(), 50, True, use_symeig_workaround=False, return_curvatures=True)
    assert torch.equal(n2, out) and curv.shape == (1, 1024, 3)
    _assert_within_bounds("api sphere", "sphere", n2[0].cpu(), curv[0].cpu(), ref)
    canon = estimate_pointcloud_normals(pts.cuda(), 50, False)
    assert torch.equal(canon.abs(), out.abs()) and not torch.equal(canon, out)
    toward = estimate_pointcloud_normals(pts.cuda(), 50, viewpoint=(0.0, 0.0, 0.0))
    assert torch.equal(toward, out)                                         # towards the centre = inward = rule 1 on a sphere
    idx = knn_self(pts.cuda(), 50)
    assert idx.dtype == torch.int64 and torch.equal(idx[0].cpu(), ref["idx"])
    assert torch.equal(knn_self(R.tie_cloud().cuda(), 16)[0].cpu(), R.knn(R.tie_cloud()[0], 16))


def test_command_line_writes_normals(hip, tmp_path, capsys):
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply
    from bdm_amd.normals import main
    g = torch.Generator().manual_seed(11)
    clouds = {"a/s0.ply": R.sphere(g, 300), "a/b/s1.ply": R.sphere(g, 300), "t.ply": R.torus(g, 200)}
    for rel, p in clouds.items():
        save_pointcloud_ply(p.numpy(), tmp_path / "in" / rel)
    res = main(["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--neighborhood-size", "12", "--batch-size", "4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["files"] == 3 and res["points"] == 800
    lam = np.concatenate([R.estimate(p, 12)["curvatures"] for p in clouds.values()])
    assert abs(res["mean_surface_variation"] - float((lam[:, 0] / lam.sum(axis=1)).mean())) < 1e-5
    for rel, p in clouds.items():
        p2, nrm = load_pointcloud_ply(tmp_path / "out" / rel, with_normals=True)
        assert np.array_equal(p2, p.numpy())
        assert float(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max()) < 1e-6
        want = R.estimate(p, 12, orient=1)["normals"]
        assert float(R.cross_norm(nrm, want).max()) < 1e-3


def test_main_render_shades_on_request_only(hip, tmp_path):
    """main_render.main on a synthetic sample directory, twice: with run.render_shading=normals the `pred` render shows grey levels;
    with the default it is the file the renderer writes for a cloud without features, every foreground pixel black."""
    import main_render
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_image_png, save_pointcloud_ply
    from bdm_amd.render import render_pointcloud_batch_pytorch3d
    from PIL import Image
    batch = next(iter(SyntheticShapes(range(2), 2, seed=42, image_size=224, num_points=1024)))
    names = [f"synthetic_{j:06d}" for j in range(2)]
    assert list(batch.sequence_name) == names
    common = ["dataset=synthetic", "dataset.max_points=1024", "dataset.num_shapes=2", "dataloader.batch_size=2"]
    bg = np.array([200, 200, 200], dtype=np.uint8)
    pngs = {}
    for shading in ("normals", "none"):
        root = tmp_path / shading
        for j, name in enumerate(names):
            for kind in ("gt", "pred"):
                save_pointcloud_ply(batch.sequence_point_cloud[j].numpy(), root / kind / "chair" / f"{name}.ply")
        main_render.main([f"run.render_sample_dir={root}", "run.render_num_frames=2"] + common
                         + ([] if shading == "none" else ["run.render_shading=normals", "run.render_normals_k=16"]))
        assert sorted(os.listdir(root / "renders" / "orbit" / "chair")) == [f"{n}-{f}.png" for n in names for f in range(2)]
        pngs[shading] = root / "renders"
    for j, name in enumerate(names):
        plain = np.asarray(Image.open(pngs["none"] / "pred" / "chair" / f"{name}.png"))
        fg = (plain != bg).any(axis=-1)
        assert int(fg.sum()) > 50 and bool((plain[fg] == 0).all())          # black silhouettes, as before
        direct = render_pointcloud_batch_pytorch3d([batch.camera[j].to("cuda")], Pointclouds(batch.sequence_point_cloud[j:j + 1].cuda(), None))
        save_image_png(direct[0].cpu().permute(2, 0, 1).numpy(), tmp_path / "direct.png")
        assert (pngs["none"] / "pred" / "chair" / f"{name}.png").read_bytes() == (tmp_path / "direct.png").read_bytes()
        for kind, stem in (("gt", name), ("pred", name), ("orbit", f"{name}-1")):
            shaded = np.asarray(Image.open(pngs["normals"] / kind / "chair" / f"{stem}.png"))
            base = np.asarray(Image.open(pngs["none"] / kind / "chair" / f"{stem}.png"))
            sfg = (base != bg).any(axis=-1)                                  # the same pixels are covered
            assert int(sfg.sum()) > 50 and bool((shaded[~sfg] == bg).all())
            levels = np.unique(shaded[sfg], axis=0)
            assert len(levels) > 2 and bool((levels[:, 0] == levels[:, 1]).all() and (levels[:, 1] == levels[:, 2]).all())
            assert int(shaded[sfg].min()) >= int(0.8 * 0.3 * 255) - 1 and int(shaded[sfg].max()) <= int(0.8 * 255) + 1
