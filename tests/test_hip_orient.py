"""bdm_orient_normals (csrc/orient.hip) and its Python surface on the GPU against the CPU restatement tests/orient_ref.py: every
output (normals_out, votes, seen, undecided) with torch.equal, the bit-exact pins, the error paths, and the feature end to end.

Every decision of the rule is an integer, so nothing here has a tolerance.  The figures of an MI355X run (undecided points and
fallback rounds per input) are listed in DESIGN.md section 15."""
import json
import os

import numpy as np
import pytest
import torch

import orient_ref as O

pytestmark = pytest.mark.gpu
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n].view(*shape)


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _call(pts, nrm, idx, views, par, info=True, check_guards=True, **override):
    """One bdm_orient_normals call on guarded outputs -> (rc, dict of host tensors).  override: any of the integer arguments
    (b, n, k, v, r, splat, eps, kg, rounds) as the error paths pass them, alias=True (normals_out = normals_in), null=<name>."""
    from bdm_amd import _lib as L
    b, n, k, v = pts.shape[0], pts.shape[1], idx.shape[2], views.shape[0]
    a = dict(b=b, n=n, k=k, v=v, r=par["resolution"], splat=par["splat"], eps=O.eps_of(par["depth_tolerance_px"], par["resolution"]),
             kg=par["fallback_k"], rounds=par["fallback_rounds"])
    a.update({key: val for key, val in override.items() if key in a})
    dev = {"points": pts.cuda().contiguous(), "normals_in": nrm.cuda().contiguous(), "knn_idx": idx.int().cuda().contiguous(),
           "views": views.cuda().contiguous()}
    wn, vn = _guarded((b, n, 3), torch.float32)
    wv, vv = _guarded((b, n), torch.int32) if info else (None, None)
    ws_, vs = _guarded((b, n), torch.int32) if info else (None, None)
    wu, vu = _guarded((b,), torch.int32) if info else (None, None)
    lib = L.lib()
    work = torch.empty(max(1, b * n * v), dtype=torch.uint8, device="cuda")
    assert lib.bdm_orient_normals_workspace_bytes(b, n, v) == b * n * v
    ptrs = {name: L.ptr(t) for name, t in dev.items()}
    ptrs.update(normals_out=L.ptr(vn), workspace=L.ptr(work))
    if override.get("alias"):
        ptrs["normals_out"] = ptrs["normals_in"]
    if override.get("null"):
        ptrs[override["null"]] = None
    rc = lib.bdm_orient_normals(a["b"], a["n"], a["k"], a["v"], a["r"], a["splat"], a["eps"], a["kg"], a["rounds"], ptrs["points"],
                                ptrs["normals_in"], ptrs["knn_idx"], ptrs["views"], ptrs["normals_out"], L.ptr(vv), L.ptr(vs),
                                L.ptr(vu), ptrs["workspace"], L.stream())
    torch.cuda.synchronize()
    wholes = [w for w in (wn, wv, ws_, wu) if w is not None]
    if not check_guards:
        return rc, wholes
    assert all(_untouched(w) for w in wholes), "sentinel bytes around an output were overwritten"
    got = {"normals_out": vn.cpu()}
    if info:
        got.update(votes=vv.cpu(), seen=vs.cpu(), undecided=vu.cpu())
    return rc, got


def _assert_equals_restatement(name, got, refs):
    for c, ref in enumerate(refs):
        print(f"{name}[{c}]: undecided after voting {int((ref['s_vote'] == 0).sum())}, after the fallback {ref['undecided']}, "
              f"rounds run {ref['rounds_run']}, GPU undecided {int(got['undecided'][c])}")
        assert torch.equal(got["votes"][c], ref["votes"]), f"{name}[{c}]: {int((got['votes'][c] != ref['votes']).sum())} votes differ"
        assert torch.equal(got["seen"][c], ref["seen"]), f"{name}[{c}]: {int((got['seen'][c] != ref['seen']).sum())} seen counts differ"
        assert int(got["undecided"][c]) == ref["undecided"]
        assert O.same_bits(got["normals_out"][c], ref["normals_out"]), f"{name}[{c}]: normals differ"


@pytest.mark.parametrize("name", list(O.CASES))
def test_cases_against_the_restatement(hip, name):
    inputs = O.case_inputs(name)
    rc, got = _call(*inputs)
    assert rc == 0
    _assert_equals_restatement(name, got, O.case_ref(name))


def test_largest_configuration_size(hip):
    """(1, 16384, 3): normals and neighbour lists from the GPU estimator (tested on its own), the orientation against the restatement."""
    from bdm_amd.normals import estimate_pointcloud_normals, knn_self
    name, make, k, par = O.LARGE_CASE
    pts = make()
    nrm, idx = estimate_pointcloud_normals(pts.cuda(), k, False).cpu(), knn_self(pts.cuda(), k).cpu()
    views = O.default_views(par["num_views"])
    rc, got = _call(pts, nrm, idx, views, par)
    assert rc == 0
    _assert_equals_restatement(name, got, O.orient_batch(pts, nrm, idx, views, par))
    assert int((got["seen"] > 0).sum()) > 16000


# ---- bit-exact pins -------------------------------------------------------------------------------------------------------------------
def test_batch_rows_equal_single_calls_and_calls_repeat(hip):
    pts, nrm, idx, views, par = O.case_inputs("b3_n1025_ellipsoids")
    _, whole = _call(pts, nrm, idx, views, par)
    _, again = _call(pts, nrm, idx, views, par)
    for key in whole:
        assert O.same_bits(again[key], whole[key]) if key == "normals_out" else torch.equal(again[key], whole[key])
    for c in (2, 0, 1):
        _, one = _call(pts[c:c + 1], nrm[c:c + 1], idx[c:c + 1], views, par)
        assert O.same_bits(one["normals_out"][0], whole["normals_out"][c]) and int(one["undecided"][0]) == int(whole["undecided"][c])
        assert torch.equal(one["votes"][0], whole["votes"][c]) and torch.equal(one["seen"][0], whole["seen"][c])
    _, bare = _call(pts, nrm, idx, views, par, info=False)                       # votes, seen, undecided are optional
    assert O.same_bits(bare["normals_out"], whole["normals_out"])


def test_sign_flips_of_the_input_and_a_second_pass(hip):
    pts, nrm, idx, views, par = O.case_inputs("b1_n1024_slab")
    ref = O.case_ref("b1_n1024_slab")[0]
    _, got = _call(pts, nrm, idx, views, par)
    flip = torch.rand(pts.shape[1], generator=torch.Generator().manual_seed(3104)) < 0.5
    flipped = torch.where(flip[:, None], -nrm[0], nrm[0])[None]
    _, other = _call(pts, flipped, idx, views, par)
    decided = ref["s"] != 0
    assert 0 < int((~decided).sum()) < 50 and int(other["undecided"][0]) == int((~decided).sum())
    assert O.same_bits(other["normals_out"][0][decided], got["normals_out"][0][decided])
    assert O.same_bits(other["normals_out"][0][~decided], flipped[0][~decided])
    assert torch.equal(other["votes"][0].abs(), got["votes"][0].abs()) and torch.equal(other["seen"], got["seen"])
    _, twice = _call(pts, got["normals_out"], idx, views, par)                   # orienting the output again returns it
    assert O.same_bits(twice["normals_out"], got["normals_out"])


def test_true_and_false_keep_their_bits(hip):
    from bdm_amd import _lib as L
    from bdm_amd.normals import estimate_pointcloud_normals
    pts = O.case_inputs("b3_n1025_ellipsoids")[0].cuda()
    for flag, orient in ((True, 1), (False, 0), (1, 1), (0, 0)):
        direct = torch.empty_like(pts)
        assert L.lib().bdm_estimate_normals(3, 1025, 16, orient, L.ptr(pts), None, None, L.ptr(direct), None, None, L.stream()) == 0
        assert O.same_bits(estimate_pointcloud_normals(pts, 16, flag).cpu(), direct.cpu())


# ---- through the public interface -----------------------------------------------------------------------------------------------------
def test_visibility_points_outwards_on_a_sphere(hip):
    from bdm_amd.normals import estimate_pointcloud_normals
    pts, truth = O.sphere(torch.Generator().manual_seed(3100), 1024)
    out = estimate_pointcloud_normals(pts[None].cuda(), 16, "visibility")
    assert out.shape == (1, 1024, 3) and out.is_cuda
    assert O.wrong_share(out[0].cpu(), truth, well=None) == (0, 1024)
    inward = estimate_pointcloud_normals(pts[None].cuda(), 16, True)            # the neighbour-majority rule points inwards here
    assert O.wrong_share(inward[0].cpu(), truth, well=None) == (1024, 1024)
    assert O.same_bits(out.abs().cpu(), inward.abs().cpu())
    both, curv = estimate_pointcloud_normals(pts[None].cuda(), 16, "visibility", return_curvatures=True)
    assert O.same_bits(both.cpu(), out.cpu()) and curv.shape == (1, 1024, 3)


def test_thin_table_through_the_api(hip):
    from bdm_amd.normals import estimate_pointcloud_normals, knn_self, orient_normals_by_visibility
    pts, truth = O.table(torch.Generator().manual_seed(3103), 4000)
    dev = pts[None].cuda()
    got = estimate_pointcloud_normals(dev, 16, "visibility").cpu()
    canonical, idx = estimate_pointcloud_normals(dev, 16, False), knn_self(dev, 16)
    ref = O.orient_batch(pts[None], canonical.cpu(), idx.cpu(), O.default_views(32), O.DEFAULTS)[0]
    assert O.same_bits(got[0], ref["normals_out"])
    wrong, counted = O.wrong_share(got[0], truth, canonical[0].cpu())
    print(f"thin table on the GPU: {wrong} of {counted} well-estimated normals wrong, {ref['undecided']} undecided, {ref['rounds_run']} rounds")
    assert counted > 3000 and wrong <= 0.05 * counted
    out, info = orient_normals_by_visibility(dev, canonical, idx, return_info=True)
    assert O.same_bits(out.cpu(), got) and torch.equal(info["votes"][0].cpu(), ref["votes"]) and torch.equal(info["seen"][0].cpu(), ref["seen"])
    assert info["undecided"].tolist() == [ref["undecided"]]
    own = orient_normals_by_visibility(dev, canonical)                           # neighbour lists looked up by the function: k = 16
    assert O.same_bits(own.cpu(), got)
    few = orient_normals_by_visibility(dev, canonical, idx, num_views=4, resolution=64, splat=1, depth_tolerance_px=1.0, fallback_k=4,
                                       fallback_rounds=2, return_info=True)
    want = O.orient(pts, canonical[0].cpu(), idx[0].cpu(), O.default_views(4), 64, 1, 1024, 4, 2)
    assert O.same_bits(few[0][0].cpu(), want["normals_out"]) and int(few[1]["undecided"][0]) == want["undecided"]


def test_command_line_orients_by_visibility(hip, tmp_path, capsys):
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply
    from bdm_amd.normals import main
    g = torch.Generator().manual_seed(3108)
    clouds = {"a/s0.ply": O.sphere(g, 1000), "a/b/s1.ply": O.sphere(g, 1000), "t.ply": O.two_spheres(g, 600)}
    for rel, (p, _) in clouds.items():
        save_pointcloud_ply(p.numpy(), tmp_path / "in" / rel)
    res = main(["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--neighborhood-size", "12", "--orient", "visibility"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["files"] == 3 and res["points"] == 2600
    assert 0.0 <= res["undecided_fraction"] < 0.05
    for rel, (p, truth) in clouds.items():
        p2, nrm = load_pointcloud_ply(tmp_path / "out" / rel, with_normals=True)
        assert np.array_equal(p2, p.numpy())
        wrong, counted = O.wrong_share(nrm, truth, well=None)
        assert counted == p.shape[0] and wrong == 0                              # closed, densely sampled surfaces: all outward
    res1 = main(["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out1"), "--neighborhood-size", "12"])
    assert "undecided_fraction" not in res1
    capsys.readouterr()


def test_one_sided_shading_on_the_device(hip):
    from bdm_amd.cameras import PerspectiveCameras, look_at_view_transform
    from bdm_amd.render import shade_by_normals
    g = torch.Generator().manual_seed(3107)
    pts = torch.randn(2, 40, 3, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(2, 40, 3, generator=g), dim=-1)
    Rm, T = look_at_view_transform(dist=3.0, elev=[10.0, 50.0], azim=[0.0, 120.0], degrees=True)
    v = -torch.bmm(T[:, None, :], Rm.transpose(1, 2)) - pts
    cos = (nrm * (v / v.norm(dim=-1, keepdim=True))).sum(-1, keepdim=True)
    want = torch.tensor([0.8, 0.8, 0.8]) * (0.3 + 0.7 * cos.clamp_min(0.0))
    got = shade_by_normals(pts.cuda(), nrm.cuda(), PerspectiveCameras(R=Rm, T=T, device="cuda"), two_sided=False)
    assert got.is_cuda and float((got.cpu() - want).abs().max()) < 1e-5


def test_main_render_oriented_and_normals(hip, tmp_path):
    """run.render_shading=oriented writes its pictures, lit one-sided; run.render_shading=normals writes the bytes the renderer gives
    for two-sided shading by the neighbour-majority normals, as before."""
    import main_render
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_image_png, save_pointcloud_ply
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.render import render_pointcloud_batch_pytorch3d, shade_by_normals
    from PIL import Image
    batch = next(iter(SyntheticShapes(range(2), 2, seed=42, image_size=224, num_points=1024)))
    names = [f"synthetic_{j:06d}" for j in range(2)]
    common = ["dataset=synthetic", "dataset.max_points=1024", "dataset.num_shapes=2", "dataloader.batch_size=2", "run.render_normals_k=16"]
    bg = np.array([200, 200, 200], dtype=np.uint8)
    roots = {}
    for shading in ("oriented", "normals"):
        roots[shading] = tmp_path / shading
        for j, name in enumerate(names):
            save_pointcloud_ply(batch.sequence_point_cloud[j].numpy(), roots[shading] / "pred" / "chair" / f"{name}.ply")
        main_render.main([f"run.render_sample_dir={roots[shading]}", "run.render_num_frames=2", f"run.render_shading={shading}"] + common)
        assert sorted(os.listdir(roots[shading] / "renders" / "orbit" / "chair")) == [f"{n}-{f}.png" for n in names for f in range(2)]
    for j, name in enumerate(names):
        pts = batch.sequence_point_cloud[j:j + 1].cuda()
        cam = [batch.camera[j].to("cuda")]
        for shading, flag, two_sided in (("normals", True, True), ("oriented", "visibility", False)):
            colours = shade_by_normals(pts, estimate_pointcloud_normals(pts, 16, flag), cam, two_sided=two_sided)
            direct = render_pointcloud_batch_pytorch3d(cam, Pointclouds(pts, colours))
            save_image_png(direct[0].cpu().permute(2, 0, 1).numpy(), tmp_path / "direct.png")
            assert (roots[shading] / "renders" / "pred" / "chair" / f"{name}.png").read_bytes() == (tmp_path / "direct.png").read_bytes()
        lit = np.asarray(Image.open(roots["oriented"] / "renders" / "pred" / "chair" / f"{name}.png"))
        fg = (lit != bg).any(axis=-1)
        levels = np.unique(lit[fg], axis=0)
        assert int(fg.sum()) > 50 and len(levels) > 2 and bool((levels[:, 0] == levels[:, 1]).all() and (levels[:, 1] == levels[:, 2]).all())
        assert int(lit[fg].max()) <= int(0.8 * 255) + 1


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    inputs = O.case_inputs("b2_n300_nonfinite")
    lib = L.lib()
    bad = {"b < 0": dict(b=-1), "n = 0": dict(n=0), "n = 32769": dict(n=32769), "k = 0": dict(k=0, kg=0), "b n k = 2^31": dict(b=4096, n=32768, k=16),
           "v = 0": dict(v=0), "v = 257": dict(v=257), "r = 0": dict(r=0), "r = 129": dict(r=129), "splat = -1": dict(splat=-1),
           "splat = 5": dict(splat=5), "eps = -1": dict(eps=-1), "eps = 65536": dict(eps=65536), "kg = 0": dict(kg=0), "kg = k + 1": dict(kg=17),
           "rounds = -1": dict(rounds=-1), "rounds = 33": dict(rounds=33), "alias": dict(alias=True), "no points": dict(null="points"),
           "no normals": dict(null="normals_in"), "no lists": dict(null="knn_idx"), "no views": dict(null="views"),
           "no output": dict(null="normals_out"), "no workspace": dict(null="workspace")}
    for what, kw in bad.items():
        rc, wholes = _call(*inputs, check_guards=False, **kw)
        assert rc == 1, what
        assert all(_untouched(w, body=True) for w in wholes), what
        assert lib.bdm_last_error(), what
    assert lib.bdm_orient_normals(0, 300, 16, 32, 128, 2, 1024, 8, 8, None, None, None, None, None, None, None, None, None, L.stream()) == 0
    assert lib.bdm_orient_normals_workspace_bytes(16, 16384, 32) == 16 * 16384 * 32
    for b, n, v in ((-1, 300, 32), (2, 0, 32), (2, 32769, 32), (2, 300, 0), (2, 300, 257)):
        assert lib.bdm_orient_normals_workspace_bytes(b, n, v) == 0
    assert not hasattr(lib, "bdm_orient_normals_variant")                       # one kernel form: there is no variant to pin
