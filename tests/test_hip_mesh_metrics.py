"""bdm_mesh_sample_points and bdm_point_mesh_distance (csrc/mesh_metrics.hip) and their Python surface on the GPU against the CPU
restatement tests/mesh_metrics_ref.py: every output with torch.equal, floats compared as bits, in every case; the pins of the launch
path, the error paths, and the feature end to end.

Every float operation of the rule is rounded on its own and every sum that decides something is an integer sum, so nothing here has a
tolerance except the end-to-end distance of samples to their own mesh, which is bounded by the host test's measured float32 gap."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_metrics_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
SAMPLE_OUTPUTS = ("points", "face_idx", "normals")
DIST_OUTPUTS = ("sqdist", "face_idx")


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _inputs(verts_list, faces_list):
    """Device and host arrays of a batch in the ABI's form; an empty side still gets one (unread) row: no NULL among the inputs.
    Indices beyond int32 become -1 (what bdm_amd.mesh_metrics does): invalid under the rule either way."""
    nv, nf = [v.shape[0] for v in verts_list], [f.shape[0] for f in faces_list]
    verts = torch.cat(verts_list).float().cuda() if sum(nv) else torch.zeros(1, 3, device="cuda")
    faces = torch.cat([torch.where((f >= 0) & (f < 2 ** 31), f, -1) for f in faces_list]).int().cuda() if sum(nf) else \
        torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    return {"b": len(nv), "verts": verts.contiguous(), "faces": faces.contiguous(), "vert_first": torch.tensor([0] + nv).cumsum(0),
            "face_first": torch.tensor([0] + nf).cumsum(0), "sum_f": sum(nf), "max_f": max(nf) if nf else 0}


def _keys(keys):
    return torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in keys], dtype=torch.int64).cuda()


def _call_sample(c, outputs=SAMPLE_OUTPUTS, expect=0):
    """One ABI call on guarded outputs and a workspace pre-filled with 0xA5 -> the dict of mesh_metrics_ref.sample_batch (host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    a = _inputs(c["verts"], c["faces"])
    B, S = a["b"], c["S"]
    nbytes = lib.bdm_mesh_sample_workspace_bytes(B, a["sum_f"], a["max_f"])
    assert nbytes >= 12 * a["sum_f"]
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    shapes = {"points": ((B, S, 3), torch.float32), "face_idx": ((B, S), torch.int32), "normals": ((B, S, 3), torch.float32)}
    bufs = {k: _guarded(int(np.prod(s)), dt) for k, (s, dt) in shapes.items()}
    keys = _keys(c["keys"])
    ptr = lambda k: L.ptr(bufs[k][1]) if k in outputs else None   # noqa: E731
    rc = lib.bdm_mesh_sample_points(B, S, a["max_f"], L.ptr(a["verts"]), L.ptr(a["faces"]), a["vert_first"].data_ptr(), a["face_first"].data_ptr(),
                                    L.ptr(keys), c["draw"], M.MESH_PURPOSE, ptr("points"), ptr("face_idx"), ptr("normals"), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(whole, body=k not in outputs) for k, (whole, _) in bufs.items()), "sentinels around (or a NULL) output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    return {k: bufs[k][1].view(shapes[k][0]).cpu() for k in outputs}


def _call_dist(c, form=0, order=None, expect=0):
    """One ABI call on guarded outputs and a workspace pre-filled with 0xA5 -> the dict of mesh_metrics_ref.distance_batch (host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    a = _inputs(c["verts"], c["faces"])
    B, P = c["points"].shape[:2]
    nbytes = lib.bdm_point_mesh_distance_workspace_bytes(B, a["sum_f"])
    assert nbytes >= 64 * a["sum_f"]
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {"sqdist": _guarded(B * P, torch.float32), "face_idx": _guarded(B * P, torch.int32)}
    pts = c["points"].cuda().contiguous()
    order = None if order is None else order.int().cuda().contiguous()
    rc = lib.bdm_point_mesh_distance(B, P, form, L.ptr(a["verts"]), L.ptr(a["faces"]), a["vert_first"].data_ptr(), a["face_first"].data_ptr(),
                                     L.ptr(pts), L.ptr(order), L.ptr(bufs["sqdist"][1]), L.ptr(bufs["face_idx"][1]), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(whole, body=expect != 0) for whole, _ in bufs.values()), "sentinels around an output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    return {k: bufs[k][1].view(B, P).cpu() for k in DIST_OUTPUTS}


def _assert_equal(name, got, want, keys=None):
    for k in (keys or got):
        gb, wb = M.bits(got[k]), M.bits(want[k])
        bad = gb != wb
        assert torch.equal(gb, wb), f"{name}: {k} differs at {int(bad.sum())} of {gb.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.SAMPLE_CASES)
def test_sample_cases_equal_the_restatement(hip, name):
    c, want = M.sample_case(name), M.sample_ref(name)
    got = _call_sample(c)
    print(f"{name}: {int((want['face_idx'] >= 0).sum())} samples on {sum(f.shape[0] for f in c['faces'])} faces")
    _assert_equal(name, got, want)


def test_sample_rows_equal_single_calls_and_calls_repeat(hip):
    c = M.sample_case("batch3")
    whole, again = _call_sample(c), _call_sample(c)
    _assert_equal("repeat", again, whole)
    for j in (2, 0, 1):
        alone = dict(c, verts=c["verts"][j:j + 1], faces=c["faces"][j:j + 1], keys=c["keys"][j:j + 1])
        _assert_equal(f"mesh {j} alone", _call_sample(alone), {k: whole[k][j:j + 1] for k in SAMPLE_OUTPUTS})


def test_sample_optional_outputs_may_be_null(hip):
    c = M.sample_case("degenerate")
    full = _call_sample(c)
    for kept in (("points",), ("points", "face_idx"), ("points", "normals")):
        _assert_equal(f"only {kept}", _call_sample(c, outputs=kept), full, kept)


def test_sample_indices_beyond_the_last_full_workgroup_of_2_31(hip):
    """S = 2^31 - 1 samples of one mesh (25.8 GB of points, no optional outputs): the last workgroup's thread indices pass 2^31 - 1, so
    a 32-bit index would wrap to a negative sample number and write before the buffer.  The tail of the output equals the
    restatement and the sentinels on both sides of the buffer stand."""
    from bdm_amd import _lib as L
    lib = L.lib()
    S, tail = 2 ** 31 - 1, 300
    verts, faces = M.box_mesh(1.0, 2.0, 3.0)
    a = _inputs([verts], [faces])
    key = M.sample_keys(1, 6)
    try:
        whole = torch.empty(3 * S + 2 * PAD, dtype=torch.float32, device="cuda")
    except torch.OutOfMemoryError:
        pytest.skip("needs 26 GB of free device memory")
    whole[:PAD], whole[-PAD:] = F_SENTINEL, F_SENTINEL
    body = whole[PAD:PAD + 3 * S]
    ws = torch.full((lib.bdm_mesh_sample_workspace_bytes(1, 12, 12) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.bdm_mesh_sample_points(1, S, 12, L.ptr(a["verts"]), L.ptr(a["faces"]), a["vert_first"].data_ptr(), a["face_first"].data_ptr(),
                                    L.ptr(_keys(key)), 2, M.MESH_PURPOSE, L.ptr(body), None, None, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert _untouched(whole) and bool((ws[-256:] == 0xA5).all())
    want, _, _ = M.sample_mesh(verts, faces, tail, key[0], draw=2, first=S - tail)
    head, _, _ = M.sample_mesh(verts, faces, tail, key[0], draw=2)
    assert torch.equal(M.bits(body[-3 * tail:].cpu().view(tail, 3)), M.bits(want))
    assert torch.equal(M.bits(body[:3 * tail].cpu().view(tail, 3)), M.bits(head))
    del whole, body
    torch.cuda.empty_cache()


# ---- the distance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", M.DIST_CASES)
def test_distance_cases_equal_the_restatement_in_any_order(hip, name, form):
    from bdm_amd import _lib as L
    c, want = M.dist_case(name), M.dist_ref(name)
    B, P = c["points"].shape[:2]
    sum_f = sum(f.shape[0] for f in c["faces"])
    assert L.lib().bdm_point_mesh_distance_variant(B, P, sum_f, 0) == 1 == L.lib().bdm_point_mesh_distance_variant(B, P, sum_f, 1)   # the pin
    _assert_equal(f"{name} natural", _call_dist(c, form), want)
    _assert_equal(f"{name} morton", _call_dist(c, form, M.morton_order(c["points"])), want)
    g = torch.Generator().manual_seed(5)
    shuffled = torch.stack([torch.randperm(P, generator=g) for _ in range(B)])
    _assert_equal(f"{name} shuffled", _call_dist(c, form, shuffled), want)


def test_distance_rows_equal_single_calls_and_calls_repeat(hip):
    c = M.dist_case("batch3")
    whole, again = _call_dist(c), _call_dist(c)
    _assert_equal("repeat", again, whole)
    for j in (2, 0, 1):
        alone = dict(c, verts=c["verts"][j:j + 1], faces=c["faces"][j:j + 1], points=c["points"][j:j + 1])
        _assert_equal(f"mesh {j} alone", _call_dist(alone), {k: whole[k][j:j + 1] for k in DIST_OUTPUTS})


def test_an_order_entry_out_of_range_is_skipped(hip):
    c = M.dist_case("special")
    want = M.dist_ref("special")
    P = c["points"].shape[1]
    order = torch.arange(P)[None].clone()
    order[0, 3], order[0, 7] = -1, P
    got = _call_dist(c, 1, order)
    keep = torch.ones(P, dtype=torch.bool)
    keep[[3, 7]] = False
    assert torch.equal(M.bits(got["sqdist"][0][keep]), M.bits(want["sqdist"][0][keep]))
    assert torch.equal(got["face_idx"][0][keep], want["face_idx"][0][keep])
    assert bool((got["sqdist"][0][~keep] == F_SENTINEL).all()) and bool((got["face_idx"][0][~keep] == I_SENTINEL).all())


def test_the_culled_form_is_refused(hip):
    _call_dist(M.dist_case("special"), form=2, expect=1)
    _call_dist(M.dist_case("special"), form=3, expect=1)


# ---- limits ----------------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    c = M.sample_case("batch3")
    a = _inputs(c["verts"], c["faces"])
    B, S = 3, 16
    keys = _keys(c["keys"])
    pts_in = M.dist_case("batch3")["points"][:, :S].cuda().contiguous()
    order = torch.arange(S, dtype=torch.int32).repeat(B, 1).cuda()
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    bufs = {"points": _guarded(B * S * 3, torch.float32), "face_idx": _guarded(B * S, torch.int32), "normals": _guarded(B * S * 3, torch.float32),
            "sqdist": _guarded(B * S, torch.float32)}
    p = {k: L.ptr(v[1]) for k, v in bufs.items()}
    vf, ff = a["vert_first"], a["face_first"]
    good_s = dict(b=B, s=S, max_faces=a["max_f"], verts=L.ptr(a["verts"]), faces=L.ptr(a["faces"]), vert_first=vf.data_ptr(),
                  face_first=ff.data_ptr(), keys=L.ptr(keys), draw=0, purpose=5, points=p["points"], face_idx=p["face_idx"],
                  normals=p["normals"], ws=L.ptr(ws), stream=L.stream())
    good_d = dict(b=B, p=S, form=1, verts=L.ptr(a["verts"]), faces=L.ptr(a["faces"]), vert_first=vf.data_ptr(), face_first=ff.data_ptr(),
                  points=L.ptr(pts_in), order=L.ptr(order), sqdist=p["sqdist"], face_idx=p["face_idx"], ws=L.ptr(ws), stream=L.stream())
    assert lib.bdm_mesh_sample_points(*good_s.values()) == 0 and lib.bdm_point_mesh_distance(*good_d.values()) == 0
    torch.cuda.synchronize()
    for whole, body in bufs.values():
        body.fill_(I_SENTINEL if body.dtype == torch.int32 else F_SENTINEL)
    down = ff.clone()
    down[2] = down[1] - 1
    late = ff + 1
    huge = torch.tensor([0, (1 << 24) + 1, (1 << 24) + 1, (1 << 24) + 1])
    bad_s = [dict(b=-1), dict(b=65536), dict(s=-1), dict(b=3, s=1 << 30), dict(max_faces=a["max_f"] + 1), dict(verts=None), dict(faces=None),
             dict(vert_first=None), dict(face_first=None), dict(keys=None), dict(points=None), dict(ws=None), dict(ws=L.ptr(ws) + 4),
             dict(face_first=down.data_ptr()), dict(face_first=late.data_ptr()), dict(face_first=huge.data_ptr(), max_faces=(1 << 24) + 1),
             dict(points=L.ptr(a["verts"])), dict(normals=p["points"]), dict(face_idx=L.ptr(a["faces"])), dict(ws=p["points"]),
             dict(points=L.ptr(keys))]
    for change in bad_s:
        assert lib.bdm_mesh_sample_points(*dict(good_s, **change).values()) == 1, change
        assert lib.bdm_last_error()
    bad_d = [dict(b=-1), dict(b=65536), dict(p=-1), dict(b=3, p=1 << 30), dict(form=2), dict(form=-1), dict(verts=None), dict(faces=None),
             dict(vert_first=None), dict(face_first=None), dict(points=None), dict(sqdist=None), dict(face_idx=None), dict(ws=None),
             dict(ws=L.ptr(ws) + 8), dict(face_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(face_first=huge.data_ptr()),
             dict(sqdist=L.ptr(pts_in)), dict(face_idx=L.ptr(order)), dict(sqdist=p["face_idx"]), dict(ws=L.ptr(a["verts"])),
             dict(face_idx=L.ptr(a["faces"]))]
    for change in bad_d:
        assert lib.bdm_point_mesh_distance(*dict(good_d, **change).values()) == 1, change
        assert lib.bdm_last_error()
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values()), "a refused call wrote to an output"
    # nothing to do: 0, and nothing is touched (not even NULL pointers are looked at)
    assert lib.bdm_mesh_sample_points(*dict(good_s, b=0, verts=None).values()) == 0
    assert lib.bdm_mesh_sample_points(*dict(good_s, s=0, points=None).values()) == 0
    assert lib.bdm_point_mesh_distance(*dict(good_d, b=0, verts=None).values()) == 0
    assert lib.bdm_point_mesh_distance(*dict(good_d, p=0, sqdist=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values())
    assert lib.bdm_mesh_sample_workspace_bytes(-1, 10, 10) == 0 and lib.bdm_mesh_sample_workspace_bytes(1, 10, 11) == 0
    assert lib.bdm_mesh_sample_workspace_bytes(1, 1 << 31, 5) == 0 and lib.bdm_point_mesh_distance_workspace_bytes(65536, 5) == 0
    assert lib.bdm_point_mesh_distance_variant(3, 1 << 30, 5, 0) == 0


# ---- the Python surface, end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_mesh(hip):
    """A 4096-point sphere through the chain: visibility-oriented normals -> surface nets."""
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import reconstruct_surface
    g = torch.Generator().manual_seed(0)
    pts = (torch.nn.functional.normalize(torch.randn(1, 4096, 3, generator=g), dim=-1) * 0.5).cuda()
    normals = estimate_pointcloud_normals(pts, 50, "visibility")
    verts, faces = reconstruct_surface(pts, normals)
    assert faces[0].shape[0] > 1000
    return pts, verts, faces


def test_samples_of_a_reconstructed_sphere_lie_on_it(hip, sphere_mesh):
    from bdm_amd import mesh_metrics as MM
    from bdm_amd.cameras import Meshes
    pts, verts, faces = sphere_mesh
    samples, normals, fidx = MM.sample_points_from_meshes(Meshes(verts, faces), 4096, return_normals=True, seed=3, return_face_idx=True)
    assert samples.shape == (1, 4096, 3) and normals.shape == (1, 4096, 3) and fidx.dtype == torch.int64 and int(fidx.min()) >= 0
    sq, near = MM.point_mesh_sqdist((verts, faces), samples)
    sq_m, near_m = MM.point_mesh_sqdist((verts, faces), samples, order="morton", form="exhaustive")
    assert torch.equal(sq.view(torch.int32), sq_m.view(torch.int32)) and torch.equal(near, near_m)
    print(f"samples to their own mesh: largest squared distance {float(sq.max()):.3e} (bound {M.UNIT_GAP_ABS:.3e})")
    # a sample lies within float32 rounding of its face (1e-14 squared), so the rule's float32 value is within the measured float32
    # gap of zero; it is not exactly zero
    assert float(sq.max()) <= M.UNIT_GAP_ABS
    radius = samples.norm(dim=-1)
    assert 0.45 < float(radius.min()) and float(radius.max()) < 0.55
    assert float((normals * torch.nn.functional.normalize(samples, dim=-1)).sum(-1).mean()) > 0.9   # outward, like the faces
    # the same mesh in another batch slot, with the matching global index, gets the same samples
    box = [t.cuda() for t in M.box_mesh()]
    two = MM.sample_points_from_meshes(([box[0], verts[0]], [box[1], faces[0]]), 4096, seed=3, first_index=-1)
    assert torch.equal(two[1], samples[0])
    # the cloud the mesh was made from lies close to it
    sq_gt, _ = MM.point_mesh_sqdist((verts, faces), pts)
    assert float(sq_gt.mean()) < 1e-3


def _write_tree(tmp_path, sphere_mesh):
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    pts, verts, faces = sphere_mesh
    box_v, box_f = M.box_mesh(0.6, 0.8, 1.0, (0.05, 0.0, -0.1))
    meshes = {"a/sphere.ply": (verts[0].cpu(), faces[0].cpu()), "b/box.ply": (box_v, box_f)}
    gts = {"a/sphere.ply": pts[0, :1024].cpu(), "b/box.ply": M.sample_mesh(box_v, box_f, 1024, M.sample_keys(1, 9)[0])[0]}
    for rel, (v, f) in meshes.items():
        save_mesh_ply(v.numpy(), f.numpy(), tmp_path / "mesh" / rel)
        save_pointcloud_ply(gts[rel].numpy(), str(tmp_path / "gt" / rel))
    save_mesh_ply(box_v.numpy(), box_f.numpy(), tmp_path / "mesh" / "c" / "unmatched.ply")
    return meshes, gts


def test_evaluate_mesh_dirs_equals_the_numbers_composed_from_the_restatement(hip, sphere_mesh, tmp_path):
    from bdm_amd import evaluation as E
    from bdm_amd import mesh_metrics as MM
    from bdm_amd.io import load_mesh_ply, load_pointcloud_ply
    _write_tree(tmp_path, sphere_mesh)
    got = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=11)
    rows = []
    for i, rel in enumerate(["a/sphere.ply", "b/box.ply"]):   # sorted order: file i draws from shape index i
        v, f = (torch.from_numpy(x) for x in load_mesh_ply(tmp_path / "mesh" / rel))
        gt = torch.from_numpy(load_pointcloud_ply(str(tmp_path / "gt" / rel)))
        samples, _, _ = M.sample_mesh(v, f, gt.shape[0], M.ref_rng.shape_key(11, i))
        sq, _ = M.distance_mesh(v, f, gt)
        s, g = samples[None].cuda(), gt[None].cuda()
        rows.append((float(E.chamfer_distance_x1000(s, g)[0]), float(E.f1_score(s - s.mean(1, keepdim=True), g - g.mean(1, keepdim=True))[0]),
                     sq.double().numpy()))
    want = MM.compose_scores(rows)
    print(json.dumps(got))
    assert got == want and got["num"] == 2 and got["empty"] == 0
    assert got["gt_to_surface_x1000"] < 1.0 and got["gt_within_0.01"] > 0.99 and got["f1_at_0.01"] > 0.9
    fixed = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", num_samples=500, seed=11, batch_size=1)
    assert fixed["num"] == 2 and fixed["gt_to_surface_x1000"] == got["gt_to_surface_x1000"] and fixed["cd_x1000"] != got["cd_x1000"]


def test_cli_prints_the_same_json(hip, sphere_mesh, tmp_path):
    from bdm_amd import mesh_metrics as MM
    _write_tree(tmp_path, sphere_mesh)
    want = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=4)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_metrics", "--mesh_dir", str(tmp_path / "mesh"), "--gt_dir", str(tmp_path / "gt"),
                          "--seed", "4"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == want
