"""bdm_face_point_distance (csrc/face_point.hip) and its Python surface on the GPU against the CPU restatement
tests/face_point_ref.py: every output with torch.equal, floats compared as bits, in every case, under the chooser, the resident
form and the split form at two chunk counts; the pins of the launch path, the error paths, and the feature end to end.

Every float operation of the rule is rounded on its own and the split form combines with an integer minimum, so nothing here has a
tolerance except the symmetric value, a float64 sum whose order is torch's."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import face_point_ref as R
import mesh_metrics_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
OUTPUTS = ("sqdist", "point_idx")


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _inputs(c):
    """Device and host arrays of a case in the ABI's form; an empty side still gets one (unread) row: no NULL among the inputs."""
    nv, nf, npt = [v.shape[0] for v in c["verts"]], [f.shape[0] for f in c["faces"]], [p.shape[0] for p in c["clouds"]]
    verts = torch.cat(c["verts"]).float().cuda() if sum(nv) else torch.zeros(1, 3, device="cuda")
    faces = torch.cat([torch.where((f >= 0) & (f < 2 ** 31), f, -1) for f in c["faces"]]).int().cuda() if sum(nf) else \
        torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    points = torch.cat(c["clouds"]).float().cuda() if sum(npt) else torch.zeros(1, 3, device="cuda")
    return {"b": len(nv), "verts": verts.contiguous(), "faces": faces.contiguous(), "points": points.contiguous(),
            "vert_first": torch.tensor([0] + nv).cumsum(0), "face_first": torch.tensor([0] + nf).cumsum(0),
            "point_first": torch.tensor([0] + npt).cumsum(0), "sum_f": sum(nf), "sum_p": sum(npt), "max_p": max(npt) if npt else 0}


def _call(c, form=0, chunks=0, expect=0):
    """One ABI call on guarded outputs and a workspace pre-filled with 0xA5 -> the dict of face_point_ref.face_point_batch (host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    a = _inputs(c)
    nbytes = lib.bdm_face_point_distance_workspace_bytes(a["b"], a["sum_f"])
    assert nbytes >= 72 * a["sum_f"]
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {"sqdist": _guarded(a["sum_f"], torch.float32), "point_idx": _guarded(a["sum_f"], torch.int32)}
    rc = lib.bdm_face_point_distance(a["b"], form, chunks, L.ptr(a["verts"]), L.ptr(a["faces"]), a["vert_first"].data_ptr(), a["face_first"].data_ptr(),
                                     L.ptr(a["points"]), a["point_first"].data_ptr(), L.ptr(bufs["sqdist"][1]), L.ptr(bufs["point_idx"][1]), L.ptr(ws),
                                     L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(whole, body=expect != 0) for whole, _ in bufs.values()), "sentinels around an output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    return {k: bufs[k][1].cpu() for k in OUTPUTS}


def _assert_equal(name, got, want):
    for k in OUTPUTS:
        gb, wb = R.bits(got[k]), R.bits(want[k])
        bad = gb != wb
        assert torch.equal(gb, wb), f"{name}: {k} differs at {int(bad.sum())} of {gb.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_cases_equal_the_restatement_under_every_form(hip, name):
    from bdm_amd import _lib as L
    lib = L.lib()
    c, want = R.case(name), R.ref(name)
    a = _inputs(c)
    sizes = (a["b"], a["sum_f"], a["sum_p"], a["max_p"], R.workgroups_of(c["faces"]))
    form, chunks = R.variant(*sizes)
    assert (lib.bdm_face_point_distance_variant(*sizes), lib.bdm_face_point_distance_chunks(*sizes)) == (form, chunks)   # the pin
    print(f"{name}: {a['sum_f']} faces, {a['sum_p']} points, chooser ({form}, {chunks}), {int((want['point_idx'] >= 0).sum())} faces scored")
    _assert_equal(f"{name} chooser", _call(c, 0), want)
    _assert_equal(f"{name} resident", _call(c, 1), want)
    _assert_equal(f"{name} resident, chunks = 1", _call(c, 1, 1), want)
    _assert_equal(f"{name} split, its own count", _call(c, 2), want)
    for k in R.chunk_counts(name):
        _assert_equal(f"{name} split in {k}", _call(c, 2, k), want)


def test_rows_equal_single_calls_and_calls_repeat(hip):
    c = R.case("ragged")
    for form, chunks in ((0, 0), (1, 0), (2, 2), (2, 7)):
        whole, again = _call(c, form, chunks), _call(c, form, chunks)
        _assert_equal("repeat", again, whole)
        _assert_equal("batch", whole, R.ref("ragged"))
        cuts = np.cumsum([0] + [f.shape[0] for f in c["faces"]])
        for j in (3, 0, 2, 1):
            alone = {k: c[k][j:j + 1] for k in ("verts", "faces", "clouds")}
            _assert_equal(f"mesh {j} alone, form {form}", _call(alone, form, chunks), {k: whole[k][cuts[j]:cuts[j + 1]] for k in OUTPUTS})


def test_the_chooser_splits_a_small_mesh_against_a_large_cloud(hip):
    """What the chooser picks on its own: the 513-face soup against 2049 points is 3 workgroups and 3 tiles -> split in 3."""
    name = f"soup_f{2 * R.THREADS + 1}_p{2 * R.TILE + 1}"
    assert R.variant(1, 2 * R.THREADS + 1, 2 * R.TILE + 1, 2 * R.TILE + 1, 3) == (2, 3)
    _assert_equal(name, _call(R.case(name), 0), R.ref(name))


# ---- limits ----------------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    c = R.case("ragged")
    a = _inputs(c)
    B = a["b"]
    nbytes = lib.bdm_face_point_distance_workspace_bytes(B, a["sum_f"])
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {"sqdist": _guarded(a["sum_f"], torch.float32), "point_idx": _guarded(a["sum_f"], torch.int32)}
    vf, ff, pf = a["vert_first"], a["face_first"], a["point_first"]
    good = dict(b=B, form=0, chunks=0, verts=L.ptr(a["verts"]), faces=L.ptr(a["faces"]), vert_first=vf.data_ptr(), face_first=ff.data_ptr(),
                points=L.ptr(a["points"]), point_first=pf.data_ptr(), sqdist=L.ptr(bufs["sqdist"][1]), point_idx=L.ptr(bufs["point_idx"][1]),
                ws=L.ptr(ws), stream=L.stream())
    assert lib.bdm_face_point_distance(*good.values()) == 0
    torch.cuda.synchronize()
    for whole, body in bufs.values():
        body.fill_(I_SENTINEL if body.dtype == torch.int32 else F_SENTINEL)
    ws.fill_(0xA5)
    down = ff.clone()
    down[2] = down[1] - 1
    pdown = pf.clone()
    pdown[3] = pdown[2] - 1
    late = pf + 1
    huge = torch.tensor([0, (1 << 24) + 1, (1 << 24) + 1, (1 << 24) + 1, (1 << 24) + 1])
    many = torch.tensor([0, 1 << 30, 1 << 31, 1 << 31, 1 << 31])
    bad = [dict(b=-1), dict(b=65536), dict(form=3), dict(form=-1), dict(chunks=-1), dict(chunks=65536), dict(form=0, chunks=2),
           dict(form=1, chunks=2), dict(verts=None), dict(faces=None), dict(vert_first=None), dict(face_first=None), dict(points=None),
           dict(point_first=None), dict(sqdist=None), dict(point_idx=None), dict(ws=None), dict(ws=L.ptr(ws) + 8),
           dict(face_first=down.data_ptr()), dict(point_first=pdown.data_ptr()), dict(point_first=late.data_ptr()),
           dict(vert_first=late.data_ptr()), dict(face_first=huge.data_ptr()), dict(point_first=many.data_ptr()),
           dict(vert_first=many.data_ptr()), dict(sqdist=L.ptr(a["points"])), dict(point_idx=L.ptr(a["faces"])),
           dict(sqdist=L.ptr(bufs["point_idx"][1])), dict(ws=L.ptr(a["verts"])), dict(point_idx=L.ptr(ws) + nbytes - 4),
           dict(sqdist=L.ptr(a["verts"]) + 4)]
    for change in bad:
        assert lib.bdm_face_point_distance(*dict(good, **change).values()) == 1, change
        assert lib.bdm_last_error()
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    # nothing to do: 0, and nothing is touched (not even NULL pointers are looked at)
    none = torch.zeros(B + 1, dtype=torch.int64)
    assert lib.bdm_face_point_distance(*dict(good, b=0, verts=None, vert_first=None).values()) == 0
    assert lib.bdm_face_point_distance(*dict(good, face_first=none.data_ptr(), sqdist=None, ws=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values()) and bool((ws == 0xA5).all())
    assert lib.bdm_face_point_distance_workspace_bytes(-1, 10) == 0 == lib.bdm_face_point_distance_workspace_bytes(1, 1 << 31)
    assert lib.bdm_face_point_distance_variant(1, 5, 1 << 31, 5, 1) == 0 == lib.bdm_face_point_distance_chunks(65536, 5, 5, 5, 1)


# ---- the Python surface, end to end ------------------------------------------------------------------------------------------------
def _cuda(c):
    return [v.cuda() for v in c["verts"]], [f.cuda() for f in c["faces"]], [p.cuda() for p in c["clouds"]]


def test_face_point_sqdist_takes_lists_tensors_and_pointclouds(hip):
    from bdm_amd import mesh_metrics as MM
    from bdm_amd.cameras import Meshes, Pointclouds
    c, want = R.case("ragged"), R.ref("ragged")
    verts, faces, clouds = _cuda(c)
    for kw in ({}, {"form": "resident"}, {"form": "split"}, {"form": "split", "chunks": 5}):
        sq, idx = MM.face_point_sqdist(Meshes(verts, faces), clouds, **kw)
        assert [t.shape[0] for t in sq] == [f.shape[0] for f in faces] and all(t.dtype == torch.float32 for t in sq)
        assert all(t.dtype == torch.int64 for t in idx)
        _assert_equal(f"ragged {kw}", {"sqdist": torch.cat(sq).cpu(), "point_idx": torch.cat(idx).int().cpu()}, want)
    t = R.case("ties")
    padded = torch.stack([t["clouds"][0], t["clouds"][0].flip(0)]).cuda()
    two = ([t["verts"][0].cuda()] * 2, [t["faces"][0].cuda()] * 2)
    a, b = MM.face_point_sqdist(two, padded), MM.face_point_sqdist(two, Pointclouds(padded))
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert torch.equal(R.bits(a[0][0].cpu()), R.bits(R.ref("ties")["sqdist"])) and torch.equal(a[1][0].int().cpu(), R.ref("ties")["point_idx"])
    assert torch.equal(R.bits(a[0][1].cpu()), R.bits(a[0][0].cpu())) and not torch.equal(a[1][1], a[1][0])
    empty = MM.face_point_sqdist(([t["verts"][0].cuda()], [torch.zeros(0, 3, dtype=torch.int64, device="cuda")]), padded[:1])
    assert empty[0][0].shape == (0,) and empty[1][0].shape == (0,)


def test_point_mesh_face_distance_equals_the_float64_composition(hip):
    from bdm_amd import mesh_metrics as MM
    c = R.case("ragged")
    keep = [0, 1, 3]   # the meshes with faces (a mean over no faces is NaN)
    vl, fl, cl = [c["verts"][i] for i in keep], [c["faces"][i] for i in keep], [c["clouds"][i] for i in keep]
    cl[0] = M.cloud(7, 2)
    for clouds in (cl, [M.cloud(65, 3), M.cloud(65, 4, centre=R.FAR), M.cloud(65, 5)]):   # ragged, and one size (one call of the point side)
        want, count = R.symmetric(vl, fl, clouds)
        got = MM.point_mesh_face_distance(([v.cuda() for v in vl], [f.cuda() for f in fl]), [p.cuda() for p in clouds])
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        print(f"{float(got)!r} against {want!r}: relative {abs(float(got) - want) / want:.3e}, bound {count * 2.0 ** -52:.3e}")
        assert math.isfinite(want) and abs(float(got) - want) <= count * 2.0 ** -52 * want
    d = R.case("degenerate")   # invalid faces take part with +inf
    assert float(MM.point_mesh_face_distance(([d["verts"][0].cuda()], [d["faces"][0].cuda()]), [d["clouds"][0].cuda()])) == math.inf


def _write_tree(tmp_path):
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    box_v, box_f = M.box_mesh(0.5, 0.75, 1.0, (0.0625, 0.0, -0.125))
    blob_v, blob_f = M.box_mesh(0.125, 0.125, 0.125, (2.0, 0.0, 0.0))
    ico_v, ico_f = M.icosphere(2, 0.5)
    meshes = {"a/box_blob.ply": (torch.cat([box_v, blob_v]), torch.cat([box_f, blob_f + 8])), "b/ico.ply": (ico_v, ico_f)}
    gts = {"a/box_blob.ply": M.sample_mesh(box_v, box_f, 1024, M.sample_keys(1, 9)[0])[0],
           "b/ico.ply": M.sample_mesh(ico_v, ico_f, 1024, M.sample_keys(1, 10)[0])[0]}
    for rel, (v, f) in meshes.items():
        save_mesh_ply(v.numpy(), f.numpy(), tmp_path / "mesh" / rel)
        save_pointcloud_ply(gts[rel].numpy(), str(tmp_path / "gt" / rel))
    return meshes, gts


def test_evaluate_mesh_dirs_two_sided_equals_the_numbers_composed_by_hand(hip, tmp_path):
    from bdm_amd import mesh_metrics as MM
    from bdm_amd.io import load_mesh_ply, load_pointcloud_ply
    _write_tree(tmp_path)
    one = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=11)
    two = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=11, two_sided=True)
    print(json.dumps(two))
    assert {k: two[k] for k in one} == one and list(two)[6:] == ["surface_to_gt_x1000", "surface_within_0.01", "face_distance_x1000"]
    s2g, within, sym = [], [], []
    for rel in ("a/box_blob.ply", "b/ico.ply"):
        v, f = (torch.from_numpy(x) for x in load_mesh_ply(tmp_path / "mesh" / rel))
        gt = torch.from_numpy(load_pointcloud_ply(str(tmp_path / "gt" / rel)))
        face_sq, face_pt = R.face_point_mesh(v, f, gt)
        assert bool((face_pt >= 0).all())
        t = v.double()[f.long()]
        area = 0.5 * torch.linalg.norm(torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), dim=1).numpy()
        sq = face_sq.double().numpy()
        s2g.append(float((area * sq).sum() / area.sum()))
        within.append(float(area[sq < 0.01].sum() / area.sum()))
        sym.append(float(M.distance_mesh(v, f, gt)[0].double().numpy().mean()) + float(sq.mean()))
    assert two["surface_to_gt_x1000"] == float(np.mean(s2g)) * 1000.0 and two["surface_within_0.01"] == float(np.mean(within))
    assert two["face_distance_x1000"] == float(np.mean(sym)) * 1000.0
    assert within[0] == pytest.approx(3.25 / 3.34375, rel=1e-15) and within[1] == 1.0 and two["gt_within_0.01"] == 1.0


def test_island_removal_shows_in_surface_within(hip):
    """The island mesh of the cleaning tests (a sphere of radius 0.4 and a clump 0.6 away) scored against the big sphere's own cloud,
    before and after remove_small_components: the island is the part of the surface the ground truth has nothing near."""
    import mesh_clean_ref as C
    from bdm_amd import mesh_clean as MC
    from bdm_amd import mesh_metrics as MM
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    v, f = C.island_mesh()
    big = C.island_cloud()[0][:1024]   # the big sphere's own points; the clump's 48 come after them
    cv, cf = MC.remove_small_components(([v.cuda()], [f.cuda()]))
    assert cf[0].shape[0] < f.shape[0]
    import tempfile
    scores = []
    for verts, faces in ((v, f), (cv[0].cpu(), cf[0].cpu())):
        with tempfile.TemporaryDirectory() as tmp:
            save_mesh_ply(verts.numpy(), faces.numpy(), os.path.join(tmp, "mesh", "a.ply"))
            save_pointcloud_ply(big.numpy(), os.path.join(tmp, "gt", "a.ply"))
            scores.append(MM.evaluate_mesh_dirs(os.path.join(tmp, "mesh"), os.path.join(tmp, "gt"), two_sided=True))
    before, after = scores
    print(json.dumps(before), json.dumps(after))
    assert before["surface_within_0.01"] < 0.99 < after["surface_within_0.01"]
    assert after["surface_to_gt_x1000"] < before["surface_to_gt_x1000"] and after["face_distance_x1000"] < before["face_distance_x1000"]
    assert after["gt_to_surface_x1000"] == before["gt_to_surface_x1000"]   # the one-sided score cannot see the island


def test_cli_prints_the_same_json(hip, tmp_path):
    from bdm_amd import mesh_metrics as MM
    _write_tree(tmp_path)
    want = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=4, two_sided=True)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_metrics", "--mesh_dir", str(tmp_path / "mesh"), "--gt_dir", str(tmp_path / "gt"),
                          "--seed", "4", "--two-sided"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == want
