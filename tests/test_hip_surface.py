"""bdm_surface_grid / bdm_surface_extract (csrc/surface.hip) and their Python surface on the GPU against the CPU restatement
tests/surface_ref.py: SW, SU, counts, verts and faces with torch.equal (the vertices as bits), the bit-exact pins, the error paths,
and the feature end to end.

Every sum of the rule is an integer and every float operation is rounded on its own, so nothing here has a tolerance."""
import json

import numpy as np
import pytest
import torch

import surface_ref as S

pytestmark = pytest.mark.gpu
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5


def _guarded(rows, cols, dtype):
    whole = torch.full((rows * cols + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + rows * cols].view(rows, cols)


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _call(pts, nrm, R, s, min_weight=0.0):
    """The two ABI calls on guarded outputs -> list of per-cloud dicts shaped like surface_ref.reconstruct's."""
    from bdm_amd import _lib as L
    lib = L.lib()
    b, n = pts.shape[0], pts.shape[1]
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    nbytes = lib.bdm_surface_workspace_bytes(b, n, R, s)
    assert nbytes >= 3 * 4 * b * R ** 3
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")      # contents irrelevant before: not zero
    wc, counts = _guarded(b, 4, torch.int32)
    assert lib.bdm_surface_grid(b, n, R, s, min_weight, L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(ws), L.stream()) == 0
    host = counts.cpu()
    nv, nf = host[:, 0].long(), host[:, 1].long()
    offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).cuda()
    wv, verts = _guarded(max(1, int(nv.sum())), 3, torch.float32)
    wf, faces = _guarded(max(1, int(nf.sum())), 3, torch.int32)
    assert lib.bdm_surface_extract(b, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(wc) and _untouched(wv) and _untouched(wf), "sentinel bytes around an output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    assert bool((verts[int(nv.sum()):] == F_SENTINEL).all()) and bool((faces[int(nf.sum()):] == I_SENTINEL).all())
    grids = ws[:2 * b * R ** 3 * 4].view(torch.int32).view(2, b, R, R, R).cpu()
    verts, faces = verts.cpu(), faces.cpu()
    out = []
    for c in range(b):
        v0, f0 = int(offsets[0, c]), int(offsets[1, c])
        out.append({"SW": grids[0, c], "SU": grids[1, c], "counts": host[c].tolist(), "verts": verts[v0:v0 + int(nv[c])],
                    "faces": faces[f0:f0 + int(nf[c])]})
    return out


def _assert_equals_restatement(name, got, refs):
    assert len(got) == len(refs)
    for c, (g, ref) in enumerate(zip(got, refs)):
        print(f"{name}[{c}]: V / F / skipped / valid {ref['counts']}, GPU {g['counts']}")
        assert torch.equal(g["SW"], ref["SW"]), f"{name}[{c}]: {int((g['SW'] != ref['SW']).sum())} SW nodes differ"
        assert torch.equal(g["SU"], ref["SU"]), f"{name}[{c}]: {int((g['SU'] != ref['SU']).sum())} SU nodes differ"
        assert g["counts"] == ref["counts"], f"{name}[{c}]"
        assert torch.equal(g["verts"].view(torch.int32), ref["verts"].view(torch.int32)), f"{name}[{c}]: vertices differ"
        assert torch.equal(g["faces"], ref["faces"]), f"{name}[{c}]: faces differ"


@pytest.mark.parametrize("name", list(S.CASES))
def test_cases_against_the_restatement(hip, name):
    pts, nrm, R, s, mw = S.case_inputs(name)
    _assert_equals_restatement(name, _call(pts, nrm, R, s, mw), S.case_ref(name))


@pytest.mark.parametrize("case", [S.LARGE_CASE, S.FINE_CASE], ids=lambda c: c[0])
def test_large_grids(hip, case):
    """(1, 16384, 3) at R = 128, s = 4, and R = 256 at s = 2 (finer than the sampling: mostly skipped quads)."""
    name, make = case
    pts, nrm, R, s, mw = make()
    _assert_equals_restatement(name, _call(pts, nrm, R, s, mw), S.reconstruct_batch(pts, nrm, R, s, mw))


# ---- bit-exact pins -------------------------------------------------------------------------------------------------------------------
def test_batch_rows_equal_single_calls_and_calls_repeat(hip):
    pts, nrm, R, s, mw = S.case_inputs("b3_n1025_ellipsoids_R32_s3")
    whole, again = _call(pts, nrm, R, s, mw), _call(pts, nrm, R, s, mw)
    assert all(S.same_mesh(a, b) for a, b in zip(whole, again))
    for c in (2, 0, 1):
        assert S.same_mesh(_call(pts[c:c + 1], nrm[c:c + 1], R, s, mw)[0], whole[c])


# ---- through the public interface -----------------------------------------------------------------------------------------------------
def test_estimated_normals_then_the_mesher_on_a_sphere(hip):
    from bdm_amd.cameras import Pointclouds
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import mesh_stats, reconstruct_surface
    pts, _ = S.sphere(torch.Generator().manual_seed(3206), 4096)
    dev = pts[None].cuda()
    nrm = estimate_pointcloud_normals(dev, 16, "visibility")
    verts, faces, info, (SW, SU) = reconstruct_surface(dev, nrm, return_info=True, return_grid=True)
    assert info["resolution"] == 32 and info["support"] == 3
    ref = S.reconstruct(pts, nrm[0].cpu(), 32, 3)
    assert len(verts) == len(faces) == 1 and verts[0].is_cuda and faces[0].is_cuda and faces[0].dtype == torch.int64
    got = {"SW": SW[0].cpu(), "SU": SU[0].cpu(), "counts": info["counts"][0].tolist(), "verts": verts[0].cpu(), "faces": faces[0].int().cpu()}
    _assert_equals_restatement("sphere_4096_estimated_normals", [got], [ref])
    st = mesh_stats(verts[0], faces[0])
    print(f"sphere, 4096 points, estimated normals, R 32, s 3: {st}")
    assert st["vertices"] == ref["counts"][0] and st["faces"] == ref["counts"][1] and st["signed_volume"] > 0
    bare = reconstruct_surface(Pointclouds(dev, nrm))                               # the normals as the cloud's features
    assert len(bare) == 2 and torch.equal(bare[0][0], verts[0]) and torch.equal(bare[1][0], faces[0])
    fine = reconstruct_surface(dev, nrm, resolution=48, support=2, min_weight=0.05, return_info=True)
    want = S.reconstruct(pts, nrm[0].cpu(), 48, 2, 0.05)
    assert fine[2]["counts"][0].tolist() == want["counts"] and torch.equal(fine[0][0].cpu().view(torch.int32), want["verts"].view(torch.int32))
    assert torch.equal(fine[1][0].cpu().int(), want["faces"])
    empty = reconstruct_surface(torch.full((2, 40, 3), 0.5, device="cuda"), torch.ones(2, 40, 3, device="cuda"), return_info=True)
    assert [v.shape for v in empty[0]] == [(0, 3)] * 2 and [f.shape for f in empty[1]] == [(0, 3)] * 2
    assert empty[2]["counts"].tolist() == [[0, 0, 0, 40]] * 2


def test_command_line_on_a_two_file_tree(hip, tmp_path, capsys):
    from bdm_amd.io import load_mesh_ply, load_pointcloud_ply, save_pointcloud_ply, save_pointcloud_ply_normals
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import main, mesh_stats, reconstruct_surface
    g = torch.Generator().manual_seed(3207)
    with_normals, without = S.torus(g, 1500), S.sphere(g, 1024)
    save_pointcloud_ply_normals(with_normals[0].numpy(), with_normals[1].numpy(), tmp_path / "in" / "a" / "torus.ply")
    save_pointcloud_ply(without[0].numpy(), tmp_path / "in" / "sphere.ply")
    res = main(["--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / "out"), "--resolution", "24", "--neighborhood-size", "16"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["files"] == 2
    want = {"a/torus.ply": reconstruct_surface(with_normals[0][None].cuda(), with_normals[1][None].cuda(), resolution=24),
            "sphere.ply": reconstruct_surface(without[0][None].cuda(), estimate_pointcloud_normals(without[0][None].cuda(), 16, "visibility"),
                                              resolution=24)}
    total_v = total_f = edges = open_edges = 0
    for rel, (verts, faces) in want.items():
        v, f = load_mesh_ply(tmp_path / "out" / rel)
        assert np.array_equal(v.view(np.int32), verts[0].cpu().numpy().view(np.int32)) and np.array_equal(f, faces[0].cpu().numpy())
        assert np.array_equal(load_pointcloud_ply(tmp_path / "out" / rel), v)
        st = mesh_stats(v, f)
        total_v, total_f, edges, open_edges = total_v + v.shape[0], total_f + f.shape[0], edges + st["edges"], open_edges + st["open_edges"]
    assert (res["vertices"], res["faces"], res["open_edge_fraction"]) == (total_v, total_f, open_edges / edges)
    assert mesh_stats(*load_mesh_ply(tmp_path / "out" / "a" / "torus.ply"))["open_edges"] == 0        # analytic normals: closed
    assert total_f > 1000 and res["skipped_quads"] >= 0


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    pts, nrm, R, s, _ = S.case_inputs("b2_n300_nonfinite_R16_s3")
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    ws = torch.zeros(lib.bdm_surface_workspace_bytes(2, 300, R, s), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    good = dict(b=2, n=300, r=R, s=s, min_weight=0.0)
    sizes = {"b < 0": dict(b=-1), "n = 0": dict(n=0), "n = 65537": dict(n=65537), "r = 15": dict(r=15), "r = 257": dict(r=257), "s = 1": dict(s=1),
             "s = 5": dict(s=5), "b r^3 = 2^31": dict(b=128, r=256)}
    grid_only = {"min_weight < 0": dict(min_weight=-0.001), "min_weight > 1": dict(min_weight=1.001), "min_weight NaN": dict(min_weight=float("nan"))}
    for what, kw in {**sizes, **grid_only}.items():
        a = {**good, **kw}
        wc, counts = _guarded(2, 4, torch.int32)
        rc = lib.bdm_surface_grid(a["b"], a["n"], a["r"], a["s"], a["min_weight"], L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wc, body=True) and lib.bdm_last_error(), what
        if what in sizes:
            assert lib.bdm_surface_workspace_bytes(a["b"], a["n"], a["r"], a["s"]) == 0, what
    for what, kw in sizes.items():
        a = {**good, **kw}
        wv, verts = _guarded(8, 3, torch.float32)
        wf, faces = _guarded(8, 3, torch.int32)
        rc = lib.bdm_surface_extract(a["b"], a["n"], a["r"], a["s"], L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wv, body=True) and _untouched(wf, body=True) and lib.bdm_last_error(), what
    wc, counts = _guarded(2, 4, torch.int32)
    as_int = lambda t: t.view(torch.int32)
    grid_ptrs = dict(points=L.ptr(dp), normals=L.ptr(dn), counts=L.ptr(counts), workspace=L.ptr(ws))
    bad_ptrs = {f"no {k}": {k: None} for k in grid_ptrs}
    bad_ptrs.update({"counts = points": dict(counts=L.ptr(as_int(dp))), "counts = normals": dict(counts=L.ptr(as_int(dn))),
                     "workspace = points": dict(workspace=L.ptr(dp)), "workspace = counts": dict(workspace=L.ptr(counts))})
    for what, kw in bad_ptrs.items():
        p = {**grid_ptrs, **kw}
        rc = lib.bdm_surface_grid(2, 300, R, s, 0.0, p["points"], p["normals"], p["counts"], p["workspace"], L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wc, body=True) and lib.bdm_last_error(), what
    wv, verts = _guarded(8, 3, torch.float32)
    wf, faces = _guarded(8, 3, torch.int32)
    ext_ptrs = dict(vo=L.ptr(offsets[0]), fo=L.ptr(offsets[1]), verts=L.ptr(verts), faces=L.ptr(faces), workspace=L.ptr(ws))
    bad_ext = {f"no {k}": {k: None} for k in ext_ptrs}
    bad_ext.update({"verts = faces": dict(verts=L.ptr(faces)), "verts = workspace": dict(verts=L.ptr(ws)), "faces = offsets": dict(faces=L.ptr(offsets[1]))})
    for what, kw in bad_ext.items():
        p = {**ext_ptrs, **kw}
        rc = lib.bdm_surface_extract(2, 300, R, s, p["vo"], p["fo"], p["verts"], p["faces"], p["workspace"], L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wv, body=True) and _untouched(wf, body=True) and lib.bdm_last_error(), what
    assert lib.bdm_surface_grid(0, 300, R, s, 0.0, None, None, None, None, L.stream()) == 0
    assert lib.bdm_surface_extract(0, 300, R, s, None, None, None, None, None, L.stream()) == 0
    assert lib.bdm_surface_workspace_bytes(16, 4096, 64, 3) > 0
