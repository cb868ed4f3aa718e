"""bdm_surface_poisson_grid / bdm_surface_poisson_density (csrc/surface_poisson.hip) with bdm_surface_extract on their workspace, and
their Python surface, on the GPU against the CPU restatement tests/surface_poisson_ref.py: the four integer grids, D, phi as bits
after the last cycle, the bits of iso and scale, SW, SU, counts, verts as bits, faces and density as bits, all with torch.equal; the
bit-exact pins, the error paths, the refactored section-12 entry points, and the feature end to end.

Every sum of the rule is an integer and every float operation is rounded on its own, so nothing here has a tolerance."""
import json
import subprocess
import sys
import time

import pytest
import torch

import surface_poisson_ref as P
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


def _call(pts, nrm, R, s, cycles):
    """The three ABI calls on guarded outputs -> list of per-cloud dicts shaped like surface_poisson_ref.reconstruct's."""
    from bdm_amd import _lib as L
    lib = L.lib()
    b, n = pts.shape[0], pts.shape[1]
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    nbytes, head = lib.bdm_surface_poisson_workspace_bytes(b, n, R, s), lib.bdm_surface_workspace_bytes(b, n, R, s)
    r3 = 4 * b * R ** 3
    assert nbytes >= head + 6 * r3
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")      # contents irrelevant before: not zero
    wc, counts = _guarded(b, 4, torch.int32)
    wi, info = _guarded(b, 3, torch.int32)
    assert lib.bdm_surface_poisson_grid(b, n, R, s, cycles, L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(info), L.ptr(ws), L.stream()) == 0
    host, hinfo = counts.cpu(), info.cpu()
    nv, nf = host[:, 0].long(), host[:, 1].long()
    offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).cuda()
    wv, verts = _guarded(max(1, int(nv.sum())), 3, torch.float32)
    wf, faces = _guarded(max(1, int(nf.sum())), 3, torch.int32)
    wd, density = _guarded(max(1, int(nv.sum())), 1, torch.float32)
    assert lib.bdm_surface_extract(b, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream()) == 0
    assert lib.bdm_surface_poisson_density(b, R, L.ptr(offsets[0]), L.ptr(density), L.ptr(ws), L.stream()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w) for w in (wc, wi, wv, wf, wd)), "sentinel bytes around an output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    assert bool((verts[int(nv.sum()):] == F_SENTINEL).all()) and bool((faces[int(nf.sum()):] == I_SENTINEL).all())
    assert bool((density[int(nv.sum()):] == F_SENTINEL).all())
    grids = ws[:2 * r3].view(torch.int32).view(2, b, R, R, R).cpu()
    ints = ws[head:head + 4 * r3].view(torch.int32).view(4, b, R, R, R).cpu()
    flts = ws[head + 4 * r3:head + 6 * r3].view(torch.float32).view(2, b, R, R, R).cpu()
    verts, faces, density = verts.cpu(), faces.cpu(), density.cpu().flatten()
    out = []
    for c in range(b):
        v0, f0 = int(offsets[0, c]), int(offsets[1, c])
        out.append({"W": ints[0, c], "Vx": ints[1, c], "Vy": ints[2, c], "Vz": ints[3, c], "D": flts[0, c], "phi": flts[1, c],
                    "border_raised": int(hinfo[c, 0]), "iso": hinfo[c, 1].view(torch.float32), "scale": hinfo[c, 2].view(torch.float32),
                    "SW": grids[0, c], "SU": grids[1, c], "counts": host[c].tolist(), "verts": verts[v0:v0 + int(nv[c])],
                    "faces": faces[f0:f0 + int(nf[c])], "density": density[v0:v0 + int(nv[c])]})
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


def _assert_equals_restatement(name, got, refs):
    assert len(got) == len(refs)
    for c, (g, ref) in enumerate(zip(got, refs)):
        print(f"{name}[{c}]: V / F / skipped / valid {ref['counts']}, border_raised {ref['border_raised']}, iso {float(ref['iso']):.6g}; "
              f"GPU {g['counts']}, {g['border_raised']}, {float(g['iso']):.6g}")
        for k in ("W", "Vx", "Vy", "Vz"):
            assert torch.equal(g[k], ref[k]), f"{name}[{c}]: {int((g[k] != ref[k]).sum())} {k} nodes differ"
        assert torch.equal(_bits(g["D"]), _bits(ref["D"].float())), f"{name}[{c}]: D differs"
        assert torch.equal(_bits(g["phi"]), _bits(ref["phi"])), f"{name}[{c}]: {int((_bits(g['phi']) != _bits(ref['phi'])).sum())} phi nodes differ"
        assert torch.equal(_bits(g["iso"]), _bits(ref["iso"])) and torch.equal(_bits(g["scale"]), _bits(ref["scale"])), f"{name}[{c}]: iso / scale"
        assert torch.equal(g["SW"], ref["SW"]), f"{name}[{c}]: SW differs"
        assert torch.equal(g["SU"], ref["SU"]), f"{name}[{c}]: {int((g['SU'] != ref['SU']).sum())} SU nodes differ"
        assert g["border_raised"] == ref["border_raised"] and g["counts"] == ref["counts"], f"{name}[{c}]"
        assert torch.equal(_bits(g["verts"]), _bits(ref["verts"])), f"{name}[{c}]: vertices differ"
        assert torch.equal(g["faces"], ref["faces"]), f"{name}[{c}]: faces differ"
        assert torch.equal(_bits(g["density"]), _bits(ref["density"])), f"{name}[{c}]: densities differ"
        assert ref["counts"][2] == 0


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in P.KEYS_INT) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in P.KEYS_BITS) and \
        a["counts"] == b["counts"] and a["border_raised"] == b["border_raised"]


@pytest.mark.parametrize("name", list(P.CASES))
def test_cases_against_the_restatement(hip, name):
    pts, nrm, R, s, cycles = P.case_inputs(name)
    _assert_equals_restatement(name, _call(pts, nrm, R, s, cycles), P.case_ref(name))


def test_three_global_levels_at_128(hip):
    """(1, 16384, 3) torus at R = 128, s = 4, 2 cycles.  The restatement takes under two seconds here, so it is the reference (the
    issue's bound is ten); the time is printed."""
    name, make = P.LARGE_CASE
    pts, nrm, R, s, cycles = make()
    t0 = time.perf_counter()
    ref = P.reconstruct_batch(pts, nrm, R, s, cycles)
    print(f"{name}: restatement {time.perf_counter() - t0:.1f} s")
    _assert_equals_restatement(name, _call(pts, nrm, R, s, cycles), ref)


# ---- bit-exact pins -------------------------------------------------------------------------------------------------------------------
def test_batch_rows_equal_single_calls_and_calls_repeat(hip):
    pts, nrm, R, s, cycles = P.case_inputs("b3_n1025_ellipsoids_R32_s3_c4")
    whole, again = _call(pts, nrm, R, s, cycles), _call(pts, nrm, R, s, cycles)
    assert all(_same(a, b) for a, b in zip(whole, again))
    for c in (2, 0, 1):
        assert _same(_call(pts[c:c + 1], nrm[c:c + 1], R, s, cycles)[0], whole[c])


@pytest.mark.parametrize("name", ["b1_n65_R16_s2_c3", "b3_n1025_ellipsoids_R32_s3_c4", "torus_R40_s3_c3"])
def test_staged_call_and_the_per_level_solve_have_the_same_bits(hip, name):
    """bdm_surface_poisson_grid_staged (tools/surface_poisson_bench.py): the three stages one after another, and the solve run one
    launch per level and operator in place of the LDS tail, leave the workspace, counts and info of the single call."""
    from bdm_amd import _lib as L
    lib = L.lib()
    pts, nrm, R, s, cycles = P.case_inputs(name)
    b, n = pts.shape[0], pts.shape[1]
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    nbytes, head = lib.bdm_surface_poisson_workspace_bytes(b, n, R, s), lib.bdm_surface_workspace_bytes(b, n, R, s)
    results = []
    for plan in ([(7, 0)], [(1, 0), (2, 0), (4, 0)], [(3, 1), (4, 1)]):
        ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        counts, info = torch.empty(b, 4, dtype=torch.int32, device="cuda"), torch.empty(b, 3, dtype=torch.int32, device="cuda")
        for stages, per_level in plan:
            assert lib.bdm_surface_poisson_grid_staged(b, n, R, s, cycles, stages, per_level, L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(info),
                                                       L.ptr(ws), L.stream()) == 0
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all())
        results.append((ws[:3 * 4 * b * R ** 3].clone(), ws[head:head + 6 * 4 * b * R ** 3].clone(), counts.cpu(), info.cpu()))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0], other))
    ref = P.case_ref(name)
    assert results[0][2].tolist() == [r["counts"] for r in ref]
    wc, counts = _guarded(b, 4, torch.int32)
    for stages, per_level in ((0, 0), (8, 0), (7, 2), (7, -1)):
        rc = lib.bdm_surface_poisson_grid_staged(b, n, R, s, cycles, stages, per_level, L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(info), L.ptr(ws),
                                                 L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wc, body=True)


@pytest.mark.parametrize("name", ["b1_n65_R16_s2", "b3_n1025_ellipsoids_R32_s3", "b2_n300_nonfinite_R16_s3"])
def test_section_12_entry_points_after_the_refactoring(hip, name):
    """bdm_surface_grid / bdm_surface_extract still equal tests/surface_ref.py: their frame and mark stage are now host functions that
    bdm_surface_poisson_grid calls as well."""
    from bdm_amd import _lib as L
    lib = L.lib()
    pts, nrm, R, s, mw = S.case_inputs(name)
    b, n = pts.shape[0], pts.shape[1]
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    ws = torch.full((lib.bdm_surface_workspace_bytes(b, n, R, s),), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.empty(b, 4, dtype=torch.int32, device="cuda")
    assert lib.bdm_surface_grid(b, n, R, s, mw, L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(ws), L.stream()) == 0
    host = counts.cpu()
    nv, nf = host[:, 0].long(), host[:, 1].long()
    offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).cuda()
    verts = torch.empty(max(1, int(nv.sum())), 3, device="cuda")
    faces = torch.empty(max(1, int(nf.sum())), 3, dtype=torch.int32, device="cuda")
    assert lib.bdm_surface_extract(b, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream()) == 0
    grids = ws[:2 * b * R ** 3 * 4].view(torch.int32).view(2, b, R, R, R).cpu()
    verts, faces = verts.cpu(), faces.cpu()
    for c, ref in enumerate(S.case_ref(name)):
        v0, f0 = int(offsets[0, c]), int(offsets[1, c])
        got = {"SW": grids[0, c], "SU": grids[1, c], "counts": host[c].tolist(), "verts": verts[v0:v0 + int(nv[c])], "faces": faces[f0:f0 + int(nf[c])]}
        assert S.same_mesh(got, ref), f"{name}[{c}]"


# ---- through the public interface -----------------------------------------------------------------------------------------------------
def test_sparse_sphere_voxelises_without_disagreement_where_imls_does_not(hip):
    """The row of DESIGN.md section 25 that no existing tool closes: 512 points at 32^3."""
    from bdm_amd.mesh_voxel import voxelize_meshes
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import mesh_stats, reconstruct_surface, trim_by_density
    pts, _, R, s = P.closure_inputs("sphere_512_R32_s2")
    dev = pts[None].cuda()
    nrm = estimate_pointcloud_normals(dev, 16, "visibility")
    verts, faces, density, info, (SW, SU, phi) = reconstruct_surface(dev, nrm, resolution=R, support=s, method="poisson", return_density=True,
                                                                     return_info=True, return_grid="all")
    ref = P.reconstruct(pts, nrm[0].cpu(), R, s)
    got = {"SW": SW[0].cpu(), "SU": SU[0].cpu(), "phi": phi[0].cpu(), "verts": verts[0].cpu(), "faces": faces[0].int().cpu(), "density": density[0].cpu()}
    for k in ("SW", "SU", "faces"):
        assert torch.equal(got[k], ref[k]), k
    for k in ("phi", "verts", "density"):
        assert torch.equal(_bits(got[k]), _bits(ref[k])), k
    assert info["counts"][0].tolist() == ref["counts"] and info["cycles"] == P.DEFAULT_CYCLES and int(info["border_raised"][0]) == 0
    assert torch.equal(_bits(info["iso"][0]), _bits(ref["iso"])) and info["resolution"] == R
    st = mesh_stats(verts[0], faces[0])
    _, vox = voxelize_meshes((verts, faces), 32, return_info=True)
    verts_i, faces_i = reconstruct_surface(dev, nrm, resolution=R, support=s)
    _, vox_i = voxelize_meshes((verts_i, faces_i), 32, return_info=True)
    print(f"sphere 512, R 32, s 2: poisson {st}, disagree {int(vox['counts']['disagree'][0])}; imls open edges "
          f"{mesh_stats(verts_i[0], faces_i[0])['open_edges']}, disagree {int(vox_i['counts']['disagree'][0])}")
    assert st["open_edges"] == 0 and st["inconsistent_edges"] == 0 and st["signed_volume"] > 0 and info["counts"][0, 2] == 0
    assert int(vox["counts"]["disagree"][0]) == 0
    assert int(vox_i["counts"]["disagree"][0]) > 0
    kept = trim_by_density(verts[0], faces[0], density[0], 0.0)
    assert torch.equal(kept[0], verts[0]) and torch.equal(kept[1], faces[0])
    auto = reconstruct_surface(dev, nrm, method="poisson", return_info=True)            # 512 points: default_resolution 16, accepted
    assert auto[2]["resolution"] == 16 and len(auto) == 3
    with pytest.raises(ValueError, match="nearest accepted one is 64"):
        reconstruct_surface(dev, nrm, method="poisson", resolution=72)
    empty = reconstruct_surface(torch.full((2, 40, 3), 0.5, device="cuda"), torch.ones(2, 40, 3, device="cuda"), method="poisson",
                                resolution=16, return_info=True, return_density=True)
    assert [v.shape for v in empty[0]] == [(0, 3)] * 2 and [d.shape for d in empty[2]] == [(0,)] * 2
    assert empty[3]["counts"].tolist() == [[0, 0, 0, 40]] * 2 and empty[3]["border_raised"].tolist() == [0, 0]


def test_command_line_in_a_child_process(hip, tmp_path):
    from bdm_amd.io import load_mesh_ply, save_pointcloud_ply_normals
    from bdm_amd.surface import mesh_stats, reconstruct_surface
    pts, nrm = S.sphere(torch.Generator().manual_seed(3305), 700)
    plane = S.lattice_plane(32)
    save_pointcloud_ply_normals(pts.numpy(), nrm.numpy(), tmp_path / "in" / "sphere.ply")
    save_pointcloud_ply_normals(plane[0].numpy(), plane[1].numpy(), tmp_path / "in" / "a" / "plane.ply")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda out, *more: json.loads(subprocess.run(
        [sys.executable, "-m", "bdm_amd.surface", "--in_dir", str(tmp_path / "in"), "--out_dir", str(tmp_path / out), "--method", "poisson",
         "--resolution", "32", "--cycles", "6", *more], cwd=root, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
    res = run("out")
    want_s = reconstruct_surface(pts[None].cuda(), nrm[None].cuda(), resolution=32, method="poisson", cycles=6)
    want_p = reconstruct_surface(plane[0][None].cuda(), plane[1][None].cuda(), resolution=32, method="poisson", cycles=6, return_density=True)
    v, f = load_mesh_ply(tmp_path / "out" / "sphere.ply")
    assert torch.equal(_bits(torch.from_numpy(v)), _bits(want_s[0][0].cpu())) and torch.equal(torch.from_numpy(f).long(), want_s[1][0].cpu())
    vp, fp = load_mesh_ply(tmp_path / "out" / "a" / "plane.ply")
    # the inside of the open sheet is the half space below it, out to the border: the lower half of the border layer is raised
    assert res["files"] == 2 and res["skipped_quads"] == 0 and res["border_raised"] == (32 ** 3 - 30 ** 3) // 2 and res["open_edge_fraction"] == 0.0
    assert res["vertices"] == v.shape[0] + vp.shape[0] and res["faces"] == f.shape[0] + fp.shape[0]
    cut = 8.0                                       # half the density of the sheet's own vertices; the invented back has none
    trimmed = run("trimmed", "--trim-density", repr(cut))
    vt, ft = load_mesh_ply(tmp_path / "trimmed" / "a" / "plane.ply")
    assert vt.shape[0] == int((want_p[2][0] >= cut).sum()) < vp.shape[0] and trimmed["open_edge_fraction"] > 0.0
    assert mesh_stats(vt, ft)["open_edges"] > 0


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    pts, nrm, R, s, cycles = P.case_inputs("b2_n300_nonfinite_R16_s3_c2")
    dp, dn = pts.cuda().contiguous(), nrm.cuda().contiguous()
    ws = torch.zeros(lib.bdm_surface_poisson_workspace_bytes(2, 300, R, s), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(2, dtype=torch.int64, device="cuda")
    good = dict(b=2, n=300, r=R, s=s, cycles=cycles)
    sizes = {"b < 0": dict(b=-1), "n = 0": dict(n=0), "n = 65537": dict(n=65537), "r = 8": dict(r=8), "r = 257": dict(r=257), "s = 1": dict(s=1),
             "s = 5": dict(s=5), "b r^3 = 2^31": dict(b=128, r=256)}
    sizes.update({f"r = {r}": dict(r=r) for r in range(16, 257) if r not in P.ACCEPTED and (r % 8 == 0 or r in (17, 20, 36, 255))})
    grid_only = {"cycles = 0": dict(cycles=0), "cycles = 33": dict(cycles=33), "cycles < 0": dict(cycles=-1)}
    for what, kw in {**sizes, **grid_only}.items():
        a = {**good, **kw}
        wc, counts = _guarded(2, 4, torch.int32)
        wi, info = _guarded(2, 3, torch.int32)
        rc = lib.bdm_surface_poisson_grid(a["b"], a["n"], a["r"], a["s"], a["cycles"], L.ptr(dp), L.ptr(dn), L.ptr(counts), L.ptr(info), L.ptr(ws),
                                          L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wc, body=True) and _untouched(wi, body=True) and lib.bdm_last_error(), what
        if what in sizes:
            assert lib.bdm_surface_poisson_workspace_bytes(a["b"], a["n"], a["r"], a["s"]) == 0, what
    for r in P.ACCEPTED:
        assert lib.bdm_surface_poisson_workspace_bytes(1, 300, r, 3) > lib.bdm_surface_workspace_bytes(1, 300, r, 3) + 24 * r ** 3
    for what, kw in {k: v for k, v in sizes.items() if "r" in v}.items():
        a = {**good, **kw}
        wd, density = _guarded(8, 1, torch.float32)
        rc = lib.bdm_surface_poisson_density(a["b"], a["r"], L.ptr(offsets), L.ptr(density), L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wd, body=True) and lib.bdm_last_error(), what
    wc, counts = _guarded(2, 4, torch.int32)
    wi, info = _guarded(2, 3, torch.int32)
    as_int = lambda t: t.view(torch.int32)
    ptrs = dict(points=L.ptr(dp), normals=L.ptr(dn), counts=L.ptr(counts), info=L.ptr(info), workspace=L.ptr(ws))
    bad = {f"no {k}": {k: None} for k in ptrs}
    bad.update({"counts = points": dict(counts=L.ptr(as_int(dp))), "info = normals": dict(info=L.ptr(as_int(dn))), "info = counts": dict(info=L.ptr(counts)),
                "workspace = points": dict(workspace=L.ptr(dp)), "workspace = counts": dict(workspace=L.ptr(counts)),
                "workspace = info": dict(workspace=L.ptr(info))})
    for what, kw in bad.items():
        p = {**ptrs, **kw}
        rc = lib.bdm_surface_poisson_grid(2, 300, R, s, cycles, p["points"], p["normals"], p["counts"], p["info"], p["workspace"], L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wc, body=True) and _untouched(wi, body=True) and lib.bdm_last_error(), what
    wd, density = _guarded(8, 1, torch.float32)
    dptrs = dict(vo=L.ptr(offsets), density=L.ptr(density), workspace=L.ptr(ws))
    bad_d = {f"no {k}": {k: None} for k in dptrs}
    bad_d.update({"density = workspace": dict(density=L.ptr(ws)), "density = offsets": dict(density=L.ptr(offsets))})
    for what, kw in bad_d.items():
        p = {**dptrs, **kw}
        rc = lib.bdm_surface_poisson_density(2, R, p["vo"], p["density"], p["workspace"], L.stream())
        torch.cuda.synchronize()
        assert rc == 1 and _untouched(wd, body=True) and lib.bdm_last_error(), what
    assert lib.bdm_surface_poisson_grid(0, 300, R, s, cycles, None, None, None, None, None, L.stream()) == 0
    assert lib.bdm_surface_poisson_density(0, R, None, None, None, L.stream()) == 0
