"""The solid-voxelisation rule on the CPU: the restatement tests/mesh_voxel_ref.py against closed forms on hand-built meshes and
against the consequence of the rule on closed meshes (the three rays agree on every cell), its mutants, the snap and its guard, the
IoU, the binvox reader and writer, and the host side of bdm_amd.mesh_voxel and of its command line.  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

import mesh_voxel_ref as R
from bdm_amd import _lib as L
from bdm_amd import mesh_voxel as MV
from bdm_amd.io import load_binvox, load_mesh_ply, save_binvox, save_mesh_ply, save_pointcloud_ply
from bdm_amd.ragged import mesh_lists


def _hand(name, Rs=8, **kw):
    v, f, o, c = R.hand_meshes()[name]
    return R.voxelize(v, f, Rs, o, c, **kw)


def _block(Rs, lo, hi):
    want = torch.zeros(Rs, Rs, Rs, dtype=torch.bool)
    want[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return want


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_lattice_box_is_the_low_inclusive_high_exclusive_block_on_all_three_axes():
    """Every face of the box passes exactly through cell centres: the perturbed centre (+eps, +eps^2, +eps^3) is inside at the low
    faces and outside at the high ones."""
    r = _hand("lattice_box")
    want = _block(8, (1, 2, 1), (6, 5, 7))
    for axis, grid in zip("xyz", r["inside"]):
        assert torch.equal(grid, want), axis
    assert torch.equal(r["occupancy"], want) and torch.equal(r["axes"], want.to(torch.uint8) * 7)
    assert r["counts"] == [12, 0, 90, 90, 90, 90, 0, 0] and list(r["info"]) == list(R.COUNT_KEYS)
    cube = _hand("lattice_cube")   # the face diagonals pass through centres as well
    assert all(torch.equal(g, _block(8, (1, 1, 1), (6, 6, 6))) for g in cube["inside"])


@pytest.mark.parametrize("name", ["octahedron", "uv_sphere"])
def test_the_three_axis_grids_of_a_closed_hand_mesh_are_equal(name):
    r = _hand(name)
    assert torch.equal(r["inside"][0], r["inside"][1]) and torch.equal(r["inside"][1], r["inside"][2])
    assert r["counts"][6] == 0 and r["counts"][5] > 30
    if name == "octahedron":   # |dx| + |dy| + |dz| < 3 around cell 3, ties decided by the perturbation: a vertex cell is in on the low side
        inside = r["occupancy"]
        assert bool(inside[3, 3, 3]) and bool(inside[0, 3, 3]) and not bool(inside[6, 3, 3]) and not bool(inside[3, 3, 6])
    else:
        v, f, _, _ = R.hand_meshes()[name]
        assert f.shape[0] == 2208
        fine = R.voxelize(v, f, 32)   # the volume of the polyhedron, within the cells its surface crosses
        assert abs(fine["counts"][5] / 32 ** 3 - (4 / 3 * math.pi * 0.4 ** 3) / (0.8 ** 3)) < 0.02


def test_every_closed_mesh_of_the_batch_has_no_disagreeing_cell():
    closed = 0
    for row in R.batch():
        name, v, f, _, _ = row
        if f.shape[0] == 0 or R.odd_degree_edges(f, v.shape[0]):
            continue
        for Rs in (8, 32):
            r = R.voxelize(v, f, Rs, *R.frame_of(row, Rs))
            assert r["counts"][6] == 0 and r["counts"][2] == r["counts"][3] == r["counts"][4] == r["counts"][5], (name, Rs, r["counts"])
        closed += 1
    names = [n for n, *_ in R.batch()]
    assert closed >= 10 and all(k in names for k in ("sphere", "torus", "ellipsoid", "two_spheres"))
    for k in ("sphere", "torus", "ellipsoid", "two_spheres"):
        v, f = R.surface_mesh(k)
        assert R.odd_degree_edges(f, v.shape[0]) == 0 and f.shape[0] > 200, k


def test_an_open_mesh_disagrees_and_the_vote_is_the_majority():
    v, f = R.surface_mesh("open_sphere")
    assert R.odd_degree_edges(f, v.shape[0]) > 0
    r = R.voxelize(v, f, 32)
    assert r["counts"][6] > 1000 and len({r["counts"][2], r["counts"][3], r["counts"][4]}) > 1
    votes = sum(g.long() for g in r["inside"])
    assert torch.equal(r["occupancy"], votes >= 2) and r["counts"][6] == int(((votes == 1) | (votes == 2)).sum())
    for k, mode in enumerate("xyz"):
        one = R.voxelize(v, f, 32, mode=mode)
        assert torch.equal(one["occupancy"], r["inside"][k]) and one["counts"][5] == r["counts"][2 + k] and one["counts"][:5] == r["counts"][:5]
    box = _hand("open_box")   # two faces of one side are missing: the ray that leaves through the hole is the one that is wrong
    assert box["counts"][2] == 0 and box["counts"][3] == box["counts"][4] == box["counts"][5] > 0 and box["counts"][6] == box["counts"][5]


def test_reversing_the_winding_of_every_other_face_changes_nothing():
    a, b = _hand("uv_sphere"), _hand("uv_sphere_mixed_winding")
    assert torch.equal(a["axes"], b["axes"]) and a["counts"] == b["counts"]
    for name in ("octahedron", "lattice_box", "big_triangle"):
        v, f, o, c = R.hand_meshes()[name]
        assert torch.equal(R.voxelize(v, f, 8, o, c)["axes"], R.voxelize(v, R.reversed_every_other(f), 8, o, c)["axes"]), name
        assert torch.equal(R.voxelize(v, f, 8, o, c)["axes"], R.voxelize(v, f[:, [0, 2, 1]], 8, o, c)["axes"]), name


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _snap_box():
    """A box whose high faces lie 0.6 / 256 of a cell above cell centres: rounded they are above the centre (the cell is inside),
    truncated they are on it (high-exclusive: outside)."""
    hi = 4.5 + 0.6 / 256
    return R.box((1.5, 1.5, 1.5), (hi, hi, hi))


def test_every_mutant_is_told_apart_on_a_hand_mesh():
    v, f, o, c = R.hand_meshes()["octahedron"]
    base = R.voxelize(v, f, 8, o, c)
    for mutant in ("render_owns", "tie_not_below", "owns_both", "no_swap", "cyclic_uv"):
        assert not torch.equal(R.voxelize(v, f, 8, o, c, mutant=mutant)["axes"], base["axes"]), mutant
    v, f, o, c = R.hand_meshes()["lattice_box"]
    base = R.voxelize(v, f, 8, o, c)
    for mutant in ("render_owns", "owns_both", "no_swap"):
        assert not torch.equal(R.voxelize(v, f, 8, o, c, mutant=mutant)["axes"], base["axes"]), mutant
    v, f = _snap_box()
    base, cut = R.voxelize(v, f, 8, (0, 0, 0), 1.0), R.voxelize(v, f, 8, (0, 0, 0), 1.0, mutant="truncate_snap")
    assert torch.equal(base["occupancy"], _block(8, (1, 1, 1), (5, 5, 5))) and torch.equal(cut["occupancy"], _block(8, (1, 1, 1), (4, 4, 4)))
    assert set(R.MUTANTS) == {"render_owns", "tie_not_below", "owns_both", "no_swap", "cyclic_uv", "truncate_snap"}


# ---- the snap, its guard, dropped faces -------------------------------------------------------------------------------------------------
def test_a_vertex_exactly_at_a_half_snaps_half_even():
    x = [0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, -1.5 / 256, 3.25 / 256]
    q, usable = R.snap(np.array([[a, 0, 0] for a in x], dtype=np.float32), (0, 0, 0), 1.0)
    assert q[:, 0].tolist() == [0, 2, 2, 0, -2, 3] and usable.all()
    q, _ = R.snap(np.array([[1.0 + 2.5 / 256, 0, 0]], dtype=np.float32), (1.0, 0, 0), 1.0)   # the subtraction is exact, the tie survives
    assert q[0, 0] == 2
    q, _ = R.snap(np.array([[0.1, 0.7, 1.3]], dtype=np.float32), (0.05, -0.2, 0.3), 0.37)     # float32, operation by operation
    want = [int(np.rint(np.float32(np.float32(np.float32(a) - np.float32(b)) / np.float32(0.37)) * np.float32(256))) for a, b in
            ((0.1, 0.05), (0.7, -0.2), (1.3, 0.3))]
    assert q[0].tolist() == want


def test_a_vertex_at_the_guard_is_usable_and_one_step_beyond_drops_its_faces():
    v, f, o, c = R.hand_meshes()["beyond_guard"]
    q, usable = R.snap(v.numpy(), o, c)
    assert q[8, 0] == 2 ** 19 and usable[8] and not usable[9] and usable[:8].all()
    r = R.voxelize(v, f, 8, o, c)
    assert r["counts"][:2] == [13, 1]
    q, usable = R.snap(np.array([[-2048.0, 0, 0], [-2048.00390625, 0, 0], [3e38, 0, 0]], dtype=np.float32), (0, 0, 0), 1.0)
    assert usable.tolist() == [True, False, False]
    q, usable = R.snap(np.array([[3e38, 0, 0]], dtype=np.float32), (-3e38, 0, 0), 1.0)   # the difference overflows: unusable, no error
    assert not usable[0]


def test_faces_with_bad_indices_or_non_finite_vertices_are_dropped_and_counted():
    v, f, o, c = R.hand_meshes()["bad_indices"]
    plain = R.voxelize(v, f[:12], 8, o, c)   # the box alone
    bad, nonfinite = _hand("bad_indices"), _hand("nonfinite")
    assert bad["counts"][:2] == [12, 3] and nonfinite["counts"][:2] == [12, 2]
    assert torch.equal(bad["axes"], plain["axes"]) and torch.equal(nonfinite["axes"], plain["axes"]) and plain["counts"][6] == 0


def test_a_face_above_the_grid_flips_its_whole_columns_and_one_below_flips_nothing():
    v, f, o, c = R.hand_meshes()["above_and_below"]
    q, _ = R.snap(v.numpy(), o, c)
    above = R.axis_flips(q, f[:1].numpy(), 8, 2)
    assert above.sum() == above[:, :, 7].sum() == 10 and bool((above[:, :, :7] == 0).all())   # c == R: the flip sits on the top cell
    assert R.axis_flips(q, f[1:].numpy(), 8, 2).sum() == 0                                      # c == 0
    r = R.voxelize(v, f, 8, o, c)
    column = r["inside"][2].all(dim=2)
    assert int(column.sum()) == 10 and bool((r["inside"][2].any(dim=2) == column).all()) and r["counts"][4] == 80
    assert r["counts"][2] == r["counts"][3] == 0 and r["counts"][5] == 0 and r["counts"][6] == 80


def test_an_empty_mesh_and_a_mesh_without_faces():
    for name in ("empty", "no_faces"):
        r = _hand(name)
        assert r["counts"] == [0] * 8 and not bool(r["occupancy"].any()) and r["occupancy"].shape == (8, 8, 8)
    o, h = R.default_frame(np.zeros((0, 3), dtype=np.float32), 4)
    assert o.tolist() == [0, 0, 0] and h == np.float32(0.25)
    o, h = R.default_frame(np.array([[1, 2, 3], [1, 2, 3], [np.nan, 0, 0]], dtype=np.float32), 4)   # zero extent: side 1
    assert o.tolist() == [1, 2, 3] and h == np.float32(0.25)
    o, h = R.default_frame(np.array([[0, 0, 0], [3, 1, 2]], dtype=np.float32), 6)
    assert o.tolist() == [0, 0, 0] and h == np.float32(0.5)


# ---- IoU ------------------------------------------------------------------------------------------------------------------------------
def test_iou_of_identical_disjoint_overlapping_and_empty_grids():
    a = R.voxelize(*R.lattice_box((1, 1, 1), (5, 5, 5)), 8, (0, 0, 0), 1.0)["occupancy"]
    b = R.voxelize(*R.lattice_box((3, 1, 1), (7, 5, 5)), 8, (0, 0, 0), 1.0)["occupancy"]
    c = R.voxelize(*R.lattice_box((5, 5, 5), (7, 7, 7)), 8, (0, 0, 0), 1.0)["occupancy"]
    none = torch.zeros(8, 8, 8, dtype=torch.bool)
    assert R.iou(a, a) == (1.0, 64, 64) and R.iou(a, c) == (0.0, 0, 72) and R.iou(a, b) == (32 / 96, 32, 96)
    assert math.isnan(R.iou(none, none)[0]) and R.iou(none, none)[1:] == (0, 0)
    iou, inter, union = MV.voxel_iou(torch.stack([a, a, a, none]), torch.stack([a, c, b, none]))
    assert iou.dtype == torch.float64 and inter.dtype == torch.int64 and inter.tolist() == [64, 0, 32, 0] and union.tolist() == [64, 72, 96, 0]
    assert iou[:3].tolist() == [1.0, 0.0, 32 / 96] and math.isnan(float(iou[3]))
    single = MV.voxel_iou(a.to(torch.uint8), b.to(torch.uint8))
    assert single[0].shape == () and float(single[0]) == 32 / 96
    with pytest.raises(ValueError):
        MV.voxel_iou(a, torch.zeros(4, 4, 4))


# ---- binvox ---------------------------------------------------------------------------------------------------------------------------
def test_binvox_reads_a_hand_written_file_in_its_order(tmp_path):
    # linear index x D^2 + z D + y at D = 2: cells (x, y, z) = (0,0,0) (0,1,0) (0,0,1) (0,1,1) (1,0,0) (1,1,0) (1,0,1) (1,1,1)
    body = bytes([1, 1, 0, 2, 1, 1, 0, 3, 1, 1])   # set: linear 0, 3, 7 -> (0,0,0), (0,1,1), (1,1,1)
    path = tmp_path / "hand.binvox"
    path.write_bytes(b"#binvox 1\ndim 2 2 2\ntranslate -0.5 0.25 1\nscale 2.5\ndata\n" + body)
    vox, translate, scale = load_binvox(path)
    assert vox.dtype == bool and vox.shape == (2, 2, 2) and translate.tolist() == [-0.5, 0.25, 1.0] and scale == 2.5
    assert sorted(map(tuple, np.argwhere(vox).tolist())) == [(0, 0, 0), (0, 1, 1), (1, 1, 1)]
    one = np.zeros((2, 2, 2), dtype=bool)
    one[1, 0, 1] = True   # linear 4 + 2 + 0 = 6
    save_binvox(one, tmp_path / "one.binvox", (0, 0, 0), 1.0)
    assert (tmp_path / "one.binvox").read_bytes().split(b"data\n", 1)[1] == bytes([0, 6, 1, 1, 0, 1])


def test_binvox_splits_long_runs_and_a_round_trip_is_the_identity(tmp_path):
    g = np.random.default_rng(7)
    grids = [np.zeros((8, 8, 8), dtype=bool), np.ones((7, 7, 7), dtype=bool), g.random((9, 9, 9)) < 0.4, g.random((32, 32, 32)) < 0.02]
    grids[0][3, 4, 5] = True
    for k, vox in enumerate(grids):
        path = tmp_path / "sub" / f"{k}.binvox"
        save_binvox(vox, path, (0.125, -3.0, 1e-3), 0.7)
        raw = path.read_bytes()
        assert raw == R.binvox_bytes(vox, (0.125, -3.0, 1e-3), 0.7), k   # the restatement's loop over the cells
        pairs = np.frombuffer(raw.split(b"data\n", 1)[1], dtype=np.uint8).reshape(-1, 2)
        assert pairs[:, 1].min() >= 1 and int(pairs[:, 1].astype(np.int64).sum()) == vox.size
        back, translate, scale = load_binvox(path)
        assert np.array_equal(back, vox) and translate.tolist() == [0.125, -3.0, 1e-3] and scale == 0.7
    runs = np.frombuffer((tmp_path / "sub" / "1.binvox").read_bytes().split(b"data\n", 1)[1], dtype=np.uint8).reshape(-1, 2)
    assert runs.tolist() == [[1, 255], [1, 343 - 255]]


def test_malformed_binvox_files_raise(tmp_path):
    good = R.binvox_bytes(np.ones((2, 2, 2), dtype=bool))
    head, body = good.split(b"data\n", 1)
    cases = {
        "magic": good.replace(b"#binvox 1", b"#binvoy 1"),
        "not_cubic": good.replace(b"dim 2 2 2", b"dim 2 2 4"),
        "no_scale": good.replace(b"scale 1.0\n", b""),
        "order": good.replace(b"dim 2 2 2\n", b"").replace(b"data\n", b"dim 2 2 2\ndata\n"),
        "short": head + b"data\n" + bytes([1, 7]),
        "long": head + b"data\n" + bytes([1, 8, 0, 1]),
        "odd": good + b"\x01",
        "value": head + b"data\n" + bytes([2, 8]),
        "zero_count": head + b"data\n" + bytes([1, 8, 0, 0]),
        "truncated_header": b"#binvox 1\ndim 2 2 2\n",
        "words": good.replace(b"dim 2 2 2", b"dim two 2 2"),
    }
    for name, raw in cases.items():
        path = tmp_path / f"{name}.binvox"
        path.write_bytes(raw)
        with pytest.raises(ValueError):
            load_binvox(path)
    with pytest.raises(ValueError):
        save_binvox(np.zeros((2, 2, 3), dtype=bool), tmp_path / "x.binvox")


# ---- the Python surface, host side ----------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    v, f, _, _ = R.hand_meshes()["octahedron"]
    mesh = ([v], [f])
    for kw in (dict(resolution=0), dict(resolution=513), dict(resolution=8.0), dict(resolution=True), dict(mode="w"), dict(mode=0),
               dict(origin=(0, 0, 0)), dict(cell_size=1.0), dict(origin=(0, 0, 0), cell_size=0.0), dict(origin=(0, 0, 0), cell_size=-1.0),
               dict(origin=(0, 0, 0), cell_size=float("inf")), dict(origin=(0, float("nan"), 0), cell_size=1.0),
               dict(origin=(0, 0), cell_size=1.0), dict(origin=(0, 0, 0), cell_size=[1.0, 2.0]), dict(origin=[[0, 0, 0]] * 2, cell_size=1.0)):
        with pytest.raises(ValueError):
            MV.voxelize_meshes(mesh, **kw)
        with pytest.raises(ValueError):
            MV.volumetric_iou(mesh, mesh, **kw)
    with pytest.raises(ValueError, match="2\\^31"):
        MV.voxelize_meshes(([v] * 17, [f] * 17), resolution=512)
    with pytest.raises(ValueError):
        MV.voxelize_meshes(([v], [f.float()]))
    with pytest.raises(ValueError):
        MV.voxelize_meshes(v)
    with pytest.raises(ValueError, match="against"):
        MV.volumetric_iou(mesh, ([v, v], [f, f]))
    with pytest.raises(L.BdmHipError, match="CPU tensor"):   # no CPU path
        MV.voxelize_meshes(mesh, resolution=8)
    with pytest.raises(L.BdmHipError, match="CPU tensor"):
        MV.volumetric_iou(mesh, mesh, resolution=8)
    grids, info = MV.voxelize_meshes(([], []), resolution=4, return_info=True)
    assert grids.shape == (0, 4, 4, 4) and grids.dtype == torch.bool and list(info["counts"]) == list(R.COUNT_KEYS)
    assert MV.volumetric_iou(([], []), ([], [])).shape == (0,)
    assert MV.COUNT_KEYS == R.COUNT_KEYS and MV.MODES == R.MODES and MV.MAX_R == R.MAX_R


def test_the_host_frames_are_the_restatements():
    rows = [r for r in R.batch() if r[0] in ("uv_sphere", "tilted_box", "empty", "nonfinite", "open_sphere")]
    verts = [v for _, v, *_ in rows] + [torch.tensor([[1.0, 2.0, 3.0]]), torch.tensor([[float("nan"), 0.0, 0.0]])]
    for Rs in (8, 33):
        origin, cell = MV._cube_frame(MV._bounds(verts), Rs)
        for m, v in enumerate(verts):
            o, h = R.default_frame(v.numpy(), Rs)
            assert origin[m].tolist() == o.tolist() and cell[m] == h and cell.dtype == np.float32, m
    both = MV._bounds(verts[:2] + verts[2:4])
    pair = np.stack([np.minimum(both[:2, 0], both[2:, 0]), np.maximum(both[:2, 1], both[2:, 1])], axis=1)
    origin, cell = MV._cube_frame(pair, 16)
    for m in range(2):
        o, h = R.pair_frame(verts[m].numpy(), verts[2 + m].numpy(), 16)
        assert origin[m].tolist() == o.tolist() and cell[m] == h


# ---- the command line with the kernel replaced by the restatement ---------------------------------------------------------------------
def _ref_voxelize(meshes, resolution=32, *, origin=None, cell_size=None, mode="vote", return_info=False):
    verts_list, faces_list = mesh_lists(meshes)
    B = len(verts_list)
    frame = MV._given_frame(origin, cell_size, B)
    o, h = frame if frame is not None else MV._cube_frame(MV._bounds(verts_list), resolution)
    runs = [R.voxelize(v, f, resolution, o[m], h[m], mode) for m, (v, f) in enumerate(zip(verts_list, faces_list))]
    grids = torch.stack([r["occupancy"] for r in runs])
    counts = torch.tensor([r["counts"] for r in runs], dtype=torch.int64)
    info = {"counts": {k: counts[:, i] for i, k in enumerate(R.COUNT_KEYS)}, "axes": torch.stack([r["axes"] for r in runs]),
            "origin": torch.from_numpy(np.array(o)), "cell_size": torch.from_numpy(np.array(h))}
    return (grids, info) if return_info else grids


@pytest.fixture
def ref_kernel(monkeypatch):
    monkeypatch.setattr(MV, "voxelize_meshes", _ref_voxelize)


def _tree(tmp_path):
    """Three predicted meshes; ground truth: a mesh for two of them, a binvox grid for the third."""
    sv, sf = R.surface_mesh("sphere")
    tv, tf = R.surface_mesh("torus")
    ov, of = R.surface_mesh("open_sphere")
    ev, ef = R.surface_mesh("ellipsoid")
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "a" / "sphere.ply")
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "mesh" / "a" / "torus.ply")
    save_mesh_ply(ov.numpy(), of.numpy(), tmp_path / "mesh" / "b" / "open.ply")
    save_mesh_ply(ev.numpy(), ef.numpy(), tmp_path / "gt" / "a" / "sphere.ply")
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "gt" / "a" / "torus.ply")
    truth = R.voxelize(sv, sf, 16, (-0.5, -0.5, -0.5), 1.0 / 16)["occupancy"]
    save_binvox(truth.numpy(), tmp_path / "gt" / "b" / "open.binvox", (-0.5, -0.5, -0.5), 1.0)
    return (sv, sf), (tv, tf), (ov, of), (ev, ef), truth


def test_cli_walk_with_the_kernel_replaced_by_the_restatement(ref_kernel, tmp_path, capsys):
    (sv, sf), (tv, tf), (ov, of), (ev, ef), truth = _tree(tmp_path)
    got = MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "gt", resolution=24, batch_size=2, out_dir=tmp_path / "out", device="cpu")
    assert list(got) == ["num", "iou", "empty", "disagree_fraction", "faces_dropped"]
    o, h = R.pair_frame(sv.numpy(), ev.numpy(), 24)
    a, b = R.voxelize(sv, sf, 24, o, h), R.voxelize(ev, ef, 24, o, h)
    to, th = R.default_frame(tv.numpy(), 24)
    t = R.voxelize(tv, tf, 24, to, th)
    p = R.voxelize(ov, of, 16, (-0.5, -0.5, -0.5), np.float32(1.0) / np.float32(16))
    ious = [R.iou(a["occupancy"], b["occupancy"])[0], 1.0, R.iou(p["occupancy"], truth)[0]]
    assert got["num"] == 3 and got["empty"] == 0 and got["faces_dropped"] == 0 and got["iou"] == sum(ious) / 3 and 0.2 < ious[0] < 0.9
    assert got["disagree_fraction"] == (0 + 0 + p["counts"][6] / 16 ** 3) / 3 and p["counts"][6] > 0
    for rel, want, origin, side in (("a/sphere", a, o, np.float32(h) * np.float32(24)), ("a/torus", t, to, np.float32(th) * np.float32(24)),
                                    ("b/open", p, (-0.5, -0.5, -0.5), 1.0)):
        vox, translate, scale = load_binvox(tmp_path / "out" / (rel + ".binvox"))
        assert np.array_equal(vox, want["occupancy"].numpy()) and translate.tolist() == [float(x) for x in origin] and scale == float(side), rel
    # one axis alone (main() itself needs a device and is run by the GPU test)
    z = MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "gt", resolution=24, mode="z", batch_size=16, device="cpu")
    assert z["num"] == 3 and z["iou"] != got["iou"] and z["disagree_fraction"] == got["disagree_fraction"]
    assert json.loads(json.dumps(got)) == got
    args = MV.parse_args(["--mesh_dir", "m", "--gt_dir", "g"])
    assert (args.resolution, args.mode, args.batch_size, args.out_dir) == (32, "vote", 16, None)
    for bad in (["--resolution", "0"], ["--resolution", "513"], ["--mode", "w"], ["--batch-size", "0"]):
        with pytest.raises(SystemExit):
            MV.parse_args(["--mesh_dir", "m", "--gt_dir", "g"] + bad)
    capsys.readouterr()


def test_cli_refuses_a_ground_truth_cloud_and_a_missing_file(ref_kernel, tmp_path):
    sv, sf = R.surface_mesh("sphere")
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "s.ply")
    save_pointcloud_ply(sv.numpy(), str(tmp_path / "gt" / "s.ply"))
    with pytest.raises(ValueError, match="python -m bdm_amd.surface"):
        MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "gt", device="cpu")
    save_mesh_ply(sv.numpy(), np.zeros((0, 3), dtype=np.int64), tmp_path / "gt2" / "s.ply")   # a mesh file without a face
    with pytest.raises(ValueError, match="python -m bdm_amd.surface"):
        MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "gt2", device="cpu")
    with pytest.raises(FileNotFoundError):
        MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "nothing", device="cpu")
    with pytest.raises(ValueError):
        MV.evaluate_voxel_dirs(tmp_path / "mesh", tmp_path / "gt", batch_size=0, device="cpu")
    empty = MV.evaluate_voxel_dirs(tmp_path / "nothing", tmp_path / "gt", device="cpu")
    assert empty == {"num": 0, "iou": None, "empty": 0, "disagree_fraction": 0.0, "faces_dropped": 0}
    assert load_mesh_ply(tmp_path / "mesh" / "s.ply")[1].shape[0] == sf.shape[0]
