"""The hole-filling rule on the CPU: the restatement tests/mesh_fill_ref.py against literal expectations on hand-built meshes and
against the rule's three post-conditions on surface_ref meshes, its mutants, the derived bound of the fixed-point mean, and the host
side of bdm_amd.mesh_fill and of both command lines.  No GPU."""
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_clean_ref as CR
import mesh_fill_ref as R
from bdm_amd import mesh_clean as MC
from bdm_amd import mesh_fill as MF
from bdm_amd.ragged import mesh_lists


def _fill(name, **kw):
    v, f, cap = {**R.hand_meshes(), **R.nonfinite_meshes()}[name]
    return R.fill(v, f, cap, **kw), v, f


# ---- literal expectations -------------------------------------------------------------------------------------------------------------
def test_open_tetrahedron_gets_one_vertex_and_three_faces_wound_like_their_neighbours():
    r, v, f = _fill("tetra_open")
    assert r["loop_sizes"].tolist() == [3] and r["loop_flags"].tolist() == [R.FILLED] and r["labels"] == [2]
    assert r["halfedge_loop"].tolist() == [[-1, -1, 2], [2, -1, -1], [-1, 2, -1]]
    assert r["faces"].tolist() == [[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 4], [3, 0, 4], [2, 3, 4]]
    assert r["verts"].shape == (5, 3) and torch.equal(r["verts"][:4], v)
    assert torch.allclose(r["verts"][4].double(), v[[2, 0, 3]].double().mean(0), atol=1e-7)
    assert r["info"] == dict(zip(R.INFO_KEYS, (3, 1, 1, 0, 0, 0, 0, 1, 3)))


def test_two_holes_that_touch_at_a_vertex_are_paired_by_rotation():
    r, v, f = _fill("two_triangles_one_vertex")
    assert r["loop_sizes"].tolist() == [3, 3] and r["loop_flags"].tolist() == [R.FILLED, R.FILLED] and r["labels"] == [0, 3]
    assert r["verts"].shape[0] == 7 and r["faces"].shape[0] == 8
    assert r["faces"][2:].tolist() == [[1, 0, 5], [2, 1, 5], [0, 2, 5], [3, 0, 6], [4, 3, 6], [0, 4, 6]]


def test_irregular_edges_block_their_boundary_and_nothing_is_added():
    for name, n in (("fin", 6), ("same_winding", 4)):
        r, v, f = _fill(name)
        assert r["info"]["boundary_edges"] == n and r["info"]["blocked_edges"] == n and r["info"]["loops"] == 0, name
        assert int((r["halfedge_loop"] == -2).sum()) == n and torch.equal(r["verts"], v) and torch.equal(r["faces"], f), name


def test_pinched_too_large_and_non_finite_loops_stay_open_and_are_counted():
    r, v, f = _fill("octa_pinched")
    assert r["loop_sizes"].tolist() == [6] and r["loop_flags"].tolist() == [R.PINCHED] and r["info"]["pinched_loops"] == 1
    assert torch.equal(r["faces"], f) and torch.equal(r["verts"], v)
    r, v, f = _fill("octa_too_large")
    assert r["loop_sizes"].tolist() == [4] and r["loop_flags"].tolist() == [R.TOO_LARGE] and r["info"]["too_large_loops"] == 1 and r["faces"].shape == f.shape
    assert R.fill(v, f, 4)["info"]["filled_loops"] == 1 and R.fill(v, f, 4)["faces"].shape[0] == f.shape[0] + 4
    r, v, f = _fill("nan_on_rim")
    assert r["loop_flags"].tolist() == [R.NONFINITE] and r["info"]["nonfinite_loops"] == 1 and r["faces"].shape == f.shape
    r, v, f = _fill("inf_off_rim")
    assert r["loop_flags"].tolist() == [R.FILLED] and bool(torch.isfinite(r["verts"][6]).all())


def test_faces_that_are_not_connected_are_passed_through_in_place():
    r, v, f = _fill("octa_bad_faces")
    assert r["info"]["filled_loops"] == 1 and torch.equal(r["faces"][:9], f) and r["faces"][7:9].tolist() == [[0, 0, 1], [0, 1, 9]]
    assert r["faces"][9:].tolist() == [[2, 0, 6], [0, 1, 6], [1, 2, 6]] and r["halfedge_loop"][7:].tolist() == [[-1] * 3] * 2


def test_empty_meshes_are_legal_and_come_back_unchanged():
    for name in ("empty", "no_faces", "octa_closed"):
        r, v, f = _fill(name)
        assert torch.equal(r["verts"], v) and torch.equal(r["faces"], f) and r["info"] == dict.fromkeys(R.INFO_KEYS, 0), name
        assert r["halfedge_loop"].shape == (f.shape[0], 3) and r["loop_sizes"].numel() == 0


def test_attributes_ride_along_and_a_non_finite_channel_gives_nan():
    v, f, cap = R.hand_meshes()["tetra_open"]
    attrs = torch.tensor([[10.0, 1.0], [20.0, float("nan")], [30.0, 2.0], [41.0, float("inf")]])
    r = R.fill(v, f, cap, attrs=attrs)
    assert r["attrs"].shape == (5, 2) and R.same_floats(r["attrs"][:4], attrs)
    assert float(r["attrs"][4, 0]) == 27.0 and bool(torch.isnan(r["attrs"][4, 1]))   # loop vertices 2, 0, 3: (30 + 10 + 41) / 3; the inf is on the loop
    assert R.uint8_mean([1, 2]) == 2 and R.uint8_mean([2, 3]) == 2 and R.uint8_mean([255, 255, 255]) == 255 and R.uint8_mean([0, 0, 1]) == 0
    # the float32 mean of uint8 values, rounded half to even, is the integer rule (mesh_fill.py rounds the kernel's float32 this way)
    g = torch.Generator().manual_seed(7)
    for n in (2, 3, 4, 6, 7, 32, 64):
        for _ in range(50):
            col = torch.randint(0, 256, (n,), generator=g).tolist()
            fm = R.fixed_mean(np.asarray(col, dtype=np.float32), R.scale_exp(np.float32(255)))
            assert int(MF._round_uint8(torch.tensor([float(fm)]))) == R.uint8_mean(col), col


def test_fans_put_hub_segments_on_both_sides_of_the_sort_threshold():
    """A vertex has two records per connected face around it; the kernel sorts up to 32 by insertion and more by heap sort."""
    want = {"fan_16": (32, R.FILLED), "fan_17": (34, R.FILLED), "fan_70": (140, R.TOO_LARGE)}
    for name, (v, f, cap) in R.fan_meshes().items():
        records = 2 * torch.bincount(f.flatten(), minlength=v.shape[0])
        assert cap == 64 and int(records[0]) == want[name][0] and int(records[1:].max()) == 4, name
        r = R.fill(v, f, cap)
        assert r["labels"] == [1] and r["loop_sizes"].tolist() == [f.shape[0]] and r["loop_flags"].tolist() == [want[name][1]], name
        filled = want[name][1] == R.FILLED
        assert r["faces"].shape[0] == f.shape[0] * (2 if filled else 1) and r["verts"].shape[0] == v.shape[0] + filled, name
        assert R.fill(v, f, 3)["loop_flags"].tolist() == [R.TOO_LARGE] and R.fill(v, f, 3)["info"]["new_faces"] == 0, name


def test_closed_form_of_separate_triangles_is_what_fill_gives():
    """tests/test_hip_mesh_fill.py uses the closed form at a size where fill()'s loop over the half-edges takes seconds."""
    v, f = R.separate_triangles(64, 10, 77)
    r, c = R.fill(v, f, 32), R.separate_triangles_filled(f, v.shape[0])
    assert v.shape[0] == 202 and sorted(c) == ["faces", "halfedge_loop", "info", "labels", "loop_flags", "loop_sizes"]
    assert all(torch.equal(r[k], c[k]) for k in ("faces", "halfedge_loop", "loop_sizes", "loop_flags")) and r["labels"] == c["labels"] and r["info"] == c["info"]
    e = R.scale_exp(v.numpy())
    means = np.stack([[R.fixed_mean(v.numpy()[tri, d], e) for d in range(3)] for tri in f.tolist()])
    assert R.same_floats(r["verts"][:202], v) and R.same_floats(r["verts"][202:], torch.from_numpy(means))


# ---- the post-conditions on meshes of the mesher ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, loops, filled", [("sphere600", 48, 44), ("torus1500", 1, 1), ("lattice32", 1, 0)])
def test_post_conditions_on_surface_meshes(name, loops, filled):
    from bdm_amd.surface import mesh_stats
    v, f = R.surface_mesh(name)
    r = R.fill(v, f, 64)
    before, after = mesh_stats(v, f), mesh_stats(r["verts"], r["faces"])
    print(name, r["info"], before["open_edges"], after["open_edges"], before["euler_characteristic"], after["euler_characteristic"])
    assert (r["info"]["loops"], r["info"]["filled_loops"]) == (loops, filled) and r["info"]["blocked_edges"] == 0
    filled_edges = int(r["loop_sizes"][r["loop_flags"] == R.FILLED].sum())
    assert before["open_edges"] - after["open_edges"] == filled_edges == r["info"]["new_faces"]
    assert before["inconsistent_edges"] == after["inconsistent_edges"]
    assert after["euler_characteristic"] - before["euler_characteristic"] == r["info"]["filled_loops"]
    assert int(r["loop_sizes"].sum()) == r["info"]["boundary_edges"] == before["open_edges"] and int(r["loop_sizes"].min()) >= 3
    if name == "torus1500":
        assert r["loop_sizes"].tolist() == [14] and after["open_edges"] == 0 and after["euler_characteristic"] == 0
    if name == "lattice32":
        assert r["loop_sizes"].tolist() == [104] and torch.equal(r["faces"], f)
    if name == "sphere600":
        assert abs(after["signed_volume"]) > abs(before["signed_volume"])   # closer to the sphere's 0.268


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (torch.equal(a["faces"], b["faces"]) and R.same_floats(a["verts"], b["verts"]) and torch.equal(a["halfedge_loop"], b["halfedge_loop"])
            and a["info"] == b["info"])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_an_output_of_the_gpu_inputs(mutant):
    told = [name for name, v, f, cap in R.batch() if not _same(R.fill(v, f, cap), R.fill(v, f, cap, mutant=mutant))]
    print(mutant, told)
    assert told, f"no case tells {mutant} from the rule"


# ---- the mean -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale, shift", [(1e-3, (0, 0, 0)), (1.0, (0, 0, 0)), (1e3, (0, 0, 0)), (1.0, (100.0, -50.0, 25.0))])
def test_fixed_point_mean_stays_within_the_derived_bound_of_the_exact_mean(scale, shift):
    g = torch.Generator().manual_seed(23)
    worst = 0.0
    for n in (3, 4, 7, 32, 64, 1000):
        v = ((torch.rand(n + 5, 3, generator=g, dtype=torch.float64) - 0.5) * scale + torch.tensor(shift, dtype=torch.float64)).float().numpy()
        e = R.scale_exp(v)
        for d in range(3):
            col = v[:n, d]
            exact = sum(Fraction(float(c)) for c in col) / n
            got = R.fixed_mean(col, e)
            bound = R.mean_bound(v, float(exact))
            err = abs(Fraction(float(got)) - exact)
            worst = max(worst, float(err) / bound)
            assert err <= Fraction(bound), (n, d, float(err), bound)
            assert abs(float(got) - float(np.mean(col.astype(np.float64)))) <= bound * (1 + 1e-6) + n * 2.0 ** -52 * float(np.abs(col).max())
    print(f"scale {scale} shift {shift}: worst error / bound = {worst:.3f}")
    assert all(abs(round(float(c) * 2.0 ** e)) < 2 ** 40 for c in v.reshape(-1))


# ---- the host side of the module ------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    from bdm_amd import _lib as L
    v, f, _ = R.hand_meshes()["tetra_open"]
    for cap in (2, 0, -1, 65536, 3.5, "4", True, None):
        with pytest.raises(ValueError):
            MF.fill_holes(([v], [f]), cap)
        with pytest.raises(ValueError):
            MF.boundary_loops(([v], [f]), cap)
    for colours in ([], [torch.zeros(3, 3)], [torch.zeros(4)], [torch.zeros(4, 17)], [torch.zeros(4, 3, dtype=torch.int32)], torch.zeros(4, 3)):
        with pytest.raises(ValueError):
            MF.fill_holes(([v], [f]), colors_list=colours)
    with pytest.raises(ValueError):
        MF.fill_holes(([v, v], [f, f]), colors_list=[torch.zeros(4, 3), torch.zeros(4, 2)])   # one width per batch
    for fn in (MF.fill_holes, MF.boundary_loops):
        with pytest.raises(ValueError):
            fn(v)
        with pytest.raises(ValueError):
            fn(([v], [f.float()]))
        with pytest.raises(L.BdmHipError):
            fn(([v], [f]))                                       # host tensors: no CPU path
    assert MF.fill_holes(([], [])) == ([], []) and MF.fill_holes(([], []), colors_list=[], return_info=True) == ([], [], [], [])
    assert MF.INFO_KEYS == R.INFO_KEYS == MC.FILL_KEYS and (MF.FILLED, MF.TOO_LARGE, MF.PINCHED, MF.NONFINITE) == (1, 2, 4, 8)


def test_limits_are_refused_on_the_host_side_of_the_abi():
    from bdm_amd import _lib as L
    lib = L.lib()
    wb = lib.bdm_mesh_fill_workspace_bytes
    assert wb(-1, 1, 1) == 0 and wb(65536, 1, 1) == 0 and wb(1, 1, 357913942) == 0 and wb(1, -1, 0) == 0 and wb(1, 2 ** 31 - 2, 1) == 0
    assert wb(3, 10, 4) > 0 and wb(3, 10, 4) % 16 == 0 and wb(0, 0, 0) % 16 == 0
    first = torch.zeros(65537, dtype=torch.int64)
    none = [None] * 6
    assert lib.bdm_mesh_boundary_loops(65536, 32, None, None, first.data_ptr(), first.data_ptr(), *none) == 1 and lib.bdm_last_error()
    assert lib.bdm_mesh_boundary_loops(0, 32, None, None, None, None, *none) == 0
    assert lib.bdm_mesh_boundary_loops(1, 2, None, None, first.data_ptr(), first.data_ptr(), *none) == 1        # max_hole_edges
    assert lib.bdm_mesh_boundary_loops(1, 65536, None, None, first.data_ptr(), first.data_ptr(), *none) == 1
    down = torch.tensor([0, 5, 3])
    assert lib.bdm_mesh_boundary_loops(2, 32, None, None, down.data_ptr(), down.data_ptr(), *none) == 1
    assert lib.bdm_mesh_fill_holes(1, 17, None, None, None, first.data_ptr(), first.data_ptr(), first.data_ptr(), first.data_ptr(), *none[:5]) == 1
    assert lib.bdm_mesh_fill_holes(1, -1, None, None, None, first.data_ptr(), first.data_ptr(), first.data_ptr(), first.data_ptr(), *none[:5]) == 1
    assert lib.bdm_mesh_fill_holes(0, 3, None, None, None, None, None, None, None, *none[:5]) == 0
    ff = torch.tensor([0, 3, 3, 1355])
    assert lib.bdm_mesh_fill_variant(3, ff.data_ptr()) == 256 + 13 and lib.bdm_mesh_fill_variant(2, ff.data_ptr()) == 256 + 5
    assert lib.bdm_mesh_fill_variant(0, ff.data_ptr()) == 0 and lib.bdm_mesh_fill_variant(1, first.data_ptr()) == 0


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
def _ref_fill_holes(meshes, max_hole_edges=32, colors_list=None, return_info=False):
    MF._check_cap(max_hole_edges)
    verts_list, faces_list = mesh_lists(meshes)
    if colors_list is not None:
        MF._check_colors(colors_list, verts_list)
    rows = [R.fill(v, f, max_hole_edges, attrs=None if colors_list is None else colors_list[m]) for m, (v, f) in enumerate(zip(verts_list, faces_list))]
    out = ([r["verts"] for r in rows], [r["faces"] for r in rows])
    return out + (([r["attrs"] for r in rows],) if colors_list is not None else ()) + (([r["info"] for r in rows],) if return_info else ())


@pytest.fixture()
def ref_kernels(monkeypatch):
    """Both modules with their device paths replaced by the restatements."""
    def ref_components(meshes):
        verts_list, faces_list = mesh_lists(meshes)
        return [tuple(CR.components(f, v.shape[0])[k] for k in ("vert_comp", "face_comp", "comp_verts", "comp_faces")) for v, f in zip(verts_list, faces_list)]
    monkeypatch.setattr(MC, "connected_components", ref_components)
    monkeypatch.setattr(MF, "fill_holes", _ref_fill_holes)


def _tree(tmp_path):
    from bdm_amd.io import save_mesh_ply
    tv, tf = R.surface_mesh("torus1500")
    ov, of, _ = R.hand_meshes()["octa_too_large"]
    colours = (torch.arange(tv.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "in" / "b" / "torus.ply", colors=colours.numpy())
    save_mesh_ply(ov.numpy(), of.numpy(), tmp_path / "in" / "a" / "octa.ply")
    return (tv, tf, colours), (ov, of)


def test_mesh_fill_cli_walk_with_the_kernels_replaced_by_the_restatement(ref_kernels, tmp_path):
    from bdm_amd.io import load_mesh_ply
    from bdm_amd.surface import mesh_stats
    (tv, tf, colours), (ov, of) = _tree(tmp_path)
    seen = []

    def spy(verts_list, faces_list, colors_list):
        seen.append([x.shape[0] for x in verts_list])
        return MF.fill_batch(verts_list, faces_list, colors_list, "cpu", 8)
    got = MF.process_tree(tmp_path / "in", tmp_path / "out", spy, batch_size=16)
    assert seen == [[6, tv.shape[0]]]   # sorted paths
    rt, ro = R.fill(tv, tf, 8, attrs=colours), R.fill(ov, of, 8)
    assert rt["info"]["too_large_loops"] == 1 and ro["info"]["filled_loops"] == 1   # the torus's 14 edges exceed 8, the octahedron's 4 do not
    sums = {k: rt["info"][k] + ro["info"][k] for k in R.INFO_KEYS}
    stats = [mesh_stats(*m) for m in ((tv, tf), (ov, of), (rt["verts"], rt["faces"]), (ro["verts"], ro["faces"]))]
    assert got == MF.compose_result(2, sums, stats[0]["edges"] + stats[1]["edges"], 14 + 4, stats[2]["edges"] + stats[3]["edges"], 14)
    assert list(got) == ["files"] + list(R.INFO_KEYS) + ["open_edge_fraction_in", "open_edge_fraction_out"] and json.loads(json.dumps(got)) == got
    v, f, c = load_mesh_ply(tmp_path / "out" / "a" / "octa.ply", with_colors=True)
    assert c is None and np.array_equal(v, ro["verts"].numpy()) and np.array_equal(f, ro["faces"].numpy()) and f.shape[0] == of.shape[0] + 4
    v, f, c = load_mesh_ply(tmp_path / "out" / "b" / "torus.ply", with_colors=True)
    assert np.array_equal(v, tv.numpy()) and np.array_equal(f, tf.numpy()) and np.array_equal(c, colours.numpy())
    with pytest.raises(ValueError):
        MF.process_tree(tmp_path / "in", tmp_path / "out", spy, batch_size=0)


def test_mesh_clean_json_keeps_its_seven_keys_without_fill_holes_and_gains_the_sums_with_it(ref_kernels, tmp_path):
    from bdm_amd.io import load_mesh_ply
    (tv, tf, colours), (ov, of) = _tree(tmp_path)

    def clean_fn(**kw):
        return lambda v, f, c: MC.clean_batch(v, f, c, "cpu", taubin_iters=0, min_fraction=0.0, **kw)
    off = MC.process_tree(tmp_path / "in", tmp_path / "off", clean_fn(), batch_size=16)
    assert off == MC.compose_result(2, 6 + tv.shape[0], 6 + tf.shape[0], 6 + tv.shape[0], 6 + tf.shape[0], 2, 0)
    assert list(off) == ["files", "vertices_in", "faces_in", "vertices_out", "faces_out", "components", "removed_components"]
    zero = MC.process_tree(tmp_path / "in", tmp_path / "zero", clean_fn(fill_holes=0), batch_size=16)
    assert zero == off and list(zero) == list(off)
    for rel in ("a/octa.ply", "b/torus.ply"):
        assert (tmp_path / "off" / rel).read_bytes() == (tmp_path / "zero" / rel).read_bytes() == (tmp_path / "in" / rel).read_bytes()
    on = MC.process_tree(tmp_path / "in", tmp_path / "on", clean_fn(fill_holes=32), batch_size=16)
    rt, ro = R.fill(tv, tf, 32, attrs=colours), R.fill(ov, of, 32)
    assert list(on) == list(off) + list(R.INFO_KEYS) and all(on[k] == rt["info"][k] + ro["info"][k] for k in R.INFO_KEYS)
    assert on["vertices_out"] == off["vertices_out"] + 2 and on["faces_out"] == off["faces_out"] + 14 + 4
    v, f, c = load_mesh_ply(tmp_path / "on" / "b" / "torus.ply", with_colors=True)
    assert np.array_equal(v, rt["verts"].numpy()) and np.array_equal(f, rt["faces"].numpy()) and c.shape == (tv.shape[0] + 1, 3)
    v, f, c = load_mesh_ply(tmp_path / "on" / "a" / "octa.ply", with_colors=True)
    assert c is None and np.array_equal(f, ro["faces"].numpy())


def test_command_line_arguments():
    a = MF.parse_args(["--mesh_dir", "x", "--out_dir", "y"])
    assert (a.mesh_dir, a.out_dir, a.max_hole_edges, a.batch_size) == ("x", "y", 32, 16)
    a = MF.parse_args(["--mesh_dir", "x", "--out_dir", "y", "--max-hole-edges", "64", "--batch-size", "2"])
    assert (a.max_hole_edges, a.batch_size) == (64, 2)
    for bad in (["--batch-size", "0"], ["--max-hole-edges", "2"], ["--max-hole-edges", "65536"], ["--max-hole-edges", "1.5"]):
        with pytest.raises(SystemExit):
            MF.parse_args(["--mesh_dir", "x", "--out_dir", "y"] + bad)
    a = MC.parse_args(["--mesh_dir", "x", "--out_dir", "y"])
    assert a.fill_holes == 0
    assert MC.parse_args(["--mesh_dir", "x", "--out_dir", "y", "--fill-holes", "32"]).fill_holes == 32
    for bad in (["--fill-holes", "2"], ["--fill-holes", "-1"], ["--fill-holes", "65536"], ["--fill-holes", "x"]):
        with pytest.raises(SystemExit):
            MC.parse_args(["--mesh_dir", "x", "--out_dir", "y"] + bad)
