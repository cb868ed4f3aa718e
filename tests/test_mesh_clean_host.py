"""The restatement tests/mesh_clean_ref.py of bdm_hip.h section 16 against plain Python, its mutants, the island and smoothing claims
of DESIGN.md section 20, and the Python surface of bdm_amd.mesh_clean with the kernels replaced by the restatement.  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

import mesh_clean_ref as R
from bdm_amd import mesh_clean as MC
from bdm_amd.ragged import mesh_lists


def _case(name):
    return next((v, f) for n, v, f in R.batch() if n == name)


def _python_truth(faces, V):
    """Neighbour sets and union-find labels of one mesh in plain Python."""
    nbrs = [set() for _ in range(V)]
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    connected = []
    for a, b, c in faces.tolist():
        ok = all(0 <= i < V for i in (a, b, c)) and len({a, b, c}) == 3
        connected.append(ok)
        if ok:
            for x, y in ((a, b), (b, c), (c, a)):
                nbrs[x].add(y), nbrs[y].add(x)
                rx, ry = find(x), find(y)
                parent[max(rx, ry)] = min(rx, ry)   # the root of a set is its smallest member
    return nbrs, [find(i) for i in range(V)], connected


@pytest.mark.parametrize("name", [n for n, _, _ in R.batch()])
def test_restatement_equals_union_find_and_a_set_of_pairs(name):
    v, f = _case(name)
    V = v.shape[0]
    nbrs, roots, connected = _python_truth(f, V)
    c = R.components(f, V)
    first, nbr = c["first"].tolist(), c["nbr"].tolist()
    assert first[0] == 0 and len(first) == V + 1
    assert [nbr[first[i]:first[i + 1]] for i in range(V)] == [sorted(s) for s in nbrs]
    rank = {r: k for k, r in enumerate(sorted(set(roots)))}
    assert c["vert_comp"].tolist() == [rank[r] for r in roots]
    assert c["face_comp"].tolist() == [rank[roots[a]] if ok else -1 for (a, _, _), ok in zip(f.tolist(), connected)]
    assert c["comp_verts"].tolist() == [roots.count(r) for r in sorted(set(roots))] and int(c["comp_verts"].sum()) == V
    assert int(c["comp_faces"].sum()) == sum(connected)
    assert torch.equal(R.labels(c["first"], c["nbr"])[0], torch.tensor(roots, dtype=torch.int64))


MUTANT_CASE = {"no_dedup": "two_triangles_consistent", "descending": "one_triangle", "accept_repeated": "bad_faces", "wrap_index": "bad_faces",
               "rank_by_size": "bad_faces", "face_comp_zero": "bad_faces"}


@pytest.mark.parametrize("mutant", R.ADJ_MUTANTS)
def test_every_adjacency_mutant_changes_an_output_of_the_gpu_inputs(mutant):
    v, f = _case(MUTANT_CASE[mutant])
    good, bad = R.adjacency(f, v.shape[0]), R.adjacency(f, v.shape[0], mutant)
    assert not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1]))


@pytest.mark.parametrize("mutant", R.COMP_MUTANTS)
def test_every_component_mutant_changes_an_output_of_the_gpu_inputs(mutant):
    v, f = _case(MUTANT_CASE[mutant])
    good, bad = R.components(f, v.shape[0]), R.components(f, v.shape[0], mutant)
    assert any(not torch.equal(good[k], bad[k]) for k in ("vert_comp", "face_comp", "comp_verts", "comp_faces"))


def _smooth_inputs(mutant):
    """(verts, faces, num_iter): the GPU test's input on which the mutant is told apart."""
    if mutant == "no_eps":
        return (*R.coincident_mesh(), 1)
    if mutant == "isolated_moved":
        return (*_case("triangles_200_unused_10"), 1)
    if mutant == "one_minus_f64":
        return (*R.island_mesh(), 1)
    return (*_case("two_triangles_consistent"), 1)


@pytest.mark.parametrize("mutant", R.SMOOTH_MUTANTS)
def test_every_smoothing_mutant_changes_an_output_of_the_gpu_inputs(mutant):
    v, f, it = _smooth_inputs(mutant)
    first, nbr = R.adjacency(f, v.shape[0])
    good, bad = R.taubin(v, first, nbr, num_iter=it), R.taubin(v, first, nbr, num_iter=it, mutant=mutant)
    assert not R.same_floats(good, bad)
    assert bool(torch.isfinite(good).all())   # the coincident pair included: w = 1 / 1e-12f is finite


def test_smoothing_edge_cases_of_the_restatement():
    v, f = _case("triangles_200_unused_10")
    first, nbr = R.adjacency(f, v.shape[0])
    out = R.taubin(v, first, nbr)
    alone = (first[1:] == first[:-1])
    assert int(alone.sum()) == 10 and torch.equal(R.bits(out[alone]), R.bits(v[alone]))     # an isolated vertex keeps its bits
    assert torch.equal(R.bits(R.taubin(v, first, nbr, num_iter=0)), R.bits(v))              # num_iter == 0 copies
    v, f = R.nan_mesh()
    first, nbr = R.adjacency(f, v.shape[0])
    bad = torch.isnan(R.taubin(v, first, nbr, num_iter=1)).any(1)
    # one half-step reaches the neighbours (hub, rim 4 and 6), the second their neighbours: the hub's are the whole rim
    assert bool(bad.all())
    half = torch.isnan(R.half_step(v, first, nbr, torch.tensor(0.53), 0)).any(1)
    assert sorted(half.nonzero().flatten().tolist()) == [0, 4, 5, 6]
    # float64 gives the same formulas: close to float32, not equal to it
    v, f = R.island_mesh()
    first, nbr = R.adjacency(f, v.shape[0])
    a, b = R.taubin(v, first, nbr), R.taubin(v, first, nbr, dtype=torch.float64)
    assert b.dtype == torch.float64 and float((a.double() - b).abs().max()) < 1e-5


# ---- the island claim -----------------------------------------------------------------------------------------------------------------
def _ref_connected_components(meshes):
    verts_list, faces_list = mesh_lists(meshes)
    out = []
    for v, f in zip(verts_list, faces_list):
        c = R.components(f, v.shape[0])
        out.append((c["vert_comp"], c["face_comp"], c["comp_verts"], c["comp_faces"]))
    return out


@pytest.fixture()
def ref_kernels(monkeypatch):
    """bdm_amd.mesh_clean with its two device paths replaced by the restatement."""
    from bdm_amd.cameras import Meshes

    def ref_taubin(meshes, lambd=0.53, mu=-0.34, num_iter=10, *, weights="inverse_length"):
        MC._check_taubin(lambd, mu, num_iter, weights)
        verts_list, faces_list = mesh_lists(meshes)
        out = []
        for v, f in zip(verts_list, faces_list):
            first, nbr = R.adjacency(f, v.shape[0])
            out.append(R.taubin(v, first, nbr, lambd, mu, num_iter, MC.WEIGHTS[weights]))
        return Meshes(out, list(faces_list))
    monkeypatch.setattr(MC, "connected_components", _ref_connected_components)
    monkeypatch.setattr(MC, "taubin_smoothing", ref_taubin)


def test_the_island_is_a_second_component_and_the_default_removes_it(ref_kernels):
    from bdm_amd.surface import mesh_stats
    v, f = R.island_mesh()
    assert (v.shape[0], f.shape[0]) == (1210, 2412)
    c = R.components(f, v.shape[0])
    assert c["comp_verts"].tolist() == [1134, 76] and c["comp_faces"].tolist() == [2264, 148]
    verts, faces, info = MC.remove_small_components(([v], [f]), return_info=True)
    assert (verts[0].shape[0], faces[0].shape[0]) == (1134, 2264)
    assert info == [{"components": 2, "removed_components": 1, "removed_vertices": 76, "removed_faces": 148}]
    rv, rf = R.remove_small(v, f)
    assert torch.equal(verts[0], rv) and torch.equal(faces[0], rf)
    stats = mesh_stats(verts[0], faces[0])
    assert stats["euler_characteristic"] == 2 and stats["open_edges"] == 0 and mesh_stats(v, f)["euler_characteristic"] == 4
    verts, faces = MC.remove_small_components(([v], [f]), min_fraction=0.05)     # ceil(0.05 * 2264) = 114 <= 148
    assert torch.equal(verts[0], v) and torch.equal(faces[0], f)
    verts, faces = MC.remove_small_components(([v], [f]), min_fraction=0.0, keep_largest=True)
    assert (verts[0].shape[0], faces[0].shape[0]) == (1134, 2264)


def test_selection_rule_ties_and_keep_largest():
    sel = MC.select_components
    assert sel(torch.tensor([100, 10, 9, 0])).tolist() == [True, True, False, False]          # ceil(0.1 * 100) = 10; min_faces = 1
    assert sel(torch.tensor([100, 10, 9, 0]), min_fraction=0.0, min_faces=0).tolist() == [True] * 4
    assert sel(torch.tensor([100, 10, 9, 0]), min_fraction=0.0).tolist() == [True, True, True, False]
    assert sel(torch.tensor([101, 11, 10])).tolist() == [True, True, False]                   # ceil(10.1) = 11
    assert sel(torch.tensor([5, 7, 7, 2]), keep_largest=True).tolist() == [False, True, False, False]   # the lower rank on a tie
    assert sel(torch.tensor([5, 5]), min_fraction=1.0).tolist() == [True, True]
    assert sel(torch.tensor([3, 50]), min_faces=4, min_fraction=0.0).tolist() == [False, True]
    assert sel(torch.tensor([0, 0]), min_faces=1).tolist() == [False, False]                  # vertices no face uses
    assert sel(torch.zeros(0, dtype=torch.int64)).tolist() == []


def test_compaction_keeps_order_carries_colours_and_may_empty_a_mesh(ref_kernels):
    v, f = _case("bad_faces")
    colours = torch.arange(12.0)[:, None].expand(12, 3).contiguous()
    verts, faces, cols, info = MC.remove_small_components(([v], [f]), min_fraction=1.0, colors_list=[colours], return_info=True)
    # components {0,1,2} (1 face), {3,4,5} (2), {6}, {7}, {8,9,10} (2), {11}: the largest has 2 faces
    assert torch.equal(verts[0], v[[3, 4, 5, 8, 9, 10]]) and torch.equal(cols[0], colours[[3, 4, 5, 8, 9, 10]])
    assert faces[0].tolist() == [[0, 1, 2], [3, 4, 5], [4, 5, 3], [2, 0, 1]] and faces[0].dtype == f.dtype
    assert info == [{"components": 6, "removed_components": 4, "removed_vertices": 6, "removed_faces": 8}]
    verts, faces = MC.remove_small_components(([v], [f]), min_fraction=0.0, min_faces=0)      # only the faces that take no part go
    assert torch.equal(verts[0], v) and faces[0].shape[0] == 5
    verts, faces, info = MC.remove_small_components(([v, v[:0]], [f, f[:0]]), min_faces=3, return_info=True)
    assert all(x.shape == (0, 3) for x in verts + faces) and info[0]["removed_components"] == 6 and info[1]["components"] == 0
    from bdm_amd.cameras import Meshes
    assert len(Meshes(verts, faces)) == 2                                                      # a legal empty mesh
    assert MC.remove_small_components(([], [])) == ([], [])


def test_bad_arguments_raise_before_any_launch():
    from bdm_amd import _lib as L
    v, f = _case("one_triangle")
    for kw in (dict(min_fraction=-0.1), dict(min_fraction=1.5), dict(min_fraction="a"), dict(min_faces=-1), dict(min_faces=1.5),
               dict(colors_list=[]), dict(colors_list=[torch.zeros(2, 3)])):
        with pytest.raises(ValueError):
            MC.remove_small_components(([v], [f]), **kw)
    for kw in (dict(weights="cotangent"), dict(num_iter=-1), dict(num_iter=1.5), dict(num_iter=MC.MAX_ITER + 1), dict(lambd=float("nan")),
               dict(mu=float("inf"))):
        with pytest.raises(ValueError):
            MC.taubin_smoothing(([v], [f]), **kw)
    for fn in (MC.vertex_adjacency, MC.connected_components, MC.remove_small_components, MC.taubin_smoothing):
        with pytest.raises(ValueError):
            fn(v)                                                # neither a Meshes nor a pair of lists
        with pytest.raises(ValueError):
            fn(([v], [f.float()]))                               # float faces
        with pytest.raises(L.BdmHipError):
            fn(([v], [f]))                                       # host tensors: no CPU path


def test_limits_are_refused_on_the_host_side_of_the_abi():
    """The size checks run before anything touches a device: they hold on a box without one."""
    from bdm_amd import _lib as L
    lib = L.lib()
    adj, comp, tau = lib.bdm_mesh_adjacency_workspace_bytes, lib.bdm_mesh_components_workspace_bytes, lib.bdm_mesh_taubin_workspace_bytes
    assert adj(-1, 1, 1) == 0 and adj(65536, 1, 1) == 0 and adj(1, 2 ** 31 - 1, 1) == 0 and adj(1, 1, 357913942) == 0 and adj(1, -1, 0) == 0
    assert comp(65536, 1) == 0 and comp(1, 2 ** 31) == 0 and tau(-1, 1) == 0 and tau(1, 2 ** 31) == 0
    assert adj(1, 1, 357913941) > 0 and adj(3, 10, 4) % 16 == 0 and tau(3, 10) == 64 + 320 and comp(0, 0) % 16 == 0
    first = torch.zeros(65537, dtype=torch.int64)
    assert lib.bdm_mesh_adjacency(65536, None, first.data_ptr(), first.data_ptr(), None, None, None, None) == 1 and lib.bdm_last_error()
    assert lib.bdm_mesh_adjacency(0, None, None, None, None, None, None, None) == 0
    assert lib.bdm_mesh_adjacency(2, None, first.data_ptr(), first.data_ptr(), None, None, None, None) == 0      # sum V == 0
    down = torch.tensor([0, 5, 3])
    assert lib.bdm_mesh_taubin(2, 1, 0, 0.5, -0.3, None, down.data_ptr(), None, None, None, None, None) == 1
    assert lib.bdm_mesh_taubin(1, 1, 2, 0.5, -0.3, None, down.data_ptr(), None, None, None, None, None) == 1     # mode
    assert lib.bdm_mesh_components_rounds(1, 0, down.data_ptr(), down.data_ptr(), None, None, None, None, None) == 1


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def _ref_clean_fn(**kw):
    def clean_fn(verts_list, faces_list, colors_list):
        return MC.clean_batch(verts_list, faces_list, colors_list, "cpu", **kw)
    return clean_fn


def test_cli_walk_with_the_kernels_replaced_by_the_restatement(ref_kernels, tmp_path):
    from bdm_amd.io import load_mesh_ply, save_mesh_ply
    v, f = R.island_mesh()
    bv, bf = _case("fan_70")
    colours = (torch.arange(v.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(v.numpy(), f.numpy(), tmp_path / "in" / "b" / "island.ply", colors=colours.numpy())
    save_mesh_ply(bv.numpy(), bf.numpy(), tmp_path / "in" / "a" / "fan.ply")
    save_mesh_ply(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), tmp_path / "in" / "c.ply")
    seen = []

    def spy(verts_list, faces_list, colors_list):
        seen.append([x.shape[0] for x in verts_list])
        return _ref_clean_fn(taubin_iters=2)(verts_list, faces_list, colors_list)
    got = MC.process_tree(tmp_path / "in", tmp_path / "out", spy, batch_size=2)
    assert seen == [[71, 1210], [0]]                                        # sorted paths, batch_size files per call
    assert got == MC.compose_result(3, 1281, 2482, 1205, 2334, 3, 1) and json.loads(json.dumps(got)) == got
    rv, rf = R.remove_small(v, f)
    first, nbr = R.adjacency(rf, rv.shape[0])
    want = R.taubin(rv, first, nbr, num_iter=2)
    ov, of, oc = load_mesh_ply(tmp_path / "out" / "b" / "island.ply", with_colors=True)
    assert np.array_equal(ov, want.numpy()) and np.array_equal(of, rf.numpy())
    assert np.array_equal(oc, colours[R.components(f, 1210)["vert_comp"] == 0].numpy())
    fv, ff, fc = load_mesh_ply(tmp_path / "out" / "a" / "fan.ply", with_colors=True)
    assert fc is None and np.array_equal(ff, bf.numpy()) and not np.array_equal(fv, bv.numpy())
    ev, ef = load_mesh_ply(tmp_path / "out" / "c.ply")
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    # --taubin-iters 0 skips the smoothing: the vertices are the input's, bit for bit
    MC.process_tree(tmp_path / "in", tmp_path / "out0", _ref_clean_fn(taubin_iters=0, min_fraction=0.0), batch_size=16)
    ov, of, oc = load_mesh_ply(tmp_path / "out0" / "b" / "island.ply", with_colors=True)
    assert np.array_equal(ov, v.numpy()) and np.array_equal(of, f.numpy()) and np.array_equal(oc, colours.numpy())
    with pytest.raises(ValueError):
        MC.process_tree(tmp_path / "in", tmp_path / "out", spy, batch_size=0)


def test_command_line_arguments():
    a = MC.parse_args(["--mesh_dir", "x", "--out_dir", "y"])
    assert (a.min_fraction, a.min_faces, a.keep_largest, a.taubin_iters, a.lambd, a.mu, a.weights, a.batch_size) == \
        (0.1, 1, False, 10, 0.53, -0.34, "inverse_length", 16)
    a = MC.parse_args(["--mesh_dir", "x", "--out_dir", "y", "--keep-largest", "--taubin-iters", "0", "--weights", "uniform", "--min-fraction", "0.5"])
    assert a.keep_largest and a.taubin_iters == 0 and a.weights == "uniform" and a.min_fraction == 0.5
    for bad in (["--batch-size", "0"], ["--min-fraction", "2"], ["--taubin-iters", "-1"], ["--weights", "cotangent"], ["--min-faces", "-2"]):
        with pytest.raises(SystemExit):
            MC.parse_args(["--mesh_dir", "x", "--out_dir", "y"] + bad)


# ---- the smoothing claim --------------------------------------------------------------------------------------------------------------
def test_ten_iterations_halve_the_radial_spread_and_keep_the_volume():
    """The noise-free 1024-point sphere mesh (R = 32, s = 3) with N(0, 0.004^2) added to every coordinate: measured on the restatement,
    the relative spread of the vertex radii goes from 1.03e-2 to 3.3e-3 (inverse length) and 3.2e-3 (uniform), the signed volume from
    0.2717 to 0.2669 and 0.2666 (-1.8 %, -1.9 %).  Asserted: a spread ratio of at most 0.5 and a volume change of at most 3 %."""
    v, f = R.clean_sphere_mesh()
    assert (v.shape[0], f.shape[0]) == (2574, 5144)
    noisy = v + 0.004 * torch.randn(v.shape, generator=torch.Generator().manual_seed(3213))
    first, nbr = R.adjacency(f, v.shape[0])
    s0, v0 = R.radial_spread(noisy), R.signed_volume(noisy, f)
    for mode in (0, 1):
        out = R.taubin(noisy, first, nbr, mode=mode)
        s1, v1 = R.radial_spread(out), R.signed_volume(out, f)
        print(f"mode {mode}: spread {s0:.3e} -> {s1:.3e} (ratio {s1 / s0:.3f}), volume {v0:.5f} -> {v1:.5f} ({(v1 - v0) / v0:+.2%})")
        assert bool(torch.isfinite(out).all()) and s1 / s0 <= 0.5 and abs(v1 - v0) / v0 <= 0.03
    assert math.isclose(s0, 1.03e-2, rel_tol=0.05)
