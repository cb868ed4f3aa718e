"""The quadric edge-collapse rule (include/bdm_hip.h section 23) on the CPU, through its restatement tests/mesh_qem_ref.py: what a round
selects, what it leaves alone, the invariants on closed and open meshes, the stopping rule, and that every named mutant of the
restatement is told apart from the rule.  The argument checks of the Python surface run before any launch, so they are tested here too."""
import functools
import math

import pytest
import torch

import mesh_qem_ref as R


@functools.lru_cache(maxsize=None)
def _result(name, target, **kw):
    v, f = _mesh(name)
    return R.decimate(v, f, target, **dict(kw))


def _mesh(name):
    if name.startswith("ico"):
        return R.icosphere(int(name[3:]))
    if name == "torus":
        return R.torus()
    if name == "grid":
        return R.grid(9)
    if name == "tilted":
        return R.tilted(9)
    if name == "bent":
        v, f = R.grid(9)
        return v * torch.tensor([1.0, 1.3, 1.0]) + 0.1 * torch.sin(7.0 * v[:, :1]) * torch.tensor([0.0, 0.0, 1.0]), f
    return R.hand_meshes()[name]


@pytest.mark.parametrize("name", ["ico2", "torus", "grid", "fan40"])
def test_selected_edges_are_pairwise_non_adjacent_and_hold_the_global_minimum(name):
    v, f = _mesh(name)
    s = R.State(v, f, 0)
    for _ in range(4):
        if s.stop:
            break
        faces = [list(x) for x in s.faces]
        s.round()
        keys, chosen, ends = s.last["keys"], s.last["selected"], s.last["ends"]
        valid = [k for k in keys.values() if k != R.INVALID]
        if not valid:
            assert not chosen
            continue
        assert min(valid) in [keys[h] for h in chosen], "the cheapest valid edge was not selected"
        nbr = {}
        for a, b, c in (x for x in faces if x[0] >= 0):
            for p, q in ((a, b), (b, c), (c, a)):
                nbr.setdefault(p, set()).add(q)
                nbr.setdefault(q, set()).add(p)
        touched = [set(ends[h]) for h in chosen]
        for i, x in enumerate(touched):
            for y in touched[i + 1:]:
                assert not x & y, "two selected edges share an endpoint"
                assert not any(nbr[p] & y for p in x), "two selected edges have neighbouring endpoints"


def test_flat_grid_collapses_cost_nothing_stay_on_the_plane_and_keep_the_corners():
    v, f = _mesh("grid")
    r = _result("grid", 12)
    assert r["info"]["max_cost_bits"] == 0, "a collapse on a plane cost something"
    assert bool((r["verts"][:, 2] == 0.25).all())
    corners = [0, 8, 72, 80]
    for c in corners:
        assert bool((r["verts"][r["vert_map"][c]] == v[c]).all()) and R.State(v, f, 0).vlive[c]
    assert sorted(r["vert_map"][corners].tolist()) == sorted(set(r["vert_map"][corners].tolist()))
    lo, hi = r["verts"].min(0).values, r["verts"].max(0).values
    assert lo.tolist() == [0.0, 0.0, 0.25] and hi.tolist() == [1.0, 1.0, 0.25]
    top = R.topology(r["faces"])
    assert top["loops"] == 1 and top["euler"] == 1 and top["inconsistent_edges"] == 0 and top["multi_edges"] == 0
    area = sum(abs(x) for x in [0.5 * R.normal(*[[float(c) for c in r["verts"][i]] for i in face])[2] for face in r["faces"].tolist()])
    assert abs(area - 1.0) < 1e-6


def test_tetrahedra_and_the_fin_stay_untouched_with_the_reason_counted():
    for name, reason, edges in (("tetrahedron", "valence", 6), ("two_tetrahedra", "valence", 12), ("fin", "nonmanifold", 7)):
        v, f = _mesh(name)
        r = R.decimate(v, f, 0)
        assert R.same_floats(r["verts"], v) and torch.equal(r["faces"], f), name
        assert r["info"]["stop"] == 2 and r["info"]["rounds"] == 1 and r["info"]["collapses"] == 0 and r["info"]["candidates"] == edges
        assert r["info"]["rejected_" + reason] == edges, name
        assert torch.equal(r["vert_map"], torch.arange(v.shape[0])) and torch.equal(r["face_map"], torch.arange(f.shape[0]))


def test_the_octahedron_ends_as_a_tetrahedron_and_refuses_the_equator_of_the_bipyramid_by_the_link_condition():
    v, f = _mesh("octahedron")
    s = R.State(v, f, 0)
    s.round()
    assert s.collapses == 1 and s.live_faces == 6   # a triangular bipyramid: its three equator edges have three common neighbours
    s.round()
    assert s.rejected["link"] == 3 and s.collapses == 2 and s.live_faces == 4
    s.round()
    assert s.stop == 2 and s.rejected["valence"] == 6 and s.collapses == 2
    top = R.topology(s.finish()["faces"])
    assert top["euler"] == 2 and top["open_edges"] == 0


@pytest.mark.parametrize("name", ["ico2", "ico3", "torus"])
def test_closed_meshes_stay_closed_manifolds_down_to_a_tenth(name):
    v, f = _mesh(name)
    before = R.topology(f)
    r = _result(name, f.shape[0] // 10)
    after = R.topology(r["faces"])
    assert r["info"]["stop"] == 1 and r["faces"].shape[0] <= f.shape[0] // 10
    assert r["faces"].shape[0] > f.shape[0] // 10 - 2 * r["info"]["selected"], "more than the last round's removals below the target"
    assert after["open_edges"] == 0 and after["inconsistent_edges"] == 0 and after["multi_edges"] == 0 and after["duplicate_faces"] == 0
    assert after["euler"] == before["euler"]
    assert R.signed_volume(r["verts"], r["faces"]) * R.signed_volume(v, f) > 0
    assert r["verts"].shape[0] == r["info"]["vertices_out"] == v.shape[0] - r["info"]["collapses"]
    assert sorted(set(r["faces"].flatten().tolist())) == list(range(r["verts"].shape[0])), "a surviving vertex without a face"
    kept = r["face_map"] >= 0
    assert int(kept.sum()) == r["faces"].shape[0] and bool((r["face_map"][~kept] == R.COLLAPSED).all())
    assert torch.equal(r["face_map"][kept], torch.arange(int(kept.sum())))
    assert torch.equal(r["vert_map"][f[kept]], r["faces"]), "a surviving face is the old one through vert_map, in its winding"


@pytest.mark.parametrize("name", ["grid", "bent", "tilted", "fan40"])
def test_open_sheets_keep_their_boundary_loops(name):
    v, f = _mesh(name)
    r = _result(name, max(f.shape[0] // 8, 4))
    before, after = R.topology(f), R.topology(r["faces"])
    assert after["loops"] == before["loops"] == 1 and after["euler"] == before["euler"]
    assert after["inconsistent_edges"] == 0 and after["multi_edges"] == 0 and after["duplicate_faces"] == 0


def test_stop_reasons_and_the_error_bound():
    v, f = _mesh("torus")
    assert R.decimate(v, f, 256)["info"]["stop"] == 1 and R.decimate(v, f, 256)["info"]["rounds"] == 0   # at the target before a round
    assert R.decimate(v, f, 300)["info"]["rounds"] == 0
    r = R.decimate(v, f, 25, max_rounds=3)
    assert r["info"]["stop"] == 3 and r["info"]["rounds"] == 3 and r["faces"].shape[0] > 25
    r = R.decimate(v, f, 25, maximum_error=1e-3)
    assert r["info"]["stop"] == 2 and r["info"]["rejected_cost"] > 0 and r["faces"].shape[0] > 25
    assert float(torch.tensor(r["info"]["max_cost_bits"], dtype=torch.int32).view(torch.float32)) <= 1e-3
    r = R.decimate(v, f, 25, maximum_error=0.0)
    assert r["info"]["collapses"] == 0 and r["info"]["stop"] == 2 and torch.equal(r["faces"], f)
    assert _result("torus", 25)["info"]["stop"] == 1


def test_rounds_in_chunks_and_interleaved_meshes_change_nothing():
    for name, target in (("torus", 25), ("ico2", 32), ("bent", 16)):
        v, f = _mesh(name)
        whole = _result(name, target)
        for chunk in (1, 3, 8):
            r = R.decimate(v, f, target, chunk=chunk)
            assert R.same_floats(r["verts"], whole["verts"]) and torch.equal(r["faces"], whole["faces"]) and r["info"] == whole["info"]
    a, b = R.State(*_mesh("torus"), 25), R.State(*_mesh("ico2"), 32)
    while a.stop == 0 or b.stop == 0:   # two meshes advanced in turn, as a batch does
        a.run(1)
        b.run(2)
    for s, (name, target) in ((a, ("torus", 25)), (b, ("ico2", 32))):
        r, whole = s.finish(), _result(name, target)
        assert R.same_floats(r["verts"], whole["verts"]) and torch.equal(r["faces"], whole["faces"]) and r["info"] == whole["info"]


def test_locked_vertices_and_bad_faces_stay_in_place():
    v, f = R.icosphere(2)
    v = v.clone()
    v[7, 1] = float("nan")
    f2 = torch.cat([f, torch.tensor([[0, 0, 5], [3, 400, 2], [-1, 2, 3]])])
    r = R.decimate(v, f2, 32, attrs=R.attrs_for(v.shape[0], 1))
    assert r["info"]["locked_vertices"] == 5 and r["info"]["bad_faces"] == 3 and r["face_map"][-3:].tolist() == [R.BAD] * 3
    for i in (0, 2, 3, 5, 7):
        assert R.same_floats(r["verts"][r["vert_map"][i]], v[i]), f"locked vertex {i} moved"
        assert r["members"][int(r["vert_map"][i])] == [i]
    sizes = [len(m) for m in r["members"]]
    assert sum(sizes) == v.shape[0] and max(sizes) > 1
    big = sizes.index(max(sizes))
    assert bool(torch.isfinite(r["attrs"][big]).all())


MUTANT_CASES = {"one_hop": ("ico1", 8), "no_link": ("torus", 12), "no_flip": ("tilted", 16), "quadric_order": ("bent", 16), "b_survives": ("ico2", 32),
                "no_boundary_quadric": ("bent", 16), "cost_before_clamp": ("tilted", 16)}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_told_apart(mutant):
    assert set(MUTANT_CASES) == set(R.MUTANTS)
    name, target = MUTANT_CASES[mutant]
    v, f = _mesh(name)
    # neighbouring collapses do not commute: past its first round the one-hop mutant has no mesh left to speak of
    rule, other = _result(name, target, max_rounds=1 if mutant == "one_hop" else 256), R.decimate(v, f, target, mutant=mutant,
                                                                                                   max_rounds=1 if mutant == "one_hop" else 256)
    same = rule["verts"].shape == other["verts"].shape and R.same_floats(rule["verts"], other["verts"]) and torch.equal(rule["faces"], other["faces"])
    assert not same, f"{mutant} gives the rule's result on {name}"
    if mutant == "quadric_order":
        a, b = R.State(v, f, target).quadrics(), R.State(v, f, target, mutant=mutant).quadrics()
        assert not torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.allclose(a, b, rtol=1e-12, atol=1e-15)
    if mutant == "one_hop":
        s = R.State(v, f, target, mutant=mutant)
        s.round()
        ends = [set(s.last["ends"][h]) for h in s.last["selected"]]
        nbr = {}
        for x in f.tolist():
            for p in x:
                nbr.setdefault(p, set()).update(x)
        assert any(any(nbr[p] & y for p in x) for i, x in enumerate(ends) for y in ends[i + 1:]), "one-hop selection chose no neighbouring pair"
    if mutant == "no_link":
        top = R.topology(other["faces"])
        assert top["multi_edges"] + top["duplicate_faces"] + top["open_edges"] > 0 or top["euler"] != 0


def test_target_and_cost_on_a_corner_and_on_a_plane():
    """Three orthogonal planes through (1, 2, 3): the optimum is that point at cost 0; one plane alone is singular and falls back to the
    cheapest of the ends and the midpoint, the first of equals."""
    q = [0.0] * 10
    for n, d in (((1.0, 0.0, 0.0), -1.0), ((0.0, 1.0, 0.0), -2.0), ((0.0, 0.0, 1.0), -3.0)):
        q = [x + y for x, y in zip(q, R.plane_quadric(n, d, 1.0))]
    t, c = R.target_and_cost(q, (0.5, 2.0, 3.0), (1.5, 2.0, 3.0))
    assert t == (1.0, 2.0, 3.0) and c == 0.0
    t, c = R.target_and_cost(q, (10.5, 2.0, 3.0), (11.5, 2.0, 3.0))   # the optimum lies further than |b - a| from the midpoint
    assert t == (10.5, 2.0, 3.0) and c == 9.5 ** 2
    plane = R.plane_quadric((0.0, 0.0, 1.0), -3.0, 1.0)
    t, c = R.target_and_cost(plane, (0.0, 0.0, 3.0), (1.0, 0.0, 3.0))
    assert t == (0.0, 0.0, 3.0) and c == 0.0
    t, c = R.target_and_cost(plane, (0.0, 0.0, 4.0), (1.0, 0.0, 3.0))
    assert t == (1.0, 0.0, 3.0) and c == 0.0
    assert math.isnan(R.clamp(float("nan"))) and R.clamp(-1.0) == 0.0 and math.copysign(1.0, R.clamp(-0.0)) == 1.0


def test_argument_errors_come_before_any_launch():
    from bdm_amd import mesh_decimate as MD
    v, f = R.icosphere(1)
    for kw in (dict(), dict(target_fraction=0.5, target_number_of_triangles=5), dict(target_fraction=0.0), dict(target_fraction=1.5),
               dict(target_fraction=float("nan")), dict(target_fraction="half"), dict(target_number_of_triangles=-1), dict(target_number_of_triangles=2.5),
               dict(target_number_of_triangles=True), dict(target_number_of_triangles=[1, 2]), dict(target_fraction=[0.5, 0.5]),
               dict(target_fraction=0.5, maximum_error=-1.0), dict(target_fraction=0.5, maximum_error=float("nan")),
               dict(target_fraction=0.5, boundary_weight=-1.0), dict(target_fraction=0.5, boundary_weight=float("inf")),
               dict(target_fraction=0.5, max_rounds=0), dict(target_fraction=0.5, max_rounds=2 ** 20 + 1), dict(target_fraction=0.5, max_rounds=1.5)):
        with pytest.raises(ValueError):
            MD.simplify_quadric_decimation(([v], [f]), **kw)
    with pytest.raises(Exception, match="CPU tensor"):
        MD.simplify_quadric_decimation(([v], [f]), target_fraction=0.5)
    assert MD.simplify_quadric_decimation(([], []), target_number_of_triangles=5) == ([], [])
    assert MD.QEM_INFO_KEYS == R.INFO_KEYS and MD.QEM_STOPS == R.STOPS
    for bad in (["--method", "quadric"], ["--method", "quadric", "--resolution", "8"], ["--target-fraction", "0.5"],
                ["--method", "quadric", "--target-fraction", "2"], ["--method", "quadric", "--target-faces", "5", "--max-error", "-1"]):
        with pytest.raises(SystemExit):
            MD.parse_args(["--mesh_dir", "a", "--out_dir", "b"] + bad)
    assert MD.parse_args(["--mesh_dir", "a", "--out_dir", "b", "--method", "quadric", "--target-faces", "5"]).target_faces == 5
    from bdm_amd import mesh_clean as MC
    with pytest.raises(SystemExit):
        MC.parse_args(["--mesh_dir", "a", "--out_dir", "b", "--decimate-fraction", "0.5", "--decimate-resolution", "8"])
    assert MC.parse_args(["--mesh_dir", "a", "--out_dir", "b", "--decimate-fraction", "0.5"]).decimate_fraction == 0.5
