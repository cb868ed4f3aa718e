"""The restatement tests/face_point_ref.py of bdm_hip.h section 17 against a plain Python double loop and against the existing
point-to-face half, its mutants on the GPU test's own inputs, the sign claim the split form's keys rest on, analytic values, what the
two-sided scores say about a mesh with a floating island, the chooser, the argument errors and the directory walk with the kernels
replaced by the restatement.  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

import face_point_ref as R
import mesh_metrics_ref as M
from bdm_amd import mesh_metrics as MM

f32 = np.float32


# ---- the restatement against a plain double loop ---------------------------------------------------------------------------------------
def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _sub(a, b):
    return [f32(a[i] - b[i]) for i in range(3)]


def _cross(a, b):
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def _pair(x, v):
    """Section 14's d of a point and a face's three vertices in numpy float32 scalars, or None for an invalid face."""
    if not all(np.isfinite(c) for vi in v for c in vi):
        return None
    e = [_sub(v[(i + 1) % 3], v[i]) for i in range(3)]
    n = _cross(e[0], _sub(v[2], v[0]))
    nn = _dot(n, n)
    if not (nn > 0 and nn < math.inf):
        return None
    d_e, inside = None, True
    for i in range(3):
        r = _sub(x, v[i])
        l2 = _dot(e[i], e[i])
        t = f32(0) if l2 == 0 else f32(_dot(e[i], r) / l2)
        t = t if t > 0 else f32(0)
        t = t if t < 1 else f32(1)
        w = _sub(x, [f32(v[i][k] + f32(t * e[i][k])) for k in range(3)])
        d = _dot(w, w)
        d_e = d if d_e is None or d < d_e else d_e
        inside = inside and bool(_dot(n, _cross(e[i], r)) >= 0)
    if inside:
        k = _dot(n, _sub(x, v[0]))
        d_p = f32(f32(k * k) / nn)
        if d_p < d_e:
            return d_p
    return d_e


def _double_loop(verts, faces, points):
    V = verts.shape[0]
    vs, out = verts.numpy().astype(f32), []
    with np.errstate(all="ignore"):
        for face in faces.tolist():
            best, idx = f32(math.inf), -1
            if all(0 <= i < V for i in face):
                for j, x in enumerate(points.numpy().astype(f32)):
                    d = _pair(list(x), [list(vs[i]) for i in face])
                    if d is not None and d < best:
                        best, idx = d, j
            out.append((best, idx))
    return torch.tensor([float(o[0]) for o in out], dtype=torch.float32), torch.tensor([o[1] for o in out], dtype=torch.int32)


@pytest.mark.parametrize("name", ["degenerate", "ties", "no_valid_face"])
def test_restatement_equals_a_plain_double_loop(name):
    c = R.case(name)
    pts = c["clouds"][0][:40] if name == "degenerate" else c["clouds"][0]   # 40 points hold the NaN and the infinite ones (5, 17)
    sq, idx = R.face_point_mesh(c["verts"][0], c["faces"][0], pts)
    want_sq, want_idx = _double_loop(c["verts"][0], c["faces"][0], pts)
    assert torch.equal(R.bits(sq), R.bits(want_sq)) and torch.equal(idx, want_idx)


# ---- one matrix, two minima --------------------------------------------------------------------------------------------------------------
def _matrices():
    for name in R.CASES:
        c = R.case(name)
        for v, f, pts in zip(c["verts"], c["faces"], c["clouds"]):
            if f.shape[0] and pts.shape[0]:
                yield name, v, f, pts, M.pair_sqdist(M.face_quantities(v, f), pts)


def test_both_halves_are_minima_of_the_same_matrix_and_no_pair_has_its_sign_bit_set():
    pairs = 0
    for name, v, f, pts, d in _matrices():
        assert bool((d.view(torch.int32) >= 0).all()), f"{name}: a d with its sign bit set"   # so the keys order like (d, index)
        pairs += d.numel()
        rows, cols = d.min(dim=1).values, d.min(dim=0).values
        assert torch.equal(R.bits(M.distance_mesh(v, f, pts)[0]), R.bits(rows)), name
        sq, idx = R.face_point_mesh(v, f, pts)
        assert torch.equal(R.bits(sq), R.bits(cols)), name
        hit = idx >= 0
        assert bool((cols[~hit] == math.inf).all()) and torch.equal(d[idx[hit].long(), torch.nonzero(hit)[:, 0]], cols[hit]), name
        # a pair that is NaN or +inf is never chosen: no chosen point has a non-finite coordinate
        assert bool(torch.isfinite(pts[idx[hit].long()]).all()) and bool(torch.isfinite(sq[hit]).all()), name
    print(f"{pairs} pairs")
    assert pairs > 5_000_000


def test_nonfinite_points_are_never_chosen_and_their_pairs_are_not_finite():
    c = R.case("degenerate")
    pts = c["clouds"][0]
    bad = ~torch.isfinite(pts).all(dim=1)
    assert int(bad.sum()) == 4
    d = M.pair_sqdist(M.face_quantities(c["verts"][0], c["faces"][0]), pts)
    assert bool((d[bad] == math.inf).all())
    assert not bool(torch.isin(R.ref("degenerate")["point_idx"].long(), torch.nonzero(bad)[:, 0]).any())


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
SMALL = ["ragged", "degenerate", "ties", "no_valid_face"]


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_changes_an_output_of_a_gpu_case(mutant):
    told = [name for name in SMALL if not R.same(R.ref(name), R.ref(name, mutant))]
    print(mutant, told)
    assert told, f"no case tells '{R.MUTANTS[mutant]}' from the rule"
    expect = {"highest_on_ties": "ties", "nonfinite_eligible": "degenerate", "invalid_scored": "degenerate", "packed_index": "ragged",
              "neighbour_cloud": "ragged"}
    assert expect[mutant] in told


def test_the_signed_key_mutant_is_equivalent_because_no_sign_bit_is_set():
    """The split form in integers: the minimum of the keys equals the restatement at every chunk count, and it is the same minimum
    when the keys are compared as signed -- bit 63 of every key is the sign bit of a d, which is clear.  With one key whose bit 63
    is set the two orders do differ, so the equivalence is a property of the rule, not of the arithmetic used here."""
    assert set(R.EQUIVALENT_MUTANTS) == {"signed_key"}
    for name in [f"soup_f{R.THREADS + 1}_p{2 * R.TILE + 1}"] + SMALL:
        c = R.case(name)
        cuts = np.cumsum([0] + [f.shape[0] for f in c["faces"]])
        for chunks in sorted({1, 5} | set(R.chunk_counts(name))):
            for signed in (False, True):
                for m, (v, f, pts) in enumerate(zip(c["verts"], c["faces"], c["clouds"])):
                    sq, idx = R.split_by_keys(v, f, pts, chunks, signed)
                    want = {k: t[cuts[m]:cuts[m + 1]] for k, t in R.ref(name).items()}
                    assert R.same({"sqdist": sq, "point_idx": idx}, want), (name, chunks, signed, m)
    minus_zero = np.array([(0x80000000 << 32) | 3, (0x3F800000 << 32) | 1], dtype=np.uint64)
    assert int(np.argmin(minus_zero)) == 1 and int(np.argmin(minus_zero.view(np.int64))) == 0
    assert R.KEY_NONE < 2 ** 63


# ---- analytic values -------------------------------------------------------------------------------------------------------------------
def test_unit_cube_against_its_corners_and_its_centre():
    v, f = M.box_mesh()
    sq, idx = R.face_point_mesh(v, f, v.clone())
    assert torch.equal(sq, torch.zeros(12)) and bool((idx >= 0).all())
    assert all(int(idx[k]) in f[k].tolist() or bool((v[int(idx[k])] == v[f[k]]).all(dim=1).any()) for k in range(12))
    sq, idx = R.face_point_mesh(v, f, torch.zeros(1, 3))
    assert torch.equal(sq, torch.full((12,), 0.25)) and torch.equal(idx, torch.zeros(12, dtype=torch.int32))
    sq64, _ = R.face_point_mesh(v, f, torch.zeros(1, 3), dtype=torch.float64)
    assert sq64.dtype == torch.float64 and torch.equal(sq64, torch.full((12,), 0.25, dtype=torch.float64))


def _row(verts, faces, gt):
    """A two-sided row of compose_scores from the restatement (the sampled entries are not under test: 0)."""
    face_sq, face_pt = R.face_point_mesh(verts, faces, gt)
    gt_sq, _ = M.distance_mesh(verts, faces, gt)
    return (0.0, 0.0, gt_sq.double().numpy(), face_sq.double().numpy(), MM.face_areas(verts.numpy(), faces.numpy(), (face_pt >= 0).numpy()))


def test_a_detached_blob_shows_in_the_two_sided_scores_and_nowhere_else():
    """A box and the same box with a small box floating 2 away, against ground truth sampled on the box alone.  The one-sided score
    cannot see the blob (the nearest face of every ground-truth point stays on the box); surface_to_gt grows, and
    surface_within_0.01 is exactly the box's share of the area."""
    box_v, box_f = M.box_mesh()
    blob_v, blob_f = M.box_mesh(0.125, 0.125, 0.125, (2.5, 0.0, 0.0))   # exact in float32
    both_v, both_f = torch.cat([box_v, blob_v]), torch.cat([box_f, blob_f + 8])
    gt = M.sample_mesh(box_v, box_f, 6000, M.sample_keys(1, 3)[0])[0]
    alone, both = MM.compose_scores([_row(box_v, box_f, gt)]), MM.compose_scores([_row(both_v, both_f, gt)])
    print(json.dumps(alone), json.dumps(both))
    assert both["gt_to_surface_x1000"] == alone["gt_to_surface_x1000"] and both["gt_within_0.01"] == alone["gt_within_0.01"] == 1.0
    assert alone["surface_within_0.01"] == 1.0 and alone["surface_to_gt_x1000"] < 1.0
    assert both["surface_to_gt_x1000"] > alone["surface_to_gt_x1000"] + 1000 * 0.015 * 3.75   # the blob: 1.5 % of the area, 1.9375^2 away or more
    assert both["surface_within_0.01"] == pytest.approx(6.0 / 6.09375, rel=1e-15)
    assert both["face_distance_x1000"] > alone["face_distance_x1000"] + 1000.0


def test_compose_scores_returns_the_old_dictionary_for_3_tuples():
    rows = [(1.0, 0.5, np.array([0.0, 0.02])), None, (3.0, 1.0, np.array([0.004]))]
    old = {"num": 3, "cd_x1000": 2.0, "f1_at_0.01": 0.75, "gt_to_surface_x1000": 7.0, "gt_within_0.01": 0.75, "empty": 1}
    assert MM.compose_scores(rows) == old and list(MM.compose_scores(rows)) == list(old)
    area, sq = np.array([1.0, 3.0, 0.0]), np.array([0.02, 0.004, math.inf])
    long = MM.compose_scores([rows[0] + (sq, area), None])
    assert list(long)[:6] == list(old) and list(long)[6:] == ["surface_to_gt_x1000", "surface_within_0.01", "face_distance_x1000"]
    assert long["surface_to_gt_x1000"] == (0.02 + 3 * 0.004) / 4 * 1000 and long["surface_within_0.01"] == 0.75
    assert long["face_distance_x1000"] == math.inf   # every face takes part in the symmetric value: the invalid one with +inf
    empty = MM.compose_scores([None], two_sided=True)
    assert all(math.isnan(empty[k]) for k in ("surface_to_gt_x1000", "surface_within_0.01", "face_distance_x1000"))
    assert "surface_to_gt_x1000" not in MM.compose_scores([None])


# ---- the chooser -----------------------------------------------------------------------------------------------------------------------
CHOOSER_ROWS = [  # b, sum_f, sum_p, max_p, workgroups
    (16, 297480, 65536, 4096, 1170), (16, 753538, 131072, 8192, 2951), (16, 1379036, 262144, 16384, 5395), (2, 900, 32768, 16384, 4),
    (1, 255, 1024, 1024, 1), (1, 255, 1025, 1025, 1), (1, 255, 2049, 2049, 1), (1, 524032, 4096, 4096, 2047), (1, 524288, 4096, 4096, 2048),
    (3, 600, 3000, 1000, 3), (1, 300, 10 ** 6, 10 ** 6, 2), (1, 256, 2 ** 31 - 1, 2 ** 31 - 1, 1), (4, 0, 100, 50, 0), (0, 0, 0, 0, 0),
    (65536, 5, 5, 5, 1), (-1, 5, 5, 5, 1), (1, 2 ** 31, 5, 5, 1), (1, 5, 2 ** 31, 5, 1), (1, 5, 5, 6, 1), (1, 5, 5, 5, 6), (1, 5, 5, 5, -1)]


def test_the_chooser_is_the_headers_function_of_sizes():
    from bdm_amd import _lib as L
    lib = L.lib()
    for row in CHOOSER_ROWS:
        form, chunks = R.variant(*row)
        assert lib.bdm_face_point_distance_variant(*row) == form, row
        assert lib.bdm_face_point_distance_chunks(*row) == chunks, row
    assert R.variant(2, 900, 32768, 16384, 4) == (2, 16) and R.variant(1, 255, 2049, 2049, 1) == (2, 3)
    assert R.variant(1, 524032, 4096, 4096, 2047) == (2, 3) and R.variant(1, 524288, 4096, 4096, 2048) == (1, 1)
    assert R.variant(1, 256, 2 ** 31 - 1, 2 ** 31 - 1, 1) == (2, 4096) and R.variant(1, 300, 10 ** 6, 10 ** 6, 2) == (2, 977)
    # the project's own meshes: B = 16 at 64^3 is 4.6 workgroups per compute unit and splits in 4, 96^3 and 128^3 stay resident
    assert R.variant(16, 297480, 65536, 4096, 1170) == (2, 4) and R.variant(16, 753538, 131072, 8192, 2951) == (1, 1)
    assert lib.bdm_face_point_distance_workspace_bytes(3, 100) >= 72 * 100 + 3 * 8 * 4
    assert lib.bdm_face_point_distance_workspace_bytes(65536, 5) == 0 == lib.bdm_face_point_distance_workspace_bytes(1, 2 ** 31)
    assert lib.bdm_face_point_distance_workspace_bytes(0, 0) % 16 == 0


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    v, f = M.box_mesh()
    pts = torch.zeros(1, 5, 3)
    bad = [lambda: MM.face_point_sqdist(([v], [f]), pts, form="exhaustive"), lambda: MM.face_point_sqdist(([v], [f]), pts, form=1),
           lambda: MM.face_point_sqdist(([v], [f]), pts, chunks=2), lambda: MM.face_point_sqdist(([v], [f]), pts, form="resident", chunks=2),
           lambda: MM.face_point_sqdist(([v], [f]), pts, form="split", chunks=0),
           lambda: MM.face_point_sqdist(([v], [f]), pts, form="split", chunks=65536),
           lambda: MM.face_point_sqdist(([v], [f]), pts, form="split", chunks=2.0),
           lambda: MM.face_point_sqdist(([v], [f]), pts[0]), lambda: MM.face_point_sqdist(([v], [f]), [pts[0], pts[0]]),
           lambda: MM.face_point_sqdist(([v], [f]), [pts[0].long()]), lambda: MM.face_point_sqdist(([v], [f]), [torch.zeros(5, 2)]),
           lambda: MM.face_point_sqdist(([v], [f]), "cloud"), lambda: MM.face_point_sqdist((v, f), pts),
           lambda: MM.face_point_sqdist(([v], [f.float()]), pts),
           lambda: MM.point_mesh_face_distance(([v], [f]), pts, min_triangle_area=5e-3),
           lambda: MM.point_mesh_face_distance(([v], [f]), pts, 0.0), lambda: MM.point_mesh_face_distance(([v], [f]), torch.zeros(2, 5, 3)),
           lambda: MM.point_mesh_face_distance(([], []), []), lambda: MM.point_mesh_face_distance(([v], [f]), [torch.zeros(5)])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="no area floor"):
        MM.point_mesh_face_distance(([v], [f]), pts, min_triangle_area=5e-3)
    assert MM.face_point_sqdist(([], []), []) == ([], [])
    with pytest.raises(SystemExit):
        MM.parse_args(["--mesh_dir", "a", "--gt_dir", "b", "--two-sided", "yes"])
    assert MM.parse_args(["--mesh_dir", "a", "--gt_dir", "b", "--two-sided"]).two_sided is True
    assert MM.parse_args(["--mesh_dir", "a", "--gt_dir", "b"]).two_sided is False


# ---- the walk, with the kernels replaced by the restatement -------------------------------------------------------------------------
@pytest.fixture()
def ref_kernels(monkeypatch):
    """bdm_amd.mesh_metrics on the host: its three device operators and the two cloud scores replaced by restatements."""
    from bdm_amd import evaluation as E
    from bdm_amd.ragged import mesh_lists

    def sample(meshes, num_samples=10000, return_normals=False, *, seed=0, first_index=0, return_face_idx=False):
        vl, fl = mesh_lists(meshes)
        rows = [M.sample_mesh(v, f, num_samples, M.ref_rng.shape_key(seed, first_index + m)) for m, (v, f) in enumerate(zip(vl, fl))]
        return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]).long()

    def point_side(meshes, points, **_):
        vl, fl = mesh_lists(meshes)
        out = M.distance_batch(vl, fl, points)
        return out["sqdist"], out["face_idx"].long()

    def face_side(meshes, points, **_):
        vl, fl = mesh_lists(meshes)
        rows = [R.face_point_mesh(v, f, p) for v, f, p in zip(vl, fl, MM._cloud_list(points, len(vl)))]
        return [r[0] for r in rows], [r[1].long() for r in rows]

    def nn(a, b):
        return torch.cdist(a.double(), b.double()).pow(2).min(dim=2).values

    monkeypatch.setattr(MM, "sample_points_from_meshes", sample)
    monkeypatch.setattr(MM, "point_mesh_sqdist", point_side)
    monkeypatch.setattr(MM, "face_point_sqdist", face_side)
    monkeypatch.setattr(E, "chamfer_distance_x1000", lambda s, g: (nn(s, g).mean(1) + nn(g, s).mean(1)) * 1000.0)
    monkeypatch.setattr(E, "f1_score", lambda s, g, thr=0.01: (nn(s, g) < thr).double().mean(1))


def _tree(tmp_path):
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    box_v, box_f = M.box_mesh(0.5, 0.75, 1.0, (0.0625, 0.0, -0.125))   # every coordinate exact in float32: area 3.25
    blob_v, blob_f = M.box_mesh(0.125, 0.125, 0.125, (2.0, 0.0, 0.0))   # area 0.09375
    ico_v, ico_f = M.icosphere(1, 0.5)
    meshes = {"a/box_blob.ply": (torch.cat([box_v, blob_v]), torch.cat([box_f, blob_f + 8])), "b/ico.ply": (ico_v, ico_f),
              "c/none.ply": (ico_v, torch.tensor([[0, 0, 1]]))}
    gts = {"a/box_blob.ply": M.sample_mesh(box_v, box_f, 300, M.sample_keys(1, 9)[0])[0], "b/ico.ply": M.cloud(300, 8, spread=1.0),
           "c/none.ply": M.cloud(300, 9)}
    for rel, (v, f) in meshes.items():
        save_mesh_ply(v.numpy(), f.numpy(), tmp_path / "mesh" / rel)
        save_pointcloud_ply(gts[rel].numpy(), str(tmp_path / "gt" / rel))
    return meshes, gts


def test_evaluate_mesh_dirs_two_sided_and_the_cli_walk(ref_kernels, tmp_path, monkeypatch, capsys):
    meshes, gts = _tree(tmp_path)
    one = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=3, device="cpu")
    two = MM.evaluate_mesh_dirs(tmp_path / "mesh", tmp_path / "gt", seed=3, device="cpu", two_sided=True)
    assert list(one) == ["num", "cd_x1000", "f1_at_0.01", "gt_to_surface_x1000", "gt_within_0.01", "empty"]
    assert {k: two[k] for k in one} == one and one["num"] == 3 and one["empty"] == 1
    rows = [_row(*meshes[rel], gts[rel]) for rel in ("a/box_blob.ply", "b/ico.ply")]
    want = MM.compose_scores(rows + [None])
    for k in ("surface_to_gt_x1000", "surface_within_0.01", "face_distance_x1000"):
        assert two[k] == want[k], k
    # by hand: the blob is 0.09375 of the first mesh's area 3.34375 and its only part farther than 0.1 from the ground truth
    ico_sq, ico_area = rows[1][3], rows[1][4]
    assert two["surface_within_0.01"] == pytest.approx((3.25 / 3.34375 + ico_area[ico_sq < 0.01].sum() / ico_area.sum()) / 2, rel=1e-15)
    assert two["surface_to_gt_x1000"] > 1000 * (0.09375 / 3.34375) * 1.5 ** 2 / 2
    sym = [float(M.distance_mesh(*meshes[rel], gts[rel])[0].double().mean() + r[3].mean()) for rel, r in zip(("a/box_blob.ply", "b/ico.ply"), rows)]
    assert two["face_distance_x1000"] == float(np.mean(sym)) * 1000.0
    # the command line: the same walk, the flag decides what is printed
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    walk = MM.evaluate_mesh_dirs
    monkeypatch.setattr(MM, "evaluate_mesh_dirs", lambda *a, **k: walk(*a, device="cpu", **k))
    args = ["--mesh_dir", str(tmp_path / "mesh"), "--gt_dir", str(tmp_path / "gt"), "--seed", "3"]
    assert MM.main(args) == one and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(one))
    assert MM.main(args + ["--two-sided"]) == two
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(two))


def test_symmetric_distance_is_the_float64_composition():
    c = R.case("ragged")
    keep = [0, 1, 3]   # the meshes with faces (a mean over no faces is NaN)
    vl, fl, cl = [c["verts"][i] for i in keep], [c["faces"][i] for i in keep], [c["clouds"][i] for i in keep]
    cl[0] = M.cloud(7, 2)
    want, count = R.symmetric(vl, fl, cl)
    got = MM.symmetric_distance([M.distance_mesh(v, f, p)[0] for v, f, p in zip(vl, fl, cl)], [R.face_point_mesh(v, f, p)[0] for v, f, p in zip(vl, fl, cl)])
    print(got, want, count)
    assert math.isfinite(want) and abs(got - want) <= count * 2.0 ** -52 * want
