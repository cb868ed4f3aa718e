"""The CPU restatement of the mesh metrics (tests/mesh_metrics_ref.py, bdm_hip.h section 14) checked on its own, without a GPU:
against a float64 evaluation of the same formulas, against analytic distances, against the statistics a surface sampler owes, and
against its mutants; plus the argument checks of bdm_amd.mesh_metrics that need no device.

The GPU test (tests/test_hip_mesh_metrics.py) compares the kernels with this restatement bit for bit; this file is what makes the
restatement worth comparing with."""
import math

import pytest
import torch

import mesh_metrics_ref as M


@pytest.mark.parametrize("name", list(M.GAP))
def test_float32_rule_stays_within_the_measured_gap_of_float64(name):
    """Per (point, valid face) pair: |d32 - d64| <= GAP_MARGIN x the worst case tools/mesh_metrics_gap.py measured on these inputs
    (absolute, and relative where d64 >= 1e-6).  The margin of 2 leaves room for a libm or torch that rounds a division differently;
    a wrong formula misses by orders of magnitude."""
    worst_abs, worst_rel, pairs = M.pair_gap(name)
    bound_abs, bound_rel = (M.GAP_MARGIN * g for g in M.GAP[name])
    print(f"{name}: {pairs} pairs, absolute gap {worst_abs:.3e} (bound {bound_abs:.3e}), relative {worst_rel:.3e} (bound {bound_rel:.3e})")
    assert pairs > 100
    assert worst_abs <= bound_abs and worst_rel <= bound_rel


def test_float32_argmin_matches_float64_away_from_ties():
    """The nearest face agrees between the two precisions wherever the float64 runner-up is clearly farther."""
    c = M.dist_case(f"soup_f{2 * M.TILE + 1}_p{M.THREADS + 1}")
    got = M.distance_mesh(c["verts"][0], c["faces"][0], c["points"][0])
    fq = M.face_quantities(c["verts"][0], c["faces"][0], torch.float64)
    d64 = M.pair_sqdist(fq, c["points"][0].double())
    two = d64.topk(2, dim=1, largest=False)
    clear = two.values[:, 1] - two.values[:, 0] > 1e-5
    assert int(clear.sum()) > 200
    assert torch.equal(got[1][clear].long(), two.indices[clear, 0])
    assert float((got[0].double() - two.values[:, 0]).abs().max()) <= M.UNIT_GAP_ABS


def test_box_distances_are_the_analytic_ones():
    verts, faces = M.box_mesh()   # the unit cube around the origin
    rows = [((0.1, 0.2, 0.3), 0.04), ((0.0, 0.0, 0.0), 0.25),                               # inside
            ((0.5, 0.1, 0.2), 0.0), ((0.125, -0.5, 0.25), 0.0),                             # on a face
            ((0.5, 0.5, 0.1), 0.0), ((-0.5, 0.25, 0.5), 0.0),                               # on an edge
            ((0.5, 0.5, 0.5), 0.0), ((-0.5, 0.5, -0.5), 0.0),                               # at a vertex
            ((0.0, 0.0, 2.0), 2.25), ((1.0, 1.0, 0.0), 0.5), ((1.0, 1.0, 1.0), 0.75), ((-2.5, 0.25, 0.25), 4.0)]   # outside
    pts = torch.tensor([r[0] for r in rows])
    want = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    sq, idx = M.distance_mesh(verts, faces, pts)
    assert bool((idx >= 0).all())
    assert float((sq.double() - want).abs().max()) <= 4 * 2.0 ** -24 * 4.0   # a few roundings at the largest value in play
    assert bool((sq[2:8] == 0).all())   # the cube's coordinates and these points are exact in float32: exactly zero


def test_icosphere_distances_are_the_analytic_ones():
    verts, faces = M.icosphere(1)
    tri = verts.double()[faces]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = ((n * tri[:, 0]).sum(1) / n.norm(dim=1)) ** 2          # squared distance of every face's plane from the centre
    pts = torch.cat([torch.zeros(1, 3), verts[:5], ((verts[faces[:5, 0]] + verts[faces[:5, 1]]) / 2), tri[:5].mean(dim=1).float(),
                     verts[:3] * 2.0])
    sq, idx = M.distance_mesh(verts, faces, pts)
    # the centre projects inside every face: the nearest plane; vertices, edge midpoints and centroids lie on the surface up to the
    # rounding of the point itself (one ulp of a coordinate below 1: 6e-8, squared); 2 v is |v| = 1 away from its vertex
    assert abs(float(sq[0]) - float(plane.min())) <= 1e-6
    assert bool((sq[1:6] == 0).all())
    assert float(sq[6:16].max()) <= (4 * 2.0 ** -24) ** 2
    assert float((sq[16:].double() - 1.0).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", ["ico_s4097", "batch3", "box", "degenerate"])
def test_samples_lie_on_their_reported_face(name):
    c, ref = M.sample_case(name), M.sample_ref(name)
    for verts, faces, pts, idx, nrm in zip(c["verts"], c["faces"], ref["points"], ref["face_idx"], ref["normals"]):
        if faces.shape[0] == 0:
            assert bool((idx == -1).all()) and bool((pts == 0).all()) and bool((nrm == 0).all())
            continue
        fq32 = M.face_quantities(verts, faces)
        assert bool((idx >= 0).all()) and bool(fq32["valid"][idx.long()].all())
        fq = M.face_quantities(verts, faces[idx.long()], torch.float64)
        d = M.pair_sqdist(fq, pts.double()).diagonal()
        scale = float(verts[torch.isfinite(verts).all(dim=1)].abs().max())
        # three products and two sums of coordinates up to `scale`, each rounded to float32: the point is within 4 ulp of the face
        assert float(d.max()) <= (4 * 2.0 ** -24 * scale) ** 2 * 3
        assert float((nrm.double().norm(dim=1) - 1).abs().max()) <= 4 * 2.0 ** -24


def test_sample_counts_follow_the_areas():
    """Pearson's chi-square statistic of the face counts of 200 000 samples of a 1 x 2 x 3 box (12 faces, areas 3, 3, 3, 3, 1.5 x 4,
    1 x 4 of 22) against the area shares, 11 degrees of freedom: below 31.26, the 0.999 quantile.  Seed index 0 of SEED: the first
    one tried (a correct sampler fails one seed in a thousand; the no_sqrt and q_truncated mutants leave the counts alone, a
    sampler that ignores the areas gives a statistic in the tens of thousands)."""
    verts, faces = M.box_mesh(1.0, 2.0, 3.0)
    S = 200000
    _, idx, _ = M.sample_mesh(verts, faces, S, M.sample_keys(1, 0)[0])
    counts = torch.bincount(idx.long(), minlength=12).double()
    fq = M.face_quantities(verts, faces, torch.float64)
    share = fq["nn"].sqrt() / fq["nn"].sqrt().sum()
    assert torch.allclose(share * 22, torch.tensor([3.0] * 4 + [1.5] * 4 + [1.0] * 4, dtype=torch.float64))
    stat = float(((counts - S * share) ** 2 / (S * share)).sum())
    print(f"chi-square statistic {stat:.2f} (11 degrees of freedom, 0.999 quantile 31.26)")
    assert stat < 31.26
    uniform = float(((counts - S / 12) ** 2 / (S / 12)).sum())
    assert uniform > 1000   # the same counts against equal shares: the test can tell


def test_barycentric_weights_are_uniform_over_the_face():
    """With the square root the samples of one triangle are uniform: the mean of every barycentric weight is 1 / 3 (without it the
    first weight's mean is 1 / 2)."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    pts, _, _ = M.sample_mesh(verts, torch.tensor([[0, 1, 2]]), 20000, M.sample_keys(1, 1)[0])
    b1, b2 = pts[:, 0].double(), pts[:, 1].double()
    means = torch.stack([1 - b1 - b2, b1, b2]).mean(dim=1)
    assert float((means - 1 / 3).abs().max()) < 0.01   # sigma of a mean of 20 000 weights is 0.0017


@pytest.mark.parametrize("mutant", list(M.DIST_MUTANTS))
def test_distance_cases_tell_every_mutant_from_the_rule(mutant):
    hit = [n for n in M.DIST_CASES if not M.same(M.dist_ref(n), M.dist_ref(n, mutant))]
    print(f"{mutant} ({M.DIST_MUTANTS[mutant]}): told apart by {hit}")
    assert hit


@pytest.mark.parametrize("mutant", list(M.SAMPLE_MUTANTS))
def test_sample_cases_tell_every_mutant_from_the_rule(mutant):
    hit = [n for n in M.SAMPLE_CASES if not M.same(M.sample_ref(n), M.sample_ref(n, mutant))]
    print(f"{mutant} ({M.SAMPLE_MUTANTS[mutant]}): told apart by {hit}")
    assert hit


def test_the_l2_shortcut_is_unreachable_on_valid_faces():
    """Why the mutant that drops `t = 0 when l2 == 0` is exempt (mesh_metrics_ref.EQUIVALENT_MUTANTS): on every test input a face
    with a zero-length edge has nn == 0 and is invalid, and the mutant changes no output."""
    seen = 0
    for name in M.DIST_CASES:
        c = M.dist_case(name)
        for verts, faces in zip(c["verts"], c["faces"]):
            fq = M.face_quantities(verts, faces)
            zero_edge = (fq["l2"] == 0).any(dim=1)
            seen += int(zero_edge.sum())
            assert not bool((zero_edge & fq["valid"]).any())
        assert M.same(M.dist_ref(name), M.dist_ref(name, "no_l2_shortcut"))
    assert seen >= 3   # the degenerate case does hold such faces


def test_the_tiny_case_reaches_the_small_faces_and_a_second_scan_pass():
    c, ref = M.sample_case("tiny"), M.sample_ref("tiny")
    F = c["faces"][0].shape[0]
    q, C, _, _ = M.face_weights(c["verts"][0], c["faces"][0])
    assert F > M.SCAN_SPAN and bool((q[:-1] == 2).all()) and int(q[-1]) == 1 << 30
    assert int((ref["face_idx"][0] < F - 1).sum()) >= 1


def test_a_sliver_face_defeats_any_tile_bound():
    """Why the culled form is not built: a VALID sliver face (its middle vertex one ulp off the line through the
    other two) whose computed normal is rounding noise.  A point on the sliver's axis, 1.76 beyond its tip, passes the inside test and
    lies in the computed plane: the rule gives 0 where the true squared distance is 3.1.  No bound derived from the distance to a
    box around such a face can stay below the rule's value."""
    off = torch.nextafter(torch.tensor(0.3), torch.tensor(1.0))
    verts = torch.tensor([[0.1, 0.1, 0.1], [0.3, 0.3, float(off)], [0.7, 0.7, 0.7]])
    faces = torch.tensor([[0, 1, 2]])
    assert bool(M.face_quantities(verts, faces)["valid"][0])
    pts = torch.full((1, 3), 1.7160909175872803)
    d32, idx = M.distance_mesh(verts, faces, pts)
    true = M.pair_sqdist(M.face_quantities(verts, faces, torch.float64), pts.double())[0, 0]
    print(f"computed {float(d32[0]):.3e}, float64 {float(true):.4f}")
    assert int(idx[0]) == 0 and float(d32[0]) == 0.0 and 3.09 < float(true) < 3.10


def test_morton_order_is_a_permutation():
    pts = M.dist_case("degenerate")["points"]
    order = M.morton_order(pts)
    assert torch.equal(torch.sort(order.long(), dim=1).values, torch.arange(pts.shape[1])[None])


def test_python_surface_refuses_bad_arguments_before_any_launch():
    from bdm_amd import mesh_metrics as MM
    from bdm_amd import rng
    from bdm_amd._lib import BdmHipError
    assert rng.MESH == M.MESH_PURPOSE == 5
    verts, faces = M.box_mesh()
    with pytest.raises(ValueError):
        MM.sample_points_from_meshes(([verts], [faces.float()]), 10)
    with pytest.raises(ValueError):
        MM.sample_points_from_meshes(([verts], [faces.bool()]), 10)
    with pytest.raises(ValueError):
        MM.sample_points_from_meshes(([verts], [faces]), 0)
    with pytest.raises(ValueError):
        MM.sample_points_from_meshes(verts, 10)
    with pytest.raises(ValueError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(1, 4, 3), form="culled")
    with pytest.raises(ValueError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(2, 4, 3))
    with pytest.raises(ValueError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(1, 4, 2))
    with pytest.raises(ValueError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(1, 4, 3), order=torch.zeros(1, 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(1, 4, 3), order="hilbert")
    with pytest.raises(BdmHipError):   # host tensors: no CPU fallback
        MM.sample_points_from_meshes(([verts], [faces]), 10)
    with pytest.raises(BdmHipError):
        MM.point_mesh_sqdist(([verts], [faces]), torch.zeros(1, 4, 3))
    if not torch.cuda.is_available():
        with pytest.raises(BdmHipError):
            MM.main(["--mesh_dir", "a", "--gt_dir", "b"])
    assert math.isnan(MM.compose_scores([])["cd_x1000"]) and MM.compose_scores([None])["empty"] == 1
