"""The alignment rule without a GPU: the restatement tests/align_ref.py against the float64 SVD definition, ICP recovering a known
motion, the mutants against the GPU test's own inputs, the argument errors of bdm_amd.alignment and the evaluator's new fields on a
stub."""
import json
import math

import numpy as np
import pytest
import torch

import align_ref as A
from bdm_amd import alignment as AL   # the feature itself: without it this file fails at import

GAP_GENERAL, GAP_NEAR_REFLECTION = A.GAP_GENERAL, A.GAP_NEAR_REFLECTION   # four times what tools/align_gap.py measures


# ---- the solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "planar", "collinear", "single", "near_reflection"])
def test_solve_equals_the_svd_definition(name):
    bound = GAP_NEAR_REFLECTION if name == "near_reflection" else GAP_GENERAL
    worst = 0.0
    for m, e, estimate_scale in A.solve_cases()[name]:
        gap = A.solve_gap(m, e, estimate_scale, collinear=name == "collinear")
        worst = max(worst, gap)
        R = torch.tensor([float(v) for v in A.solve(m, e, estimate_scale)[0]], dtype=torch.float64).view(3, 3)
        assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14 and abs(float(torch.det(R)) - 1.0) < 1e-14   # a proper rotation
    print(f"{name}: largest gap {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def test_single_pair_and_zero_moments_give_the_identity():
    m, e, _ = A.solve_cases()["single"][0]
    R, T, s, mse = A.solve(m, e)
    assert [float(v) for v in R] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and float(s) == 1.0 and float(mse) == 0.0
    # T = y - x on the fixed-point grid: amax = 3 leaves steps of 2^-22, half a step per coordinate of x and of y
    assert float((A.to_f32(R, T, s)[9:12].double() - torch.tensor([0.7, 2.2, 2.1], dtype=torch.float64)).abs().max()) <= 2.0 ** -22 + 2.0 ** -23


def test_near_reflection_is_where_the_determinant_correction_acts():
    for m, e, _ in A.solve_cases()["near_reflection"]:
        M = A.central_moments(m, e)[3]
        plain = torch.tensor([float(v) for v in A.svd_rotation(M, det_fix=False)], dtype=torch.float64).view(3, 3)
        assert float(torch.det(plain)) < -0.99          # the unconstrained optimum is a reflection
        fixed = torch.tensor([float(v) for v in A.solve(m, e)[0]], dtype=torch.float64).view(3, 3)
        assert float(torch.det(fixed)) > 0.99


def test_the_sweep_count_leaves_two_spare():
    """align_solve.h runs 10 sweeps; on every case here the off-diagonal falls below 1e-17 of the largest eigenvalue within 8."""
    for rows in A.solve_cases().values():
        for m, e, _ in rows:
            M = A.central_moments(m, e)[3]
            assert A.horn_rotation(M, A.SWEEPS - 2, return_offdiag=True)[1] < 1e-17


def test_fixed_point_rule():
    x = torch.tensor([[1.5, -0.25, 0.0], [float("nan"), 9.0, 9.0]])
    y = torch.tensor([[0.5, 0.5, -3.0], [100.0, float("inf"), 0.0]])
    e = A.scale_exp(x, y)                                  # amax = 3 (the non-finite rows do not count): E = 1, bits = 24
    assert e == 24 - 1 - 1
    assert A.scale_exp(torch.zeros(1, 3), torch.zeros(1, 3)) == 23 + 126
    assert A.scale_exp(torch.ones(16385, 3), torch.ones(1, 3)) == (62 - 15) // 2 - 1 - 0
    assert A.scale_exp(torch.ones(2 ** 20, 3), torch.ones(1, 3)) == 21 - 1
    m = A.moments(x, y, torch.tensor([0, -1]), e)
    q = 2 ** e
    assert m[0] == 1 and m[1:4] == [int(1.5 * q), int(-0.25 * q), 0] and m[4:7] == [q // 2, q // 2, -3 * q]
    assert m[7] == int(1.5 * q) * (q // 2) and m[16] == int(1.5 * q) ** 2 + int(0.25 * q) ** 2 and m[17] == 2 * (q // 2) ** 2 + 9 * q * q
    assert A.quantise(torch.tensor([[0.5, 1.5, 2.5]]), 0) == [[0, 2, 2]]          # half to even


# ---- ICP ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, degrees, scale", [(512, 10.0, 1.0), (512, 10.0, 1.1), (257, 5.0, 1.0), (1025, 10.0, 1.0)])
def test_icp_recovers_a_permuted_rotated_translated_copy(n, degrees, scale):
    """Float32 inputs: y is rounded once to float32 (relative 6e-8 of coordinates below 1), so R and T come back to 1e-6."""
    x = A.box(n, 200 + n)
    shift = (0.05, 0.02, -0.04)
    y = A.moved(x, degrees, shift, scale=scale, seed=300 + n)
    res = A.icp([x], [y], max_iterations=30, estimate_scale=scale != 1.0)[0]
    print(f"n = {n}, {degrees} degrees, scale {scale}: {res['iterations']} iterations, mse {float(res['mse']):.3e}")
    assert res["converged"] and res["iterations"] < 30
    want = torch.cat([A.rotation_matrix((1.0, 2.0, 3.0), degrees).reshape(-1), torch.tensor(shift, dtype=torch.float64), torch.tensor([scale], dtype=torch.float64)])
    assert float((res["tr"].double() - want).abs().max()) < 1e-6
    assert float(res["mse"]) < 1e-12


def test_gpu_cases_hold_what_they_are_there_for():
    ref = A.icp_ref("rigid")
    assert all(r["converged"] for r in ref) and [r["iterations"] > 2 for r in ref] == [True] * 3 and float(ref[2]["mse"]) > 1e-4
    assert all(len(r["history"]) == r["iterations"] for r in ref)
    stop = A.icp_ref("stop")
    assert stop[0]["iterations"] == 2 and stop[0]["converged"] and stop[1]["iterations"] > 2
    ident = A.icp_ref("identical")[0]
    assert ident["iterations"] == 1 and ident["converged"] and float(ident["mse"]) == 0.0 and torch.equal(ident["tr"], A.identity())
    cap = A.icp_ref("capped")
    assert [(r["iterations"], r["converged"]) for r in cap] == [(3, False), (0, False), (0, False)]
    assert math.isnan(float(cap[1]["mse"])) and torch.equal(cap[2]["tr"], A.identity())
    c = A.moment_case()
    assert [(x.shape[0], y.shape[0]) for x, y in zip(c["x"], c["y"])] == list(A.MOMENT_SIZES)
    assert int((~torch.isfinite(c["x"][4]).all(1)).sum()) >= 5 and int((~torch.isfinite(c["y"][1]).all(1)).sum()) >= 5
    assert torch.unique(c["y"][2], dim=0).shape[0] <= 100 and float(c["x"][3].mean()) > 49.0
    ref = A.moment_ref(0)
    assert [m[0] for m, _, _ in ref][5:] == [0, 0] and all(m[0] > 0 for m, _, _ in ref[:5]) and ref[4][0][0] < 300
    assert all(abs(v) < 2 ** 62 for m, _, _ in ref for v in m)
    scale = A.icp_ref("scale")
    assert abs(float(scale[1]["tr"][12]) - 1.1) < 1e-5


MUTANT_SHOWS = {"ties_latest": "partner", "no_det_fix": "paired", "transposed_R": "rigid", "scale_from_yvar": "scale", "incremental": "rigid",
                "batch_stop": "stop", "no_zero_stop": "identical"}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_mutant_changes_an_output_on_a_gpu_case(mutant):
    where = MUTANT_SHOWS[mutant]
    if where == "partner":
        changed = sum(int((g[2] != b[2]).sum()) for g, b in zip(A.moment_ref(0), A.moment_ref(0, mutant)))
    elif where == "paired":
        changed = sum(int((A.bits(g[0]) != A.bits(b[0])).sum()) for g, b in zip(A.paired_ref(False), A.paired_ref(False, mutant)))
    else:
        changed = 0
        for g, b in zip(A.icp_ref(where), A.icp_ref(where, mutant)):
            changed += int((A.bits(g["tr"]) != A.bits(b["tr"])).sum()) + int(g["iterations"] != b["iterations"]) + int(g["converged"] != b["converged"])
    print(f"{mutant} on {where}: {changed} outputs differ")
    assert changed > 0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch():
    from bdm_amd import _lib as L
    assert AL.ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history") and AL.SimilarityTransform._fields == ("R", "T", "s")
    x, y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    with pytest.raises(NotImplementedError, match="allow_reflection"):
        AL.iterative_closest_point(x, y, allow_reflection=True)
    with pytest.raises(NotImplementedError, match="allow_reflection"):
        AL.corresponding_points_alignment(x, x, allow_reflection=True)
    with pytest.raises(NotImplementedError, match="weights"):
        AL.corresponding_points_alignment(x, x, weights=torch.full((2, 5), 0.5))
    with pytest.raises(ValueError, match="weights"):
        AL.corresponding_points_alignment(x, x, weights=torch.ones(2, 4))
    with pytest.raises(ValueError, match="same number of points"):
        AL.corresponding_points_alignment(x, y)
    with pytest.raises(ValueError, match="eps"):
        AL.corresponding_points_alignment(x, x, eps=-1.0)
    with pytest.raises(ValueError, match="same number of batches"):
        AL.iterative_closest_point(x, y[:1])
    with pytest.raises(ValueError, match="D = 3"):
        AL.iterative_closest_point(torch.zeros(2, 5, 2), y)
    with pytest.raises(ValueError, match="D = 3"):
        AL.iterative_closest_point([torch.zeros(5, 2)], [y[0]])
    with pytest.raises(ValueError, match="Pointclouds"):
        AL.iterative_closest_point("x", y)
    for bad in (0, -1, 2.5, 10001):
        with pytest.raises(ValueError, match="max_iterations"):
            AL.iterative_closest_point(x, y, max_iterations=bad)
    with pytest.raises(ValueError, match="relative_rmse_thr"):
        AL.iterative_closest_point(x, y, relative_rmse_thr=float("nan"))
    with pytest.raises(ValueError, match="init_transform"):
        AL.iterative_closest_point(x, y, init_transform=(torch.eye(3)[None], torch.zeros(1, 3), torch.ones(1)))
    with pytest.raises(ValueError, match="transform of 2 entries"):
        AL.apply_similarity_transform(x, torch.eye(3)[None], torch.zeros(2, 3), torch.ones(2))
    for call in (lambda: AL.iterative_closest_point(x, y), lambda: AL.corresponding_points_alignment(x, x, weights=torch.ones(2, 5)),
                 lambda: AL.apply_similarity_transform(x, torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.ones(2)),
                 lambda: AL.iterative_closest_point([x[0]], [y[0]])):
        with pytest.raises(L.BdmHipError):   # host tensors are refused: no CPU path
            call()
    empty = AL.iterative_closest_point([], [])
    assert empty.Xt == [] and empty.converged.shape == (0,) and empty.t_history == []
    import inspect
    sig = inspect.signature(AL.iterative_closest_point).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("init_transform", None), ("max_iterations", 100), ("relative_rmse_thr", 1e-6),
                                                            ("estimate_scale", False), ("allow_reflection", False), ("verbose", False)]
    sig = inspect.signature(AL.corresponding_points_alignment).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("weights", None), ("estimate_scale", False), ("allow_reflection", False), ("eps", 1e-9)]


# ---- the evaluator --------------------------------------------------------------------------------------------------------------------
def test_evaluator_reports_the_alignment_fields_on_a_stub(tmp_path, monkeypatch):
    from bdm_amd import evaluation as E
    from bdm_amd.io import save_pointcloud_ply
    sizes = {"a/one.ply": 40, "a/two.ply": 50, "b/three.ply": 60}
    for rel, n in sizes.items():
        gt = A.box(n, n)
        pred = (gt.double() @ A.rotation_matrix((1.0, 2.0, 3.0), 8.0) + 0.3).float()
        save_pointcloud_ply(gt.numpy(), tmp_path / "gt" / rel)
        save_pointcloud_ply(pred.numpy(), tmp_path / "pred" / rel)
    save_pointcloud_ply(np.zeros((3, 3)), tmp_path / "pred" / "lonely.ply")
    calls = []

    def nn_stub(src, tgt):
        return ((src[:, :, None] - tgt[:, None]) ** 2).sum(-1).min(dim=2).values

    def align_stub(pred_list, gt_list, scale=False):
        calls.append(([p.shape[0] for p in pred_list], scale))
        res = A.icp(pred_list, gt_list, max_iterations=100, estimate_scale=scale)
        return ([r["xt"] for r in res], torch.tensor([r["converged"] for r in res]), torch.tensor([r["iterations"] for r in res], dtype=torch.int32),
                torch.stack([r["mse"] for r in res]))
    monkeypatch.setattr(E, "nn_sqdist", nn_stub)
    monkeypatch.setattr(E, "align_batch", align_stub)
    plain = E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), device="cpu")
    assert sorted(plain) == ["cd_x1000", "f1_at_0.01", "num"] and plain["num"] == 3
    res = E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), device="cpu", align="icp", batch_size=2)
    assert calls == [([40, 50], False), ([60], False)]
    assert sorted(res) == ["cd_x1000", "cd_x1000_unaligned", "f1_at_0.01", "f1_at_0.01_unaligned", "icp_converged", "icp_iterations_mean",
                           "icp_mse_mean", "num"]
    json.dumps(res)
    assert res["num"] == 3 and res["icp_converged"] == 3 and res["icp_iterations_mean"] >= 2.0 and res["icp_mse_mean"] < 1e-10
    assert abs(res["cd_x1000_unaligned"] - plain["cd_x1000"]) < 1e-9 * plain["cd_x1000"] and res["f1_at_0.01_unaligned"] == plain["f1_at_0.01"]
    assert res["cd_x1000"] < 1e-6 < res["cd_x1000_unaligned"] and res["f1_at_0.01"] > 0.999
    with_emd = E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), device="cpu", align="icp", align_scale=True, batch_size=16)
    assert calls[-1] == ([40, 50, 60], True) and "emd" not in with_emd
    with pytest.raises(ValueError, match="align"):
        E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), device="cpu", align="procrustes")
    with pytest.raises(ValueError, match="batch_size"):
        E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), device="cpu", align="icp", batch_size=0)
    args = E.parse_args(["--pred_dir", "p", "--gt_dir", "g", "--icp", "--icp-scale"])
    assert args.icp and args.icp_scale and args.batch_size == 16 and not E.parse_args(["--pred_dir", "p", "--gt_dir", "g"]).icp
    with pytest.raises(SystemExit):
        E.parse_args(["--pred_dir", "p", "--gt_dir", "g", "--icp-scale"])
