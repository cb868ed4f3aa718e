"""Host side of the generation metrics (bdm_amd/metrics.py): the MMD / COV / 1-NNA reductions on hand-built matrices, the float64
restatement of the approximate-match EMD checked by properties that owe nothing to a kernel (with mutants that must trip them),
and the command line with the GPU calls stubbed.  No GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from bdm_amd import metrics as M


# ---- MMD / COV ---------------------------------------------------------------------------------------------------------------
def test_mmd_cov_known_answer_with_coverage_below_one():
    dist = torch.tensor([[1.0, 5.0, 9.0], [2.0, 0.5, 8.0]])   # 2 samples x 3 references; reference 2 is nobody's nearest
    out = M.mmd_cov(dist)
    assert out["mmd"] == pytest.approx((1.0 + 0.5 + 8.0) / 3.0, rel=1e-15)
    assert out["mmd_smp"] == pytest.approx((1.0 + 0.5) / 2.0, rel=1e-15)
    assert out["cov"] == pytest.approx(2.0 / 3.0, rel=1e-15)
    assert all(isinstance(v, float) for v in out.values())


def test_mmd_cov_tie_goes_to_the_lower_index():
    # sample 0 is equally near references 0 and 1, sample 1 nearest to 0: lowest index -> {0} = 1/3; highest index would give {1, 0} = 2/3
    dist = np.array([[1.0, 1.0, 5.0], [1.0, 5.0, 5.0]], dtype=np.float32)
    assert M.mmd_cov(dist)["cov"] == pytest.approx(1.0 / 3.0, rel=1e-15)


# ---- 1-NNA -------------------------------------------------------------------------------------------------------------------
def test_one_nn_tie_lower_index_and_diagonal_excluded():
    dxx = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    dyy = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    dxy = torch.tensor([[1.0, 3.0], [3.0, 1.0]])
    # rows of the stacked matrix (diagonal = inf): s0 [inf 1 1 3] -> item 1 (sample, tie with item 2), s1 [1 inf 3 1] -> item 0,
    # r0 [1 3 inf 1] -> item 0 (sample, tie with item 3), r1 [3 1 1 inf] -> item 1 (sample).  With the zero diagonal left in, every
    # item would pick itself (accuracy 1); with ties to the higher index the two halves would swap.
    out = M.one_nn_accuracy(dxx, dxy, dyy)
    assert out == {"acc": 0.5, "acc_sample": 1.0, "acc_ref": 0.0}


def test_one_nn_two_separated_clusters():
    rng = np.random.default_rng(0)
    x, y = rng.normal(0.0, 0.1, (5, 3)), rng.normal(10.0, 0.1, (7, 3))
    d = lambda p, q: ((p[:, None] - q[None]) ** 2).sum(-1)
    out = M.one_nn_accuracy(d(x, x), d(x, y), d(y, y))
    assert out == {"acc": 1.0, "acc_sample": 1.0, "acc_ref": 1.0}


def test_one_nn_identical_sets_is_exactly_zero():
    """sample == ref, distinct items: each item's nearest OTHER item is its copy in the other set at distance 0 (its own entry is the
    removed diagonal), so every prediction is wrong: accuracy 0 by hand, in all three figures."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=(6, 3))
    d = ((x[:, None] - x[None]) ** 2).sum(-1)
    out = M.one_nn_accuracy(d, d, d)
    assert out == {"acc": 0.0, "acc_sample": 0.0, "acc_ref": 0.0}


def test_one_nn_unequal_set_sizes():
    # 1 sample, 3 references on a line at 0 | 1, 2, 3: sample -> r0 (wrong); r0 -> sample (distance 1, tie with r1: lower index, wrong);
    # r1 -> r0 (tie with r2: lower), r2 -> r1: acc 2/4
    pts = np.array([0.0, 1.0, 2.0, 3.0])
    d = np.abs(pts[:, None] - pts[None])
    out = M.one_nn_accuracy(d[:1, :1], d[:1, 1:], d[1:, 1:])
    assert out == {"acc": 0.5, "acc_sample": 0.0, "acc_ref": pytest.approx(2.0 / 3.0, rel=1e-15)}


# ---- approximate-match EMD: properties of the float64 restatement ------------------------------------------------------------
def lattice_cloud(seed):
    """512 points on an 8^3 lattice of pitch 0.25 jittered by +-0.05: every two points are at least 0.15 apart."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.stack(np.meshgrid(*[np.arange(8) * 0.25 - 0.875] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g + rng.uniform(-0.05, 0.05, g.shape)).astype(np.float32)


def restatement_failures(fn, sizes=(256, 1024)):
    """Names of the properties `fn` (a variant of metrics_ref.emd_approx_ref) violates.
    1. mass: the ten levels match all of the mass: |sum w - n| <= 1e-6 n (the 1e-9 of the denominators leaves ~5e-10 per point).
    2. lower bound: a feasible transport plan costs at least the optimal one: value >= exact EMD (scipy's optimal assignment).
    3. self-distance: the first level's kernel exp(-16384 d^2) is < exp(-368) between two points >= 0.15 apart, so a cloud is
       matched to itself at distance 0 but for the 1e-9 the denominator holds back per point, which later levels move at most one
       diameter (< 4): cost(a, a) / n <= 1e-8.  (Level order matters here and only here: a coarse first level spreads the mass.)"""
    failed = []
    for n in sizes:
        a, b = R.gaussian(1, n, 7)[0], R.uniform(1, n, 8)[0]
        value, mass = fn(a, b, return_mass=True)
        if not abs(mass - n) <= 1e-6 * n:
            failed.append(f"mass n={n}: {mass / n - 1:+.2e}")
        exact = R.emd_exact(a, b)
        if not value >= exact:
            failed.append(f"lower bound n={n}: {value} < {exact}")
    self_cost = fn(lattice_cloud(3), lattice_cloud(3))
    if not 0.0 <= self_cost <= 1e-8:
        failed.append(f"self-distance: {self_cost:.3e}")
    return failed


def test_emd_restatement_properties():
    assert restatement_failures(R.emd_approx_ref) == []
    value, mass = R.emd_approx_ref(R.gaussian(1, 2048, 7)[0], R.uniform(1, 2048, 8)[0], return_mass=True)
    assert abs(mass - 2048) <= 1e-6 * 2048
    assert 0.05 < value < 1.0


def test_emd_restatement_is_not_symmetric():
    a, b = R.gaussian(1, 256, 7)[0], R.uniform(1, 256, 8)[0]
    assert abs(R.emd_approx_ref(a, b) - R.emd_approx_ref(b, a)) > 1e-6


@pytest.mark.parametrize("name,kwargs,trips", [
    ("levels_reversed", {"level_order": R.LEVELS[::-1]}, "self-distance"),
    ("pass2_without_min", {"clamp": False}, "mass"),
])
def test_emd_restatement_mutants_trip_a_property(name, kwargs, trips):
    failed = restatement_failures(lambda a, b, **kw: R.emd_approx_ref(a, b, **kwargs, **kw), sizes=(256,))
    assert any(f.startswith(trips) for f in failed), f"mutant {name} passed every property: {failed}"


def test_chamfer_reference_known_answer():
    a = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    b = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [1.0, 0.0, 1.0]], dtype=np.float32)
    ab, ba = R.chamfer_ref(a, b)
    assert ab == pytest.approx((0.0 + 1.0) / 2.0, rel=1e-15)
    assert ba == pytest.approx((0.0 + 4.0 + 1.0) / 3.0, rel=1e-15)


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    args = M.parse_args(["--sample", "s.npy", "--ref", "r.npy"])
    assert args.metrics == ("cd", "emd") and args.normalize is False and args.batch_size is None
    args = M.parse_args(["--sample", "s", "--ref", "r", "--metrics", "emd", "--normalize", "--batch-size", "7"])
    assert args.metrics == ("emd",) and args.normalize is True and args.batch_size == 7
    with pytest.raises(SystemExit):
        M.parse_args(["--sample", "s", "--ref", "r", "--metrics", "jsd"])
    with pytest.raises(SystemExit):
        M.parse_args(["--sample", "s"])


def test_loaders_npy_and_ply_directory(tmp_path):
    from bdm_amd.io import save_pointcloud_ply
    clouds = R.gaussian(3, 17, 5)
    np.save(tmp_path / "c.npy", clouds.astype(np.float64))
    got = M.load_clouds(str(tmp_path / "c.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, clouds)
    os.makedirs(tmp_path / "plys")
    for i, c in enumerate(clouds):
        save_pointcloud_ply(c, str(tmp_path / "plys" / f"shape_{i:02d}.ply"))
    assert np.array_equal(M.load_clouds(str(tmp_path / "plys")), clouds)
    np.save(tmp_path / "bad.npy", np.zeros((3, 17)))
    with pytest.raises(ValueError):
        M.load_clouds(str(tmp_path / "bad.npy"))
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError):
        M.load_clouds(str(tmp_path / "empty"))


def test_normalize_unit_sphere():
    out = M.normalize_unit_sphere(R.gaussian(4, 50, 9, scale=3.0, offset=10.0))
    assert out.dtype == np.float32
    assert np.abs(out.mean(axis=1)).max() < 1e-6
    assert np.allclose(np.sqrt((out ** 2).sum(-1)).max(axis=1), 1.0, atol=1e-6)


def test_cli_end_to_end_with_stubbed_gpu(tmp_path, monkeypatch, capsys):
    """main(): load, normalise, all six figures per distance, one JSON line -- the two distance matrices come from the float64
    references instead of the kernels."""
    sample, ref = R.gaussian(4, 32, 11), R.uniform(5, 32, 12)
    np.save(tmp_path / "s.npy", sample)
    np.save(tmp_path / "r.npy", ref)
    calls = []

    def fake_chamfer(a, b, batch_size=None):
        calls.append(("cd", batch_size))
        ab, ba = R.chamfer_matrix_ref(a.numpy(), b.numpy())
        return torch.from_numpy(ab + ba)

    def fake_emd(a, b, batch_size=None):
        calls.append(("emd", batch_size))
        return torch.tensor([[R.emd_approx_ref(p, q) for q in b.numpy()] for p in a.numpy()])

    monkeypatch.setattr(M, "_to_device", torch.from_numpy)
    monkeypatch.setattr(M, "pairwise_chamfer", fake_chamfer)
    monkeypatch.setattr(M, "pairwise_emd", fake_emd)
    M.main(["--sample", str(tmp_path / "s.npy"), "--ref", str(tmp_path / "r.npy"), "--normalize", "--batch-size", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    keys = {f"{k}-{m}" for k in ("mmd", "mmd_smp", "cov", "1nna", "1nna_sample", "1nna_ref") for m in ("cd", "emd")}
    assert keys <= set(out) and out["num_sample"] == 4 and out["num_ref"] == 5 and out["num_points"] == 32
    assert all(isinstance(out[k], float) for k in keys)
    assert calls == [("cd", 2)] * 3 + [("emd", 2)] * 3
    s_n, r_n = M.normalize_unit_sphere(sample), M.normalize_unit_sphere(ref)
    ab, ba = R.chamfer_matrix_ref(s_n, r_n)
    assert out["mmd-cd"] == pytest.approx(float((ab + ba).min(axis=0).mean()), rel=1e-12)
    assert 0.0 < out["cov-cd"] <= 1.0 and 0.0 <= out["1nna-emd"] <= 1.0


def test_device_only_no_cpu_fallback():
    from bdm_amd import _lib
    with pytest.raises(_lib.BdmHipError):
        M.pairwise_chamfer(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(_lib.BdmHipError):
        M.pairwise_emd(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError):
        M.pairwise_emd(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(ValueError):
        M.compute_all_metrics(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), metrics=("jsd",))
