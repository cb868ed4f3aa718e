"""Host side of the occupancy-grid measures (bdm_amd/metrics.py): the grid against a literal triple loop, the Jensen-Shannon
divergence by its properties and against the float64 restatement (tests/jsd_ref.py), the occupancy entropy from hand-made counts,
and the command line.  No GPU needed."""
import warnings

import numpy as np
import pytest
import torch

import jsd_ref as J
from bdm_amd import metrics as M

KEPT_28 = len(J.kept_cells(28)[0])   # what the literal loop and the float32 norm give; pinned below


# ---- grid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 4, 28])
def test_grid_equals_the_literal_triple_loop(r):
    want, want_spacing = J.grid_loop(r)
    got, spacing = M.unit_cube_grid_point_cloud(r)
    assert got.dtype == np.float32 and got.shape == (r, r, r, 3) and spacing == want_spacing
    assert np.array_equal(got, want)
    clipped, spacing = M.unit_cube_grid_point_cloud(r, clip_sphere=True)
    flat = want.reshape(-1, 3)
    assert clipped.dtype == np.float32 and spacing == want_spacing
    assert np.array_equal(clipped, flat[np.linalg.norm(flat, axis=1) <= 0.5])
    assert np.array_equal(clipped.astype(np.float64), J.kept_cells(r)[0])


def test_kept_cells_at_28_and_small_grids():
    assert KEPT_28 == 10144   # what the literal loop gives at the resolution the literature's JSD uses
    assert len(M.unit_cube_grid_point_cloud(28, True)[0]) == KEPT_28
    assert len(M.unit_cube_grid_point_cloud(3, True)[0]) == 7     # the centre and the six axis cells, which sit ON the sphere
    assert len(M.unit_cube_grid_point_cloud(5, True)[0]) == 33
    assert len(M.unit_cube_grid_point_cloud(2, True)[0]) == 0     # all eight corners lie outside
    axis = M.unit_cube_grid_point_cloud(28)[0][:, 0, 0, 0]
    assert axis[0] == -0.5 and axis[27] == 0.5 and axis[13] == np.float32(13 * (1.0 / 27) - 0.5)


# ---- Jensen-Shannon divergence -----------------------------------------------------------------------------------------------
def histograms(seed, n=500, zeros=0.3):
    rng = np.random.default_rng(seed)
    P, Q = rng.integers(0, 1000, n).astype(np.float64), rng.integers(0, 1000, n).astype(np.float64)
    P[rng.random(n) < zeros] = 0
    Q[rng.random(n) < zeros] = 0
    return P, Q


def test_jsd_of_a_distribution_with_itself_is_zero():
    P, _ = histograms(1)
    assert M.jensen_shannon_divergence(P, P) == 0.0
    assert M.jensen_shannon_divergence(P, 3.0 * P) == pytest.approx(0.0, abs=1e-15)


def test_jsd_is_symmetric():
    P, Q = histograms(2)
    assert M.jensen_shannon_divergence(P, Q) == M.jensen_shannon_divergence(Q, P)
    assert 0.0 < M.jensen_shannon_divergence(P, Q) < 1.0


def test_jsd_of_disjoint_supports_is_exactly_one():
    assert M.jensen_shannon_divergence(np.array([1.0, 0.0]), np.array([0.0, 1.0])) == 1.0
    assert M.jensen_shannon_divergence(np.array([3.0, 3.0, 0.0, 0.0]), np.array([0.0, 0.0, 5.0, 5.0])) == 1.0
    P, Q = histograms(3, zeros=0.0)
    P[::2], Q[1::2] = 0, 0
    assert M.jensen_shannon_divergence(P + (np.arange(500) % 2), Q + ((np.arange(500) + 1) % 2)) == pytest.approx(1.0, abs=1e-14)


def test_jsd_does_not_depend_on_the_scale_of_its_inputs():
    P, Q = histograms(4)
    base = M.jensen_shannon_divergence(P, Q)
    assert M.jensen_shannon_divergence(4.0 * P, 0.5 * Q) == base   # powers of two scale exactly
    assert M.jensen_shannon_divergence(7.0 * P, Q / 3.0) == pytest.approx(base, abs=1e-14)


def test_jsd_value_errors():
    with pytest.raises(ValueError, match="Negative values"):
        M.jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="Negative values"):
        M.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([1.0, -1.0, 2.0]))   # checked before the sizes
    with pytest.raises(ValueError, match="Non equal size"):
        M.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([1.0, 1.0, 2.0]))


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_jsd_agrees_with_the_restatement(seed):
    P, Q = histograms(seed, n=10144)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # the module's own cross-check of its two formulas stays silent
        got = M.jensen_shannon_divergence(P, Q)
    assert got == pytest.approx(J.jsd_ref(P, Q), abs=1e-12)
    as_tensors = M.jensen_shannon_divergence(torch.from_numpy(P).long(), torch.from_numpy(Q).long())   # CPU tensors, integer counts
    assert as_tensors == got
    assert M.jensen_shannon_divergence(list(P), Q) == got


def test_jsd_warns_when_its_two_formulas_disagree(monkeypatch):
    monkeypatch.setattr(M, "_jsd_kl_form", lambda p, q, mix: 0.5)
    with pytest.warns(UserWarning, match="two JSD methods"):
        M.jensen_shannon_divergence(np.array([1.0, 2.0]), np.array([1.0, 2.0]))
    monkeypatch.setattr(M, "_jsd_kl_form", lambda p, q, mix: 0.9e-4)   # inside the 10e-5 the cross-check allows
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.jensen_shannon_divergence(np.array([1.0, 2.0]), np.array([1.0, 2.0]))


# ---- occupancy entropy -------------------------------------------------------------------------------------------------------
def test_occupancy_entropy_from_hand_made_counts():
    # 4 clouds, 5 cells hit by 0, 1, 2, 3, 4 of them: H(0) = H(1) = 0, H(1/2) = ln 2, H(1/4) = H(3/4) = ln 4 - (3/4) ln 3
    active = np.array([0, 1, 2, 3, 4])
    h_quarter = np.log(4.0) - 0.75 * np.log(3.0)
    want = (0.0 + h_quarter + np.log(2.0) + h_quarter + 0.0) / 5.0
    assert M._occupancy_entropy(active, 4) == pytest.approx(want, rel=1e-15)
    assert M._occupancy_entropy(torch.from_numpy(active), 4) == pytest.approx(want, rel=1e-15)
    assert M._occupancy_entropy(active, 4) == pytest.approx(J.bernoulli_entropy_mean(active, 4), rel=1e-14)
    assert M._occupancy_entropy(np.zeros(7), 3) == 0.0 and M._occupancy_entropy(np.full(7, 3), 3) == 0.0
    rng = np.random.default_rng(8)
    active = rng.integers(0, 41, 1000)
    assert M._occupancy_entropy(active, 40) == pytest.approx(J.bernoulli_entropy_mean(active, 40), rel=1e-13)


def test_entropy_of_occupancy_grid_composes_the_histograms(monkeypatch):
    """The (entropy, hits) pair from stubbed histograms: entropy from `active` over the number of clouds, hits as float64."""
    hits, active = torch.tensor([5, 0, 7, 4]), torch.tensor([2, 0, 3, 1])
    seen = []

    def fake(clouds, resolution=28, in_sphere=True):
        seen.append((tuple(clouds.shape), resolution, in_sphere))
        return hits, active

    monkeypatch.setattr(M, "occupancy_grid", fake)
    ent, got = M.entropy_of_occupancy_grid(torch.zeros(3, 16, 3), 4, True)
    assert seen == [((3, 16, 3), 4, True)]
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, [5.0, 0.0, 7.0, 4.0])
    assert ent == pytest.approx(J.bernoulli_entropy_mean([2, 0, 3, 1], 3), rel=1e-14)
    P = torch.tensor([5, 0, 7, 4])
    monkeypatch.setattr(M, "occupancy_grid", lambda c, resolution=28, in_sphere=True: (P + (c.shape[0] == 2) * torch.tensor([0, 9, 0, 0]), P))
    want = J.jsd_ref([5, 0, 7, 4], [5, 9, 7, 4])
    assert M.jsd_between_point_cloud_sets(torch.zeros(3, 16, 3), torch.zeros(2, 16, 3), resolution=4) == pytest.approx(want, abs=1e-12)


def test_occupancy_grid_is_device_only():
    from bdm_amd import _lib
    with pytest.raises(_lib.BdmHipError):
        M.occupancy_grid(torch.zeros(1, 4, 3))
    with pytest.raises(_lib.BdmHipError):
        M.occupancy_grid(np.zeros((1, 4, 3), dtype=np.float32))


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_cli_jsd_arguments():
    args = M.parse_args(["--sample", "s.npy", "--ref", "r.npy"])
    assert args.jsd is False and args.jsd_resolution == 28
    assert args.metrics == ("cd", "emd") and args.normalize is False and args.batch_size is None   # the earlier defaults
    args = M.parse_args(["--sample", "s", "--ref", "r", "--jsd"])
    assert args.jsd is True and args.jsd_resolution == 28 and args.metrics == ("cd", "emd")
    args = M.parse_args(["--sample", "s", "--ref", "r", "--jsd", "--jsd-resolution", "16", "--metrics", "cd"])
    assert args.jsd is True and args.jsd_resolution == 16 and args.metrics == ("cd",)
    with pytest.raises(SystemExit):
        M.parse_args(["--sample", "s", "--ref", "r", "--jsd", "--metrics", "jsd"])   # JSD is a flag, not a value of --metrics
    with pytest.raises(SystemExit):
        M.parse_args(["--sample", "s", "--ref", "r", "--jsd-resolution", "many"])


def test_cli_json_line_with_and_without_jsd(tmp_path, monkeypatch, capsys):
    """main() with the GPU calls stubbed: --jsd adds exactly three keys; without it the line is what it was."""
    rng = np.random.default_rng(9)
    np.save(tmp_path / "s.npy", rng.uniform(-0.3, 0.3, (4, 32, 3)).astype(np.float32))
    np.save(tmp_path / "r.npy", rng.uniform(-0.3, 0.3, (5, 32, 3)).astype(np.float32))
    monkeypatch.setattr(M, "_to_device", torch.from_numpy)
    monkeypatch.setattr(M, "compute_all_metrics", lambda s, r, metrics, batch_size: {"mmd-cd": 0.25})

    def fake_grid(clouds, resolution=28, in_sphere=True):
        assert resolution == 6 and in_sphere is True
        S = clouds.shape[0]
        return torch.tensor([S, 2 * S, 0, 5]), torch.tensor([1, S, 0, 2])

    monkeypatch.setattr(M, "occupancy_grid", fake_grid)
    argv = ["--sample", str(tmp_path / "s.npy"), "--ref", str(tmp_path / "r.npy")]
    plain = M.main(argv)
    with_jsd = M.main(argv + ["--jsd", "--jsd-resolution", "6"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2
    assert set(plain) == {"mmd-cd", "num_sample", "num_ref", "num_points"}
    assert set(with_jsd) - set(plain) == {"jsd", "occupancy_entropy_sample", "occupancy_entropy_ref"}
    assert with_jsd["jsd"] == pytest.approx(J.jsd_ref([4, 8, 0, 5], [5, 10, 0, 5]), abs=1e-12)
    assert with_jsd["occupancy_entropy_sample"] == pytest.approx(J.bernoulli_entropy_mean([1, 4, 0, 2], 4), rel=1e-13)
    assert with_jsd["occupancy_entropy_ref"] == pytest.approx(J.bernoulli_entropy_mean([1, 5, 0, 2], 5), rel=1e-13)
    assert all(isinstance(with_jsd[k], float) for k in ("jsd", "occupancy_entropy_sample", "occupancy_entropy_ref"))
