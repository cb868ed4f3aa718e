"""GPU tests of the occupancy-grid histograms (csrc/occupancy.hip behind bdm_amd/metrics.py) and of the JSD built on them, against
the float64 brute-force restatement tests/jsd_ref.py: exact equality of `hits` and `active` on every path of the kernel (rounded cell
kept; rounded cell masked out and the kept cells searched; both in one workgroup), small / odd / largest grids, the shapes the indexing
can get wrong, order independence, the C ABI's null outputs and error codes, and the measures end to end.

Which points can be compared exactly.  The kernel picks the cell that minimises d = fl(fl(fl(dx)^2 + fl(dy)^2) + fl(dz)^2) in fp32,
dx = fl(x - gx); the restatement minimises the same expression in float64, where it is exact to ~2^-53.  With u = 2^-24 one rounding:
fl(dx) carries 1 u, its square 2 u + 1 u, and each of the two additions of non-negative terms adds 1 u, so |d32 - d| <= 5 u d to first
order; 6 u d covers the second-order terms.  If the kernel prefers a cell c' to the true nearest c then d32(c') <= d32(c), so
d(c') (1 - 6 u) <= d(c) (1 + 6 u), i.e. d(c') - d(c) <= 6 u (d(c') + d(c)) <= 12 u d(c').  Every cell other than c is at least the
second-best distance away, so a point whose margin (second best - best) exceeds 12 u x second best cannot be assigned differently; the
tests use 13 u x second best = 7.7e-7 relative (at the squared distances of these inputs, <= 1.1, an absolute 8.5e-7) and DROP the
points below it (replacing each by the first comparable point of its cloud, in the kernel's input and the restatement's alike);
a case fails if that drops more than 1 % of its points.  The fast path is covered by the same argument: the rounded-and-refined cell
minimises d32 over the whole grid, because fp32 rounding is monotone in each of dx^2, dy^2, dz^2."""
import ctypes
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import jsd_ref as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MARGIN_FACTOR = 13 * U
MAX_DROPPED = 0.01


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def fast_points(S, N, r, seed, jitter=0.3):
    """Kept cell centres plus at most `jitter` spacings per axis: the rounded cell is the point's own, kept, cell."""
    rng = rng_of(seed)
    cells, _ = J.kept_cells(r)
    pick = rng.integers(0, len(cells), (S, N))
    return (cells[pick] + rng.uniform(-jitter, jitter, (S, N, 3)) / (r - 1)).astype(np.float32)


def slow_points(S, N, seed):
    """Three equal groups whose rounded cell is (mostly) masked out: inside the cube but outside the sphere (the corners), outside
    the cube (up to +-0.8 per axis), and on a shell of radius 0.5 +- 0.02."""
    rng = rng_of(seed)
    n = S * N
    corners = np.empty((0, 3))
    while len(corners) < n:
        c = rng.uniform(-0.5, 0.5, (4 * n, 3))
        corners = np.concatenate([corners, c[np.linalg.norm(c, axis=1) > 0.5]])
    outside = np.empty((0, 3))
    while len(outside) < n:
        c = rng.uniform(-0.8, 0.8, (4 * n, 3))
        outside = np.concatenate([outside, c[np.abs(c).max(axis=1) > 0.5]])
    direction = rng.normal(size=(n, 3))
    shell = direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(0.48, 0.52, (n, 1))
    group = rng.integers(0, 3, n)
    pts = np.where(group[:, None] == 0, corners[:n], np.where(group[:, None] == 1, outside[:n], shell))
    return pts.reshape(S, N, 3).astype(np.float32)


def mixed_points(S, N, r, seed):
    """Fast and slow points shuffled together inside every cloud."""
    pts = np.concatenate([fast_points(S, N - N // 2, r, seed), slow_points(S, N // 2, seed + 1)], axis=1) if N > 1 else slow_points(S, 1, seed)
    rng = rng_of(seed + 2)
    return np.stack([c[rng.permutation(N)] for c in pts])


def rounded_cell_is_kept(clouds, r, in_sphere=True):
    """Per point: does the cell it rounds to (clamped to the grid) belong to the kept ones -- the kernel's fast path."""
    idx = np.clip(np.rint((clouds.astype(np.float64) + 0.5) * (r - 1)), 0, r - 1).astype(np.int64)
    flat = (idx[..., 0] * r + idx[..., 1]) * r + idx[..., 2]
    return np.isin(flat, J.kept_cells(r, in_sphere)[1])


def comparable(clouds, r, in_sphere=True):
    """The clouds with every point below the margin bound replaced by the first comparable point of its cloud, the restatement's
    counts on them, and the dropped share (asserted <= 1 %)."""
    _, _, best, margin = J.occupancy_ref(clouds, r, in_sphere)
    ok = margin > MARGIN_FACTOR * (best + margin)
    dropped = 1.0 - ok.mean()
    print(f"r={r} shape {clouds.shape[:2]}: {int((~ok).sum())} of {ok.size} points below the margin bound ({dropped:.2%})")
    assert dropped <= MAX_DROPPED, f"{dropped:.2%} of the points are too close to a tie to compare"
    if ok.all():
        hits, active = J.occupancy_ref(clouds, r, in_sphere)[:2]
        return clouds, hits, active
    clouds = clouds.copy()
    for s in range(len(clouds)):
        assert ok[s].any()
        clouds[s][~ok[s]] = clouds[s][ok[s].argmax()]
    hits, active = J.occupancy_ref(clouds, r, in_sphere)[:2]
    return clouds, hits, active


def check_exact(clouds, r, in_sphere=True):
    from bdm_amd import metrics as M
    clouds, want_hits, want_active = comparable(clouds, r, in_sphere)
    S, N = clouds.shape[:2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "not in unit cube / sphere": these inputs are outside on purpose
        hits, active = M.occupancy_grid(dev(clouds), r, in_sphere)
    assert hits.dtype == torch.int64 and active.dtype == torch.int64 and hits.shape == active.shape == (len(want_hits),)
    hits, active = hits.cpu(), active.cpu()
    if len(want_hits):   # conservation: every point lands in exactly one kept cell; a cloud counts at most once per cell
        assert int(hits.sum()) == S * N and int(active.max()) <= S and int(active.sum()) <= S * N
        assert bool(((hits > 0) == (active > 0)).all())
    assert torch.equal(hits, torch.from_numpy(want_hits)), f"hits differ in {int((hits != torch.from_numpy(want_hits)).sum())} cells"
    assert torch.equal(active, torch.from_numpy(want_active)), f"active differs in {int((active != torch.from_numpy(want_active)).sum())} cells"
    return hits, active


# ---- 1 - 3: the two paths ----------------------------------------------------------------------------------------------------
def test_fast_path_exact(hip):
    clouds = fast_points(3, 257, 28, 11)
    assert rounded_cell_is_kept(clouds, 28).all()
    _, _, best, margin = J.occupancy_ref(clouds, 28)
    assert (margin > MARGIN_FACTOR * (best + margin)).all()   # nothing to drop: a jitter of 0.3 spacings is far from any tie
    check_exact(clouds, 28)


def test_slow_path_exact(hip):
    clouds = slow_points(2, 300, 21)
    slow = ~rounded_cell_is_kept(clouds, 28)
    assert slow.mean() > 0.8   # the shell's inner half may round to a kept cell
    assert float(np.abs(clouds).max()) > 0.75 and float(np.linalg.norm(clouds, axis=2).min()) < 0.49
    check_exact(clouds, 28)


def test_mixed_cloud_exact(hip):
    clouds = mixed_points(2, 600, 28, 31)
    slow = ~rounded_cell_is_kept(clouds, 28)
    assert 0.3 < slow[0].mean() < 0.7 and slow[0][:64].any() and (~slow[0][:64]).any()   # both paths inside the first wave
    check_exact(clouds, 28)


# ---- 4: small, odd and the largest grids ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,in_sphere", [(4, True), (5, True), (2, False), (3, True), (32, True), (28, False)])
def test_small_odd_and_largest_grids(hip, r, in_sphere):
    rng = rng_of(40 + r)
    clouds = rng.uniform(-0.7, 0.7, (2, 64, 3)).astype(np.float32)
    if r == 5:   # the six cells ON the sphere, (+-0.5, 0, 0) and so on, are kept by the host's mask and must collect their points
        on_sphere = np.concatenate([np.eye(3), -np.eye(3)]) * 0.5
        clouds[0, :6] = (on_sphere + rng.uniform(-0.02, 0.02, (6, 3))).astype(np.float32)
    hits, _ = check_exact(clouds, r, in_sphere)
    if r == 5:
        cells = J.kept_cells(5)[0]
        for c in on_sphere:
            assert int(hits[np.flatnonzero((cells == c).all(axis=1))[0]]) >= 1


def test_grid_without_a_kept_cell(hip):
    """r = 2 clipped to the sphere keeps none of its eight corner cells: nothing to count, nothing written."""
    from bdm_amd import metrics as M
    assert len(J.kept_cells(2)[0]) == 0
    clouds = dev(rng_of(5).uniform(-0.4, 0.4, (2, 64, 3)).astype(np.float32))
    hits, active = M.occupancy_grid(clouds, 2, True)
    assert hits.shape == active.shape == (0,)
    axis, mask, _ = M._device_grid(2, True, clouds.device)
    out = torch.full((2, 8), -1, dtype=torch.int32, device="cuda")
    from bdm_amd import _lib as L
    L.check(L.lib().bdm_occupancy_grid(2, 64, 2, L.ptr(clouds), L.ptr(axis), L.ptr(mask), L.ptr(out[0]), L.ptr(out[1]), L.stream()), "r=2")
    assert int(out.abs().sum()) == 0


# ---- 5: shapes the indexing can get wrong --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N", [(3, 1), (2, 255), (2, 256), (2, 257), (1, 300), (17, 3), (1, 1024), (2, 1025), (2051, 2)],
                         ids=lambda v: str(v))
def test_shapes(hip, S, N):
    """One point per cloud; around a wave multiple; one cloud; more clouds than points; a full chunk of 1024 points and one point
    into the next chunk; more clouds than the 2048 workgroups of the launch."""
    check_exact(mixed_points(S, N, 28, 100 + S + N), 28)


# ---- 6 - 8: counts -------------------------------------------------------------------------------------------------------------
def test_active_counts_clouds_and_hits_counts_points(hip):
    from bdm_amd import metrics as M
    N = 77
    cells = J.kept_cells(28)[0]
    c = 4321
    point = (cells[c] + np.array([0.1, -0.2, 0.05]) / 27).astype(np.float32)
    one = np.broadcast_to(point, (1, N, 3)).copy()
    hits, active = M.occupancy_grid(dev(one))
    assert int(hits[c]) == N and int(active[c]) == 1 and int(hits.sum()) == N and int(active.sum()) == 1
    hits, active = M.occupancy_grid(dev(np.concatenate([one, one])))
    assert int(hits[c]) == 2 * N and int(active[c]) == 2 and int(hits.sum()) == 2 * N and int(active.sum()) == 2
    outside = np.broadcast_to(np.array([0.7, 0.1, -0.2], dtype=np.float32), (1, N, 3)).copy()   # the same through the slow path
    want = J.nearest_kept_cell(outside[0, :1], 28)[0][0]
    with pytest.warns(UserWarning, match="not in unit cube"):
        hits, active = M.occupancy_grid(dev(np.concatenate([outside, one, outside])))
    assert int(hits[want]) == 2 * N and int(active[want]) == 2 and int(hits[c]) == N and int(active[c]) == 1


def test_order_independence_and_splits(hip):
    from bdm_amd import metrics as M
    clouds = dev(mixed_points(6, 300, 28, 51))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = M.occupancy_grid(clouds)
        again = M.occupancy_grid(clouds)
        assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1]), "two identical calls differ"
        assert int(whole[0].sum()) == 6 * 300 and int(whole[1].max()) <= 6
        for cut in (1, 3):
            a, b = M.occupancy_grid(clouds[:cut]), M.occupancy_grid(clouds[cut:])
            assert torch.equal(a[0] + b[0], whole[0]) and torch.equal(a[1] + b[1], whole[1]), f"split at {cut} changes the counts"
        parts = [M.occupancy_grid(clouds[i:i + 1]) for i in range(6)]
    assert torch.equal(sum(p[0] for p in parts), whole[0]) and torch.equal(sum(p[1] for p in parts), whole[1])


def test_warnings_of_the_reference(hip):
    from bdm_amd import metrics as M
    inside = dev(fast_points(2, 50, 28, 61) * np.float32(0.9))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.occupancy_grid(inside)
    corner = inside.clone()
    corner[0, 0] = torch.tensor([0.45, 0.45, 0.45])   # inside the cube, outside the sphere
    with pytest.warns(UserWarning, match="not in unit sphere") as rec:
        M.occupancy_grid(corner)
    assert not any("unit cube" in str(w.message) for w in rec)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.occupancy_grid(corner, in_sphere=False)   # the sphere is not asked for
    corner[0, 0, 0] = 0.5 + 2e-3                       # past the reference's bound 0.5 + 10e-4
    with pytest.warns(UserWarning, match="not in unit cube"):
        M.occupancy_grid(corner, in_sphere=False)


# ---- 9: the C ABI ------------------------------------------------------------------------------------------------------------
def test_null_outputs_and_error_codes(hip):
    from bdm_amd import _lib as L, metrics as M
    r, r3 = 28, 28 ** 3
    clouds = dev(mixed_points(3, 130, r, 71))
    axis, mask, kept = M._device_grid(r, True, clouds.device)
    fn = L.lib().bdm_occupancy_grid
    both = torch.full((2, r3), -1, dtype=torch.int32, device="cuda")
    L.check(fn(3, 130, r, L.ptr(clouds), L.ptr(axis), L.ptr(mask), L.ptr(both[0]), L.ptr(both[1]), L.stream()), "both")
    assert int(both[0].sum()) == 3 * 130 and int(both[0][mask == 0].abs().sum()) == 0 and int(both[1][mask == 0].abs().sum()) == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hits, active = M.occupancy_grid(clouds)
    assert torch.equal(both[0][kept].long(), hits) and torch.equal(both[1][kept].long(), active)
    only = torch.full((r3,), -1, dtype=torch.int32, device="cuda")
    L.check(fn(3, 130, r, L.ptr(clouds), L.ptr(axis), L.ptr(mask), L.ptr(only), None, L.stream()), "hits only")
    assert torch.equal(only, both[0])
    only.fill_(-1)
    L.check(fn(3, 130, r, L.ptr(clouds), L.ptr(axis), L.ptr(mask), None, L.ptr(only), L.stream()), "active only")
    assert torch.equal(only, both[1])
    assert fn(3, 130, r, L.ptr(clouds), L.ptr(axis), L.ptr(mask), None, None, L.stream()) == 0
    scratch = torch.full((2, r3), -1, dtype=torch.int32, device="cuda")
    assert fn(0, 130, r, None, L.ptr(axis), L.ptr(mask), L.ptr(scratch[0]), L.ptr(scratch[1]), L.stream()) == 0   # s = 0: zeroed
    assert int(scratch.abs().sum()) == 0
    scratch.fill_(-1)
    for bad in ((3, 130, 1), (3, 130, 33), (3, 0, r), (-1, 130, r), (1 << 20, 1 << 11, r)):   # r < 2, r^3 beyond LDS, n < 1, s < 0, s n = 2^31
        assert fn(*bad, L.ptr(clouds), L.ptr(axis), L.ptr(mask), L.ptr(scratch[0]), L.ptr(scratch[1]), L.stream()) == 1, bad
        assert b"occupancy_grid" in L.lib().bdm_last_error()
    torch.cuda.synchronize()
    assert bool((scratch == -1).all())   # refused calls launch nothing and write nothing
    with pytest.raises(L.BdmHipError):
        M.occupancy_grid(clouds.cpu())
    with pytest.raises(L.BdmHipError, match="code 1"):
        M.occupancy_grid(clouds, resolution=33)
    with pytest.raises(ValueError):
        M.occupancy_grid(clouds, resolution=1)
    with pytest.raises(L.BdmHipError, match="float32"):
        M.occupancy_grid(clouds.double())
    assert M.occupancy_grid(clouds[:0])[0].shape == hits.shape and int(M.occupancy_grid(clouds[:0])[0].sum()) == 0


def test_exported_prototype_comes_from_the_header(hip):
    from bdm_amd import _lib as L
    restype, argtypes = L.abi_signatures()["bdm_occupancy_grid"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    assert L.lib().bdm_abi_version() == 4   # an added symbol, no signature change


# ---- 10: end to end ----------------------------------------------------------------------------------------------------------
def shape_sets():
    """Two sets of 8 clouds of 128 points inside radius 0.5: anisotropic Gaussian blobs, each cloud scaled to radius 0.5 (its farthest
    point lies ON the sphere, so some points take the slow path)."""
    sets = []
    for seed, scale in ((81, (0.30, 0.20, 0.10)), (82, (0.15, 0.25, 0.25))):
        pts = rng_of(seed).normal(size=(8, 128, 3)) * np.array(scale)
        pts /= 2.0 * np.linalg.norm(pts, axis=2).max(axis=1)[:, None, None]
        sets.append(pts.astype(np.float32))
    return sets


def test_jsd_between_sets_end_to_end(hip):
    from bdm_amd import metrics as M
    sample, ref = shape_sets()
    want = []
    for clouds in (sample, ref):
        hits, active, best, margin = J.occupancy_ref(clouds, 28)
        assert (margin > MARGIN_FACTOR * (best + margin)).all(), "a point of the fixture is too close to a tie: choose another seed"
        want.append((hits, active))
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # inside cube and sphere, and the two JSD formulas agree
        got = M.jsd_between_point_cloud_sets(dev(sample), dev(ref), resolution=28)
        same = M.jsd_between_point_cloud_sets(dev(sample), dev(sample))
        ent, hits = M.entropy_of_occupancy_grid(dev(sample), 28, True)
        from_host_array = M.jsd_between_point_cloud_sets(sample, ref)
    ref_jsd = J.jsd_ref(want[0][0], want[1][0])
    print(f"jsd {got:.6f}, restatement {ref_jsd:.6f}")
    assert 0.05 < ref_jsd < 1.0
    assert abs(got - ref_jsd) <= 1e-12 and from_host_array == got
    assert same == 0.0
    assert np.array_equal(hits, want[0][0].astype(np.float64))
    assert ent == pytest.approx(J.bernoulli_entropy_mean(want[0][1], 8), rel=1e-12)


def test_cli_with_jsd_on_npy_files(hip, tmp_path):
    sample, ref = shape_sets()
    np.save(tmp_path / "s.npy", sample[:6])
    np.save(tmp_path / "r.npy", ref[:5])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "bdm_amd.metrics", "--sample", str(tmp_path / "s.npy"), "--ref", str(tmp_path / "r.npy"),
                          "--metrics", "cd", "--jsd"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    want = J.jsd_ref(J.occupancy_ref(sample[:6], 28)[0], J.occupancy_ref(ref[:5], 28)[0])
    assert abs(out["jsd"] - want) <= 1e-12
    assert out["occupancy_entropy_sample"] == pytest.approx(J.bernoulli_entropy_mean(J.occupancy_ref(sample[:6], 28)[1], 6), rel=1e-12)
    assert out["occupancy_entropy_ref"] == pytest.approx(J.bernoulli_entropy_mean(J.occupancy_ref(ref[:5], 28)[1], 5), rel=1e-12)
    assert 0.0 < out["mmd-cd"] < 1.0 and 0.0 < out["cov-cd"] <= 1.0 and 0.0 <= out["1nna-cd"] <= 1.0   # the existing keys, unchanged
    assert out["num_sample"] == 6 and out["num_ref"] == 5 and out["num_points"] == 128 and "mmd-emd" not in out
