"""GPU tests of the any-size approximate-match EMD (csrc/metrics_emd_large.hip behind bdm_amd.metrics.pairwise_emd_large and
paired_emd): both forms of the kernel against the float64 restatement (live up to n = 2049, goldens above), the two forms bit for
bit against each other, the independence of every entry from the rest of the call, the error paths, and the callers that are
routed to it (compute_all_metrics above 2048 points, the command line's --num-points, evaluation.evaluate_dirs(emd=True))."""
import ctypes
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import helpers
import metrics_large_ref as LR
import metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tolerance cannot be derived, so it is measured on the CPU (tools/metrics_emd_large_gap.py): EMD_G_LARGE is the largest relative
# gap between the float32 and the float64 row-blocked restatement over metrics_large_ref.large_case_pairs() (every pair of LARGE_CASES,
# n = 1 to 8192, in natural and reversed point order).  The GPU bound is 32 g_large, the factor of test_hip_metrics.EMD_BOUND for the
# same reason: in-lane sequential sums and the hardware exponential deviate from numpy's pairwise sums and libm by more than a
# reorder does.  tests/test_metrics_emd_large_host.py re-measures the gap on the cases with n <= 2049.
EMD_G_LARGE = LR.EMD_G_LARGE       # 1.339e-6, the worst is n256[0,1]; above 2049 points the largest is 3.37e-7 (n4097[0,0]rev)
EMD_LARGE_BOUND = 32 * EMD_G_LARGE  # 4.285e-5
EMD_LARGE_WORST_OBSERVED = 4.41e-7  # MI355X, the committed kernel, both forms alike: worst of the case list (n = 2049; 1.0 % of the bound);
# n = 1: 1.7e-7, 2: 8.4e-8, 63: 1.1e-7, 256: 2.1e-7, 1000: 7.9e-8, 1023: 3.6e-7, 1024: 7.2e-8, 1025: 6.0e-8, 2047: 1.4e-7, 2600: 1.2e-7,
# 4096: 9.2e-8, 4097: 9.1e-8, 8192: 3.6e-7.  One 16384-point pair takes 0.44 s (one workgroup on one CU).

RESIDENT, STREAMED = (1, LR.THREADS, LR.KPT, 0), (0, LR.THREADS, LR.KPT, LR.STAGE)   # (resident, threads, kpt, stage) of the two instantiations
FORM_OF_MODE = {1: RESIDENT, 2: STREAMED}
LIVE_NS = [c[0] for c in LR.LARGE_CASES if c[4] == "live"]
#                n      what mode 0 launches
GOLDEN_CASES = [(2600, RESIDENT), (4096, RESIDENT), (4097, STREAMED), (8192, STREAMED)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def variant(n, mode):
    """(return code, (resident, threads, kpt, stage)) of bdm_pairwise_emd_large_variant."""
    from bdm_amd import _lib as L
    v = [ctypes.c_int(-1) for _ in range(4)]
    rc = L.lib().bdm_pairwise_emd_large_variant(n, mode, *[ctypes.addressof(x) for x in v])
    return rc, tuple(x.value for x in v)


@functools.lru_cache(maxsize=None)
def live_reference(n):
    """float64 restatement (and, up to 1024 points, the exact EMD) of every pair of the live case with n points; computed once."""
    a, b = LR.large_case(n)
    ref = np.array([[R.emd_approx_ref(p, q) for q in b] for p in a])
    exact = np.array([[R.emd_exact(p, q) for q in b] for p in a]) if n <= 1024 else None
    return ref, exact


def check_against(got, ref, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    err = float((np.abs(got - ref) / ref).max())
    helpers.parity(f"{helpers.current_test()} {what}", err, EMD_LARGE_BOUND)
    print(f"emd_large {what}: worst relative error {err:.3e}, bound {EMD_LARGE_BOUND:.3e}")
    assert err <= EMD_LARGE_BOUND, f"{what}: {err:.3e} > {EMD_LARGE_BOUND:.3e}"


# ---- against float64 ---------------------------------------------------------------------------------------------------------
def test_boundary_cases_are_the_ones_the_library_reports(hip):
    rc, form = variant(5000, 2)
    assert rc == 0 and form == STREAMED, "metrics_large_ref.STAGE / THREADS / KPT no longer describe the streamed instantiation"
    _, threads, kpt, stage = form
    want = {stage - 1, stage, stage + 1, threads * kpt - 1, threads * kpt + 1, 2049}
    assert want <= set(LIVE_NS) and {1, 2, 63, 256, 1000} <= set(LIVE_NS)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", LIVE_NS)
def test_emd_large_vs_float64_restatement(hip, n, mode):
    from bdm_amd import metrics as M
    assert variant(n, mode) == (0, FORM_OF_MODE[mode]), "the case table no longer names the instance that runs"
    a, b = LR.large_case(n)
    got = M.pairwise_emd_large(dev(a), dev(b), mode=mode)
    ref, exact = live_reference(n)
    check_against(got, ref, f"n={n} mode={mode}")
    if exact is not None:   # a transport plan costs at least the optimal one
        assert (got.double().cpu().numpy() >= exact * (1.0 - EMD_LARGE_BOUND)).all(), f"n={n}: below the exact EMD"


@pytest.mark.parametrize("n,form", GOLDEN_CASES)
def test_emd_large_vs_golden(hip, n, form):
    from bdm_amd import metrics as M
    assert variant(n, 0) == (0, form), "the case table no longer names the instance that mode 0 runs"
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics_emd_large.npz"))
    case, = [c for c in LR.LARGE_CASES if c[0] == n]
    assert case[4] == "golden" and list(case[:4]) in g["cases"].tolist(), "fixture and LARGE_CASES disagree: run tools/gen_golden_metrics_emd_large.py"
    a, b = LR.large_case(n)
    check_against(M.pairwise_emd_large(dev(a), dev(b)), g[f"emd_n{n}"], f"n={n} golden")


def test_case_table_covers_both_forms_and_every_instantiation(hip):
    reported = set()
    for n in [1, 2, 3, 4, 5, 63, 64, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 16384, 65536]:
        for mode in (0, 1, 2):
            rc, form = variant(n, mode)
            if mode == 1 and n > 4096:
                assert (rc, form) == (3, (0, 0, 0, 0))
            else:
                assert rc == 0
                reported.add(form)
    assert reported == {RESIDENT, STREAMED}
    tested = {FORM_OF_MODE[m] for m in (1, 2)} | {form for _, form in GOLDEN_CASES}
    assert tested == reported
    assert variant(0, 0)[0] == 1 and variant(5, 3)[0] == 1 and variant(65537, 0) == (3, (0, 0, 0, 0))
    from bdm_amd import _lib as L
    assert L.lib().bdm_pairwise_emd_large_variant(100, 0, None, None, None, None) == 0


# ---- one algorithm, two forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1000, 2049, 4096])
def test_resident_and_streamed_give_the_same_bits(hip, n):
    from bdm_amd import metrics as M
    s, r = (2, 2) if n <= 1000 else (1, 1)
    a, b = dev(R.gaussian(s, n, 81)), dev(R.uniform(r, n, 82))
    res, stre = M.pairwise_emd_large(a, b, mode=1), M.pairwise_emd_large(a, b, mode=2)
    assert torch.equal(res, stre), f"n={n}: resident {res.tolist()} != streamed {stre.tolist()}"
    assert torch.equal(M.paired_emd(a[:1], b[:1], mode=1), M.paired_emd(a[:1], b[:1], mode=2))
    assert bool((res > 0).all()) and bool(torch.isfinite(res).all())


# ---- independence and reproducibility ----------------------------------------------------------------------------------------
def test_entry_equals_the_one_by_one_call_and_paired_is_the_diagonal(hip):
    from bdm_amd import metrics as M
    s, r, n = 3, 4, 2100
    a, b = dev(R.gaussian(s, n, 61)), dev(R.uniform(r, n, 62))
    full = M.pairwise_emd_large(a, b)
    assert torch.equal(full, M.pairwise_emd_large(a, b)), "two runs differ"
    for i in range(s):
        for j in range(r):
            assert torch.equal(full[i:i + 1, j:j + 1], M.pairwise_emd_large(a[i:i + 1], b[j:j + 1])), f"entry ({i}, {j}) depends on the rest of the call"
    paired = M.paired_emd(a, b[:s])
    assert paired.shape == (s,) and torch.equal(paired, torch.diagonal(full[:, :s]))
    assert torch.equal(paired, M.paired_emd(a, b[:s])), "two paired runs differ"
    assert torch.equal(M.paired_emd(a, b[:s], mode=2), paired)
    for bs in (1, 3):
        assert torch.equal(full, M.pairwise_emd_large(a, b, batch_size=bs)), f"batch_size={bs} changes the result"


def test_more_pairs_than_slabs(hip):
    """400 pairs on a persistent grid of at most 256 workgroups: every workgroup's slab is reused for a second pair."""
    from bdm_amd import _lib as L, metrics as M
    s = r = 20
    n = 64
    assert L.lib().bdm_pairwise_emd_large_workspace_bytes(s * r, n) < s * r * L.lib().bdm_pairwise_emd_large_workspace_bytes(1, n)
    a, b = dev(R.gaussian(s, n, 63)), dev(R.uniform(r, n, 64))
    for mode in (1, 2):
        full = M.pairwise_emd_large(a, b, mode=mode)
        assert torch.equal(full, M.pairwise_emd_large(a, b, mode=mode)), "two runs differ"
        for i, j in [(0, 0), (0, 19), (12, 15), (12, 16), (13, 0), (19, 19), (7, 3), (18, 11)]:   # 12 * 20 + 16 = 256: the first reused slab
            assert torch.equal(full[i:i + 1, j:j + 1], M.pairwise_emd_large(a[i:i + 1], b[j:j + 1], mode=mode)), f"entry ({i}, {j}), mode {mode}"
    assert torch.equal(M.paired_emd(a, b), torch.diagonal(full))


def test_emd_large_is_not_symmetrised_and_self_distance_is_small(hip):
    from bdm_amd import metrics as M
    n = 2100
    a, b = R.gaussian(2, n, 91), R.uniform(2, n, 92)
    ab, ba = M.pairwise_emd_large(dev(a), dev(b)), M.pairwise_emd_large(dev(b), dev(a))
    ref_ab, ref_ba = R.emd_approx_ref(a[0], b[1]), R.emd_approx_ref(b[1], a[0])
    assert abs(ref_ab - ref_ba) > 100 * EMD_LARGE_BOUND * ref_ab   # the restatement itself is asymmetric on this pair ...
    assert abs(float(ab[0, 1]) - ref_ab) <= EMD_LARGE_BOUND * ref_ab and abs(float(ba[1, 0]) - ref_ba) <= EMD_LARGE_BOUND * ref_ba   # ... and so is the kernel
    self_cost = M.pairwise_emd_large(dev(a), dev(a))
    assert float(torch.diagonal(self_cost).max()) < 1e-4 * float(self_cost[0, 1])


def test_sixteen_thousand_points(hip):
    from bdm_amd import metrics as M
    n = 16384
    assert variant(n, 0) == (0, STREAMED)
    a, b = dev(R.gaussian(1, n, 95)), dev(R.uniform(1, n, 96))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = float(M.paired_emd(a, b))
    print(f"emd_large n={n}: one pair in {time.perf_counter() - t0:.3f} s (one workgroup), value {got:.7f}")
    assert np.isfinite(got) and got > 0.0
    rev = float(M.paired_emd(a.flip(1).contiguous(), b.flip(1).contiguous()))
    moved = abs(rev - got) / got
    helpers.parity(f"{helpers.current_test()} reversed order", moved, EMD_LARGE_BOUND)
    assert moved <= EMD_LARGE_BOUND, f"reversing the point order moves the result by {moved:.3e} > {EMD_LARGE_BOUND:.3e}"


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(hip):
    from bdm_amd import _lib as L, metrics as M
    lib = L.lib()
    n = 100
    a, b = dev(R.gaussian(3, n, 1)), dev(R.uniform(3, n, 2))
    big = dev(R.gaussian(1, 4097, 3))
    out = torch.full((3, 3), -1.0, device="cuda")
    need = lib.bdm_pairwise_emd_large_workspace_bytes(9, n)
    assert need == 9 * 20 * n and lib.bdm_pairwise_emd_large_workspace_bytes(1000, n) == 256 * 20 * n
    assert lib.bdm_pairwise_emd_large_workspace_bytes(9, 101) == 9 * 20 * 104   # padded to a multiple of 4 points
    assert [lib.bdm_pairwise_emd_large_workspace_bytes(p, m) for p, m in ((0, n), (-1, n), (9, 0), (9, 65537))] == [0, 0, 0, 0]
    ws = torch.empty(max(need, lib.bdm_pairwise_emd_large_workspace_bytes(1, 4097)), dtype=torch.uint8, device="cuda")

    def call(s, r, n, paired, mode, pa, pb, wbytes, pw=L.ptr(ws)):
        return lib.bdm_pairwise_emd_large(s, r, n, paired, mode, pa, pb, pw, wbytes, L.ptr(out), L.stream())

    assert call(3, 3, 0, 0, 0, L.ptr(a), L.ptr(b), need) == 1                     # n = 0
    assert call(3, 2, n, 1, 0, L.ptr(a), L.ptr(b), need) == 1                     # paired with s != r
    assert call(3, 3, n, 0, 0, L.ptr(a), L.ptr(b), need - 1) == 1                 # workspace one byte short
    assert b"workspace" in lib.bdm_last_error()
    assert call(3, 3, n, 0, 0, None, L.ptr(b), need) == 1 and call(3, 3, n, 0, 0, L.ptr(a), None, need) == 1   # NULL clouds
    assert call(3, 3, n, 0, 0, L.ptr(a), L.ptr(b), need, None) == 1               # NULL workspace
    assert call(3, 3, n, 0, 3, L.ptr(a), L.ptr(b), need) == 1                     # unknown mode
    assert call(1, 1, 4097, 0, 1, L.ptr(big), L.ptr(big), ws.numel()) == 3        # mode 1 at an n that does not fit
    assert b"4097" in lib.bdm_last_error()
    assert call(1, 1, 65537, 0, 0, L.ptr(a), L.ptr(b), ws.numel()) == 3           # n above the limit (nothing is read)
    assert b"65537" in lib.bdm_last_error()
    assert call(0, 3, n, 0, 0, None, L.ptr(b), 0, None) == 0 and call(3, 0, n, 0, 0, L.ptr(a), None, 0, None) == 0   # no-ops
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((3, 3), -1.0, device="cuda")), "an error path wrote to out"
    assert call(3, 3, n, 0, 0, L.ptr(a), L.ptr(b), need) == 0                     # the same arguments with nothing wrong
    assert torch.equal(out, M.pairwise_emd_large(a, b))
    with pytest.raises(L.BdmHipError, match="code 3"):
        M.pairwise_emd_large(big, big, mode=1)
    with pytest.raises(ValueError):
        M.paired_emd(a, b[:2])
    with pytest.raises(ValueError):
        M.pairwise_emd_large(a, dev(R.uniform(2, n + 1, 5)))
    assert M.pairwise_emd_large(a[:0], b).shape == (0, 3) and M.paired_emd(a[:0], b[:0]).shape == (0,)


# ---- routing -----------------------------------------------------------------------------------------------------------------
def test_compute_all_metrics_routes_large_clouds(hip):
    from bdm_amd import metrics as M
    n = 2100
    x, y = dev(R.shape_clouds(3, n, 11)), dev(R.shape_clouds(4, n, 12))
    got = M.compute_all_metrics(x, y, metrics=("emd",), batch_size=3)
    want = M.metrics_from_matrices(M.pairwise_emd_large(x, y).cpu(), M.pairwise_emd_large(x, x).cpu(), M.pairwise_emd_large(y, y).cpu(), "emd")
    assert len(got) == 6 and got == want
    with pytest.raises(M.L.BdmHipError, match="code 3"):
        M.pairwise_emd(x, y)   # the route it did not take


def test_cli_num_points_subsamples_first(hip, tmp_path):
    from bdm_amd import metrics as M
    sample, ref = R.shape_clouds(3, 4096, 21), R.shape_clouds(2, 4096, 22)
    np.save(tmp_path / "s.npy", sample)
    np.save(tmp_path / "r.npy", ref)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "bdm_amd.metrics", "--sample", str(tmp_path / "s.npy"), "--ref", str(tmp_path / "r.npy"),
                          "--num-points", "2048"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["num_points"] == 2048 and out["num_sample"] == 3 and out["num_ref"] == 2
    sub_s, sub_r = M.subsample_fps(dev(sample), 2048), M.subsample_fps(dev(ref), 2048)
    assert sub_s.shape == (3, 2048, 3) and torch.equal(sub_s[:, 0], dev(sample)[:, 0])   # furthest-point sampling starts at point 0
    want = M.compute_all_metrics(sub_s, sub_r)
    assert {k: out[k] for k in want} == want
    with pytest.raises(ValueError, match="4097"):
        M.subsample_fps(dev(sample), 4097)


def test_evaluate_dirs_with_emd(hip, tmp_path):
    from bdm_amd import metrics as M
    from bdm_amd.evaluation import evaluate_dirs
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply
    g = torch.Generator().manual_seed(3)
    gt = torch.randn(2, 700, 3, generator=g) * 0.2
    pred = gt[:, torch.randperm(700, generator=g)] + 0.02 * torch.randn(2, 700, 3, generator=g)
    for i in range(2):
        save_pointcloud_ply(pred[i].numpy(), tmp_path / "pred" / "chair" / f"s{i}.ply")
        save_pointcloud_ply(gt[i].numpy(), tmp_path / "gt" / "chair" / f"s{i}.ply")
    save_pointcloud_ply(pred[0, :600].numpy(), tmp_path / "pred" / "chair" / "s2.ply")   # unequal counts: CD and F1 only
    save_pointcloud_ply(gt[0].numpy(), tmp_path / "gt" / "chair" / "s2.ply")
    old = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"))
    assert sorted(old) == ["cd_x1000", "f1_at_0.01", "num"] and old["num"] == 3
    new = evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), emd=True)
    assert {k: new[k] for k in old} == old and sorted(new) == ["cd_x1000", "emd", "emd_num", "f1_at_0.01", "num"]
    loaded = [[torch.from_numpy(load_pointcloud_ply(str(tmp_path / d / "chair" / f"s{i}.ply")))[None].cuda() for i in range(2)] for d in ("pred", "gt")]
    centred = [[c - c.mean(1, keepdim=True) for c in side] for side in loaded]
    want = float(np.mean([float(M.paired_emd(p, q)[0]) for p, q in zip(*centred)]))
    assert new["emd_num"] == 2 and new["emd"] == want and 0.0 < want < 0.1
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "bdm_amd.evaluation", "--pred_dir", str(tmp_path / "pred"), "--gt_dir", str(tmp_path / "gt"), "--emd"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert json.loads(run.stdout.strip().splitlines()[-1]) == new
