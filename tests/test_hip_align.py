"""bdm_similarity_apply, bdm_align_moments, bdm_corresponding_points_alignment and bdm_icp_* (csrc/align.hip) and their Python surface
on the GPU against the CPU restatement tests/align_ref.py: the integer moments, the partners, and every iteration's transform and mean
squared residual with torch.equal, floats compared as bits; independence of batch slot, repetition and chunking; the error paths; the
evaluator's --icp mode end to end.

Every operation of the rule is rounded on its own, so nothing here has a tolerance except the comparison with the float64 SVD
definition, whose bound is the host test's (tests/test_align_host.py, measured by tools/align_gap.py)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref as A
from bdm_amd import alignment as AL   # the feature itself: without it this file fails at import

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), F_SENTINEL if dtype == torch.float32 else I_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = F_SENTINEL if whole.dtype == torch.float32 else I_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _pack(rows_list):
    """Packed device rows; an empty side still gets one (unread) row: no NULL among the inputs."""
    n = sum(t.shape[0] for t in rows_list)
    return torch.cat(rows_list).float().cuda().contiguous() if n else torch.zeros(1, 3, device="cuda")


def _first(rows_list):
    return torch.tensor([0] + [t.shape[0] for t in rows_list], dtype=torch.int64).cumsum(0)


def _workspace(B):
    from bdm_amd import _lib as L
    nbytes = L.lib().bdm_align_workspace_bytes(B)
    assert nbytes >= 16 * (B + 1) + 200 * B and nbytes % 16 == 0
    return torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda"), nbytes


def _call_moments(xs, ys, mode, start=None, expect=0):
    """One bdm_align_moments call on guarded outputs -> [(moments (18 Python ints), e, partner (P,) int64)] per entry."""
    from bdm_amd import _lib as L
    lib = L.lib()
    B, np_ = len(xs), [t.shape[0] for t in xs]
    xf, yf = _first(xs), _first(ys)
    sum_p = int(xf[-1])
    ws, nbytes = _workspace(B)
    mom, exp, par = _guarded(18 * B, torch.int64), _guarded(B, torch.int32), _guarded(sum_p, torch.int32)
    x, y = _pack(xs), _pack(ys)
    tr = None if start is None else start.float().cuda().contiguous()
    rc = lib.bdm_align_moments(B, mode, L.ptr(x), L.ptr(y), xf.data_ptr(), yf.data_ptr(), L.ptr(tr), L.ptr(mom[1]), L.ptr(exp[1]), L.ptr(par[1]),
                               L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(w, body=rc != 0) for w, _ in (mom, exp, par)), "sentinels around an output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    if rc:
        return None
    m, e, p = mom[1].view(B, 18).cpu().tolist(), exp[1].cpu().tolist(), par[1].cpu().long().split(np_)
    return list(zip(m, e, p))


def _run_icp(xs, ys, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False, start=None, chunk=1, observe=False):
    """The ABI's init / rounds / finish on a workspace pre-filled with 0xA5.  chunk: rounds per call.  observe: call finish after every
    rounds call as well and keep what it wrote.  -> (final dict, [dict per rounds call], history (B, max_iterations, 13) host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    B, np_ = len(xs), [t.shape[0] for t in xs]
    xf, yf = _first(xs), _first(ys)
    sum_p = int(xf[-1])
    ws, nbytes = _workspace(B)
    x, y = _pack(xs), _pack(ys)
    tr = None if start is None else start.float().cuda().contiguous()
    hist = torch.full((B, max_iterations, 13), F_SENTINEL, dtype=torch.float32, device="cuda")
    active = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    xp, yp, xfp, yfp = L.ptr(x), L.ptr(y), xf.data_ptr(), yf.data_ptr()
    L.check(lib.bdm_icp_init(B, xp, yp, xfp, yfp, L.ptr(tr), L.ptr(ws), L.stream()), "icp_init")

    def finish():
        xt, rows, mse = _guarded(3 * sum_p, torch.float32), _guarded(13 * B, torch.float32), _guarded(B, torch.float32)
        conv, its = _guarded(B, torch.int32), _guarded(B, torch.int32)
        L.check(lib.bdm_icp_finish(B, xp, xfp, yfp, L.ptr(xt[1]), L.ptr(rows[1]), L.ptr(mse[1]), L.ptr(conv[1]), L.ptr(its[1]), L.ptr(ws), L.stream()),
                "icp_finish")
        torch.cuda.synchronize()
        assert all(_untouched(w) for w, _ in (xt, rows, mse, conv, its))
        return {"xt": xt[1].view(sum_p, 3).cpu().split(np_), "tr": rows[1].view(B, 13).cpu(), "mse": mse[1].cpu(), "converged": conv[1].cpu().tolist(),
                "iterations": its[1].cpu().tolist()}
    steps, spent = [], 0
    while True:
        L.check(lib.bdm_icp_rounds(B, chunk, max_iterations, int(estimate_scale), relative_rmse_thr, A.EPS, xp, yp, xfp, yfp, L.ptr(hist), L.ptr(active),
                                   L.ptr(ws), L.stream()), "icp_rounds")
        spent += chunk
        left = int(active.item())
        if observe:
            steps.append(finish())
        if left == 0:
            break
        assert spent < max_iterations, f"{left} entries still active after {spent} rounds"
    final = finish()
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    return final, steps, hist.cpu()


def _same(name, got, want):
    assert torch.equal(A.bits(got), A.bits(want)), f"{name}: {int((A.bits(got) != A.bits(want)).sum())} of {got.numel()} differ; got {got.flatten()[:13].tolist()}, want {want.flatten()[:13].tolist()}"


def _assert_final(name, final, ref, hist=None):
    for i, r in enumerate(ref):
        assert final["iterations"][i] == r["iterations"] and bool(final["converged"][i]) == r["converged"], \
            f"{name} entry {i}: ({final['iterations'][i]}, {final['converged'][i]}) for ({r['iterations']}, {r['converged']})"
        _same(f"{name} entry {i} transform", final["tr"][i], r["tr"])
        _same(f"{name} entry {i} mse", final["mse"][i], r["mse"])
        _same(f"{name} entry {i} Xt", final["xt"][i], r["xt"])
        if hist is not None:
            for t, (tr, _) in enumerate(r["history"]):
                _same(f"{name} entry {i} history {t}", hist[i, t], tr)
            assert bool((hist[i, r["iterations"]:] == F_SENTINEL).all()), "rows past the last iteration were written"


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_integer_moments_and_partners_equal_the_restatement(hip, mode):
    c, want = A.moment_case(), A.moment_ref(mode)
    xs, ys = c["x"], c["y"]
    if mode == 1:
        n = [min(x.shape[0], y.shape[0]) for x, y in zip(xs, ys)]
        xs, ys = [x[:k] for x, k in zip(xs, n)], [y[:k] for y, k in zip(ys, n)]
    got = _call_moments(xs, ys, mode, start=c["start"] if mode == 0 else None)
    for i, ((gm, ge, gp), (wm, we, wp)) in enumerate(zip(got, want)):
        print(f"entry {i}: W = {gm[0]} of {xs[i].shape[0]} x {ys[i].shape[0]}, e = {ge}")
        assert ge == we, f"entry {i}: exponent {ge} for {we}"
        assert torch.equal(gp, wp), f"entry {i}: {int((gp != wp).sum())} partners differ"
        assert gm == wm, f"entry {i}: moments differ at {[k for k in range(18) if gm[k] != wm[k]]}"


def test_moments_do_not_depend_on_the_batch_slot(hip):
    c = A.moment_case()
    whole = _call_moments(c["x"], c["y"], 0, start=c["start"])
    again = _call_moments(c["x"], c["y"], 0, start=c["start"])
    for j in (4, 0, 3):
        alone = _call_moments(c["x"][j:j + 1], c["y"][j:j + 1], 0, start=c["start"][j:j + 1])[0]
        assert alone[0] == whole[j][0] == again[j][0] and torch.equal(alone[2], whole[j][2])


# ---- the iteration --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigid", "scale", "capped"])
def test_every_iteration_equals_the_restatement(hip, name):
    """rounds one at a time, finish after each: the transform, the mean squared residual, the counters and Xt after every iteration."""
    c, ref = A.icp_case(name), A.icp_ref(name)
    final, steps, hist = _run_icp(c["x"], c["y"], **c["kw"], chunk=1, observe=True)
    print(f"{name}: iterations {final['iterations']}, converged {final['converged']}, mse {final['mse'].tolist()}")
    assert len(steps) == max(max(r["iterations"] for r in ref), 1)
    for t, step in enumerate(steps, start=1):
        for i, r in enumerate(ref):
            done = min(t, r["iterations"])
            assert step["iterations"][i] == done
            if done:
                tr, mse = r["history"][done - 1]
                _same(f"{name} entry {i} iteration {t} transform", step["tr"][i], tr)
                _same(f"{name} entry {i} iteration {t} mse", step["mse"][i], torch.tensor(mse, dtype=torch.float64).float())
                _same(f"{name} entry {i} iteration {t} Xt", step["xt"][i], A.apply(c["x"][i], tr))
    _assert_final(name, final, ref, hist)


def test_a_start_transform_at_the_abi(hip):
    c = A.icp_case("rigid")
    start = A.moment_case()["start"][:3]
    ref = A.icp(c["x"], c["y"], start=start, **c["kw"])
    final, _, hist = _run_icp(c["x"], c["y"], **c["kw"], start=start, chunk=2)
    _assert_final("start", final, ref, hist)
    empty = _run_icp([A.box(4, 1)], [torch.zeros(0, 3)], start=start[:1])[0]
    assert empty["iterations"] == [0] and empty["converged"] == [0] and math.isnan(float(empty["mse"][0]))
    _same("the start transform comes back", empty["tr"][0], start[0])


def test_results_do_not_depend_on_slot_repetition_or_chunking(hip):
    c = A.icp_case("rigid")
    whole, _, hist = _run_icp(c["x"], c["y"], **c["kw"], chunk=1)
    for chunk in (3, 30):
        other, _, hist2 = _run_icp(c["x"], c["y"], **c["kw"], chunk=chunk)
        assert other["iterations"] == whole["iterations"] and other["converged"] == whole["converged"]
        _same(f"chunk {chunk}", other["tr"], whole["tr"])
        _same(f"chunk {chunk} mse", other["mse"], whole["mse"])
        _same(f"chunk {chunk} history", hist2, hist)
        assert all(torch.equal(A.bits(a), A.bits(b)) for a, b in zip(other["xt"], whole["xt"]))
    for j in (2, 0):
        alone = _run_icp(c["x"][j:j + 1], c["y"][j:j + 1], **c["kw"], chunk=4)[0]
        assert alone["iterations"][0] == whole["iterations"][j]
        _same(f"entry {j} alone", alone["tr"][0], whole["tr"][j])
        _same(f"entry {j} alone Xt", alone["xt"][0], whole["xt"][j])


def test_every_entry_stops_on_its_own(hip):
    c, ref = A.icp_case("stop"), A.icp_ref("stop")
    final, _, hist = _run_icp(c["x"], c["y"], **c["kw"], chunk=1)
    _assert_final("stop", final, ref, hist)
    assert final["iterations"][0] == 2 and final["iterations"][1] > 2
    alone = _run_icp(c["x"][:1], c["y"][:1], **c["kw"])[0]
    assert alone["iterations"] == [2] and alone["converged"] == [1]
    _same("entry 0 alone", alone["tr"][0], final["tr"][0])
    _same("entry 0 alone mse", alone["mse"][0], final["mse"][0])


def test_identical_clouds_converge_in_one_iteration(hip):
    """On a dyadic lattice every moment is exact in float64, so the analytic mse is exactly 0.  On a generic cloud it is rounding noise
    of either sign before the clamp (bdm_hip.h section 18): then the entry converges in one iteration or in two."""
    c, ref = A.icp_case("identical"), A.icp_ref("identical")
    final, _, _ = _run_icp(c["x"], c["y"], **c["kw"])
    _assert_final("identical", final, ref)
    assert final["iterations"] == [1] and final["converged"] == [1] and float(final["mse"][0]) == 0.0
    _same("identity", final["tr"][0], A.identity())
    x = A.box(333, 5)
    generic = _run_icp([x], [x.clone()], max_iterations=30)[0]
    _assert_final("generic identical", generic, A.icp([x], [x.clone()], max_iterations=30))
    assert generic["converged"] == [1] and generic["iterations"][0] <= 2 and float(generic["mse"][0]) < 1e-12


# ---- paired alignment -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimate_scale", [False, True])
def test_paired_alignment_equals_the_restatement(hip, estimate_scale):
    from bdm_amd import _lib as L
    GAP_GENERAL = A.GAP_GENERAL
    lib = L.lib()
    c, ref = A.paired_case(), A.paired_ref(estimate_scale)
    B = len(c["x"])
    xf, yf = _first(c["x"]), _first(c["y"])
    ws, nbytes = _workspace(B)
    rows, mse = _guarded(13 * B, torch.float32), _guarded(B, torch.float32)
    x, y = _pack(c["x"]), _pack(c["y"])
    L.check(lib.bdm_corresponding_points_alignment(B, int(estimate_scale), A.EPS, L.ptr(x), L.ptr(y), xf.data_ptr(), yf.data_ptr(), L.ptr(rows[1]),
                                                   L.ptr(mse[1]), L.ptr(ws), L.stream()), "corresponding_points_alignment")
    torch.cuda.synchronize()
    assert _untouched(rows[0]) and _untouched(mse[0]) and bool((ws[nbytes:] == 0xA5).all())
    got, got_mse = rows[1].view(B, 13).cpu(), mse[1].cpu()
    for i, (tr, m, _, _) in enumerate(ref):
        _same(f"entry {i} transform", got[i], tr)
        _same(f"entry {i} mse", got_mse[i], m)
    assert float(torch.det(got[c["reflection"], :9].view(3, 3).double())) > 0.99      # a proper rotation where the plain SVD reflects
    for i in c["well"]:
        m, e = A._moment_rows(c["x"][i], c["y"][i])
        R, T, s, _ = A.solve(m, e, estimate_scale, rotation=A.svd_rotation)
        want = torch.tensor([float(v) for v in list(R) + list(T) + [s]], dtype=torch.float64)
        gap = float((got[i].double() - want).abs().max())
        print(f"entry {i}: gap to the SVD definition {gap:.3e}, bound {GAP_GENERAL:.3e}")
        assert gap <= GAP_GENERAL


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface(hip):
    from bdm_amd.cameras import Pointclouds
    c, ref = A.icp_case("init"), A.icp_ref("init")
    init = AL.SimilarityTransform(c["init"][:, :9].view(3, 3, 3).cuda(), c["init"][:, 9:12].cuda(), c["init"][:, 12].cuda())
    xs, ys = [x.cuda() for x in c["x"]], [y.cuda() for y in c["y"]]
    sol = AL.iterative_closest_point(xs, ys, init_transform=init, **c["kw"])
    assert isinstance(sol, AL.ICPSolution) and isinstance(sol.Xt, list) and sol.converged.dtype == torch.bool and sol.converged.shape == (3,)
    assert len(sol.t_history) == max(r["iterations"] for r in ref)
    for i, r in enumerate(ref):
        assert bool(sol.converged[i]) == r["converged"]
        _same(f"entry {i} R", sol.RTs.R[i].cpu().reshape(-1), r["tr"][:9])
        _same(f"entry {i} T", sol.RTs.T[i].cpu(), r["tr"][9:12])
        _same(f"entry {i} s", sol.RTs.s[i].cpu(), r["tr"][12])
        _same(f"entry {i} rmse", sol.rmse[i].cpu(), r["mse"])
        _same(f"entry {i} Xt", sol.Xt[i].cpu(), r["xt"])
        for t, h in enumerate(sol.t_history):
            tr = r["history"][min(t, r["iterations"] - 1)][0]
            _same(f"entry {i} t_history {t}", torch.cat([h.R[i].reshape(-1), h.T[i], h.s[i:i + 1]]).cpu(), tr)
    moved = AL.apply_similarity_transform(xs, *init)
    for i in range(3):
        _same(f"apply {i}", moved[i].cpu(), A.apply(c["x"][i], c["init"][i]))
    # padded tensors and Pointclouds give their own forms; a padded batch of equal clouds repeats the list's bits
    x2, y2 = torch.stack([xs[0], xs[0]]), torch.stack([ys[0], ys[0]])
    padded = AL.iterative_closest_point(x2, y2, max_iterations=30)
    alone = AL.iterative_closest_point([xs[0]], [ys[0]], max_iterations=30)
    assert padded.Xt.shape == (2, 257, 3) and torch.equal(padded.Xt[0], padded.Xt[1]) and torch.equal(padded.Xt[1], alone.Xt[0])
    clouds = AL.iterative_closest_point(Pointclouds([xs[0]]), Pointclouds([ys[0]]), max_iterations=30)
    assert isinstance(clouds.Xt, Pointclouds) and torch.equal(clouds.Xt.points_list()[0], alone.Xt[0])
    # paired alignment with a 0/1 mask equals the alignment of the kept rows
    pc = A.paired_case()
    a, ya = pc["x"][0].cuda(), pc["y"][0].cuda()
    mask = (torch.arange(300) % 3 != 0).cuda()
    masked = AL.corresponding_points_alignment(a[None], ya[None], weights=mask[None].float(), estimate_scale=True)
    kept = AL.corresponding_points_alignment([a[mask]], [ya[mask]], estimate_scale=True)
    want = A.corresponding_points_alignment(pc["x"][0][mask.cpu()], pc["y"][0][mask.cpu()], True)[0]
    _same("kept rows", torch.cat([kept.R[0].reshape(-1), kept.T[0], kept.s]).cpu(), want)
    # a masked row is a NaN source row: its pair is left out, its target row still counts towards amax and the entry keeps its length
    blanked = torch.where(mask.cpu()[:, None], pc["x"][0], torch.full((), float("nan")))
    _same("mask", torch.cat([masked.R[0].reshape(-1), masked.T[0], masked.s]).cpu(), A.corresponding_points_alignment(blanked, pc["y"][0], True)[0])


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    x, y = [A.box(5, 1), A.box(3, 2)], [A.box(4, 3), A.box(6, 4)]
    assert _call_moments(x, y, 2, expect=1) is None                                    # mode
    assert _call_moments(x, y, 1, expect=1) is None                                    # paired with unequal lengths
    assert lib.bdm_align_workspace_bytes(-1) == 0 and lib.bdm_align_workspace_bytes(65536) == 0 and lib.bdm_similarity_apply_workspace_bytes(65536) == 0
    B = 2
    xf, yf = _first(x), _first(y)
    ws, _ = _workspace(B)
    xd, yd = _pack(x), _pack(y)
    rows, mse, xt = _guarded(13 * B, torch.float32), _guarded(B, torch.float32), _guarded(3 * 8, torch.float32)
    conv, its, act = _guarded(B, torch.int32), _guarded(B, torch.int32), _guarded(1, torch.int32)
    bad_first = torch.tensor([0, 5, 4], dtype=torch.int64)                             # decreasing
    big_first = torch.tensor([0, 2 ** 20 + 1, 2 ** 20 + 2], dtype=torch.int64)         # an entry above 2^20 points
    sum_first = torch.tensor([0, 2 ** 20, 2 ** 31], dtype=torch.int64)
    P = L.ptr
    st = L.stream()
    calls = {
        "negative b": lambda: lib.bdm_icp_init(-1, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(ws), st),
        "b above 65535": lambda: lib.bdm_icp_init(65536, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(ws), st),
        "decreasing offsets": lambda: lib.bdm_icp_init(B, P(xd), P(yd), bad_first.data_ptr(), yf.data_ptr(), None, P(ws), st),
        "entry above 2^20": lambda: lib.bdm_icp_init(B, P(xd), P(yd), big_first.data_ptr(), yf.data_ptr(), None, P(ws), st),
        "sum at 2^31": lambda: lib.bdm_icp_init(B, P(xd), P(yd), xf.data_ptr(), sum_first.data_ptr(), None, P(ws), st),
        "NULL offsets": lambda: lib.bdm_icp_init(B, P(xd), P(yd), None, yf.data_ptr(), None, P(ws), st),
        "NULL workspace": lambda: lib.bdm_icp_init(B, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, None, st),
        "misaligned workspace": lambda: lib.bdm_icp_init(B, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(ws) + 8, st),
        "NULL points": lambda: lib.bdm_icp_init(B, None, P(yd), xf.data_ptr(), yf.data_ptr(), None, P(ws), st),
        "rounds = 0": lambda: lib.bdm_icp_rounds(B, 0, 10, 0, 1e-6, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st),
        "max_iterations = 0": lambda: lib.bdm_icp_rounds(B, 1, 0, 0, 1e-6, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st),
        "max_iterations above 10000": lambda: lib.bdm_icp_rounds(B, 1, 10001, 0, 1e-6, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st),
        "negative eps": lambda: lib.bdm_icp_rounds(B, 1, 10, 0, 1e-6, -1.0, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st),
        "NaN threshold": lambda: lib.bdm_icp_rounds(B, 1, 10, 0, float("nan"), 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st),
        "NULL counter": lambda: lib.bdm_icp_rounds(B, 1, 10, 0, 1e-6, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, None, P(ws), st),
        "counter inside the workspace": lambda: lib.bdm_icp_rounds(B, 1, 10, 0, 1e-6, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), None, P(ws) + 64, P(ws), st),
        "NULL output": lambda: lib.bdm_icp_finish(B, P(xd), xf.data_ptr(), yf.data_ptr(), P(xt[1]), None, P(mse[1]), P(conv[1]), P(its[1]), P(ws), st),
        "Xt over the points": lambda: lib.bdm_icp_finish(B, P(xd), xf.data_ptr(), yf.data_ptr(), P(xd), P(rows[1]), P(mse[1]), P(conv[1]), P(its[1]), P(ws), st),
        "paired lengths": lambda: lib.bdm_corresponding_points_alignment(B, 0, 1e-9, P(xd), P(yd), xf.data_ptr(), yf.data_ptr(), P(rows[1]), P(mse[1]), P(ws), st),
        "paired eps": lambda: lib.bdm_corresponding_points_alignment(B, 0, float("inf"), P(xd), P(xd), xf.data_ptr(), xf.data_ptr(), P(rows[1]), P(mse[1]), P(ws), st),
        "apply NULL transform": lambda: lib.bdm_similarity_apply(B, P(xd), xf.data_ptr(), None, P(xt[1]), P(ws), st),
        "apply in place": lambda: lib.bdm_similarity_apply(B, P(xd), xf.data_ptr(), P(rows[1]), P(xd), P(ws), st),
    }
    before = (xd.clone(), yd.clone())
    for name, call in calls.items():
        assert call() == 1, name
        assert lib.bdm_last_error(), name
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in (rows, mse, xt, conv, its, act)), "an output of a refused call was written"
    assert torch.equal(xd, before[0]) and torch.equal(yd, before[1]) and bool((ws == 0xA5).all())
    # b == 0 and batches without a source point return 0 and launch nothing
    zero, none = torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    assert lib.bdm_icp_init(0, None, None, None, None, None, None, st) == 0
    assert lib.bdm_icp_rounds(0, 1, 10, 0, 1e-6, 1e-9, None, None, None, None, None, None, None, st) == 0
    assert lib.bdm_icp_finish(0, None, zero.data_ptr(), zero.data_ptr(), None, None, None, None, None, None, st) == 0
    assert lib.bdm_icp_init(B, P(xd), P(yd), none.data_ptr(), yf.data_ptr(), None, P(ws), st) == 0
    assert lib.bdm_icp_rounds(B, 1, 10, 0, 1e-6, 1e-9, P(xd), P(yd), none.data_ptr(), yf.data_ptr(), None, P(act[1]), P(ws), st) == 0
    assert lib.bdm_icp_finish(B, P(xd), none.data_ptr(), yf.data_ptr(), P(xt[1]), P(rows[1]), P(mse[1]), P(conv[1]), P(its[1]), P(ws), st) == 0
    assert lib.bdm_corresponding_points_alignment(B, 0, 1e-9, P(xd), P(yd), none.data_ptr(), none.data_ptr(), P(rows[1]), P(mse[1]), P(ws), st) == 0
    assert lib.bdm_similarity_apply(B, P(xd), none.data_ptr(), P(rows[1]), P(xt[1]), P(ws), st) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in (rows, mse, xt, conv, its, act)) and bool((ws == 0xA5).all())
    sol = AL.iterative_closest_point([torch.zeros(0, 3, device="cuda")], [A.box(4, 1).cuda()])
    assert sol.converged.tolist() == [False] and math.isnan(float(sol.rmse[0])) and sol.Xt[0].shape == (0, 3) and sol.t_history == []
    assert torch.equal(sol.RTs.R[0].cpu(), torch.eye(3))


# ---- the evaluator --------------------------------------------------------------------------------------------------------------------
def test_evaluator_aligns_before_it_scores(hip, tmp_path):
    from bdm_amd import evaluation as E
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply
    rels = {"a/one.ply": 300, "a/two.ply": 400, "b/three.ply": 500}
    for k, (rel, n) in enumerate(rels.items()):
        gt = A.box(n, 500 + k)
        pred = (gt.double() @ A.rotation_matrix((1.0, 2.0, 3.0), 6.0 + k) + 0.002 * torch.randn(n, 3, generator=torch.Generator().manual_seed(k), dtype=torch.float64))
        save_pointcloud_ply(gt.numpy(), tmp_path / "gt" / rel)
        save_pointcloud_ply(pred.float().numpy(), tmp_path / "pred" / rel)
    plain = E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"))
    res = E.evaluate_dirs(str(tmp_path / "pred"), str(tmp_path / "gt"), align="icp", batch_size=2)
    print(res)
    assert sorted(plain) == ["cd_x1000", "f1_at_0.01", "num"] and res["num"] == 3
    assert res["cd_x1000"] < res["cd_x1000_unaligned"] and res["f1_at_0.01"] >= res["f1_at_0.01_unaligned"]
    assert abs(res["cd_x1000_unaligned"] - plain["cd_x1000"]) <= 1e-6 * plain["cd_x1000"] and abs(res["f1_at_0.01_unaligned"] - plain["f1_at_0.01"]) <= 1e-6
    preds = [torch.from_numpy(load_pointcloud_ply(tmp_path / "pred" / rel)).float().cuda() for rel in rels]
    gts = [torch.from_numpy(load_pointcloud_ply(tmp_path / "gt" / rel)).float().cuda() for rel in rels]
    preds, gts = [p - p.mean(0, keepdim=True) for p in preds], [g - g.mean(0, keepdim=True) for g in gts]
    sol = AL.iterative_closest_point(preds, gts)
    xt, conv, its, mse = AL.icp_align_lists(preds, gts)
    assert all(torch.equal(a, b) for a, b in zip(sol.Xt, xt)) and torch.equal(conv, sol.converged) and torch.equal(A.bits(mse), A.bits(sol.rmse))
    assert res["icp_converged"] == int(sol.converged.sum()) == 3
    assert res["icp_iterations_mean"] == float(np.mean(its.cpu().tolist())) and res["icp_mse_mean"] == float(np.mean([float(v) for v in sol.rmse.cpu().tolist()]))
    cds = [float(E.cd_x1000_as_is(a[None], g[None])[0]) for a, g in zip(sol.Xt, gts)]
    f1s = [float(E.f1_score(a[None], g[None])[0]) for a, g in zip(sol.Xt, gts)]
    assert res["cd_x1000"] == float(np.mean(cds)) and res["f1_at_0.01"] == float(np.mean(f1s))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "bdm_amd.evaluation", "--pred_dir", str(tmp_path / "pred"), "--gt_dir", str(tmp_path / "gt"), "--icp",
                          "--batch-size", "2"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == res
