"""CPU tests behind the any-size approximate-match EMD: the row-blocked float64 restatement that writes the goldens against
metrics_ref.emd_approx_ref, the measured tolerance constant, the header's new declarations as the generators see them, the routing
threshold of compute_all_metrics and the argument parsing of the two command lines.  No kernel runs here."""
import ctypes
import os

import numpy as np
import pytest

import metrics_large_ref as LR
import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocked_restatement_equals_the_unblocked_one():
    a, b = R.emd_case(300, 1, 1, 7)
    want = R.emd_approx_ref(a[0], b[0])
    for block, cache in ((128, 1 << 28), (128, 0), (77, 0), (512, 0)):   # several blocks kept | recomputed per pass | uneven blocks | one block
        got = LR.emd_approx_blocked(a[0], b[0], block=block, cache_bytes=cache)
        assert abs(got - want) <= 1e-12 * want, f"block={block} cache={cache}: {got} vs {want}"
    assert LR.emd_approx_blocked(a[0], b[0], block=512) == want   # one block: operation for operation
    assert LR.emd_approx_blocked(a[0], b[0], np.float32, block=512) == R.emd_approx_ref(a[0], b[0], np.float32)


def test_case_list_and_golden_file_agree():
    ns = [c[0] for c in LR.LARGE_CASES]
    assert len(set(ns)) == len(ns)
    assert {LR.STAGE - 1, LR.STAGE, LR.STAGE + 1, LR.THREADS * LR.KPT - 1, LR.THREADS * LR.KPT + 1, 2049} <= set(ns)
    assert all(n <= 2100 for n, _, _, _, kind in LR.LARGE_CASES if kind == "live")   # live float64 work stays at seconds per pair
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics_emd_large.npz"))
    golden = [list(c[:4]) for c in LR.LARGE_CASES if c[4] == "golden"]
    assert g["cases"].tolist() == golden and [n for n, _, _, _ in golden] == [2600, 4096, 4097, 8192]
    for n, s, r, _ in golden:
        m = g[f"emd_n{n}"]
        assert m.shape == (s, r) and m.dtype == np.float64 and (m > 0.2).all() and (m < 0.5).all()
    a, b = LR.large_case(2600)   # the fixture is the restatement's output (the cheapest golden pair, ~3 s)
    assert g["emd_n2600"][1, 0] == pytest.approx(LR.emd_approx_blocked(a[1], b[0]), rel=1e-12)


PAIRS_UP_TO_2049 = list(LR.large_case_pairs(max_n=2049))


def test_gap_constant_covers_the_cases_up_to_2049_points():
    """g_large re-measured on every pair with n <= 2049 (natural and reversed order): none exceeds the recorded constant, and the
    pair that set it reproduces it."""
    worst, worst_name = 0.0, None
    for name, a, b in PAIRS_UP_TO_2049:
        g, _ = LR.gap(a, b)
        if g > worst:
            worst, worst_name = g, name
    print(f"g over n <= 2049: {worst:.3e} at {worst_name}; recorded g_large {LR.EMD_G_LARGE:.3e}")
    assert worst <= LR.EMD_G_LARGE
    assert worst >= 0.99 * LR.EMD_G_LARGE and worst_name.startswith("n256[0,1]"), "the recorded constant is no longer the measured one: run tools/metrics_emd_large_gap.py"


def test_header_declarations_reach_both_generators(tmp_path):
    import sys
    from bdm_amd import _lib as L
    sigs = L.abi_signatures()
    assert sigs["bdm_pairwise_emd_large_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert sigs["bdm_pairwise_emd_large_variant"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4)
    assert sigs["bdm_pairwise_emd_large"] == (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p])
    assert sigs["bdm_pairwise_emd_approx"] == (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4)   # untouched
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_tape_thunks
    finally:
        sys.path.pop(0)
    out = tmp_path / "thunks.inc"
    gen_tape_thunks.main(L.HEADER, str(out))
    text = out.read_text()
    assert '{"bdm_pairwise_emd_large", thunk_bdm_pairwise_emd_large, 11}' in text
    assert "(size_t)(int64_t)a[8]" in text and '{"bdm_pairwise_emd_large_variant", thunk_bdm_pairwise_emd_large_variant, 6}' in text
    assert "thunk_bdm_pairwise_emd_large_workspace_bytes" not in text   # a size query is not a step


def test_routing_threshold():
    from bdm_amd import metrics as M
    assert M.EMD_SMALL_MAX_POINTS == 2048
    assert M.emd_route(1) is M.pairwise_emd and M.emd_route(2048) is M.pairwise_emd
    assert M.emd_route(2049) is M.pairwise_emd_large and M.emd_route(16384) is M.pairwise_emd_large


def test_metrics_command_line_num_points(tmp_path):
    from bdm_amd import metrics as M
    args = M.parse_args(["--sample", "s.npy", "--ref", "r.npy"])
    assert args.num_points is None
    args = M.parse_args(["--sample", "s.npy", "--ref", "r.npy", "--num-points", "2048", "--metrics", "emd"])
    assert args.num_points == 2048 and args.metrics == ("emd",)
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit):
            M.parse_args(["--sample", "s.npy", "--ref", "r.npy", "--num-points", bad])
    np.save(tmp_path / "s.npy", R.shape_clouds(2, 40, 1))
    np.save(tmp_path / "r.npy", R.shape_clouds(2, 50, 2))
    with pytest.raises(ValueError, match="--num-points 41"):   # more than one of the sets has: refused before any device work
        M.main(["--sample", str(tmp_path / "s.npy"), "--ref", str(tmp_path / "r.npy"), "--num-points", "41"])


def test_evaluation_command_line():
    from bdm_amd import evaluation as E
    args = E.parse_args(["--pred_dir", "p", "--gt_dir", "g"])
    assert (args.pred_dir, args.gt_dir, args.emd) == ("p", "g", False)
    assert E.parse_args(["--pred_dir", "p", "--gt_dir", "g", "--emd"]).emd is True
    with pytest.raises(SystemExit):
        E.parse_args(["--pred_dir", "p"])
    import inspect
    assert inspect.signature(E.evaluate_dirs).parameters["emd"].default is False


def test_host_only_queries_and_argument_errors():
    """What the library answers before any GPU call: the variant query, the workspace size, and the argument errors (code 1 / 3)."""
    from bdm_amd import _lib as L
    lib = L.lib()

    def variant(n, mode):
        v = [ctypes.c_int(-1) for _ in range(4)]
        return lib.bdm_pairwise_emd_large_variant(n, mode, *[ctypes.addressof(x) for x in v]), tuple(x.value for x in v)

    resident, streamed = (1, LR.THREADS, LR.KPT, 0), (0, LR.THREADS, LR.KPT, LR.STAGE)
    assert variant(1, 0) == (0, resident) and variant(4096, 0) == (0, resident) and variant(4097, 0) == (0, streamed)
    assert variant(5, 2) == (0, streamed) and variant(4096, 1) == (0, resident) and variant(16384, 0) == (0, streamed)
    assert variant(4097, 1) == (3, (0, 0, 0, 0)) and variant(65537, 0) == (3, (0, 0, 0, 0)) and variant(65536, 2) == (0, streamed)
    assert variant(0, 0)[0] == 1 and variant(5, 3)[0] == 1 and variant(5, -1)[0] == 1
    size = lib.bdm_pairwise_emd_large_workspace_bytes
    assert size(9, 100) == 9 * 20 * 100 and size(9, 101) == 9 * 20 * 104 and size(400 * 400, 4096) == 256 * 20 * 4096
    assert [size(0, 100), size(-1, 100), size(9, 0), size(9, 65537)] == [0, 0, 0, 0]
    call = lib.bdm_pairwise_emd_large
    assert call(3, 3, 0, 0, 0, None, None, None, 0, None, None) == 1
    assert call(3, 2, 10, 1, 0, None, None, None, 0, None, None) == 1 and b"paired" in lib.bdm_last_error()
    assert call(3, 3, 10, 0, 0, None, None, None, 0, None, None) == 1 and b"null" in lib.bdm_last_error()
    assert call(1, 1, 65537, 0, 0, None, None, None, 0, None, None) == 3 and b"65537" in lib.bdm_last_error()
    assert call(0, 3, 10, 0, 0, None, None, None, 0, None, None) == 0 and call(3, 0, 10, 1, 0, None, None, None, 0, None, None) == 1
