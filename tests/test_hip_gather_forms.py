"""Bit equality of the re-parallelised gather kernels with the forms they replace (all comparisons are torch.equal):

* avg-voxelise onto the occupied rows (csrc/sparse_conv.hip: sparse_vox_features_lds_kernel<OUT>: one cell record per occupied
  row, one maximum atomic per workgroup) against the global-memory form (BDM_STAGING=0, read per call: the switch of
  test_hip_dense.py), for both record formats and the per-shape maximum;
* the cell records of the voxel plan (csrc/common.h: VoxWs) against cnt / start / sorted of the same plan, for both plan kernels;
* the FP-module input assembly from LDS-staged rows (csrc/pvcnn_ops.hip: fp_assemble_lds_kernel) against the per-point kernel
  (bdm_fp_assemble_form) and against the three-term expression in torch float32.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

REC, REC_PTS = 8, 6   # ints per cell record, list entries it holds (csrc/common.h)


@pytest.fixture(scope="module")
def ops(hip):
    from bdm_amd import ops as o
    return o


# ---- voxel plans from explicit integer coordinates -------------------------------------------------------------------------------
def _vox_coords(B, n, r, seed, occupied=None):
    """(B, 3, n) int32 cells.  Shape 0 opens with NINE points in one cell (a list longer than the record and than two rounds of
    the four-entry walk); `occupied` = per shape the exact number of occupied cells (the first `occupied[b]` points take
    distinct cells, the others fall into those)."""
    g = torch.Generator().manual_seed(seed)
    r3 = r ** 3
    v = torch.randint(0, r3, (B, n), generator=g)
    if occupied is not None:
        for b, k in enumerate(occupied):
            cells = torch.randperm(r3, generator=g)[:k]
            v[b, :k] = cells
            v[b, k:] = cells[torch.randint(0, k, (n - k,), generator=g)]
    elif n >= 9:
        v[0, :9] = v[0, 0]
    return torch.stack([v // (r * r), (v // r) % r, v % r], 1).int().cuda()


def _plan(ops, vox, r, full=True):
    """Plan of integer voxel coordinates: bdm_voxelize_plan_full (cell records), or the three-launch form without them."""
    L = ops.L
    B, _, n = vox.shape
    p = ops.VoxelPlan(vox, r)
    if full:
        L.check(L.lib().bdm_voxelize_plan_full(B, n, r, p.n_max, L.ptr(vox), L.ptr(p.ind), L.ptr(p.cnt), L.ptr(p.ws), L.ptr(p.occ_index),
                                               L.ptr(p.occ_list), L.ptr(p.n_occ), L.ptr(p.rowocc), L.stream()), "plan_full")
    else:
        L.check(L.lib().bdm_voxelize_plan(B, n, r, L.ptr(vox), L.ptr(p.ind), L.ptr(p.cnt), L.ptr(p.ws), L.stream()), "plan")
        L.check(L.lib().bdm_voxel_compact(B, r, p.n_max, L.ptr(p.cnt), L.ptr(p.occ_index), L.ptr(p.occ_list), L.ptr(p.n_occ), L.stream()),
                "compact")
    return p


def _ws_fields(p, B, n, r):
    """start (B, r3), flags (B,), records (B, rows, REC), sorted (B, n) of a plan's workspace (csrc/common.h: VoxWs)"""
    r3, rows = r ** 3, min(n, r ** 3)
    ws = p.ws.view(torch.int32).cpu()
    off = (B * r3 + B + 3) & ~3
    assert ws.numel() == off + B * rows * REC + 2 * B * n
    return (ws[:B * r3].view(B, r3), ws[B * r3:B * r3 + B], ws[off:off + B * rows * REC].view(B, rows, REC),
            ws[ws.numel() - B * n:].view(B, n))


# (B, C, N, r): C below / not a multiple of 8, N not a multiple of 4 (scalar staging), both workgroup sizes (n_max <= / > 1024),
# 65 channel groups per shape on few cells (many workgroups race for a shape's maximum)
VOX_CASES = [(1, 4, 64, 4), (2, 12, 200, 4), (3, 32, 1000, 8), (2, 64, 1024, 8), (2, 72, 4096, 16), (2, 35, 1001, 8), (2, 520, 64, 4)]


def _features_both(ops, monkeypatch, p, B, C, n, r, feat):
    """{staging: (fp32 records, amax, bf16-triple records)} for BDM_STAGING = "0" (global-memory kernels) and unset"""
    L = ops.L
    f, _, _, _, bs_f, ld_f = ops._bcl(feat)
    assert f.data_ptr() == feat.data_ptr()
    G = (C + 7) // 8
    out = {}
    for staging in ("0", None):
        if staging is None:
            monkeypatch.delenv("BDM_STAGING", raising=False)
        else:
            monkeypatch.setenv("BDM_STAGING", staging)
        xr = torch.full((B, G, p.n_max, 8), 7.0, dtype=torch.float32, device="cuda")
        amax = torch.zeros(B, dtype=torch.float32, device="cuda")
        xs = torch.full((B, G, 3, p.n_max, 8), 7.0, dtype=torch.bfloat16, device="cuda")   # rows past the last GEMM tile stay as they are
        L.check(L.lib().bdm_sparse_voxel_features_f32(B, C, n, r, p.n_max, L.ptr(f), bs_f, ld_f, L.ptr(p.cnt), L.ptr(p.ws),
                                                      L.ptr(p.occ_list), L.ptr(p.n_occ), L.ptr(xr), L.ptr(amax), L.stream()), "f32")
        L.check(L.lib().bdm_sparse_voxel_features_s3(B, C, n, r, p.n_max, L.ptr(f), bs_f, ld_f, L.ptr(p.cnt), L.ptr(p.ws),
                                                     L.ptr(p.occ_list), L.ptr(p.n_occ), L.ptr(xs), L.stream()), "s3")
        out[staging] = (xr, amax, xs)
    monkeypatch.delenv("BDM_STAGING", raising=False)
    return out


def _check_features(ops, monkeypatch, p, B, C, n, r, feat):
    res = _features_both(ops, monkeypatch, p, B, C, n, r, feat)
    (xr0, am0, xs0), (xr1, am1, xs1) = res["0"], res[None]
    assert torch.equal(xr1, xr0) and torch.equal(am1, am0)
    assert torch.equal(xs1.view(torch.int16), xs0.view(torch.int16))
    nocc = p.n_occ.cpu()
    for b in range(B):
        k = int(nocc[b])
        assert not bool(xr1[b, :, k:].any())                                   # fp32 records: rows beyond n_occ are zeros
        lim = min((k + 127) & ~127, p.n_max)
        assert bool((xs1[b, :, :, lim:] == 7.0).all())                          # bf16 triples: rows beyond the GEMM's last tile are skipped
        assert not bool(xs1[b, :, :, k:lim].float().any())
    assert float(am1.min()) > 0


@pytest.mark.parametrize("B,C,n,r", VOX_CASES)
@pytest.mark.parametrize("offset", [0, 1])
def test_voxelise_from_cell_records_equals_global_gather(ops, monkeypatch, B, C, n, r, offset):
    """offset = 1: the feature view starts one float into its buffer (rows not 16-byte aligned: scalar staging)."""
    vox = _vox_coords(B, n, r, seed=C + n)
    p = _plan(ops, vox, r)
    g = torch.Generator().manual_seed(n + C)
    flat = torch.randn(B * C * n + 1, generator=g).cuda()
    feat = flat[offset:offset + B * C * n].view(B, C, n)
    _check_features(ops, monkeypatch, p, B, C, n, r, feat)


@pytest.mark.parametrize("occupied", [(127, 128, 129), (255, 1, 257)])
def test_voxelise_row_skip_around_a_tile_boundary(ops, monkeypatch, occupied):
    """n_occ just under / on / over a multiple of the GEMM's 128-row tile: the bf16-triple form writes whole tiles only."""
    B, C, n, r = 3, 20, 300, 8
    vox = _vox_coords(B, n, r, seed=sum(occupied), occupied=occupied)
    p = _plan(ops, vox, r)
    assert tuple(int(x) for x in p.n_occ.cpu()) == occupied
    feat = torch.randn(B, C, n, generator=torch.Generator().manual_seed(5)).cuda()
    _check_features(ops, monkeypatch, p, B, C, n, r, feat)


def test_voxelise_on_a_plan_without_cell_records(ops, monkeypatch):
    """bdm_voxelize_plan + bdm_voxel_compact know no records (flag 0): the kernel walks occ_list -> cnt / start -> sorted."""
    B, C, n, r = 2, 24, 501, 8
    vox = _vox_coords(B, n, r, seed=3)
    p = _plan(ops, vox, r, full=False)
    torch.cuda.synchronize()
    assert not bool(_ws_fields(p, B, n, r)[1].any())
    feat = torch.randn(B, C, n, generator=torch.Generator().manual_seed(6)).cuda()
    _check_features(ops, monkeypatch, p, B, C, n, r, feat)
    q = _plan(ops, vox, r, full=True)
    a, b = _features_both(ops, monkeypatch, p, B, C, n, r, feat)[None], _features_both(ops, monkeypatch, q, B, C, n, r, feat)[None]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("B,n,r,staging", [(1, 64, 4, None), (2, 200, 4, None), (3, 1000, 8, None), (2, 1024, 8, None), (2, 4096, 16, None),
                                            (2, 4096, 32, None), (2, 4096, 32, "0"), (2, 1001, 32, None)])
def test_plan_cell_records_restate_the_lists(ops, monkeypatch, B, n, r, staging):
    """Record k of a shape = {cnt, start, first six list entries (zeros past the list)} of its k-th occupied cell; 32^3 plans come
    from the eight-slab kernel, or with BDM_STAGING=0 from the one-workgroup kernel like the smaller grids."""
    if staging is None:
        monkeypatch.delenv("BDM_STAGING", raising=False)
    else:
        monkeypatch.setenv("BDM_STAGING", staging)
    vox = _vox_coords(B, n, r, seed=n + r)
    p = _plan(ops, vox, r)
    torch.cuda.synchronize()
    start, flag, rec, sorted_ = _ws_fields(p, B, n, r)
    cnt, occ_list, n_occ = p.cnt.cpu(), p.occ_list.cpu(), p.n_occ.cpu()
    assert bool((flag == 1).all())
    for b in range(B):
        k = int(n_occ[b])
        cells = occ_list[b, :k].long()
        want = torch.zeros(k, REC, dtype=torch.int32)
        want[:, 0], want[:, 1] = cnt[b, cells], start[b, cells]
        for q in range(REC_PTS):
            live = want[:, 0] > q
            want[live, 2 + q] = sorted_[b, (want[live, 1] + q).long()]
        assert int(want[:, 0].max()) >= (9 if b == 0 and n >= 9 else 1)
        assert torch.equal(rec[b, :k], want)


# ---- FP-module input assembly --------------------------------------------------------------------------------------------------------
def _padded(B, c, l, pad, g, fill=None):
    """(B, c, l) view with batch stride and row stride larger than the dense ones (pad = 4: 16-byte aligned rows, 3: not)"""
    big = torch.randn(B, c + 1, l + pad, generator=g).cuda() if fill is None else torch.full((B, c + 1, l + pad), fill, device="cuda")
    return big, big[:, :c, :l]


@pytest.mark.parametrize("B,m,n,c_a,c_s,c_t", [(1, 3, 5, 1, 0, 0), (2, 16, 100, 5, 3, 0), (2, 64, 256, 64, 35, 64), (2, 1024, 1000, 130, 7, 64)])
@pytest.mark.parametrize("pad", [4, 3])
def test_fp_assembly_from_staged_rows_equals_per_point_kernel(ops, B, m, n, c_a, c_s, c_t, pad):
    L = ops.L
    g = torch.Generator().manual_seed(m + n + pad)
    idx = torch.randint(0, m, (B, 3, n), generator=g).int()
    idx[:, :, : max(1, n // 4)] = idx[:, :1, : max(1, n // 4)]                  # the three neighbours coincide
    idx[:, :, -1] = m - 1
    w = torch.rand(B, 3, n, generator=g)
    w = (w / w.sum(1, keepdim=True))
    idx, w = idx.cuda(), w.cuda()
    _, fa = _padded(B, c_a, m, pad, g)
    _, ft = _padded(B, max(c_t, 1), m, pad, g)
    _, fs = _padded(B, max(c_s, 1), n, pad, g)

    def run(form):
        big0, out0 = _padded(B, c_a + c_s, n, pad, g, fill=-3.0)
        big1, out1 = _padded(B, max(c_t, 1), n, pad, g, fill=-3.0)
        L.check(L.lib().bdm_fp_assemble_form(form, B, m, n, L.ptr(idx), L.ptr(w), c_a, L.ptr(fa), fa.stride(0), fa.stride(1),
                                             c_s, L.ptr(fs) if c_s else None, fs.stride(0), fs.stride(1),
                                             c_t, L.ptr(ft) if c_t else None, ft.stride(0), ft.stride(1),
                                             L.ptr(out0), out0.stride(0), out0.stride(1), L.ptr(out1) if c_t else None, out1.stride(0),
                                             out1.stride(1), L.stream()), "fp_assemble_form")
        return big0, big1

    ref0, ref1 = run(1)                   # the per-point kernel
    for form in (2, 0):                   # the staged kernel; the dispatcher's choice (by sizes: staged here)
        got0, got1 = run(form)
        assert torch.equal(got0, ref0) and torch.equal(got1, ref1)            # padding included: nothing written outside the views

    def interp(f):
        i = idx.long()
        t = [torch.gather(f, 2, i[:, k:k + 1].expand(-1, f.shape[1], -1)) * w[:, k:k + 1] for k in range(3)]
        return (t[0] + t[1]) + t[2]

    assert torch.equal(ref0[:, :c_a, :n], interp(fa))
    if c_s:
        assert torch.equal(ref0[:, c_a:c_a + c_s, :n], fs)
    if c_t:
        assert torch.equal(ref1[:, :c_t, :n], interp(ft))
    assert bool((ref0[:, c_a + c_s:] == -3.0).all()) and bool((ref0[:, :, n:] == -3.0).all())


def test_fp_assembly_falls_back_when_a_row_exceeds_the_lds_budget(ops):
    """m > 16384 floats: the dispatcher runs the per-point kernel, and the staged form refuses."""
    L = ops.L
    B, m, n, c = 1, 16388, 64, 2
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, m, (B, 3, n), generator=g).int().cuda()
    w = torch.rand(B, 3, n, generator=g).cuda()
    fa = torch.randn(B, c, m, generator=g).cuda()
    outs = []
    for form in (0, 1):
        out = torch.zeros(B, c, n, device="cuda")
        L.check(L.lib().bdm_fp_assemble_form(form, B, m, n, L.ptr(idx), L.ptr(w), c, L.ptr(fa), c * m, m, 0, None, 0, 0, 0, None, 0, 0,
                                             L.ptr(out), c * n, n, None, 0, 0, L.stream()), "fp_assemble_form")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool(outs[0].any())
    out = torch.zeros(B, c, n, device="cuda")
    assert L.lib().bdm_fp_assemble_form(2, B, m, n, L.ptr(idx), L.ptr(w), c, L.ptr(fa), c * m, m, 0, None, 0, 0, 0, None, 0, 0,
                                        L.ptr(out), c * n, n, None, 0, 0, L.stream()) != 0
