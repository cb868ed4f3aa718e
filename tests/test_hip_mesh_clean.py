"""bdm_mesh_adjacency, bdm_mesh_components_* and bdm_mesh_taubin (csrc/mesh_clean.hip) and their Python surface on the GPU against the
CPU restatement tests/mesh_clean_ref.py: every output with torch.equal, floats compared as bits (a NaN equals any NaN: which NaN an
operation returns is not part of the rule), sentinels around every output, the workspace pre-filled with 0xA5 and checked behind its
end; the error paths; and the feature through Python and the command line.  Nothing here has a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clean_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _ptr(whole):
    """The address of a guarded body, also of an empty one (torch gives an empty view no address; the ABI takes no NULL)."""
    return whole.data_ptr() + PAD * whole.element_size()


def _addr(t):
    """The address of a device tensor; an empty one (a batch without faces has no neighbour entries) gets that of an unread word."""
    if "word" not in _UNREAD:
        _UNREAD["word"] = torch.zeros(1, dtype=torch.int32, device="cuda")   # kept alive: its address stays its own
    return t.data_ptr() if t.numel() else _UNREAD["word"].data_ptr()


_UNREAD = {}


def _workspace(nbytes):
    assert nbytes >= 16 and nbytes % 16 == 0
    return torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")


def _behind(ws):
    return bool((ws[-256:] == 0xA5).all())


class Packed:
    """The ABI's form of a list of (verts, faces) host meshes."""

    def __init__(self, meshes):
        self.nv, self.nf = [v.shape[0] for v, _ in meshes], [f.shape[0] for _, f in meshes]
        self.b, self.sum_v, self.sum_f = len(meshes), sum(self.nv), sum(self.nf)
        self.verts = torch.cat([v for v, _ in meshes] + [torch.zeros(1, 3)]).float().cuda().contiguous()       # one unread row: never NULL
        self.faces = torch.cat([f for _, f in meshes] + [torch.zeros(1, 3, dtype=torch.int64)]).int().cuda().contiguous()
        self.vert_first = torch.tensor([0] + self.nv, dtype=torch.int64).cumsum(0)
        self.face_first = torch.tensor([0] + self.nf, dtype=torch.int64).cumsum(0)


def _adjacency(p):
    """One bdm_mesh_adjacency call on guarded outputs -> (nbr_first, nbr whole upper bound) on the device; asserts what the call left alone."""
    from bdm_amd import _lib as L
    lib = L.lib()
    ws = _workspace(lib.bdm_mesh_adjacency_workspace_bytes(p.b, p.sum_v, p.sum_f))
    fw, first = _guarded(p.sum_v + 1, torch.int32)
    nw, nbr = _guarded(6 * p.sum_f, torch.int32)
    rc = lib.bdm_mesh_adjacency(p.b, L.ptr(p.faces), p.vert_first.data_ptr(), p.face_first.data_ptr(), L.ptr(first), _ptr(nw), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert _untouched(fw) and _untouched(nw) and _behind(ws), "bdm_mesh_adjacency wrote outside its outputs"
    total = int(first[-1])
    assert bool((nbr[total:] == I_SENTINEL).all()), "nbr past nbr_first[sum V] was written"
    return first, nbr


def _components(p, first, nbr, rounds):
    """init, rounds until the flag clears, finish -> (dict of host outputs, calls)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    ws = _workspace(lib.bdm_mesh_components_workspace_bytes(p.b, p.sum_v))
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    assert lib.bdm_mesh_components_init(p.b, vf, ff, L.ptr(ws), L.stream()) == 0, lib.bdm_last_error()
    cw, changed = _guarded(1, torch.int32)
    calls = 0
    while True:
        assert lib.bdm_mesh_components_rounds(p.b, rounds, vf, ff, L.ptr(first), _addr(nbr), L.ptr(changed), L.ptr(ws), L.stream()) == 0, lib.bdm_last_error()
        calls += 1
        flag = int(changed.item())
        assert flag in (0, 1)
        if flag == 0:
            break
        assert calls * rounds <= max(p.nv) + 1, "the labels still change after V rounds"
    bufs = {"vert_comp": _guarded(p.sum_v, torch.int32), "face_comp": _guarded(p.sum_f, torch.int32), "comp_count": _guarded(p.b, torch.int32),
            "comp_verts": _guarded(p.sum_v, torch.int32), "comp_faces": _guarded(p.sum_v, torch.int32)}
    rc = lib.bdm_mesh_components_finish(p.b, L.ptr(p.faces), vf, ff, *(_ptr(bufs[k][0]) for k in bufs), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert all(_untouched(w) for w, _ in bufs.values()) and _untouched(cw) and _behind(ws), "the components calls wrote outside their outputs"
    return {k: body.cpu() for k, (_, body) in bufs.items()}, calls


def _taubin(p, first, nbr, num_iter, mode, lambd=R.LAMBD, mu=R.MU):
    from bdm_amd import _lib as L
    lib = L.lib()
    ws = _workspace(lib.bdm_mesh_taubin_workspace_bytes(p.b, p.sum_v))
    ow, out = _guarded(3 * p.sum_v, torch.float32)
    rc = lib.bdm_mesh_taubin(p.b, num_iter, mode, lambd, mu, L.ptr(p.verts), p.vert_first.data_ptr(), L.ptr(first), _addr(nbr), L.ptr(out), L.ptr(ws),
                             L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert _untouched(ow) and _behind(ws), "bdm_mesh_taubin wrote outside its output"
    return list(out.view(-1, 3).cpu().split(p.nv))


def _meshes():
    return [(v, f) for _, v, f in R.batch()]


def _assert_adjacency(p, first, nbr, refs, what):
    first, nbr = first.cpu(), nbr.cpu()
    for m, c in enumerate(refs):
        lo, hi = int(p.vert_first[m]), int(p.vert_first[m + 1])
        seg = first[lo:hi + 1]
        assert torch.equal(seg - seg[0], c["first"]), f"{what}: nbr_first of mesh {m}"
        assert torch.equal(nbr[int(seg[0]):int(seg[-1])], c["nbr"]), f"{what}: nbr of mesh {m}"


def _assert_components(p, got, refs, what):
    for m, c in enumerate(refs):
        lo, hi, flo, fhi = int(p.vert_first[m]), int(p.vert_first[m + 1]), int(p.face_first[m]), int(p.face_first[m + 1])
        C = c["comp_verts"].numel()
        assert int(got["comp_count"][m]) == C, f"{what}: comp_count of mesh {m}"
        assert torch.equal(got["vert_comp"][lo:hi].long(), c["vert_comp"]) and torch.equal(got["face_comp"][flo:fhi].long(), c["face_comp"]), f"{what}: mesh {m}"
        for k in ("comp_verts", "comp_faces"):
            assert torch.equal(got[k][lo:lo + C].long(), c[k]) and int(got[k][lo + C:hi].abs().sum()) == 0, f"{what}: {k} of mesh {m}"
        assert int(got["comp_verts"][lo:hi].sum()) == hi - lo and int(got["comp_faces"][lo:hi].sum()) == int((c["face_comp"] >= 0).sum())


# ---- adjacency and components ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(hip):
    """The ragged batch through adjacency and components (8 rounds per call), once for the module."""
    p = Packed(_meshes())
    first, nbr = _adjacency(p)
    comps, calls = _components(p, first, nbr, 8)
    return p, first, nbr, comps, calls


def test_ragged_batch_equals_the_restatement(hip, whole):
    p, first, nbr, comps, calls = whole
    refs = R.batch_components()
    print(f"{p.b} meshes, {p.sum_v} vertices, {p.sum_f} faces, {int(first[-1])} neighbour entries, {calls} calls of 8 rounds")
    _assert_adjacency(p, first, nbr, refs, "batch")
    _assert_components(p, comps, refs, "batch")


@pytest.mark.parametrize("rounds", (1, 2, 8))
def test_any_round_count_per_call_gives_the_same_components_and_the_loop_repeats(hip, whole, rounds):
    """The rounds are Jacobi rounds, so their number is the restatement's: R rounds change a label (352 on the shuffled strip of 1025
    vertices), round R + 1 changes none, and the call whose last round is the first such one clears the flag."""
    p, first, nbr, comps, _ = whole
    got, calls = _components(p, first, nbr, rounds)
    need = max(c["rounds"] for c in R.batch_components())
    print(f"{rounds} rounds per call: {calls} calls for {need} changing rounds")
    assert need > 8 and calls > 1 and calls == -(-(need + 1) // rounds)
    assert all(torch.equal(got[k], comps[k]) for k in comps)


def test_every_mesh_alone_has_its_bits_of_the_batch_and_calls_repeat(hip, whole):
    p, first, nbr, comps, _ = whole
    again_first, again_nbr = _adjacency(p)
    assert torch.equal(again_first, first) and torch.equal(again_nbr, nbr)
    refs = R.batch_components()
    for m, mesh in enumerate(_meshes()):
        if mesh[0].shape[0] == 0:
            continue   # sum V == 0: the call launches nothing (its own test)
        q = Packed([mesh])
        f1, n1 = _adjacency(q)
        _assert_adjacency(q, f1, n1, refs[m:m + 1], f"mesh {m} alone")
        got, _ = _components(q, f1, n1, 8)
        _assert_components(q, got, refs[m:m + 1], f"mesh {m} alone")


# ---- smoothing ------------------------------------------------------------------------------------------------------------------------
def _assert_floats(got, want, what):
    for m, (g, w) in enumerate(zip(got, want)):
        assert R.same_floats(g, w), f"{what}, mesh {m}: {int((R.bits(g) != R.bits(w)).sum())} of {g.numel()} values differ"


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("num_iter", (0, 1, 10))
def test_smoothing_equals_the_restatement(hip, whole, mode, num_iter):
    p, first, nbr, _, _ = whole
    got = _taubin(p, first, nbr, num_iter, mode)
    _assert_floats(got, R.batch_taubin(mode, num_iter), f"mode {mode}, {num_iter} iterations")
    m = [n for n, _, _ in R.batch()].index("triangles_200_unused_10")
    ref_first = R.batch_components()[m]["first"]
    iso = ref_first[1:] == ref_first[:-1]
    assert int(iso.sum()) == 10 and torch.equal(R.bits(got[m][iso]), R.bits(R.batch()[m][1][iso]))   # an isolated vertex keeps its bits
    if num_iter == 10:   # the island mesh alone has its bits of the batch
        q = Packed([_meshes()[-1]])
        f1, n1 = _adjacency(q)
        _assert_floats(_taubin(q, f1, n1, num_iter, mode), got[-1:], "the island mesh alone")
    if num_iter == 0:
        _assert_floats(got, [v for v, _ in _meshes()], "num_iter == 0 copies")


def test_smoothing_special_inputs(hip):
    for name, (v, f), iters in (("coincident", R.coincident_mesh(), 1), ("nan", R.nan_mesh(), 1), ("nan", R.nan_mesh(), 2)):
        p = Packed([(v, f)])
        first, nbr = _adjacency(p)
        rf, rn = R.adjacency(f, v.shape[0])
        for mode in (0, 1):
            got = _taubin(p, first, nbr, iters, mode)[0]
            assert R.same_floats(got, R.taubin(v, rf, rn, num_iter=iters, mode=mode)), (name, iters, mode)
            if name == "coincident":
                assert bool(torch.isfinite(got).all())
            elif iters == 1:
                assert bool(torch.isnan(got).any(1).all())   # lambd reaches the hub, mu the whole rim
    # half an iteration's spread is visible with mu = 0: the second half-step is then the identity on finite rows
    v, f = R.nan_mesh()
    p = Packed([(v, f)])
    first, nbr = _adjacency(p)
    got = _taubin(p, first, nbr, 1, 0, 0.53, 0.0)[0]
    rf, rn = R.adjacency(f, v.shape[0])
    assert R.same_floats(got, R.taubin(v, rf, rn, 0.53, 0.0, 1, 0))
    # other factors
    v, f = R.island_mesh()
    p = Packed([(v, f)])
    first, nbr = _adjacency(p)
    rf, rn = R.adjacency(f, v.shape[0])
    for lambd, mu in ((0.33, -0.331), (1.0, 0.0), (-0.25, 0.7)):
        assert R.same_floats(_taubin(p, first, nbr, 3, 0, lambd, mu)[0], R.taubin(v, rf, rn, lambd, mu, 3, 0)), (lambd, mu)


def test_33_meshes_cross_the_launch_boundary_of_the_offsets_upload(hip):
    """b + 1 = 34 offsets are one launch more than the 32 a launch carries (csrc/ragged.hip): a wrong or missing entry of the second
    launch mis-addresses mesh 32.  Meshes of one triangle and of two triangles on a common side in turn, mesh 16 empty.
    bdm_mesh_adjacency sends both offset arrays, bdm_mesh_taubin the vertex offsets and no face offsets."""
    g = torch.Generator().manual_seed(330)
    one, two = torch.tensor([[0, 1, 2]]), torch.tensor([[0, 1, 2], [2, 1, 3]])
    meshes = [(torch.rand(3 + i % 2, 3, generator=g), two if i % 2 else one) for i in range(33)]
    meshes[16] = (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
    p = Packed(meshes)
    assert p.b == 33
    first, nbr = _adjacency(p)
    refs = [dict(zip(("first", "nbr"), R.adjacency(f, v.shape[0]))) for v, f in meshes]
    _assert_adjacency(p, first, nbr, refs, "33 meshes")
    for mode in (0, 1):
        want = [R.taubin(v, c["first"], c["nbr"], num_iter=1, mode=mode) for (v, _), c in zip(meshes, refs)]
        _assert_floats(_taubin(p, first, nbr, 1, mode), want, f"33 meshes, mode {mode}")


def test_scan_of_more_than_256_partial_sums_carries_into_its_second_trip(hip):
    """The scan's middle launch is one workgroup of 256 threads that walks the partial sums (one per 1024 entries) 256 at a time and
    carries the total along.  87 400 separate triangles and 10 unused vertices are 262 210 vertices: the sum V + 1 = 262 211 entries of
    both scans of bdm_mesh_adjacency (the entry count comes from the host) have 257 partial sums, one more than a trip takes."""
    v, f = R.separate_triangles(87400, 10, 50)
    p = Packed([(v, f)])
    assert -(-(p.sum_v + 1) // 1024) == 257
    first, nbr = _adjacency(p)
    _assert_adjacency(p, first, nbr, [dict(zip(("first", "nbr"), R.adjacency(f, v.shape[0])))], "262 210 vertices")
    assert int(first[-1]) == 6 * 87400


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_every_documented_limit_returns_1_and_leaves_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    p = Packed(_meshes()[:7])
    first, nbr = _adjacency(p)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {k: _guarded(n, torch.int32) for k, n in (("first", p.sum_v + 1), ("nbr", 6 * p.sum_f), ("changed", 1), ("vert_comp", p.sum_v),
                                                      ("face_comp", p.sum_f), ("comp_count", p.b), ("comp_verts", p.sum_v), ("comp_faces", p.sum_v))}
    bufs["out"] = _guarded(3 * p.sum_v, torch.float32)
    o = {k: L.ptr(body) for k, (_, body) in bufs.items()}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    down = p.vert_first.clone()
    down[2] = down[1] - 1
    late = p.vert_first + 1
    huge = torch.full((p.b + 1,), 1 << 31, dtype=torch.int64)
    huge[0] = 0
    many = torch.full((p.b + 1,), 357913942, dtype=torch.int64)
    many[0] = 0
    bad_offsets = [dict(vert_first=None), dict(vert_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(vert_first=huge.data_ptr()),
                   dict(b=-1), dict(b=65536), dict(ws=None), dict(ws=L.ptr(ws) + 8)]
    bad_faces_offsets = [dict(face_first=None), dict(face_first=down.data_ptr()), dict(face_first=late.data_ptr()), dict(face_first=many.data_ptr())]
    adj = dict(b=p.b, faces=L.ptr(p.faces), vert_first=vf, face_first=ff, first=o["first"], nbr=o["nbr"], ws=L.ptr(ws), stream=L.stream())
    for change in bad_offsets + bad_faces_offsets + [dict(faces=None), dict(first=None), dict(nbr=None), dict(first=L.ptr(p.faces)), dict(nbr=o["first"]),
                                                      dict(ws=o["nbr"]), dict(ws=L.ptr(p.faces))]:
        assert lib.bdm_mesh_adjacency(*dict(adj, **change).values()) == 1 and lib.bdm_last_error(), change
    init = dict(b=p.b, vert_first=vf, face_first=ff, ws=L.ptr(ws), stream=L.stream())
    for change in bad_offsets + bad_faces_offsets:
        assert lib.bdm_mesh_components_init(*dict(init, **change).values()) == 1, change
    rnd = dict(b=p.b, rounds=2, vert_first=vf, face_first=ff, first=L.ptr(first), nbr=L.ptr(nbr), changed=o["changed"], ws=L.ptr(ws), stream=L.stream())
    for change in bad_offsets + bad_faces_offsets + [dict(rounds=0), dict(rounds=-3), dict(first=None), dict(nbr=None), dict(changed=None),
                                                      dict(changed=L.ptr(first)), dict(ws=L.ptr(nbr)), dict(ws=o["changed"])]:
        assert lib.bdm_mesh_components_rounds(*dict(rnd, **change).values()) == 1, change
    fin = dict(b=p.b, faces=L.ptr(p.faces), vert_first=vf, face_first=ff, vert_comp=o["vert_comp"], face_comp=o["face_comp"], comp_count=o["comp_count"],
               comp_verts=o["comp_verts"], comp_faces=o["comp_faces"], ws=L.ptr(ws), stream=L.stream())
    for change in bad_offsets + bad_faces_offsets + [dict(faces=None), dict(vert_comp=None), dict(face_comp=None), dict(comp_count=None), dict(comp_verts=None),
                                                      dict(comp_faces=None), dict(vert_comp=L.ptr(p.faces)), dict(comp_faces=o["comp_verts"]),
                                                      dict(ws=o["vert_comp"])]:
        assert lib.bdm_mesh_components_finish(*dict(fin, **change).values()) == 1, change
    tau = dict(b=p.b, num_iter=2, mode=0, lambd=0.53, mu=-0.34, verts=L.ptr(p.verts), vert_first=vf, first=L.ptr(first), nbr=L.ptr(nbr), out=o["out"],
               ws=L.ptr(ws), stream=L.stream())
    for change in bad_offsets + [dict(num_iter=-1), dict(num_iter=10001), dict(mode=2), dict(mode=-1), dict(lambd=float("nan")), dict(mu=float("inf")),
                                 dict(verts=None), dict(first=None), dict(nbr=None), dict(out=None), dict(out=L.ptr(p.verts)), dict(out=L.ptr(first)),
                                 dict(ws=o["out"]), dict(ws=L.ptr(p.verts))]:
        assert lib.bdm_mesh_taubin(*dict(tau, **change).values()) == 1 and lib.bdm_last_error(), change
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    # nothing to do: 0, and nothing is touched (not even NULL pointers are looked at)
    zero = torch.zeros(p.b + 1, dtype=torch.int64)
    assert lib.bdm_mesh_adjacency(*dict(adj, b=0, faces=None, vert_first=None).values()) == 0
    assert lib.bdm_mesh_adjacency(*dict(adj, vert_first=zero.data_ptr(), face_first=zero.data_ptr(), ws=None).values()) == 0
    assert lib.bdm_mesh_components_init(*dict(init, b=0, ws=None).values()) == 0
    assert lib.bdm_mesh_components_rounds(*dict(rnd, vert_first=zero.data_ptr(), face_first=zero.data_ptr(), changed=None).values()) == 0
    assert lib.bdm_mesh_components_finish(*dict(fin, b=0, faces=None).values()) == 0
    assert lib.bdm_mesh_taubin(*dict(tau, vert_first=zero.data_ptr(), out=None, ws=None).values()) == 0
    assert lib.bdm_mesh_taubin(*dict(tau, b=0, verts=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()) and bool((ws == 0xA5).all())
    wb = lib.bdm_mesh_adjacency_workspace_bytes
    assert wb(-1, 10, 10) == 0 and wb(65536, 10, 10) == 0 and wb(1, 1 << 31, 1) == 0 and wb(1, 10, 357913942) == 0 and wb(1, -1, 1) == 0
    assert lib.bdm_mesh_components_workspace_bytes(65536, 1) == 0 and lib.bdm_mesh_taubin_workspace_bytes(1, 1 << 31) == 0
    assert lib.bdm_mesh_taubin_workspace_bytes(3, 10) == 64 + 320


# ---- through Python -------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_restatement(hip, whole):
    from bdm_amd import mesh_clean as MC
    from bdm_amd.cameras import Meshes
    from bdm_amd.surface import mesh_stats
    p, first, nbr, _, _ = whole
    verts, faces = [v.cuda() for v, _ in _meshes()], [f.cuda() for _, f in _meshes()]
    pf, pn = MC.vertex_adjacency(Meshes(verts, faces))
    total = int(first[-1])
    assert torch.equal(pf, first) and torch.equal(pn[:total], nbr[:total]) and bool((pn[total:] == -1).all()) and pn.numel() == 6 * p.sum_f
    for got, c in zip(MC.connected_components((verts, faces)), R.batch_components()):
        assert all(g.dtype == torch.int64 and g.is_cuda for g in got)
        assert all(torch.equal(g.cpu(), c[k]) for g, k in zip(got, ("vert_comp", "face_comp", "comp_verts", "comp_faces")))
    v, f = R.island_mesh()
    colours = torch.rand(v.shape[0], 3, generator=torch.Generator().manual_seed(5))
    ov, of, oc, info = MC.remove_small_components(([v.cuda()], [f.cuda()]), colors_list=[colours.cuda()], return_info=True)
    rv, rf = R.remove_small(v, f)
    assert torch.equal(ov[0].cpu(), rv) and torch.equal(of[0].cpu(), rf) and torch.equal(oc[0].cpu(), colours[R.components(f, 1210)["vert_comp"] == 0])
    assert info == [{"components": 2, "removed_components": 1, "removed_vertices": 76, "removed_faces": 148}]
    assert mesh_stats(ov[0], of[0])["euler_characteristic"] == 2
    for weights, mode in MC.WEIGHTS.items():
        sm = MC.taubin_smoothing(Meshes(verts, faces), weights=weights)
        assert isinstance(sm, Meshes) and all(a is b for a, b in zip(sm.faces_list(), faces))
        _assert_floats([x.cpu() for x in sm.verts_list()], _taubin(p, first, nbr, 10, mode), f"taubin_smoothing({weights})")
    sm = MC.taubin_smoothing((verts[-1:], faces[-1:]), 0.4, -0.41, 3)
    q = Packed(_meshes()[-1:])
    f1, n1 = _adjacency(q)
    _assert_floats([sm.verts_list()[0].cpu()], _taubin(q, f1, n1, 3, 0, 0.4, -0.41), "taubin_smoothing with its own factors")


def test_cli_cleans_a_tree_and_prints_the_composed_json(hip, tmp_path):
    """python -m bdm_amd.mesh_clean in a child process on a two-file tree, one file with colours: the JSON line is the one composed by
    hand from the restatement, and the files carry the restatement's vertices, faces and colours."""
    from bdm_amd import mesh_clean as MC
    from bdm_amd.io import load_mesh_ply, save_mesh_ply
    v, f = R.island_mesh()
    tv, tf = R.two_spheres_mesh()
    colours = (torch.arange(v.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(v.numpy(), f.numpy(), tmp_path / "mesh" / "a" / "island.ply", colors=colours.numpy())
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "mesh" / "b" / "two.ply")
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_clean", "--mesh_dir", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "out"),
                          "--taubin-iters", "3", "--weights", "uniform"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    rv, rf = R.remove_small(v, f)
    assert got == MC.compose_result(2, 1210 + tv.shape[0], 2412 + tf.shape[0], 1134 + tv.shape[0], 2264 + tf.shape[0], 4, 1)
    first, nbr = R.adjacency(rf, rv.shape[0])
    ov, of, oc = load_mesh_ply(tmp_path / "out" / "a" / "island.ply", with_colors=True)
    assert np.array_equal(ov, R.taubin(rv, first, nbr, num_iter=3, mode=1).numpy()) and np.array_equal(of, rf.numpy())
    assert np.array_equal(oc, colours[R.components(f, 1210)["vert_comp"] == 0].numpy())
    first, nbr = R.adjacency(tf, tv.shape[0])
    ov, of, oc = load_mesh_ply(tmp_path / "out" / "b" / "two.ply", with_colors=True)
    assert oc is None and np.array_equal(ov, R.taubin(tv, first, nbr, num_iter=3, mode=1).numpy()) and np.array_equal(of, tf.numpy())
