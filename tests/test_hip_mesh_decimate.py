"""bdm_mesh_cluster and bdm_mesh_decimate (csrc/mesh_decimate.hip) and their Python surface on the GPU against the CPU restatement
tests/mesh_decimate_ref.py: every output with torch.equal, floats compared as bits (a NaN equals any NaN), sentinels around every
output, the workspace pre-filled with 0xA5 and checked behind its end; the error paths; and the feature through Python, the three
command lines and two consumers.  Nothing here has a tolerance, and no case provokes a fault: the limit cases launch nothing.  The
launcher has one route, so there is no variant to pin the case table to."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_decimate_ref as R
import mesh_fill_ref as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
CONTRACTIONS = {"average": 0, "first": 1}
GRIDS = ("r4", "r16", "voxel")   # the batch runs at both resolutions and under one voxel size per mesh


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _ptr(whole):
    """The address of a guarded body, also of an empty one."""
    return whole.data_ptr() + PAD * whole.element_size()


class Packed:
    """The ABI's form of a list of (verts, faces, attrs) host meshes; attrs (V, C) float32."""

    def __init__(self, meshes, C):
        self.nv, self.nf = [v.shape[0] for v, _, _ in meshes], [f.shape[0] for _, f, _ in meshes]
        self.b, self.sum_v, self.sum_f, self.C = len(meshes), sum(self.nv), sum(self.nf), C
        self.verts = torch.cat([v for v, _, _ in meshes] + [torch.zeros(1, 3)]).float().cuda().contiguous()   # one unread row: never NULL
        self.attrs = torch.cat([a for _, _, a in meshes] + [torch.zeros(1, C)]).float().cuda().contiguous()
        if C == 0:
            self.attrs = torch.zeros(1, device="cuda")   # no channel: one unread word, never NULL
        self.faces = torch.cat([f for _, f, _ in meshes] + [torch.zeros(1, 3, dtype=torch.int64)]).int().cuda().contiguous()
        self.vert_first = torch.tensor([0] + self.nv, dtype=torch.int64).cumsum(0)
        self.face_first = torch.tensor([0] + self.nf, dtype=torch.int64).cumsum(0)


def _grid_args(grid):
    """dict(resolution=R) or dict(sizes=[..]) -> (resolution, the host float32 tensor or None)."""
    if "resolution" in grid:
        return grid["resolution"], None
    return 0, torch.tensor(grid["sizes"], dtype=torch.float64).float()


def _run(p, grid, contraction="average"):
    """Both calls on guarded outputs -> dict of host tensors; asserts what the calls left alone."""
    from bdm_amd import _lib as L
    lib = L.lib()
    nbytes = lib.bdm_mesh_decimate_workspace_bytes(p.b, p.sum_v, p.sum_f)
    assert nbytes >= 16 and nbytes % 16 == 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    resolution, sizes = _grid_args(grid)
    sp = None if sizes is None else sizes.data_ptr()
    bufs = {k: _guarded(n, torch.int32) for k, n in (("vert_map", p.sum_v), ("face_map", p.sum_f), ("counts", 8 * p.b))}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    rc = lib.bdm_mesh_cluster(p.b, resolution, sp, CONTRACTIONS[contraction], L.ptr(p.verts), L.ptr(p.faces), vf, ff,
                              *(_ptr(bufs[k][0]) for k in bufs), L.ptr(ws), L.stream())
    assert rc == 0, lib.bdm_last_error()
    counts = bufs["counts"][1].cpu().view(p.b, 8)   # the one read-back
    assert all(_untouched(w) for w, _ in bufs.values()) and bool((ws[-256:] == 0xA5).all()), "bdm_mesh_cluster wrote outside its outputs"
    ov = torch.tensor([0] + counts[:, 0].tolist(), dtype=torch.int64).cumsum(0)
    of = torch.tensor([0] + counts[:, 1].tolist(), dtype=torch.int64).cumsum(0)
    outs = {"verts": _guarded(3 * int(ov[-1]), torch.float32), "attrs": _guarded(p.C * int(ov[-1]), torch.float32),
            "faces": _guarded(3 * int(of[-1]), torch.int32)}
    rc = lib.bdm_mesh_decimate(p.b, resolution, sp, CONTRACTIONS[contraction], p.C, L.ptr(p.verts), L.ptr(p.attrs), L.ptr(p.faces), vf, ff,
                               ov.data_ptr(), of.data_ptr(), *(_ptr(outs[k][0]) for k in outs), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert all(_untouched(w) for w, _ in outs.values()) and bool((ws[-256:] == 0xA5).all()), "bdm_mesh_decimate wrote outside its outputs"
    got = {k: body.cpu() for k, (_, body) in {**bufs, **outs}.items()}
    assert int((got["verts"].view(torch.int32) == torch.tensor(F_SENTINEL).view(torch.int32)).sum()) == 0, "an output vertex was not written"
    assert int((got["faces"] == I_SENTINEL).sum()) == 0, "an output face was not written"
    got.update(counts=counts, out_vert_first=ov, out_face_first=of)
    return got


def _split(p, got):
    """Per mesh the dict tests compare with the restatement."""
    out = []
    for m in range(p.b):
        v0, v1, f0, f1 = (int(x[m + d]) for x in (p.vert_first, p.face_first) for d in (0, 1))
        ov0, ov1, of0, of1 = (int(got[k][m + d]) for k in ("out_vert_first", "out_face_first") for d in (0, 1))
        out.append({"vert_map": got["vert_map"][v0:v1], "face_map": got["face_map"][f0:f1], "counts": got["counts"][m].tolist(),
                    "verts": got["verts"].view(-1, 3)[ov0:ov1], "attrs": got["attrs"].view(-1, p.C)[ov0:ov1] if p.C else None,
                    "faces": got["faces"].view(-1, 3)[of0:of1]})
    return out


def _assert_mesh(g, r, C, what):
    """One mesh of the device against the restatement's dict."""
    assert g["counts"] == list(r["info"].values()), f"{what}: counts {g['counts']} != {r['info']}"
    assert torch.equal(g["vert_map"].long(), r["vert_map"]), f"{what}: vert_map"
    assert torch.equal(g["face_map"].long(), r["face_map"]), f"{what}: face_map"
    assert torch.equal(g["faces"].long(), r["faces"].long()), f"{what}: faces"
    assert R.same_floats(g["verts"], r["verts"]), f"{what}: vertices"
    if C:
        assert R.same_floats(g["attrs"], r["attrs"]), f"{what}: attributes"


def _inputs():
    return [(v, f, a) for _, v, f, a, _ in R.batch()]


def _grid(which):
    return {"r4": dict(resolution=4), "r16": dict(resolution=16), "voxel": dict(sizes=[h for *_, h in R.batch()])}[which]


@functools.lru_cache(maxsize=None)
def _refs(which, contraction):
    """The restatement of every mesh of the batch, computed once per grid and contraction."""
    out = []
    for _, v, f, a, h in R.batch():
        kw = dict(voxel_size=h) if which == "voxel" else _grid(which)
        out.append(R.decimate(v, f, contraction=contraction, attrs=a, **kw))
    return tuple(out)


@pytest.fixture(scope="module")
def whole(hip):
    """The ragged batch of every mesh of the tables, run once per grid and contraction."""
    p = Packed(_inputs(), 5)
    return p, {(which, c): _run(p, _grid(which), c) for which in GRIDS for c in CONTRACTIONS}


@pytest.mark.parametrize("contraction", list(CONTRACTIONS))
@pytest.mark.parametrize("which", GRIDS)
def test_batch_equals_the_restatement_bit_for_bit(whole, which, contraction):
    p, runs = whole
    names = [n for n, *_ in R.batch()]
    refs = _refs(which, contraction)
    for name, g, r in zip(names, _split(p, runs[(which, contraction)]), refs):
        _assert_mesh(g, r, 5, f"{name} at {which}, {contraction}")
    assert sum(r["info"]["merged_vertices"] for r in refs) > 1000 and sum(r["info"]["duplicate_faces"] for r in refs) > 5
    assert any(r["info"]["nonfinite_vertices"] for r in refs) and any(r["info"]["bad_faces"] for r in refs)
    if contraction == "average":
        merged = [torch.tensor([len(m) > 1 for m in r["clusters"]], dtype=torch.bool) for r in refs]
        assert any(bool(torch.isnan(r["attrs"][at, 4]).any()) for r, at in zip(refs, merged)), "no NaN channel among the averaged rows"
        assert any(bool(torch.isfinite(r["attrs"][at, 4]).any()) for r, at in zip(refs, merged)), "no finite mean in the channel with NaNs"


def test_first_contraction_returns_input_rows_and_singletons_keep_their_bits(whole):
    p, runs = whole
    for which in GRIDS:
        for (v, f, a), g, r in zip(_inputs(), _split(p, runs[(which, "first")]), _refs(which, "first")):
            lead = torch.tensor([m[0] for m in r["clusters"]], dtype=torch.int64)
            assert R.same_floats(g["verts"], v[lead]) and R.same_floats(g["attrs"], a[lead])
        for (v, f, a), g, r in zip(_inputs(), _split(p, runs[(which, "average")]), _refs(which, "average")):
            alone = torch.tensor([m[0] for m in r["clusters"] if len(m) == 1], dtype=torch.int64)
            at = torch.tensor([i for i, m in enumerate(r["clusters"]) if len(m) == 1], dtype=torch.int64)
            assert R.same_floats(g["verts"][at], v[alone]) and R.same_floats(g["attrs"][at], a[alone])


def test_every_mesh_alone_has_the_bits_it_has_in_the_batch_and_a_repeat_too(whole):
    p, runs = whole
    batch = _split(p, runs[("voxel", "average")])
    again = _split(p, _run(p, _grid("voxel"), "average"))
    sizes = _grid("voxel")["sizes"]
    for m, mesh in enumerate(_inputs()):
        one = Packed([mesh], 5)
        alone = _split(one, _run(one, dict(sizes=[sizes[m]]), "average"))[0]
        for other, what in ((alone, "alone"), (again[m], "repeated")):
            for k in ("vert_map", "face_map", "faces"):
                assert torch.equal(batch[m][k], other[k]), (m, what, k)
            assert batch[m]["counts"] == other["counts"], (m, what)
            assert R.same_floats(batch[m]["verts"], other["verts"]) and R.same_floats(batch[m]["attrs"], other["attrs"]), (m, what)
    r16 = _split(p, runs[("r16", "average")])
    for m in (0, len(batch) - 1, len(batch) - 2):   # by resolution too: h comes from the mesh's own bounds
        one = Packed([_inputs()[m]], 5)
        alone = _split(one, _run(one, dict(resolution=16), "average"))[0]
        assert torch.equal(r16[m]["vert_map"], alone["vert_map"]) and torch.equal(r16[m]["faces"], alone["faces"]) and R.same_floats(r16[m]["verts"], alone["verts"])


def test_5000_vertices_in_one_cell_contend_for_one_slot_and_one_sum(hip):
    """One cluster of 5000 (and three vertices apart): every insert meets on one slot, every member on one segment.  x lies in
    [1.8, 2) and nothing reaches 2: with E = 0, e = 39, its q are at least 0.9 * 2^40 and their sum, about 2^52.2, is above 2^52; y and
    z carry bits below 2^-39."""
    g = torch.Generator().manual_seed(5000)
    v = torch.rand(5003, 3, generator=g, dtype=torch.float64)
    v[:, 0] = 1.8 + 0.2 * v[:, 0]
    v[:, 1:] = v[:, 1:] * 1e-3
    v = v.float()
    v[5000:] = torch.tensor([[0.1, 0, 0], [0.1, 1.0, 0], [0.7, 1.0, 0.9]])   # lo = (0.1, 0, 0): the 5000 lie in cell (3, 0, 0) of size 0.5
    f = torch.randint(0, 5003, (300, 3), generator=g)
    a = torch.randn(5003, 2, generator=g) * 1e4
    p = Packed([(v, f, a)], 2)
    r = R.decimate(v, f, voxel_size=0.5, attrs=a)
    e = FR.scale_exp(v.numpy())
    assert r["info"]["largest_cluster"] == 5000 and r["info"]["new_vertices"] == 4 and e == 39 and sum(round(float(c) * 2.0 ** e) for c in v[:5000, 0].tolist()) > 2 ** 52
    _assert_mesh(_split(p, _run(p, dict(sizes=[0.5])))[0], r, 2, "one large cluster")
    _assert_mesh(_split(p, _run(p, dict(sizes=[0.5]), "first"))[0], R.decimate(v, f, voxel_size=0.5, attrs=a, contraction="first"), 2, "first")


def test_a_mesh_of_singletons_is_the_identity_at_the_tables_highest_load(hip):
    """3001 vertices, 3001 distinct keys in the 6003 slots of the mesh's region: the vertex table holds one key per vertex, its highest
    load, and with some 1500 probe runs a run over the region's last slot wraps to its first; every face set is its own."""
    v, f = R.surface_mesh("sphere600")
    g = torch.Generator().manual_seed(77)
    big_v = torch.cat([v, torch.rand(3001 - v.shape[0], 3, generator=g)])
    a = R.attrs_for(3001, 9)
    small = (torch.rand(5, 3, generator=g), torch.tensor([[0, 1, 2]]), R.attrs_for(5, 8))
    p = Packed([small, (big_v, f, a)], 5)
    got = _split(p, _run(p, dict(sizes=[1e-6, 1e-6])))
    for g_, (vv, ff, aa) in zip(got, [small, (big_v, f, a)]):
        assert torch.equal(g_["vert_map"].long(), torch.arange(vv.shape[0])) and torch.equal(g_["face_map"].long(), torch.arange(ff.shape[0]))
        assert R.same_floats(g_["verts"], vv) and R.same_floats(g_["attrs"], aa) and torch.equal(g_["faces"].long(), ff)
        assert g_["counts"] == [vv.shape[0], ff.shape[0], 0, 0, 0, 0, 1, 0]
    _assert_mesh(got[1], R.decimate(big_v, f, voxel_size=1e-6, attrs=a), 5, "singletons")


@pytest.mark.parametrize("merge", [False, True])
def test_scans_of_more_than_256_partial_sums_carry(hip, merge):
    """mesh_fill_ref.separate_triangles(87 400) with 10 unused vertices, every face four times: the vertex-rank and member-segment scans
    run over 262 211 entries (257 partial sums) and the face scan over 349 601 (342).  Under a voxel size of 1 nothing merges on one set
    of coordinates (only the first copy of every face stays) and every triangle collapses into one vertex on the other.  Expected
    values: R.grid_triangles' closed form, held against the restatement at 64 triangles by tests/test_mesh_decimate_host.py; the merged
    vertices, on a sample of the clusters, by the fixed-point mean."""
    n = 87400
    v, f, want = R.grid_triangles(n, 10, 50, merge)
    V = v.shape[0]
    assert -(-(V + 1) // 1024) == 257 and -(-(4 * n + 1) // 1024) == 342
    p = Packed([(v, f, torch.zeros(V, 0))], 0)
    g = _split(p, _run(p, dict(sizes=[1.0])))[0]
    assert g["counts"] == list(want["info"].values())
    assert torch.equal(g["vert_map"].long(), want["vert_map"]), "vert_map"
    assert torch.equal(g["face_map"].long(), want["face_map"]), "face_map"
    assert torch.equal(g["faces"].long(), want["faces"]), "faces"
    if not merge:
        assert R.same_floats(g["verts"], v), "vertices"
        return
    assert g["verts"].shape == (n + 10, 3)
    e, vn, tri = FR.scale_exp(v.numpy()), v.numpy(), f[:n]
    for t in sorted({0, 1, n // 2, n - 1, *range(0, n, 997)}):
        members = tri[t].tolist()
        mean = torch.tensor([float(FR.fixed_mean(vn[members, d], e)) for d in range(3)])
        assert R.same_floats(g["verts"][int(want["vert_map"][members[0]])], mean), f"the vertex of triangle {t}"
    unused = torch.nonzero(want["cell_of"] >= n).flatten()
    assert R.same_floats(g["verts"][want["vert_map"][unused]], v[unused])


@pytest.mark.parametrize("large_first", (False, True))
def test_16_channels_with_a_nonfinite_member_in_the_last_and_per_mesh_magnitudes_2_to_the_20_apart(hip, large_first):
    """c = 16 is the last channel the shared accumulator (csrc/mesh_emit.h) holds, and the attributes' largest magnitude of mesh m lives
    at stride 8 in the per-mesh statistics.  The cube of cube_r2, flattened along z so that a voxel size of 0.5 merges it into four
    clusters of two, twice: channel 15 has one non-finite member (its cluster's channel 15 is NaN, every other mean is finite) and the
    second copy's attributes are 2^20 times the first's: a mean under the other mesh's fixed point, in either order, has other bits."""
    v, f, _ = R.hand_meshes()["cube_r2"]
    v = v * torch.tensor([1.0, 1.0, 0.4])
    a = torch.randn(8, 16, generator=torch.Generator().manual_seed(2016)) * 3.0
    small, large = a.clone(), a * 2.0 ** 20
    small[5, 15], large[5, 15] = float("nan"), float("-inf")
    meshes = [(v, f, large), (v, f, small)] if large_first else [(v, f, small), (v, f, large)]
    p = Packed(meshes, 16)
    for m, (g, (v_, f_, a_)) in enumerate(zip(_split(p, _run(p, dict(sizes=[0.5, 0.5]))), meshes)):
        r = R.decimate(v_, f_, voxel_size=0.5, attrs=a_)
        assert r["info"]["new_vertices"] == 4 and r["info"]["largest_cluster"] == 2 and r["info"]["merged_vertices"] == 8
        assert torch.isnan(r["attrs"][:, 15]).tolist() == [False, True, False, False] and bool(torch.isfinite(r["attrs"][:, :15]).all())
        _assert_mesh(g, r, 16, f"mesh {m} of two at 16 channels")


def test_33_meshes_cross_the_launch_boundary_of_the_offsets_upload(hip):
    """b + 1 = 34 offsets (and 33 cell sizes) are one launch more than the 32 a launch carries: a wrong entry of the second launch
    mis-addresses mesh 32 or gives it another cell.  Squashed cubes and the two-triangle mesh in turn, mesh 16 empty."""
    g = torch.Generator().manual_seed(331)
    hand = R.hand_meshes()
    meshes, sizes = [], []
    for i in range(33):
        v, f, _ = hand["two_triangles" if i % 2 else "cube_r2"]
        meshes.append((v * (1.0 + 0.01 * i), f, torch.rand(v.shape[0], 1, generator=g)))
        sizes.append(0.3 + 0.05 * i)
    meshes[16] = (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 1))
    p = Packed(meshes, 1)
    assert p.b == 33
    refs = [R.decimate(v, f, voxel_size=float(np.float32(s)), attrs=a) for (v, f, a), s in zip(meshes, sizes)]
    assert len({tuple(r["info"].values()) for r in refs}) > 3
    for m, (g_, r) in enumerate(zip(_split(p, _run(p, dict(sizes=sizes))), refs)):
        _assert_mesh(g_, r, 1, f"mesh {m} of 33")
    for m, (g_, (v, f, a)) in enumerate(zip(_split(p, _run(p, dict(resolution=3))), meshes)):
        _assert_mesh(g_, R.decimate(v, f, resolution=3, attrs=a), 1, f"mesh {m} of 33 by resolution")


def test_every_documented_limit_returns_1_and_leaves_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    p = Packed(_inputs()[:8], 5)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.bdm_mesh_decimate_workspace_bytes(p.b, p.sum_v, p.sum_f) <= ws.numel()
    bufs = {k: _guarded(n, torch.int32) for k, n in (("vert_map", p.sum_v), ("face_map", p.sum_f), ("counts", 8 * p.b), ("faces_out", 3 * p.sum_f))}
    bufs["verts_out"], bufs["attrs_out"] = _guarded(3 * p.sum_v, torch.float32), _guarded(5 * p.sum_v, torch.float32)
    o = {k: L.ptr(body) for k, (_, body) in bufs.items()}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    down = p.vert_first.clone()
    down[2] = down[1] - 1
    late = p.vert_first + 1
    huge = torch.full((p.b + 1,), 1 << 31, dtype=torch.int64)
    huge[0] = 0
    wide = torch.full((p.b + 1,), 1 << 21, dtype=torch.int64).cumsum(0) - (1 << 21)   # every mesh 2^21 vertices
    many = torch.full((p.b + 1,), 715827883, dtype=torch.int64)
    many[0] = 0
    good = torch.full((p.b,), 0.5)
    sizes = {k: good.clone() for k in ("zero", "neg", "nan", "inf")}
    sizes["zero"][3], sizes["neg"][0], sizes["nan"][7], sizes["inf"][1] = 0.0, -1.0, float("nan"), float("inf")
    bad = [dict(vert_first=None), dict(vert_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(vert_first=huge.data_ptr()),
           dict(vert_first=wide.data_ptr()), dict(b=-1), dict(b=65536), dict(ws=None), dict(ws=L.ptr(ws) + 8), dict(face_first=None),
           dict(face_first=down.data_ptr()), dict(face_first=late.data_ptr()), dict(face_first=many.data_ptr()), dict(verts=None), dict(faces=None),
           dict(resolution=0), dict(resolution=-4), dict(resolution=1025), dict(contraction=2), dict(contraction=-1), dict(voxel=good.data_ptr()),
           *(dict(resolution=0, voxel=s.data_ptr()) for s in sizes.values())]
    cluster = dict(b=p.b, resolution=8, voxel=None, contraction=0, verts=L.ptr(p.verts), faces=L.ptr(p.faces), vert_first=vf, face_first=ff,
                   vert_map=o["vert_map"], face_map=o["face_map"], counts=o["counts"], ws=L.ptr(ws), stream=L.stream())
    for change in bad + [dict(vert_map=None), dict(face_map=None), dict(counts=None), dict(vert_map=L.ptr(p.faces)), dict(face_map=o["vert_map"]),
                         dict(counts=L.ptr(p.verts)), dict(ws=o["face_map"]), dict(ws=L.ptr(p.faces))]:
        assert lib.bdm_mesh_cluster(*dict(cluster, **change).values()) == 1 and lib.bdm_last_error(), change
    r = _refs("r16", "average")[:8]
    ov = torch.tensor([0] + [x["info"]["new_vertices"] for x in r], dtype=torch.int64).cumsum(0)
    of = torch.tensor([0] + [x["info"]["new_faces"] for x in r], dtype=torch.int64).cumsum(0)
    more_v, none_v, more_f, few_v = p.vert_first.clone(), ov.clone(), p.face_first.clone(), ov.clone()
    more_v[1:] += 1                # more vertices out than in
    none_v[1:] -= int(ov[1])       # the first mesh, of eight vertices, left with none
    more_f[1:] += 1                # more faces out than in
    few_v[1:] -= int(ov[1]) - 2    # the first mesh keeps its faces on two vertices
    dec = dict(b=p.b, resolution=16, voxel=None, contraction=0, c=5, verts=L.ptr(p.verts), attrs=L.ptr(p.attrs), faces=L.ptr(p.faces), vert_first=vf,
               face_first=ff, out_vert_first=ov.data_ptr(), out_face_first=of.data_ptr(), verts_out=o["verts_out"], attrs_out=o["attrs_out"],
               faces_out=o["faces_out"], ws=L.ptr(ws), stream=L.stream())
    assert int(ov[1]) == 8 and int(of[1]) == 12
    for change in bad + [dict(c=-1), dict(c=17), dict(attrs=None), dict(out_vert_first=None), dict(out_face_first=None), dict(verts_out=None),
                         dict(attrs_out=None), dict(faces_out=None), dict(out_vert_first=more_v.data_ptr()), dict(out_vert_first=none_v.data_ptr()),
                         dict(out_face_first=more_f.data_ptr()), dict(out_vert_first=few_v.data_ptr()), dict(out_vert_first=down.data_ptr()),
                         dict(verts_out=L.ptr(p.verts)), dict(attrs_out=o["verts_out"]), dict(faces_out=L.ptr(p.faces)), dict(ws=o["faces_out"]),
                         dict(ws=L.ptr(p.attrs))]:
        assert lib.bdm_mesh_decimate(*dict(dec, **change).values()) == 1 and lib.bdm_last_error(), change
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    # nothing to do: 0, and nothing is touched
    assert lib.bdm_mesh_cluster(*dict(cluster, b=0, verts=None, vert_first=None).values()) == 0
    assert lib.bdm_mesh_decimate(*dict(dec, b=0, faces=None, ws=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()) and bool((ws == 0xA5).all())
    wb = lib.bdm_mesh_decimate_workspace_bytes
    assert wb(-1, 10, 10) == 0 and wb(65536, 10, 10) == 0 and wb(1, 1 << 31, 1) == 0 and wb(1, 10, 715827883) == 0 and wb(1, -1, 1) == 0
    assert wb(1, 10, 10) > 0


# ---- through Python -------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_restatement(hip):
    from bdm_amd import mesh_decimate as MD
    from bdm_amd.cameras import Meshes
    rows = list(R.batch())
    verts, faces = [v.cuda() for _, v, *_ in rows], [f.cuda() for _, _, f, *_ in rows]
    u8 = [FR.colors_for(v.shape[0], i)[0] for i, (_, v, *_) in enumerate(rows)]
    fl = [FR.colors_for(v.shape[0], i)[1] for i, (_, v, *_) in enumerate(rows)]
    refs = [R.decimate(v, f, resolution=16, attrs=c.float()) for (_, v, f, *_), c in zip(rows, u8)]
    vm, fm, info = MD.cluster_vertices(Meshes(verts, faces), resolution=16)
    for a, b, i, r in zip(vm, fm, info, refs):
        assert a.dtype == torch.int64 and a.is_cuda and torch.equal(a.cpu(), r["vert_map"]) and torch.equal(b.cpu(), r["face_map"]) and i == r["info"]
    ov, of, oc, info = MD.simplify_vertex_clustering(Meshes(verts, faces), resolution=16, colors_list=[c.cuda() for c in u8], return_info=True)
    for m, (r, c) in enumerate(zip(refs, u8)):
        assert info[m] == r["info"] and torch.equal(of[m].cpu(), r["faces"]) and of[m].dtype == torch.int64 and R.same_floats(ov[m].cpu(), r["verts"])
        want = torch.tensor([[FR.uint8_mean(c[mem, ch].tolist()) for ch in range(3)] for mem in r["clusters"]], dtype=torch.uint8).reshape(-1, 3)
        assert oc[m].dtype == torch.uint8 and torch.equal(oc[m].cpu(), want), f"uint8 colours of mesh {m}"
    # float colours, one voxel size per mesh, "first", the pair form, no info
    sizes = [h for *_, h in rows]
    refs_v = [R.decimate(v, f, voxel_size=h, attrs=c, contraction="first") for (_, v, f, _, h), c in zip(rows, fl)]
    ov, of, oc = MD.simplify_vertex_clustering((verts, faces), voxel_size=sizes, contraction="first", colors_list=[c.cuda() for c in fl])
    for m, r in enumerate(refs_v):
        assert R.same_floats(ov[m].cpu(), r["verts"]) and torch.equal(of[m].cpu(), r["faces"]) and R.same_floats(oc[m].cpu(), r["attrs"])
    ov, of = MD.simplify_vertex_clustering((verts[-2:], faces[-2:]), voxel_size=0.07)
    for a, b, (_, v, f, *_) in zip(ov, of, rows[-2:]):
        r = R.decimate(v, f, voxel_size=0.07)
        assert R.same_floats(a.cpu(), r["verts"]) and torch.equal(b.cpu(), r["faces"])
    with pytest.raises(Exception, match="CPU tensor"):
        MD.simplify_vertex_clustering(([rows[0][1]], [rows[0][2]]), resolution=4)
    assert MD.simplify_vertex_clustering(([], []), resolution=4, return_info=True) == ([], [], [])


def test_decimated_meshes_are_meshes_the_scorer_and_the_rasteriser_take(hip):
    """The surface meshes at R = 16 through point_mesh_sqdist and rasterize_meshes, each against its own restatement."""
    import mesh_metrics_ref as MM
    import mesh_render_ref as MR
    from bdm_amd import mesh_decimate as MD
    from bdm_amd.cameras import Meshes
    from bdm_amd.mesh_metrics import point_mesh_sqdist
    from bdm_amd.render import rasterize_meshes
    meshes = [R.surface_mesh(n) for n in R.SURFACE_MESHES]
    ov, of = MD.simplify_vertex_clustering(([v.cuda() for v, _ in meshes], [f.cuda() for _, f in meshes]), resolution=16)
    hv, hf = [v.cpu() for v in ov], [f.cpu() for f in of]
    for (v, f), a, b in zip(meshes, hv, hf):
        r = R.decimate(v, f, resolution=16)
        assert R.same_floats(a, r["verts"]) and torch.equal(b, r["faces"])
    pts = torch.stack([MM.cloud(257, 5), MM.cloud(257, 6)]) * 0.5
    sq, idx = point_mesh_sqdist((ov, of), pts.cuda())
    want = MM.distance_batch(hv, hf, pts)
    assert R.same_floats(sq.cpu(), want["sqdist"]) and torch.equal(idx.cpu().int(), want["face_idx"]) and bool((idx >= 0).all())
    cam = MR._persp(2)
    frag = rasterize_meshes(cam.to("cuda"), Meshes(ov, of), image_size=48)
    ref = MR.render_batch(hv, hf, cam.packed(), 48, 48)
    assert torch.equal(frag.pix_to_face[..., 0].cpu().int(), ref["pix_to_face"].int()) and torch.equal(frag.zbuf[..., 0].cpu(), ref["zbuf"])
    assert torch.equal(frag.bary_coords[:, :, :, 0].cpu(), ref["bary"]) and int((ref["pix_to_face"] >= 0).sum()) > 200


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    """Two files: the sphere with colours, the torus without."""
    from bdm_amd.io import save_mesh_ply
    sv, sf = R.surface_mesh("sphere600")
    tv, tf = R.surface_mesh("torus1500")
    colours = (torch.arange(sv.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "a" / "sphere.ply", colors=colours.numpy())
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "mesh" / "b" / "torus.ply")
    return (sv, sf, colours), (tv, tf)


def _load(path):
    from bdm_amd.io import load_mesh_ply
    from bdm_amd.surface import mesh_stats
    v, f, c = load_mesh_ply(path, with_colors=True)
    return mesh_stats(torch.from_numpy(v), torch.from_numpy(f)), v, f, c


def _colours_as_saved(attrs):
    """save_mesh_ply's conversion, in float64, and load_mesh_ply's back."""
    return np.rint(np.clip(attrs.numpy().astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8).astype(np.float32) / np.float32(255.0)


@pytest.mark.parametrize("grid", [("--resolution", "16"), ("--voxel-size", "0.05", "--contraction", "first")])
def test_cli_decimates_a_tree_and_prints_the_composed_json(hip, tmp_path, grid):
    from bdm_amd import mesh_decimate as MD
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_decimate", "--mesh_dir", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "out"),
                          *grid], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    kw = dict(resolution=16) if grid[0] == "--resolution" else dict(voxel_size=float(np.float32(0.05)), contraction="first")
    rs, rt = R.decimate(sv, sf, attrs=colours, **kw), R.decimate(tv, tf, **kw)
    sums = {k: max(rs["info"][k], rt["info"][k]) if k == "largest_cluster" else rs["info"][k] + rt["info"][k] for k in R.INFO_KEYS}
    s_in, t_in = _load(tmp_path / "mesh" / "a" / "sphere.ply")[0], _load(tmp_path / "mesh" / "b" / "torus.ply")[0]
    (s_out, ov, of, oc), (t_out, tov, tof, toc) = _load(tmp_path / "out" / "a" / "sphere.ply"), _load(tmp_path / "out" / "b" / "torus.ply")
    assert got == MD.compose_result(2, sums, sv.shape[0] + tv.shape[0], sf.shape[0] + tf.shape[0], sums["new_vertices"], sums["new_faces"],
                                    s_in["edges"] + t_in["edges"], s_in["open_edges"] + t_in["open_edges"],
                                    s_out["edges"] + t_out["edges"], s_out["open_edges"] + t_out["open_edges"])
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy())
    assert np.array_equal(tov.view(np.int32), rt["verts"].numpy().view(np.int32)) and np.array_equal(tof, rt["faces"].numpy()) and toc is None
    assert np.array_equal(oc, _colours_as_saved(rs["attrs"])), "the colours are carried along"


def test_mesh_clean_cli_decimates_between_holes_and_smoothing(hip, tmp_path):
    from bdm_amd import mesh_clean as MC
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    base = [sys.executable, "-m", "bdm_amd.mesh_clean", "--mesh_dir", str(tmp_path / "mesh"), "--taubin-iters", "0", "--min-fraction", "0",
            "--min-faces", "0"]   # nothing is removed, not even the vertices no face uses: the files of "off" hold the input meshes
    runs = {}
    for name, extra in (("off", ["--decimate-resolution", "0"]), ("on", ["--decimate-resolution", "16"])):
        out = subprocess.run(base + ["--out_dir", str(tmp_path / name)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        runs[name] = json.loads(out.stdout.strip().splitlines()[-1])
        print(out.stdout.strip().splitlines()[-1])
    assert list(runs["off"]) == list(MC.compose_result(*[0] * 7))
    rs, rt = R.decimate(sv, sf, resolution=16, attrs=colours), R.decimate(tv, tf, resolution=16)
    keys = ["decimate_" + k for k in R.INFO_KEYS]
    assert list(runs["on"]) == list(runs["off"]) + keys
    for k in R.INFO_KEYS:
        both = (rs["info"][k], rt["info"][k])
        assert runs["on"]["decimate_" + k] == (max(both) if k == "largest_cluster" else sum(both)), k
    assert runs["on"]["vertices_out"] == rs["verts"].shape[0] + rt["verts"].shape[0] and runs["on"]["faces_out"] == rs["faces"].shape[0] + rt["faces"].shape[0]
    assert runs["off"]["vertices_out"] == sv.shape[0] + tv.shape[0]
    (_, ov, of, oc), (_, tov, tof, toc) = _load(tmp_path / "on" / "a" / "sphere.ply"), _load(tmp_path / "on" / "b" / "torus.ply")
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy())
    assert np.array_equal(oc, _colours_as_saved(rs["attrs"]))
    assert np.array_equal(tov.view(np.int32), rt["verts"].numpy().view(np.int32)) and np.array_equal(tof, rt["faces"].numpy()) and toc is None
