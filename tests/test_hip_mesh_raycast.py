"""bdm_mesh_bvh_keys / bdm_mesh_bvh_build / bdm_mesh_raycast / bdm_mesh_raycast_exhaustive (csrc/mesh_bvh.hip, csrc/mesh_raycast.hip)
and their Python surface on the GPU against the CPU restatement tests/mesh_raycast_ref.py: every output with torch.equal, sentinels
around every output, the workspaces and the hierarchy buffer pre-filled with 0xA5 and checked behind their end; the error paths; and
the feature through Python and the command line.  Nothing here has a tolerance, and no case provokes a fault: the limit cases launch
nothing."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_raycast_ref as R
import mesh_voxel_ref as VR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
SENTINEL = {torch.uint8: 0xEE, torch.int32: -7777, torch.float32: -7777.0, torch.int64: -7777}
OUT_TYPES = {"t": (torch.float32, 1), "face": (torch.int32, 1), "bary": (torch.float32, 2), "back": (torch.uint8, 1), "occluded": (torch.uint8, 1),
             "crossings": (torch.int32, 1)}
OF_MODE = {"closest": ("t", "face", "bary", "back"), "any": ("occluded",), "count": ("crossings",)}
NODE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("link", "<i4"), ("skip", "<i4")])


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == SENTINEL[whole.dtype]).all())


class Packed:
    """The ABI's form of a list of (verts, faces, rays) host rows."""

    def __init__(self, rows):
        self.nv, self.nf, self.nr = [v.shape[0] for v, _, _ in rows], [f.shape[0] for _, f, _ in rows], [r.shape[0] for _, _, r in rows]
        self.b, self.sum_v, self.sum_f, self.sum_r = len(rows), sum(self.nv), sum(self.nf), sum(self.nr)
        self.verts = torch.cat([v for v, _, _ in rows] + [torch.zeros(1, 3)]).float().cuda().contiguous()   # one unread row: never NULL
        self.faces = torch.cat([f for _, f, _ in rows] + [torch.zeros(1, 3, dtype=torch.int64)]).int().cuda().contiguous()
        self.rays = torch.cat([torch.from_numpy(r) for _, _, r in rows] + [torch.zeros(1, 8)]).float().cuda().contiguous()
        self.vert_first = torch.tensor([0] + self.nv, dtype=torch.int64).cumsum(0)
        self.face_first = torch.tensor([0] + self.nf, dtype=torch.int64).cumsum(0)
        self.ray_first = torch.tensor([0] + self.nr, dtype=torch.int64).cumsum(0)

    def mesh_args(self):
        from bdm_amd import _lib as L
        return (self.b, L.ptr(self.verts), L.ptr(self.faces), self.vert_first.data_ptr(), self.face_first.data_ptr())


def _build(p):
    """Both build calls on guarded buffers with a stable torch.sort between them -> (the hierarchy buffer, counts (b, 2) host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    nbytes, ws_bytes = lib.bdm_mesh_bvh_bytes(p.b, p.sum_f), lib.bdm_mesh_bvh_workspace_bytes(p.b, p.sum_v, p.sum_f)
    assert nbytes >= 16 and nbytes % 16 == 0 and ws_bytes >= 16 and ws_bytes % 16 == 0
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bvh = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    keys_whole, keys = _guarded(max(p.sum_f, 1), torch.int64)
    counts_whole, counts = _guarded(2 * p.b, torch.int32)
    rc = lib.bdm_mesh_bvh_keys(*p.mesh_args(), L.ptr(keys), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert _untouched(keys_whole) and bool((ws[-256:] == 0xA5).all()), "bdm_mesh_bvh_keys wrote outside its outputs"
    if p.sum_f:
        skeys, order = torch.sort(keys[:p.sum_f], stable=True)
    else:
        skeys, order = keys.clone(), torch.zeros(1, dtype=torch.int64, device="cuda")
    ws.fill_(0xA5)   # the contents are irrelevant before each call
    rc = lib.bdm_mesh_bvh_build(*p.mesh_args(), L.ptr(skeys.contiguous()), L.ptr(order.contiguous()), L.ptr(counts), L.ptr(bvh), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert _untouched(counts_whole) and bool((ws[-256:] == 0xA5).all()) and bool((bvh[-256:] == 0xA5).all()), "bdm_mesh_bvh_build wrote outside its outputs"
    return bvh, counts.cpu().view(p.b, 2)


def _trees(p, bvh):
    """The device buffer read back in the restatement's form: one dict per mesh."""
    raw = bvh.cpu().numpy()
    head = raw[:16 * p.b].view("<i4").reshape(p.b, 4)
    nodes = raw[16 * p.b:16 * p.b + 32 * 2 * max(p.sum_f, 1)].view(NODE)
    out = []
    for m in range(p.b):
        n, base = int(head[m, 0]), 2 * int(p.face_first[m])
        assert head[m, 2] == 0 and head[m, 3] == 0 and 0 <= n <= p.nf[m]
        part = nodes[base:base + max(2 * n - 1, 0)]
        out.append({"n": n, "dropped": int(head[m, 1]), "lo": part["lo"].copy(), "hi": part["hi"].copy(), "link": part["link"].astype(np.int64),
                    "skip": part["skip"].astype(np.int64)})
    return out


def _run(p, mode, bvh=None, outputs=None):
    """One query on guarded outputs -> dict of host tensors; bvh None: the exhaustive form.  outputs: the per-ray outputs that are not
    NULL (default: all six); asserts that everything the mode does not write, and everything behind an end, is left alone."""
    from bdm_amd import _lib as L
    lib = L.lib()
    outputs = tuple(OUT_TYPES) if outputs is None else outputs
    ws_bytes = lib.bdm_mesh_raycast_workspace_bytes(p.b)
    assert ws_bytes >= 16 and ws_bytes % 16 == 0
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {k: _guarded(max(p.sum_r, 1) * w, ty) for k, (ty, w) in OUT_TYPES.items()}
    bufs["counts"] = _guarded(5 * p.b, torch.int32)
    ptrs = [L.ptr(bufs[k][1]) if k in outputs else None for k in OUT_TYPES]
    head = (R.MODES[mode], *p.mesh_args())
    tail = (L.ptr(p.rays), p.ray_first.data_ptr(), *ptrs, L.ptr(bufs["counts"][1]), L.ptr(ws), L.stream())
    if bvh is None:
        rc = lib.bdm_mesh_raycast_exhaustive(*head, *tail)
    else:
        before = bvh.clone()
        rc = lib.bdm_mesh_raycast(*head, L.ptr(bvh), *tail)
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert all(_untouched(w) for w, _ in bufs.values()) and bool((ws[-256:] == 0xA5).all()), "a query wrote outside its outputs"
    assert bvh is None or torch.equal(bvh, before), "a query wrote to the hierarchy"
    for k in OUT_TYPES:
        if k not in OF_MODE[mode] or k not in outputs:
            assert _untouched(bufs[k][0], body=True), f"{k} is not an output of this call and was written"
        else:
            assert not bool((bufs[k][1][:p.sum_r * OUT_TYPES[k][1]] == SENTINEL[OUT_TYPES[k][0]]).any()), f"{k}: a row was not written"
    got = {k: bufs[k][1].cpu()[:p.sum_r * OUT_TYPES[k][1]] for k in OF_MODE[mode] if k in outputs}
    if "bary" in got:
        got["bary"] = got["bary"].view(-1, 2)
    got["counts"] = bufs["counts"][1].cpu().view(p.b, 5)
    return got


def _assert_mesh(got, p, m, ref, mode, what):
    lo, hi = int(p.ray_first[m]), int(p.ray_first[m + 1])
    assert got["counts"][m].tolist() == list(ref["counts"]), f"{what}: counts {got['counts'][m].tolist()} != {ref['counts']}"
    for k in OF_MODE[mode]:
        want = torch.from_numpy(np.asarray(ref[k]))
        assert torch.equal(got[k][lo:hi], want), f"{what}: {k}, {int((got[k][lo:hi] != want).sum())} entries differ"


@functools.lru_cache(maxsize=None)
def _packed_batch():
    return Packed([(v, f, rays) for _, v, f, rays in R.batch()])


@pytest.fixture(scope="module")
def packed(hip):
    return _packed_batch()


@pytest.fixture(scope="module")
def built(packed):
    return _build(packed)


def test_the_built_hierarchy_keeps_the_invariants_of_the_host_test(packed, built):
    bvh, counts = built
    rows = R.batch()
    for m, ((name, v, f, _), tree, ref) in enumerate(zip(rows, _trees(packed, bvh), R.references())):
        assert counts[m].tolist() == [ref["counts"][3], ref["counts"][4]] == [tree["n"], tree["dropped"]], name
        depth = R.check_tree(tree, v, f)
        assert depth <= 2 * max(int(np.ceil(np.log2(max(tree["n"], 1)))), 1) + 2, (name, depth)
    again, counts2 = _build(packed)
    assert torch.equal(again[:-256], bvh[:-256]) and torch.equal(counts2, counts), "a repeated build differs"


@pytest.mark.parametrize("mode", list(R.MODES))
def test_tree_and_exhaustive_equal_the_restatement_bit_for_bit(packed, built, mode):
    tree, flat = _run(packed, mode, built[0]), _run(packed, mode)
    for k in tree:
        assert torch.equal(tree[k], flat[k]), f"{mode}: the tree changes {k}"
    for m, ((name, *_), ref) in enumerate(zip(R.batch(), R.references())):
        _assert_mesh(tree, packed, m, ref, mode, f"{name}, {mode}, tree")
        _assert_mesh(flat, packed, m, ref, mode, f"{name}, {mode}, exhaustive")
    again = _run(packed, mode, built[0])
    for k in tree:
        assert torch.equal(tree[k], again[k]), f"{mode}: a repeat changes {k}"


def test_every_mesh_alone_has_the_bits_it_has_in_the_batch(packed, built):
    whole = {mode: _run(packed, mode, built[0]) for mode in R.MODES}
    for m, (name, v, f, rays) in enumerate(R.batch()):
        p = Packed([(v, f, rays)])
        bvh, _ = _build(p)
        lo, hi = int(packed.ray_first[m]), int(packed.ray_first[m + 1])
        for mode in R.MODES:
            for form in (bvh, None):
                alone = _run(p, mode, form)
                assert torch.equal(alone["counts"][0], whole[mode]["counts"][m]), (name, mode)
                for k in OF_MODE[mode]:
                    assert torch.equal(alone[k], whole[mode][k][lo:hi]), (name, mode, k)


def test_null_outputs_are_skipped_and_the_others_keep_their_bits(packed, built):
    full = _run(packed, "closest", built[0])
    for outputs in (("t",), ("face", "back"), ("bary", "occluded"), ()):
        for form in (built[0], None):
            part = _run(packed, "closest", form, outputs=outputs)
            assert torch.equal(part["counts"], full["counts"])
            for k in outputs:
                if k in full:
                    assert torch.equal(part[k], full[k]), (outputs, k)
    for mode in ("any", "count"):
        assert torch.equal(_run(packed, mode, built[0], outputs=())["counts"], full["counts"])


def test_33_meshes_cross_the_launch_boundary_of_the_offsets_upload(hip):
    """b + 1 = 34 offsets are one launch more than the 32 a launch carries, for the vertices, the faces and the rays; mesh 16 is empty and
    mesh 20 has no rays."""
    ov, of = VR.octahedron()
    bv, bf = VR.box((0.3, 0.2, 0.1), (5.1, 6.3, 7.2))
    rows = []
    for i in range(33):
        v, f = (ov, of) if i % 2 else (bv, bf)
        v = v * (1.0 + 0.01 * i)
        rows.append((v, f, R.random_rays(v, 5 + i % 7, 900 + i)))
    rows[16] = (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), R.random_rays(ov, 3, 7))
    rows[20] = (rows[20][0], rows[20][1], np.zeros((0, 8), dtype=np.float32))
    p = Packed(rows)
    bvh, _ = _build(p)
    refs = [R.exhaustive(v, f, r) for v, f, r in rows]
    assert sum(r["counts"][2] for r in refs) > 50 and refs[32]["counts"][2] > 0
    for mode in R.MODES:
        tree, flat = _run(p, mode, bvh), _run(p, mode)
        for m, ref in enumerate(refs):
            _assert_mesh(tree, p, m, ref, mode, f"mesh {m} of 33, tree")
            _assert_mesh(flat, p, m, ref, mode, f"mesh {m} of 33, exhaustive")


def test_every_documented_limit_returns_1_and_leaves_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    p = Packed([(v, f, rays) for _, v, f, rays in R.batch()[8:12]])
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    bvh = torch.full((lib.bdm_mesh_bvh_bytes(p.b, p.sum_f),), 0xA5, dtype=torch.uint8, device="cuda")
    assert 0 < lib.bdm_mesh_bvh_workspace_bytes(p.b, p.sum_v, p.sum_f) <= ws.numel() and 0 < lib.bdm_mesh_raycast_workspace_bytes(p.b) <= ws.numel()
    bufs = {k: _guarded(p.sum_r * w, ty) for k, (ty, w) in OUT_TYPES.items()}
    bufs.update(counts=_guarded(5 * p.b, torch.int32), keys=_guarded(p.sum_f, torch.int64), order=_guarded(p.sum_f, torch.int64))
    o = {k: L.ptr(body) for k, (_, body) in bufs.items()}
    down = p.vert_first.clone()
    down[2] = down[1] - 1
    late = p.vert_first + 1
    huge = torch.full((p.b + 1,), 1 << 31, dtype=torch.int64)
    huge[0] = 0
    many = torch.full((p.b + 1,), 715827883, dtype=torch.int64)
    many[0] = 0
    mesh = dict(b=p.b, verts=L.ptr(p.verts), faces=L.ptr(p.faces), vert_first=p.vert_first.data_ptr(), face_first=p.face_first.data_ptr())
    bad_mesh = [dict(b=-1), dict(b=65536), dict(verts=None), dict(faces=None), dict(vert_first=None), dict(face_first=None),
                dict(vert_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(vert_first=huge.data_ptr()), dict(face_first=down.data_ptr()),
                dict(face_first=late.data_ptr()), dict(face_first=many.data_ptr()), dict(ws=None), dict(ws=L.ptr(ws) + 8), dict(ws=L.ptr(p.verts))]
    keys_call = dict(mesh, keys=o["keys"], ws=L.ptr(ws), stream=L.stream())
    for change in bad_mesh + [dict(keys=None), dict(keys=L.ptr(p.faces))]:
        assert lib.bdm_mesh_bvh_keys(*dict(keys_call, **change).values()) == 1 and lib.bdm_last_error(), change
    build_call = dict(mesh, keys=o["keys"], order=o["order"], counts=o["counts"], bvh=L.ptr(bvh), ws=L.ptr(ws), stream=L.stream())
    for change in bad_mesh + [dict(keys=None), dict(order=None), dict(counts=None), dict(bvh=None), dict(bvh=L.ptr(bvh) + 4), dict(bvh=L.ptr(p.verts)),
                              dict(counts=o["keys"]), dict(ws=L.ptr(bvh))]:
        assert lib.bdm_mesh_bvh_build(*dict(build_call, **change).values()) == 1 and lib.bdm_last_error(), change
    rays_down = p.ray_first.clone()
    rays_down[1] = rays_down[2] + 1
    ray_call = dict(mode=0, **mesh, bvh=L.ptr(bvh), rays=L.ptr(p.rays), ray_first=p.ray_first.data_ptr(), **{k: o[k] for k in OUT_TYPES},
                    counts=o["counts"], ws=L.ptr(ws), stream=L.stream())
    bad_rays = [dict(mode=-1), dict(mode=3), dict(rays=None), dict(rays=L.ptr(p.rays) + 4), dict(ray_first=None), dict(ray_first=rays_down.data_ptr()),
                dict(ray_first=(p.ray_first + 1).data_ptr()), dict(ray_first=huge.data_ptr()), dict(counts=None), dict(t=L.ptr(p.verts)),
                dict(face=o["t"]), dict(occluded=o["back"]), dict(counts=L.ptr(p.rays)), dict(ws=o["bary"])]
    for change in bad_mesh + bad_rays + [dict(bvh=None), dict(bvh=L.ptr(bvh) + 8), dict(crossings=L.ptr(bvh))]:
        assert lib.bdm_mesh_raycast(*dict(ray_call, **change).values()) == 1 and lib.bdm_last_error(), change
    flat_call = {k: v for k, v in ray_call.items() if k != "bvh"}
    for change in bad_mesh + bad_rays:
        assert lib.bdm_mesh_raycast_exhaustive(*dict(flat_call, **change).values()) == 1 and lib.bdm_last_error(), change
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()) and bool((bvh == 0xA5).all()), "a refused call wrote to the workspace or the hierarchy"
    nothing = dict(b=0, verts=None, vert_first=None, ws=None)   # nothing to do: 0, nothing touched
    assert lib.bdm_mesh_bvh_keys(*dict(keys_call, **nothing).values()) == 0 and lib.bdm_mesh_bvh_build(*dict(build_call, **nothing).values()) == 0
    assert lib.bdm_mesh_raycast(*dict(ray_call, **nothing).values()) == 0 and lib.bdm_mesh_raycast_exhaustive(*dict(flat_call, **nothing).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()) and bool((ws == 0xA5).all()) and bool((bvh == 0xA5).all())
    nb, wb, rb = lib.bdm_mesh_bvh_bytes, lib.bdm_mesh_bvh_workspace_bytes, lib.bdm_mesh_raycast_workspace_bytes
    assert nb(-1, 10) == 0 and nb(65536, 10) == 0 and nb(1, -1) == 0 and nb(1, 715827883) == 0 and nb(1, 10) > 0 and nb(65535, 0) > 0
    assert wb(-1, 10, 10) == 0 and wb(65536, 10, 10) == 0 and wb(1, 1 << 31, 1) == 0 and wb(1, 10, 715827883) == 0 and wb(1, -1, 1) == 0 and wb(1, 10, 10) > 0
    assert rb(-1) == 0 and rb(65536) == 0 and rb(65535) > 0 and rb(1) > 0


# ---- through Python -------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_restatement_in_both_ray_forms(hip):
    from bdm_amd import mesh_raycast as MR
    from bdm_amd.cameras import Meshes
    names = [n for n, *_ in R.batch()]
    pick = [names.index(k) for k in ("octahedron", "empty", "lattice_box", "bad")]
    rows, refs = [R.batch()[i] for i in pick], [R.references()[i] for i in pick]
    verts, faces = [v.cuda() for _, v, _, _ in rows], [f.cuda() for _, _, f, _ in rows]
    o = [torch.from_numpy(r[:, 0:3]).cuda() for *_, r in rows]
    d = [torch.from_numpy(r[:, 3:6]).cuda() for *_, r in rows]
    lo, hi = [torch.from_numpy(r[:, 6]).cuda() for *_, r in rows], [torch.from_numpy(r[:, 7]).cuda() for *_, r in rows]
    bvh = MR.build_bvh(Meshes(verts, faces))
    assert bvh.counts["faces_dropped"].tolist() == [r["counts"][4] for r in refs] and len(bvh) == 4
    for target, exhaustive in ((bvh, False), (bvh, True), ((verts, faces), False), (Meshes(verts, faces), True)):
        hits = MR.cast_rays(target, o, d, lo, hi, exhaustive=exhaustive)
        occ = MR.test_occlusions(target, o, d, lo, hi, exhaustive=exhaustive)
        cnt = MR.count_intersections(target, o, d, lo, hi, exhaustive=exhaustive)
        for m, ref in enumerate(refs):
            assert torch.equal(hits.t[m].cpu(), torch.from_numpy(ref["t"])) and torch.equal(hits.face_idx[m].cpu(), torch.from_numpy(ref["face"])), m
            assert torch.equal(hits.bary[m].cpu(), torch.from_numpy(ref["bary"])) and torch.equal(hits.back[m].cpu(), torch.from_numpy(ref["back"]).bool()), m
            assert torch.equal(occ[m].cpu(), torch.from_numpy(ref["occluded"]).bool()) and torch.equal(cnt[m].cpu(), torch.from_numpy(ref["crossings"])), m
            assert [int(hits.counts[k][m]) for k in R.COUNT_KEYS] == ref["counts"], m
    # the padded form, numbers for tmin and tmax
    rays = R.random_rays(rows[0][1], 50, 77)
    pv, pf = [rows[0][1].cuda(), rows[2][1].cuda()], [rows[0][2].cuda(), rows[2][2].cuda()]
    po = torch.from_numpy(rays[:, 0:3]).cuda()[None].repeat(2, 1, 1)
    pd = torch.from_numpy(rays[:, 3:6]).cuda()[None].repeat(2, 1, 1)
    hits = MR.cast_rays((pv, pf), po, pd, 0.25, 40.0)
    assert hits.t.shape == (2, 50) and hits.bary.shape == (2, 50, 2) and hits.back.dtype == torch.bool
    rays[:, 6], rays[:, 7] = 0.25, 40.0
    for m, k in enumerate((0, 2)):
        ref = R.exhaustive(rows[k][1], rows[k][2], rays)
        assert torch.equal(hits.t[m].cpu(), torch.from_numpy(ref["t"])) and torch.equal(hits.face_idx[m].cpu(), torch.from_numpy(ref["face"])), m


def test_ambient_occlusion_is_exactly_one_on_convex_meshes_and_zero_inside_a_box(hip):
    from bdm_amd import mesh_raycast as MR
    ov, of = VR.octahedron()
    sv, sf = VR.uv_sphere(24, 48)
    bv, bf = VR.box((0.3, 0.2, 0.1), (5.1, 6.3, 7.2))
    ao, info = MR.vertex_ambient_occlusion(([ov.cuda(), sv.cuda(), bv.cuda()], [of.cuda(), sf.cuda(), bf[:, [0, 2, 1]].cuda()]), return_info=True)
    assert [a.shape[0] for a in ao] == [6, sv.shape[0], 8] and all(a.dtype == torch.float32 for a in ao)
    assert torch.equal(ao[0].cpu(), torch.ones(6)) and torch.equal(ao[1].cpu(), torch.ones(sv.shape[0]))
    assert torch.equal(ao[2].cpu(), torch.zeros(8))
    assert info["rays"] == 32 * (6 + sv.shape[0] + 8) and info["occluded"] == 32 * 8 and int(info["faces_dropped"].sum()) == 0
    near = MR.vertex_ambient_occlusion(([bv.cuda()], [bf[:, [0, 2, 1]].cuda()]), num_samples=16, max_distance=1e-5)   # the lift is 1e-3: no wall that near
    assert torch.equal(near[0].cpu(), torch.ones(8))


def test_crossing_parity_equals_the_voxeliser_on_a_box_with_integer_corners(hip):
    """Rays along +x from the cell centres of an 8^3 grid (origin 0, cell 1): the centres sit on half-integers and every edge of the box
    (1, 2, 1) .. (6, 5, 7) on integers, so no ray touches an edge and the parity of the crossings is the voxeliser's grid at every
    cell.  (lattice_box itself has its corners ON cell centres: the rays through them touch edges, which is the over-count the rule
    documents; it is asserted beside it.)"""
    from bdm_amd import mesh_raycast as MR
    from bdm_amd.mesh_voxel import voxelize_meshes
    v, f = VR.box((1, 2, 1), (6, 5, 7))
    lv, lf = VR.lattice_box()
    c = torch.arange(8, dtype=torch.float32) + 0.5
    centres = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3).cuda()
    along = torch.tensor([1.0, 0.0, 0.0], device="cuda").expand(512, 3).contiguous()
    meshes = ([v.cuda(), lv.cuda()], [f.cuda(), lf.cuda()])
    crossings = MR.count_intersections(meshes, [centres, centres], [along, along])
    grid = voxelize_meshes(meshes, 8, origin=(0, 0, 0), cell_size=1.0, mode="x")
    assert torch.equal((crossings[0] & 1).bool().view(8, 8, 8), grid[0]) and int(grid[0].sum()) == 5 * 3 * 6
    ref = R.exhaustive(lv, lf, R._rays(centres.cpu().numpy(), [(1, 0, 0)]))
    assert torch.equal(crossings[1].cpu(), torch.from_numpy(ref["crossings"])) and int(crossings[1].max()) > 2   # through edges and diagonals


def test_points_visible_on_a_sphere_from_five_radii(hip):
    from bdm_amd import mesh_raycast as MR
    from bdm_amd.cameras import Meshes
    v, f = VR.uv_sphere(24, 48)
    centre, radius = torch.tensor([0.013, -0.021, 0.034]), 0.4
    eye = centre + 5 * radius * torch.tensor([0.6, 0.48, 0.64])
    n = Meshes([v], [f]).verts_normals_packed()
    to_eye = eye[None] - v
    c = (n * (to_eye / to_eye.norm(dim=1, keepdim=True))).sum(dim=1)
    assert float((c.abs() < 0.2).sum()) / v.shape[0] <= 0.30
    meshes = ([v.cuda()], [f.cuda()])
    seen = MR.points_visible(meshes, [v.cuda()], eyes=eye[None].cuda())[0].cpu()
    assert seen.dtype == torch.bool and bool(seen[c >= 0.2].all()) and not bool(seen[c <= -0.2].any())
    towards = (eye - centre)[None]
    parallel = MR.points_visible(MR.build_bvh(meshes), [v.cuda()], directions=towards.cuda())[0].cpu()
    cp = (n * (towards / towards.norm())).sum(dim=1)
    assert bool(parallel[cp >= 0.2].all()) and not bool(parallel[cp <= -0.2].any())


def test_camera_rays_hit_what_the_rasteriser_draws(hip):
    """The closest hits of the 48 x 48 pixel rays on the GPU are those of the restatement, which the host test compares with the
    rasteriser's restatement."""
    import mesh_render_ref as RR
    from bdm_amd import mesh_raycast as MR
    v, f = VR.uv_sphere(24, 48)
    camera = RR._persp()
    o, d = MR.camera_rays(camera, 48)
    hits = MR.cast_rays(([v.cuda()], [f.cuda()]), o.cuda(), d.cuda())
    ref = R.exhaustive(v, f, R._rays(o[0].numpy(), d[0].numpy()))
    assert torch.equal(hits.face_idx[0].cpu(), torch.from_numpy(ref["face"])) and torch.equal(hits.t[0].cpu(), torch.from_numpy(ref["t"]))
    assert int((hits.face_idx[0] >= 0).sum()) > 300


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_bakes_ambient_occlusion_into_a_tree_of_two_meshes(hip, tmp_path):
    from bdm_amd.io import load_mesh_ply, save_mesh_ply
    sv, sf = VR.uv_sphere(12, 24)
    bv, bf = VR.box((0.3, 0.2, 0.1), (5.1, 6.3, 7.2))
    albedo = np.tile(np.array([[1.0, 0.5, 0.2]], dtype=np.float32), (8, 1))
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "a" / "sphere.ply")
    save_mesh_ply(bv.numpy(), bf[:, [0, 2, 1]].numpy(), tmp_path / "mesh" / "b" / "inside_out.ply", colors=albedo)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_raycast", "--mesh_dir", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "out"),
                          "--samples", "16"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    rays = 16 * (sv.shape[0] + 8)
    assert got == {"meshes": 2, "rays": rays, "occluded_fraction": 16 * 8 / rays, "faces_dropped": 0}
    v, f, c = load_mesh_ply(tmp_path / "out" / "a" / "sphere.ply", with_colors=True)
    assert np.array_equal(v, sv.numpy()) and np.array_equal(f, sf.numpy()) and np.array_equal(c, np.ones_like(v))      # convex: white
    v, f, c = load_mesh_ply(tmp_path / "out" / "b" / "inside_out.ply", with_colors=True)
    assert np.array_equal(v, bv.numpy()) and np.array_equal(c, np.zeros_like(v))                                         # closed in: black
