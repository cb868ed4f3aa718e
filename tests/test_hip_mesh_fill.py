"""bdm_mesh_boundary_loops and bdm_mesh_fill_holes (csrc/mesh_fill.hip) and their Python surface on the GPU against the CPU restatement
tests/mesh_fill_ref.py: every output with torch.equal, floats compared as bits (a NaN equals any NaN), sentinels around every output,
the workspace pre-filled with 0xA5 and checked behind its end; the error paths; and the feature through Python and the two command
lines.  Nothing here has a tolerance, and no case provokes a fault: the limit cases launch nothing."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_fill_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
CAPS = (64, 3)   # the batch runs at both: at 3 only triangular holes are filled and every other loop is too large


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


def _run(p, cap):
    """Both calls on guarded outputs -> dict of host tensors; asserts what the calls left alone."""
    from bdm_amd import _lib as L
    lib = L.lib()
    nbytes = lib.bdm_mesh_fill_workspace_bytes(p.b, p.sum_v, p.sum_f)
    assert nbytes >= 16 and nbytes % 16 == 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    H = 3 * p.sum_f
    bufs = {k: _guarded(n, torch.int32) for k, n in (("loop", H), ("size", H), ("flags", H), ("counts", 9 * p.b))}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    rc = lib.bdm_mesh_boundary_loops(p.b, cap, L.ptr(p.verts), L.ptr(p.faces), vf, ff, *(_ptr(bufs[k][0]) for k in bufs), L.ptr(ws), L.stream())
    assert rc == 0, lib.bdm_last_error()
    counts = bufs["counts"][1].cpu().view(p.b, 9)   # the one read-back
    assert all(_untouched(w) for w, _ in bufs.values()) and bool((ws[-256:] == 0xA5).all()), "bdm_mesh_boundary_loops wrote outside its outputs"
    ov = torch.tensor([0] + [n + int(c) for n, c in zip(p.nv, counts[:, 7])], dtype=torch.int64).cumsum(0)
    of = torch.tensor([0] + [n + int(c) for n, c in zip(p.nf, counts[:, 8])], dtype=torch.int64).cumsum(0)
    outs = {"verts": _guarded(3 * int(ov[-1]), torch.float32), "attrs": _guarded(p.C * int(ov[-1]), torch.float32),
            "faces": _guarded(3 * int(of[-1]), torch.int32)}
    rc = lib.bdm_mesh_fill_holes(p.b, p.C, L.ptr(p.verts), L.ptr(p.attrs), L.ptr(p.faces), vf, ff, ov.data_ptr(), of.data_ptr(),
                                 *(_ptr(outs[k][0]) for k in outs), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.bdm_last_error()
    assert all(_untouched(w) for w, _ in outs.values()) and bool((ws[-256:] == 0xA5).all()), "bdm_mesh_fill_holes wrote outside its outputs"
    got = {k: body.cpu() for k, (_, body) in {**bufs, **outs}.items()}
    got.update(counts=counts, out_vert_first=ov, out_face_first=of)
    return got


def _split(p, got):
    """Per mesh the dict tests compare with the restatement."""
    out = []
    for m in range(p.b):
        h0, h1 = 3 * int(p.face_first[m]), 3 * int(p.face_first[m + 1])
        v0, v1, f0, f1 = (int(got[k][m + d]) for k in ("out_vert_first", "out_face_first") for d in (0, 1))
        out.append({"loop": got["loop"][h0:h1], "size": got["size"][h0:h1], "flags": got["flags"][h0:h1], "counts": got["counts"][m].tolist(),
                    "verts": got["verts"].view(-1, 3)[v0:v1], "attrs": got["attrs"].view(-1, p.C)[v0:v1] if p.C else None,
                    "faces": got["faces"].view(-1, 3)[f0:f1]})
    return out


def _assert_mesh(g, r, C, what):
    """One mesh of the device against the restatement's dict."""
    assert torch.equal(g["loop"].long(), r["halfedge_loop"].flatten()), f"{what}: labels"
    size, flags = torch.zeros_like(g["size"]).long(), torch.zeros_like(g["flags"]).long()
    if r["labels"]:
        size[r["labels"]], flags[r["labels"]] = r["loop_sizes"], r["loop_flags"]
    assert torch.equal(g["size"].long(), size) and torch.equal(g["flags"].long(), flags), f"{what}: loop sizes or flags"
    assert g["counts"] == list(r["info"].values()), f"{what}: counts {g['counts']} != {r['info']}"
    assert torch.equal(g["faces"].long(), r["faces"].long()), f"{what}: faces"
    assert R.same_floats(g["verts"], r["verts"]), f"{what}: vertices"
    if C:
        assert R.same_floats(g["attrs"], r["attrs"]), f"{what}: attributes"


def _inputs():
    """(verts, faces, attrs (V, 5): three uint8 colour channels as floats and two float channels, one of them NaN at vertex 0 of the
    larger meshes) per mesh of R.batch()."""
    rows = []
    for i, (_, v, f, _) in enumerate(R.batch()):
        u8, fl = R.colors_for(v.shape[0], i)
        attrs = torch.cat([u8.float(), fl], dim=1)
        if v.shape[0] > 100:
            attrs[::7, 4] = float("nan")
        rows.append((v, f, attrs))
    return rows


@functools.lru_cache(maxsize=None)
def _refs(cap):
    return tuple(R.fill(v, f, cap, attrs=a) for v, f, a in _inputs())


@pytest.fixture(scope="module")
def whole(hip):
    """The ragged batch of every mesh of the tables, run once per cap."""
    p = Packed(_inputs(), 5)
    return p, {cap: _run(p, cap) for cap in CAPS}


@pytest.mark.parametrize("cap", CAPS)
def test_batch_equals_the_restatement_bit_for_bit(whole, cap):
    p, runs = whole
    names = [n for n, *_ in R.batch()]
    for name, g, r in zip(names, _split(p, runs[cap]), _refs(cap)):
        _assert_mesh(g, r, 5, f"{name} at cap {cap}")
    filled = sum(r["info"]["filled_loops"] for r in _refs(cap))
    assert filled >= 8 and any(r["info"]["pinched_loops"] for r in _refs(cap)) and any(r["info"]["blocked_edges"] for r in _refs(cap))
    assert any(bool(torch.isnan(r["attrs"][v.shape[0]:]).any()) for r, (v, _, _) in zip(_refs(64), _inputs())), "no NaN channel among the new rows"


def test_old_rows_are_the_inputs_bit_for_bit(whole):
    p, runs = whole
    for g, (v, f, a) in zip(_split(p, runs[64]), _inputs()):
        assert R.same_floats(g["verts"][:v.shape[0]], v) and R.same_floats(g["attrs"][:v.shape[0]], a)
        assert torch.equal(g["faces"][:f.shape[0]].long(), f.long())


def test_every_mesh_alone_has_the_bits_it_has_in_the_batch_and_a_repeat_too(whole):
    p, runs = whole
    batch = _split(p, runs[64])
    again = _split(p, _run(p, 64))
    for m, mesh in enumerate(_inputs()):
        alone = _split(Packed([mesh], 5), _run(Packed([mesh], 5), 64))[0]
        for other, what in ((alone, "alone"), (again[m], "repeated")):
            for k in ("loop", "size", "flags", "faces"):
                assert torch.equal(batch[m][k], other[k]), (m, what, k)
            assert batch[m]["counts"] == other["counts"], (m, what)
            assert R.same_floats(batch[m]["verts"], other["verts"]) and R.same_floats(batch[m]["attrs"], other["attrs"]), (m, what)


def test_variant_reaches_several_round_counts_and_an_empty_boundary_list(hip, whole):
    from bdm_amd import _lib as L
    lib = L.lib()
    p, runs = whole
    rounds = set()
    for _, v, f, _ in R.batch():
        ff = torch.tensor([0, f.shape[0]], dtype=torch.int64)
        code = lib.bdm_mesh_fill_variant(1, ff.data_ptr())
        if f.shape[0] == 0:
            assert code == 0
        else:
            assert code >> 8 == 1 and code & 255 == (3 * f.shape[0] - 1).bit_length() + 1
            rounds.add(code & 255)
    assert len(rounds) >= 3, rounds
    assert lib.bdm_mesh_fill_variant(p.b, p.face_first.data_ptr()) == 256 + (3 * max(p.nf) - 1).bit_length() + 1
    names = [n for n, *_ in R.batch()]
    closed = runs[64]["counts"][names.index("octa_closed")].tolist()
    assert closed == [0] * 9, "the closed octahedron has an empty boundary list"
    assert lib.bdm_mesh_fill_variant(0, p.face_first.data_ptr()) == 0 and lib.bdm_mesh_fill_variant(1, None) == 0


def test_33_meshes_cross_the_launch_boundary_of_the_offsets_upload(hip):
    """b + 1 = 34 offsets are one launch more than the 32 a launch carries: a wrong entry of the second launch mis-addresses mesh 32.
    Open tetrahedra and single triangles in turn, mesh 16 empty; both calls send two offset arrays."""
    g = torch.Generator().manual_seed(331)
    tet, one = torch.tensor([(0, 1, 2), (0, 3, 1), (1, 3, 2)]), torch.tensor([(0, 1, 2)])
    meshes = [(torch.rand(4 - i % 2, 3, generator=g), one if i % 2 else tet, torch.rand(4 - i % 2, 1, generator=g)) for i in range(33)]
    meshes[16] = (torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 1))
    p = Packed(meshes, 1)
    assert p.b == 33
    for m, (g_, mesh) in enumerate(zip(_split(p, _run(p, 32)), meshes)):
        _assert_mesh(g_, R.fill(mesh[0], mesh[1], 32, attrs=mesh[2]), 1, f"mesh {m} of 33")


@pytest.mark.parametrize("large_first", (False, True))
def test_16_channels_with_a_nonfinite_member_in_the_last_and_per_mesh_magnitudes_2_to_the_20_apart(hip, large_first):
    """c = 16 is the last channel the shared accumulator (csrc/mesh_emit.h) holds.  The octahedron with a square hole, twice: channel 15
    has one non-finite value on the rim of the hole (the new vertex's channel 15 is NaN, its other channels are means of four) and the
    second copy's attributes are 2^20 times the first's, so the fixed point of one mesh is not the other's: a mean that read the other
    mesh's largest magnitude, in either order of the two, has other bits."""
    v, f, _ = R.hand_meshes()["octa_too_large"]
    a = torch.randn(v.shape[0], 16, generator=torch.Generator().manual_seed(1916)) * 3.0
    small, large = a.clone(), a * 2.0 ** 20
    small[0, 15], large[0, 15] = float("nan"), float("inf")   # vertex 0 is on the rim of the hole: asserted on the new row below
    meshes = [(v, f, large), (v, f, small)] if large_first else [(v, f, small), (v, f, large)]
    p = Packed(meshes, 16)
    for m, (g, (v_, f_, a_)) in enumerate(zip(_split(p, _run(p, 32)), meshes)):
        r = R.fill(v_, f_, 32, attrs=a_)
        assert r["info"]["filled_loops"] == 1 and r["info"]["new_vertices"] == 1
        new = r["attrs"][v_.shape[0]:]
        assert bool(torch.isnan(new[:, 15]).all()) and bool(torch.isfinite(new[:, :15]).all())
        _assert_mesh(g, r, 16, f"mesh {m} of two at 16 channels")


def test_scans_of_more_than_256_partial_sums_carry_with_a_host_and_a_device_count(hip):
    """87 400 separate triangles (and 10 unused vertices) have H = 262 200 half-edges, all on the boundary: the scan of the H + 1 flags
    (count from the host) and the scans of rankv and rankf over the compacted list (its length H read from the device) each have 257
    partial sums, one more than the middle launch takes per trip.  No attribute channel.  Expected values: R.separate_triangles_filled,
    held against R.fill at 64 triangles by tests/test_mesh_fill_host.py; the new vertices, on a sample of the loops, by R.fixed_mean."""
    n = 87400
    v, f = R.separate_triangles(n, 10, 50)
    V = v.shape[0]
    p = Packed([(v, f, torch.zeros(V, 0))], 0)
    assert -(-(3 * n + 1) // 1024) == 257
    g = _split(p, _run(p, 32))[0]
    want = R.separate_triangles_filled(f, V)
    assert g["counts"] == list(want["info"].values()) == [3 * n, n, n, 0, 0, 0, 0, n, 3 * n]
    assert torch.equal(g["loop"].long(), want["halfedge_loop"].flatten()), "labels"
    slots = torch.zeros(3 * n, dtype=torch.int64)
    slots[want["labels"]] = 1
    assert torch.equal(g["size"].long(), 3 * slots) and torch.equal(g["flags"].long(), R.FILLED * slots), "loop sizes or flags"
    assert torch.equal(g["faces"].long(), want["faces"]), "faces"
    assert g["verts"].shape == (V + n, 3) and R.same_floats(g["verts"][:V], v), "old vertices"
    e, vn = R.scale_exp(v.numpy()), v.numpy()
    for loop in sorted({0, 1, n // 2, n - 1, *range(0, n, 997)}):
        mean = torch.tensor([float(R.fixed_mean(vn[f[loop].tolist(), d], e)) for d in range(3)])
        assert R.same_floats(g["verts"][V + loop], mean), f"the new vertex of loop {loop}"


def test_every_documented_limit_returns_1_and_leaves_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    p = Packed(_inputs()[:8], 5)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.bdm_mesh_fill_workspace_bytes(p.b, p.sum_v, p.sum_f) <= ws.numel()
    H = 3 * p.sum_f
    bufs = {k: _guarded(n, torch.int32) for k, n in (("loop", H), ("size", H), ("flags", H), ("counts", 9 * p.b), ("faces_out", 3 * p.sum_f + 300))}
    bufs["verts_out"], bufs["attrs_out"] = _guarded(3 * p.sum_v + 300, torch.float32), _guarded(5 * p.sum_v + 500, torch.float32)
    o = {k: L.ptr(body) for k, (_, body) in bufs.items()}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    down = p.vert_first.clone()
    down[2] = down[1] - 1
    late = p.vert_first + 1
    huge = torch.full((p.b + 1,), 1 << 31, dtype=torch.int64)
    huge[0] = 0
    many = torch.full((p.b + 1,), 357913942, dtype=torch.int64)
    many[0] = 0
    bad = [dict(vert_first=None), dict(vert_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(vert_first=huge.data_ptr()), dict(b=-1),
           dict(b=65536), dict(ws=None), dict(ws=L.ptr(ws) + 8), dict(face_first=None), dict(face_first=down.data_ptr()),
           dict(face_first=late.data_ptr()), dict(face_first=many.data_ptr()), dict(verts=None), dict(faces=None)]
    loops = dict(b=p.b, cap=32, verts=L.ptr(p.verts), faces=L.ptr(p.faces), vert_first=vf, face_first=ff, loop=o["loop"], size=o["size"],
                 flags=o["flags"], counts=o["counts"], ws=L.ptr(ws), stream=L.stream())
    for change in bad + [dict(cap=2), dict(cap=0), dict(cap=65536), dict(loop=None), dict(size=None), dict(flags=None), dict(counts=None),
                         dict(loop=L.ptr(p.faces)), dict(size=o["loop"]), dict(counts=L.ptr(p.verts)), dict(ws=o["flags"]), dict(ws=L.ptr(p.faces))]:
        assert lib.bdm_mesh_boundary_loops(*dict(loops, **change).values()) == 1 and lib.bdm_last_error(), change
    same = (p.vert_first.data_ptr(), p.face_first.data_ptr())
    fewer_v, more_v, fewer_f, more_f, lone_v = (x.clone() for x in (p.vert_first, p.vert_first, p.face_first, p.face_first, p.vert_first))
    fewer_v[1:] -= 1
    more_v[1:] += p.nf[0] + 1
    fewer_f[1:] -= 1
    more_f[1:] += 3 * p.nf[0] + 1
    lone_v[1:] += 1   # a new vertex without its three faces
    fill = dict(b=p.b, c=5, verts=L.ptr(p.verts), attrs=L.ptr(p.attrs), faces=L.ptr(p.faces), vert_first=vf, face_first=ff, out_vert_first=same[0],
                out_face_first=same[1], verts_out=o["verts_out"], attrs_out=o["attrs_out"], faces_out=o["faces_out"], ws=L.ptr(ws), stream=L.stream())
    for change in bad + [dict(c=-1), dict(c=17), dict(attrs=None), dict(out_vert_first=None), dict(out_face_first=None), dict(verts_out=None),
                         dict(attrs_out=None), dict(faces_out=None), dict(out_vert_first=fewer_v.data_ptr()), dict(out_vert_first=more_v.data_ptr()),
                         dict(out_face_first=fewer_f.data_ptr()), dict(out_face_first=more_f.data_ptr()), dict(out_vert_first=lone_v.data_ptr()),
                         dict(verts_out=L.ptr(p.verts)), dict(attrs_out=o["verts_out"]), dict(faces_out=L.ptr(p.faces)), dict(ws=o["faces_out"]),
                         dict(ws=L.ptr(p.attrs))]:
        assert lib.bdm_mesh_fill_holes(*dict(fill, **change).values()) == 1 and lib.bdm_last_error(), change
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    # nothing to do: 0, and nothing is touched
    assert lib.bdm_mesh_boundary_loops(*dict(loops, b=0, verts=None, vert_first=None).values()) == 0
    assert lib.bdm_mesh_fill_holes(*dict(fill, b=0, faces=None, ws=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()) and bool((ws == 0xA5).all())
    wb = lib.bdm_mesh_fill_workspace_bytes
    assert wb(-1, 10, 10) == 0 and wb(65536, 10, 10) == 0 and wb(1, 1 << 31, 1) == 0 and wb(1, 10, 357913942) == 0 and wb(1, -1, 1) == 0
    assert wb(1, (1 << 31) - 10, 10) == 0 and wb(1, 10, 10) > 0


# ---- through Python -------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_restatement(hip):
    from bdm_amd import mesh_fill as MF
    from bdm_amd.cameras import Meshes
    from bdm_amd.surface import mesh_stats
    rows = list(R.batch())
    verts, faces = [v.cuda() for _, v, _, _ in rows], [f.cuda() for _, _, f, _ in rows]
    u8 = [R.colors_for(v.shape[0], i)[0] for i, (_, v, _, _) in enumerate(rows)]
    fl = [R.colors_for(v.shape[0], i)[1] for i, (_, v, _, _) in enumerate(rows)]
    refs = [R.fill(v, f, 64, attrs=c.float()) for (_, v, f, _), c in zip(rows, u8)]
    loops = MF.boundary_loops(Meshes(verts, faces), 64)
    for (hl, ls, lf), r in zip(loops, refs):
        assert hl.dtype == torch.int64 and hl.is_cuda and torch.equal(hl.cpu(), r["halfedge_loop"])
        assert torch.equal(ls.cpu(), r["loop_sizes"]) and torch.equal(lf.cpu(), r["loop_flags"])
    ov, of, oc, info = MF.fill_holes(Meshes(verts, faces), 64, colors_list=[c.cuda() for c in u8], return_info=True)
    for m, ((_, v, f, _), r, c) in enumerate(zip(rows, refs, u8)):
        assert info[m] == r["info"] and torch.equal(of[m].cpu(), r["faces"]) and of[m].dtype == torch.int64
        assert R.same_floats(ov[m].cpu(), r["verts"])
        sources = {}   # loop label -> the source vertices of its half-edges
        for label, vertex in zip(r["halfedge_loop"].flatten().tolist(), f.flatten().tolist()):
            sources.setdefault(label, []).append(vertex)
        loops_of = [sources[label] for label, flag in zip(r["labels"], r["loop_flags"].tolist()) if flag == R.FILLED]
        want = torch.tensor([[R.uint8_mean(c[src, ch].tolist()) for ch in range(3)] for src in loops_of], dtype=torch.uint8).reshape(-1, 3)
        assert oc[m].dtype == torch.uint8 and torch.equal(oc[m].cpu(), torch.cat([c, want])), f"uint8 colours of mesh {m}"
        if f.shape[0] and bool(((f >= 0) & (f < v.shape[0])).all()):   # mesh_stats looks every index up
            before, after = mesh_stats(v, f), mesh_stats(ov[m].cpu(), of[m].cpu())
            filled_edges = int(r["loop_sizes"][r["loop_flags"] == R.FILLED].sum())
            assert before["open_edges"] - after["open_edges"] == filled_edges and before["inconsistent_edges"] == after["inconsistent_edges"]
            assert after["euler_characteristic"] - before["euler_characteristic"] == r["info"]["filled_loops"]
    # float colours, default cap, the pair form, no info
    refs32 = [R.fill(v, f, 32, attrs=c) for (_, v, f, _), c in zip(rows, fl)]
    ov, of, oc = MF.fill_holes((verts, faces), colors_list=[c.cuda() for c in fl])
    for m, r in enumerate(refs32):
        assert R.same_floats(ov[m].cpu(), r["verts"]) and torch.equal(of[m].cpu(), r["faces"]) and R.same_floats(oc[m].cpu(), r["attrs"])
    ov, of = MF.fill_holes((verts, faces))
    assert all(R.same_floats(a.cpu(), r["verts"]) for a, r in zip(ov, refs32)) and len(of) == len(rows)
    with pytest.raises(Exception, match="CPU tensor"):
        MF.fill_holes(([rows[0][1]], [rows[0][2]]))
    assert MF.fill_holes(([], []), return_info=True) == ([], [], []) and MF.boundary_loops(([], [])) == []


def _tree(tmp_path):
    """Two files: the hole-rich sphere with colours, the torus without."""
    from bdm_amd.io import save_mesh_ply
    sv, sf = R.surface_mesh("sphere600")
    tv, tf = R.surface_mesh("torus1500")
    colours = (torch.arange(sv.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "a" / "sphere.ply", colors=colours.numpy())
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "mesh" / "b" / "torus.ply")
    return (sv, sf, colours), (tv, tf)


def _stats(path):
    from bdm_amd.io import load_mesh_ply
    from bdm_amd.surface import mesh_stats
    v, f, c = load_mesh_ply(path, with_colors=True)
    return mesh_stats(torch.from_numpy(v), torch.from_numpy(f)), v, f, c


def test_cli_fills_a_tree_and_prints_the_composed_json(hip, tmp_path):
    from bdm_amd import mesh_fill as MF
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_fill", "--mesh_dir", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "out"),
                          "--max-hole-edges", "64"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    rs, rt = R.fill(sv, sf, 64, attrs=colours), R.fill(tv, tf, 64)
    sums = {k: rs["info"][k] + rt["info"][k] for k in R.INFO_KEYS}
    s_in, t_in = _stats(tmp_path / "mesh" / "a" / "sphere.ply")[0], _stats(tmp_path / "mesh" / "b" / "torus.ply")[0]
    (s_out, ov, of, oc), (t_out, tov, tof, toc) = _stats(tmp_path / "out" / "a" / "sphere.ply"), _stats(tmp_path / "out" / "b" / "torus.ply")
    assert got == MF.compose_result(2, sums, s_in["edges"] + t_in["edges"], s_in["open_edges"] + t_in["open_edges"],
                                    s_out["edges"] + t_out["edges"], s_out["open_edges"] + t_out["open_edges"])
    filled_edges = sum(int(r["loop_sizes"][r["loop_flags"] == R.FILLED].sum()) for r in (rs, rt))
    assert s_in["open_edges"] + t_in["open_edges"] - s_out["open_edges"] - t_out["open_edges"] == filled_edges == got["new_faces"]
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy())
    assert np.array_equal(tov.view(np.int32), rt["verts"].numpy().view(np.int32)) and np.array_equal(tof, rt["faces"].numpy()) and toc is None
    assert oc.shape == (rs["verts"].shape[0], 3) and np.array_equal(oc[:sv.shape[0]], colours.numpy())
    # save_mesh_ply's conversion, in float64, and load_mesh_ply's back
    want = np.rint(np.clip(rs["attrs"][sv.shape[0]:].numpy().astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(oc[sv.shape[0]:], want), "the new vertices carry the mean colour of their loops"


def test_mesh_clean_cli_fills_between_islands_and_smoothing(hip, tmp_path):
    from bdm_amd import mesh_clean as MC
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    base = [sys.executable, "-m", "bdm_amd.mesh_clean", "--mesh_dir", str(tmp_path / "mesh"), "--taubin-iters", "0", "--min-fraction", "0",
            "--min-faces", "0"]   # nothing is removed, not even the vertices no face uses: the files of "off" hold the input meshes
    runs = {}
    for name, extra in (("off", []), ("on", ["--fill-holes", "64"])):
        out = subprocess.run(base + ["--out_dir", str(tmp_path / name)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        runs[name] = json.loads(out.stdout.strip().splitlines()[-1])
        print(out.stdout.strip().splitlines()[-1])
    assert list(runs["off"]) == list(MC.compose_result(*[0] * 7))
    rs, rt = R.fill(sv, sf, 64, attrs=colours), R.fill(tv, tf, 64)
    sums = {k: rs["info"][k] + rt["info"][k] for k in R.INFO_KEYS}
    assert list(runs["on"]) == list(runs["off"]) + list(R.INFO_KEYS) and {k: runs["on"][k] for k in R.INFO_KEYS} == sums
    assert runs["on"]["vertices_out"] == runs["off"]["vertices_out"] + sums["new_vertices"]
    assert runs["on"]["faces_out"] == runs["off"]["faces_out"] + sums["new_faces"]
    (s_off, *_), (s_on, ov, of, oc) = _stats(tmp_path / "off" / "a" / "sphere.ply"), _stats(tmp_path / "on" / "a" / "sphere.ply")
    assert s_off["open_edges"] - s_on["open_edges"] == rs["info"]["new_faces"]
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy()) and oc.shape[0] == ov.shape[0]
    t_on, tov, tof, toc = _stats(tmp_path / "on" / "b" / "torus.ply")
    assert t_on["open_edges"] == 0 and toc is None and np.array_equal(tof, rt["faces"].numpy())
