"""bdm_mesh_qem_init / _rounds / _finish (csrc/mesh_qem.hip) and their Python surface on the GPU against the CPU restatement
tests/mesh_qem_ref.py: every output with torch.equal, floats compared as bits, sentinels around every output, the workspace
pre-filled with 0xA5 and checked behind its end; the state after init and after one round; chunked and repeated runs; the error
paths; the Python surface, the command lines and the feature end to end behind the Poisson mesher.  Nothing here has a tolerance
except the quality inequality, and no case provokes a fault: the limit cases launch nothing."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_qem_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
NC = len(R.INFO_KEYS)
C = 3


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _ptr(whole):
    return whole.data_ptr() + PAD * whole.element_size()


@functools.lru_cache(maxsize=None)
def batch():
    """(name, verts, faces, attrs, target): the ragged batch.  The level-4 icosphere (5120 faces: several workgroups, several scan
    chunks) stops at 4500 faces, after four rounds; the others run down to a tenth of their faces or until nothing is left to collapse."""
    rows = []
    hand = R.hand_meshes()
    sphere1_v, sphere1_f = R.icosphere(1)
    nan_v = sphere1_v.clone()
    nan_v[7, 1] = float("nan")
    bad_f = torch.cat([R.icosphere(2)[1], torch.tensor([[0, 0, 5], [3, 400, 2], [-1, 2, 3]])])
    table = [("empty", torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), 0), ("no_faces", torch.rand(5, 3), torch.zeros(0, 3, dtype=torch.int64), 0),
             ("nan_vertex", nan_v, sphere1_f, 8), ("fin", *hand["fin"], 0), ("fan40", *hand["fan40"], 4), ("tetrahedron", *hand["tetrahedron"], 0),
             ("two_tetrahedra", *hand["two_tetrahedra"], 0), ("octahedron", *hand["octahedron"], 0), ("grid9", *R.grid(9), 12),
             ("torus", *R.torus(), 25), ("bad_faces", R.icosphere(2)[0], bad_f, 32), ("ico4", *R.icosphere(4), 4500), ("ico2", *R.icosphere(2), 32),
             ("tilted", *R.tilted(9), 16)]
    for i, (name, v, f, target) in enumerate(table):
        rows.append((name, v, f, R.attrs_for(v.shape[0], i, C), target))
    return tuple(rows)


class Packed:
    def __init__(self, rows, channels=C):
        self.C = channels
        self.names = [r[0] for r in rows]
        self.nv, self.nf = [r[1].shape[0] for r in rows], [r[2].shape[0] for r in rows]
        self.b, self.sum_v, self.sum_f = len(rows), sum(self.nv), sum(self.nf)
        self.verts = torch.cat([r[1] for r in rows] + [torch.zeros(1, 3)]).float().cuda().contiguous()
        self.attrs = torch.cat([r[3] for r in rows] + [torch.zeros(1, channels)]).float().cuda().contiguous()
        self.faces = torch.cat([r[2] for r in rows] + [torch.zeros(1, 3, dtype=torch.int64)]).int().cuda().contiguous()
        self.vert_first = torch.tensor([0] + self.nv, dtype=torch.int64).cumsum(0)
        self.face_first = torch.tensor([0] + self.nf, dtype=torch.int64).cumsum(0)
        self.targets = torch.tensor([r[4] for r in rows], dtype=torch.int64)


class Run:
    """One run of the ABI on guarded buffers; the stages are called in order."""

    def __init__(self, p, weight=1.0, maximum_error=float("inf"), max_rounds=256):
        from bdm_amd import _lib as L
        self.p, self.L, self.lib = p, L, L.lib()
        self.maximum_error, self.max_rounds = maximum_error, max_rounds
        nbytes = self.lib.bdm_mesh_qem_workspace_bytes(p.b, p.sum_v, p.sum_f)
        assert nbytes >= 16 and nbytes % 16 == 0
        self.nbytes = nbytes
        self.ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.counts, self.active = _guarded(NC * p.b, torch.int32), _guarded(1, torch.int32)
        self.vf, self.ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
        rc = self.lib.bdm_mesh_qem_init(p.b, weight, p.targets.data_ptr(), L.ptr(p.verts), L.ptr(p.faces), self.vf, self.ff, _ptr(self.counts[0]),
                                        L.ptr(self.ws), L.stream())
        assert rc == 0, self.lib.bdm_last_error()
        self.calls = 0

    def rounds(self, n):
        rc = self.lib.bdm_mesh_qem_rounds(self.p.b, n, self.max_rounds, self.maximum_error, self.vf, self.ff, _ptr(self.counts[0]),
                                          _ptr(self.active[0]), self.L.ptr(self.ws), self.L.stream())
        assert rc == 0, self.lib.bdm_last_error()
        self.calls += 1
        return int(self.active[1].item())

    def info(self):
        torch.cuda.synchronize()
        assert _untouched(self.counts[0]) and _untouched(self.active[0]) and bool((self.ws[-256:] == 0xA5).all()), "a write outside the outputs"
        return self.counts[1].cpu().view(self.p.b, NC)

    def state(self):
        """The working arrays in the workspace, on the host."""
        p = self.p
        off = torch.zeros(6, dtype=torch.int64)
        assert self.lib.bdm_mesh_qem_layout(p.b, p.sum_v, p.sum_f, off.data_ptr()) == 0
        ws, o = self.ws.cpu(), off.tolist()
        take = lambda at, n, dt, size: ws[at:at + n * size].view(dt)   # noqa: E731
        return {"pos": take(o[0], 3 * p.sum_v, torch.float32, 4).view(-1, 3), "quad": take(o[1], 10 * p.sum_v, torch.float64, 8).view(-1, 10),
                "vlive": take(o[2], p.sum_v, torch.int32, 4), "faces": take(o[3], 3 * p.sum_f, torch.int32, 4).view(-1, 3),
                "key": take(o[4], 3 * p.sum_f, torch.int64, 8), "sel": take(o[5], 3 * p.sum_f, torch.int32, 4)}

    def finish(self):
        p, L, C = self.p, self.L, self.p.C
        rows = self.info()
        ov = torch.tensor([0] + rows[:, 6].tolist(), dtype=torch.int64).cumsum(0)
        of = torch.tensor([0] + rows[:, 4].tolist(), dtype=torch.int64).cumsum(0)
        outs = {"verts": _guarded(3 * int(ov[-1]), torch.float32), "attrs": _guarded(C * int(ov[-1]), torch.float32),
                "faces": _guarded(3 * int(of[-1]), torch.int32), "vert_map": _guarded(p.sum_v, torch.int32), "face_map": _guarded(p.sum_f, torch.int32)}
        rc = self.lib.bdm_mesh_qem_finish(p.b, C, L.ptr(p.attrs), self.vf, self.ff, ov.data_ptr(), of.data_ptr(), *(_ptr(outs[k][0]) for k in outs),
                                          L.ptr(self.ws), L.stream())
        torch.cuda.synchronize()
        assert rc == 0, self.lib.bdm_last_error()
        assert all(_untouched(w) for w, _ in outs.values()) and bool((self.ws[-256:] == 0xA5).all()), "bdm_mesh_qem_finish wrote outside its outputs"
        got = {k: body.cpu() for k, (_, body) in outs.items()}
        assert int((got["verts"].view(torch.int32) == torch.tensor(F_SENTINEL).view(torch.int32)).sum()) == 0, "an output vertex was not written"
        for k in ("faces", "vert_map", "face_map"):
            assert int((got[k] == I_SENTINEL).sum()) == 0, f"an entry of {k} was not written"
        out = []
        for m in range(p.b):
            v0, v1, f0, f1 = (int(x[m + d]) for x in (p.vert_first, p.face_first) for d in (0, 1))
            out.append({"vert_map": got["vert_map"][v0:v1], "face_map": got["face_map"][f0:f1], "counts": rows[m].tolist(),
                        "verts": got["verts"].view(-1, 3)[int(ov[m]):int(ov[m + 1])], "attrs": got["attrs"].view(-1, C)[int(ov[m]):int(ov[m + 1])],
                        "faces": got["faces"].view(-1, 3)[int(of[m]):int(of[m + 1])]})
        return out

    def whole(self, per_call):
        while self.rounds(per_call):
            assert self.calls <= 400
        return self.finish()


MAX_ROUNDS = 256   # ico4 is held to few rounds by its target of 4500 faces


@functools.lru_cache(maxsize=None)
def _states():
    """The restatement of every mesh after init and after one round, and its result: computed once."""
    out = []
    for _, v, f, a, target in batch():
        s = R.State(v, f, target, max_rounds=MAX_ROUNDS)
        q0, stop0 = s.quadrics(), s.stop
        one = None
        if s.stop == 0:
            s.round()
            one = {"keys": dict(s.last["keys"]), "selected": list(s.last["selected"]), "pos": [list(p) for p in s.pos], "vlive": list(s.vlive),
                   "faces": [list(x) for x in s.faces], "info": s.info()}
        while s.run():
            pass
        out.append({"quad": q0, "stop0": stop0, "one": one, "result": s.finish(a)})
    return tuple(out)


def _assert_mesh(g, r, what):
    assert g["counts"] == list(r["info"].values()), f"{what}: counts {g['counts']} != {r['info']}"
    assert torch.equal(g["vert_map"].long(), r["vert_map"]), f"{what}: vert_map"
    assert torch.equal(g["face_map"].long(), r["face_map"]), f"{what}: face_map"
    assert torch.equal(g["faces"].long(), r["faces"].long()), f"{what}: faces"
    assert R.same_floats(g["verts"], r["verts"]), f"{what}: vertices"
    assert R.same_floats(g["attrs"], r["attrs"]), f"{what}: attributes"


@pytest.fixture(scope="module")
def staged(hip):
    """The batch after init, after one round, and finished in calls of 8 rounds."""
    p = Packed(batch())
    run = Run(p, max_rounds=MAX_ROUNDS)
    after_init = (run.info().clone(), run.state())
    run.rounds(1)
    after_one = (run.info().clone(), run.state())
    return p, after_init, after_one, run.whole(8)


def test_init_leaves_the_quadrics_of_the_restatement_bit_for_bit(staged):
    p, (info, st), _, _ = staged
    for m, (name, ref) in enumerate(zip(p.names, _states())):
        v0, v1 = int(p.vert_first[m]), int(p.vert_first[m + 1])
        assert torch.equal(st["quad"][v0:v1].view(torch.int64), ref["quad"].view(torch.int64)), f"{name}: quadrics"
        assert int(info[m, 0]) == ref["stop0"] and int(info[m, 1]) == 0, name
        assert int(info[m, 7]) == ref["result"]["info"]["locked_vertices"] and int(info[m, 8]) == ref["result"]["info"]["bad_faces"], name
    assert any(bool((r["quad"] != 0).any()) for r in _states())


def test_one_round_leaves_the_keys_flags_positions_and_faces_of_the_restatement(staged):
    p, _, (info, st), _ = staged
    seen = 0
    for m, (name, ref) in enumerate(zip(p.names, _states())):
        one = ref["one"]
        if one is None:
            continue
        v0, v1, f0, f1 = (int(x[m + d]) for x in (p.vert_first, p.face_first) for d in (0, 1))
        keys = torch.full((3 * (f1 - f0),), -1, dtype=torch.int64)
        for h, k in one["keys"].items():
            keys[h] = k - (1 << 64) if k >= 1 << 63 else k
        sel = torch.zeros(3 * (f1 - f0), dtype=torch.int32)
        sel[one["selected"]] = 1
        assert torch.equal(st["key"][3 * f0:3 * f1], keys), f"{name}: keys"
        assert torch.equal(st["sel"][3 * f0:3 * f1], sel), f"{name}: selected flags"
        assert R.same_floats(st["pos"][v0:v1], torch.tensor(one["pos"], dtype=torch.float64).float().reshape(-1, 3)), f"{name}: positions"
        assert st["vlive"][v0:v1].tolist() == [int(x) for x in one["vlive"]], f"{name}: live flags"
        assert st["faces"][f0:f1].tolist() == one["faces"], f"{name}: faces"
        assert info[m].tolist() == list(one["info"].values()), f"{name}: counts after one round"
        seen += len(one["selected"])
    assert seen > 50   # the level-4 icosphere alone selects 42 edges in its first round


def test_batch_equals_the_restatement_bit_for_bit(staged):
    p, _, _, got = staged
    refs = [r["result"] for r in _states()]
    for name, g, r in zip(p.names, got, refs):
        _assert_mesh(g, r, name)
    stops = {r["info"]["stop"] for r in refs}
    assert {1, 2} <= stops, stops
    assert sum(r["info"]["collapses"] for r in refs) > 500 and any(r["info"]["locked_vertices"] for r in refs) and any(r["info"]["bad_faces"] for r in refs)
    assert any(len(mem) > 1 and bool(torch.isfinite(r["attrs"][i]).all()) for r in refs for i, mem in enumerate(r["members"]))


def test_rounds_one_at_a_time_and_a_repeat_have_the_bits_of_rounds_by_eight(staged):
    p, _, _, got = staged
    single = Run(p, max_rounds=MAX_ROUNDS).whole(1)
    again = Run(p, max_rounds=MAX_ROUNDS).whole(8)
    for m in range(p.b):
        for other, what in ((single[m], "one round per call"), (again[m], "repeated")):
            for k in ("vert_map", "face_map", "faces"):
                assert torch.equal(got[m][k], other[k]), (p.names[m], what, k)
            assert got[m]["counts"] == other["counts"], (p.names[m], what)
            assert R.same_floats(got[m]["verts"], other["verts"]) and R.same_floats(got[m]["attrs"], other["attrs"]), (p.names[m], what)


def test_a_mesh_alone_has_the_bits_it_has_in_the_batch_and_max_rounds_stops(staged):
    p, _, _, got = staged
    rows = batch()
    for m in (4, 8, 9, 12):
        one = Packed([rows[m]])
        alone = Run(one, max_rounds=MAX_ROUNDS).whole(8)[0]
        for k in ("vert_map", "face_map", "faces"):
            assert torch.equal(got[m][k], alone[k]), (p.names[m], k)
        assert got[m]["counts"] == alone["counts"] and R.same_floats(got[m]["verts"], alone["verts"]) and R.same_floats(got[m]["attrs"], alone["attrs"])
    _, v, f, a, _ = rows[9]   # the torus: three rounds only, a weight of 0, an error bound
    for kw in (dict(max_rounds=3), dict(boundary_weight=0.0, max_rounds=5), dict(maximum_error=1e-3)):
        one = Packed([("torus", v, f, a, 25)])
        g = Run(one, weight=kw.get("boundary_weight", 1.0), maximum_error=kw.get("maximum_error", float("inf")), max_rounds=kw.get("max_rounds", 256)).whole(8)[0]
        r = R.decimate(v, f, 25, attrs=a, **kw)
        _assert_mesh(g, r, f"torus with {kw}")
        assert r["info"]["stop"] == (2 if "maximum_error" in kw else 3)
    gv, gf = R.grid(9)   # an open sheet: the boundary quadrics decide
    for w in (0.0, 1.0, 8.0):
        one = Packed([("grid", gv * torch.tensor([1.0, 1.3, 1.0]) + 0.1 * torch.sin(7.0 * gv[:, :1]) * torch.tensor([0.0, 0.0, 1.0]), gf, R.attrs_for(81, 5, C), 20)])
        r = R.decimate(one.verts[:-1].cpu(), gf, 20, boundary_weight=w, attrs=one.attrs[:-1].cpu())
        _assert_mesh(Run(one, weight=w).whole(8)[0], r, f"bent grid at weight {w}")


@pytest.mark.parametrize("large_first", (False, True))
def test_16_channels_with_a_nonfinite_member_in_the_last_and_per_mesh_magnitudes_2_to_the_20_apart(hip, large_first):
    """c = 16 is the last channel the shared accumulator (csrc/mesh_emit.h) holds, and the attributes' largest magnitude of mesh m lives
    at stride 1 here.  The octahedron, the smallest closed mesh of the table that collapses, down to six faces, twice: vertex 1 merges
    into vertex 0 and channel 15 is non-finite at vertex 1 alone (the survivor's channel 15 is NaN, its other channels are means of
    two), and the second copy's attributes are 2^20 times the first's: a mean under the other mesh's fixed point, in either order,
    has other bits."""
    v, f = R.hand_meshes()["octahedron"]
    a = torch.randn(6, 16, generator=torch.Generator().manual_seed(2316)) * 3.0
    small, large = a.clone(), a * 2.0 ** 20
    small[1, 15], large[1, 15] = float("nan"), float("inf")
    rows = [("small", v, f, small, 6), ("large", v, f, large, 6)]
    rows = rows[::-1] if large_first else rows
    got = Run(Packed(rows, 16)).whole(8)
    for g, (name, v_, f_, a_, target) in zip(got, rows):
        r = R.decimate(v_, f_, target, attrs=a_)
        assert r["info"]["collapses"] == 1 and r["members"][0] == [0, 1]
        assert torch.isnan(r["attrs"][:, 15]).tolist() == [True] + [False] * 4 and bool(torch.isfinite(r["attrs"][:, :15]).all())
        _assert_mesh(g, r, f"{name} at 16 channels")


def test_every_documented_limit_returns_1_and_leaves_the_outputs_untouched(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    p = Packed(batch()[2:10])
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.bdm_mesh_qem_workspace_bytes(p.b, p.sum_v, p.sum_f) <= ws.numel()
    bufs = {k: _guarded(n, torch.int32) for k, n in (("vert_map", p.sum_v), ("face_map", p.sum_f), ("counts", NC * p.b), ("active", 1), ("faces_out", 3 * p.sum_f))}
    bufs["verts_out"], bufs["attrs_out"] = _guarded(3 * p.sum_v, torch.float32), _guarded(C * p.sum_v, torch.float32)
    o = {k: L.ptr(body) for k, (_, body) in bufs.items()}
    vf, ff = p.vert_first.data_ptr(), p.face_first.data_ptr()
    down = p.vert_first.clone()
    down[2] = down[1] - 1
    late = p.vert_first + 1
    huge = torch.full((p.b + 1,), 1 << 31, dtype=torch.int64)
    huge[0] = 0
    many = torch.full((p.b + 1,), 357913942, dtype=torch.int64)
    many[0] = 0
    neg = p.targets.clone()
    neg[3] = -1
    common = [dict(vert_first=None), dict(vert_first=down.data_ptr()), dict(vert_first=late.data_ptr()), dict(vert_first=huge.data_ptr()), dict(b=-1),
              dict(b=65536), dict(ws=None), dict(ws=L.ptr(ws) + 8), dict(face_first=None), dict(face_first=down.data_ptr()),
              dict(face_first=late.data_ptr()), dict(face_first=many.data_ptr())]
    init = dict(b=p.b, weight=1.0, targets=p.targets.data_ptr(), verts=L.ptr(p.verts), faces=L.ptr(p.faces), vert_first=vf, face_first=ff,
                counts=o["counts"], ws=L.ptr(ws), stream=L.stream())
    for change in common + [dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(targets=None), dict(targets=neg.data_ptr()),
                            dict(verts=None), dict(faces=None), dict(counts=None), dict(counts=L.ptr(p.verts)), dict(ws=L.ptr(p.faces))]:
        assert lib.bdm_mesh_qem_init(*dict(init, **change).values()) == 1 and lib.bdm_last_error(), change
    rounds = dict(b=p.b, rounds=8, max_rounds=256, maximum_error=float("inf"), vert_first=vf, face_first=ff, counts=o["counts"], active=o["active"],
                  ws=L.ptr(ws), stream=L.stream())
    for change in common + [dict(rounds=0), dict(rounds=(1 << 20) + 1), dict(max_rounds=0), dict(maximum_error=-1.0), dict(maximum_error=float("nan")),
                            dict(counts=None), dict(active=None), dict(active=o["counts"]), dict(ws=o["counts"])]:
        assert lib.bdm_mesh_qem_rounds(*dict(rounds, **change).values()) == 1 and lib.bdm_last_error(), change
    more_v, more_f, none_v = p.vert_first.clone(), p.face_first.clone(), p.vert_first.clone()
    more_v[1:] += 1
    more_f[1:] += 1
    none_v[1:] -= int(p.vert_first[1])
    fin = dict(b=p.b, c=C, attrs=L.ptr(p.attrs), vert_first=vf, face_first=ff, out_vert_first=vf, out_face_first=ff, verts_out=o["verts_out"],
               attrs_out=o["attrs_out"], faces_out=o["faces_out"], vert_map=o["vert_map"], face_map=o["face_map"], ws=L.ptr(ws), stream=L.stream())
    for change in common[:8] + [dict(c=-1), dict(c=17), dict(attrs=None), dict(out_vert_first=None), dict(out_face_first=None), dict(verts_out=None),
                                dict(attrs_out=None), dict(faces_out=None), dict(vert_map=None), dict(face_map=None), dict(out_vert_first=more_v.data_ptr()),
                                dict(out_face_first=more_f.data_ptr()), dict(out_vert_first=none_v.data_ptr()), dict(out_vert_first=down.data_ptr()),
                                dict(attrs_out=L.ptr(p.attrs)), dict(vert_map=o["face_map"]), dict(ws=o["faces_out"])]:
        assert lib.bdm_mesh_qem_finish(*dict(fin, **change).values()) == 1 and lib.bdm_last_error(), change
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    assert lib.bdm_mesh_qem_init(*dict(init, b=0, verts=None, vert_first=None).values()) == 0
    assert lib.bdm_mesh_qem_rounds(*dict(rounds, b=0, ws=None).values()) == 0
    assert lib.bdm_mesh_qem_finish(*dict(fin, b=0, attrs=None, ws=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(w, body=True) for w, _ in bufs.values()) and bool((ws == 0xA5).all())
    wb = lib.bdm_mesh_qem_workspace_bytes
    assert wb(-1, 10, 10) == 0 and wb(65536, 10, 10) == 0 and wb(1, 1 << 31, 1) == 0 and wb(1, 10, 357913942) == 0 and wb(1, -1, 1) == 0
    assert wb(1, 10, 10) > 0


# ---- through Python -------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_restatement(hip):
    import mesh_fill_ref as FR
    from bdm_amd import mesh_decimate as MD
    from bdm_amd.cameras import Meshes
    rows = [batch()[m] for m in (2, 4, 8, 9, 12)]
    verts, faces = [r[1].cuda() for r in rows], [r[2].cuda() for r in rows]
    u8 = [FR.colors_for(r[1].shape[0], i)[0] for i, r in enumerate(rows)]
    refs = [R.decimate(r[1], r[2], int(0.25 * r[2].shape[0]), attrs=c.float()) for r, c in zip(rows, u8)]
    ov, of, oc, info, (vm, fm) = MD.simplify_quadric_decimation(Meshes(verts, faces), target_fraction=0.25, colors_list=[c.cuda() for c in u8],
                                                                return_info=True, return_maps=True)
    for m, (r, c) in enumerate(zip(refs, u8)):
        assert {k: info[m][k] for k in R.INFO_KEYS} == r["info"] and info[m]["stop_reason"] == R.STOPS[r["info"]["stop"]]
        assert torch.equal(of[m].cpu(), r["faces"]) and of[m].dtype == torch.int64 and R.same_floats(ov[m].cpu(), r["verts"])
        assert torch.equal(vm[m].cpu(), r["vert_map"]) and torch.equal(fm[m].cpu(), r["face_map"]) and vm[m].dtype == torch.int64
        want = torch.tensor([[FR.uint8_mean(c[mem, ch].tolist()) for ch in range(3)] for mem in r["members"]], dtype=torch.uint8).reshape(-1, 3)
        assert oc[m].dtype == torch.uint8 and torch.equal(oc[m].cpu(), want), f"uint8 colours of mesh {m}"
        assert info[m]["max_cost"] == float(np.uint32(r["info"]["max_cost_bits"]).view(np.float32))
    targets = [6, 10, 40, 100, 64]
    ov, of = MD.simplify_quadric_decimation((verts, faces), target_number_of_triangles=targets, boundary_weight=2.0, maximum_error=0.5, max_rounds=6)
    for m, (r, t) in enumerate(zip(rows, targets)):
        ref = R.decimate(r[1], r[2], t, boundary_weight=2.0, maximum_error=0.5, max_rounds=6)
        assert R.same_floats(ov[m].cpu(), ref["verts"]) and torch.equal(of[m].cpu(), ref["faces"])
    for kw in (dict(), dict(target_fraction=0.5, target_number_of_triangles=5), dict(target_fraction=0.0), dict(target_fraction=1.5),
               dict(target_number_of_triangles=-1), dict(target_number_of_triangles=[1, 2]), dict(target_fraction=0.5, maximum_error=-1.0),
               dict(target_fraction=0.5, boundary_weight=float("inf")), dict(target_fraction=0.5, max_rounds=0)):
        with pytest.raises(ValueError):
            MD.simplify_quadric_decimation((verts, faces), **kw)
    with pytest.raises(Exception, match="CPU tensor"):
        MD.simplify_quadric_decimation(([rows[0][1]], [rows[0][2]]), target_fraction=0.5)
    assert MD.simplify_quadric_decimation(([], []), target_fraction=0.5, return_info=True, return_maps=True) == ([], [], [], ([], []))


def _tree(tmp_path):
    from bdm_amd.io import save_mesh_ply
    sv, sf = R.icosphere(2)
    tv, tf = R.torus()
    colours = (torch.arange(sv.shape[0]) % 256).float()[:, None].expand(-1, 3) / 255.0
    save_mesh_ply(sv.numpy(), sf.numpy(), tmp_path / "mesh" / "a" / "sphere.ply", colors=colours.numpy())
    save_mesh_ply(tv.numpy(), tf.numpy(), tmp_path / "mesh" / "b" / "torus.ply")
    return (sv, sf, colours), (tv, tf)


def _load(path):
    from bdm_amd.io import load_mesh_ply
    v, f, c = load_mesh_ply(path, with_colors=True)
    return v, f, c


@pytest.mark.parametrize("target", [("--target-fraction", "0.25"), ("--target-faces", "60", "--boundary-weight", "2", "--max-error", "0.5")])
def test_cli_decimates_a_tree_by_quadrics(hip, tmp_path, target):
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_decimate", "--mesh_dir", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "out"),
                          "--method", "quadric", *target], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    if target[0] == "--target-fraction":
        kw, ts, tt = {}, int(0.25 * sf.shape[0]), int(0.25 * tf.shape[0])
    else:
        kw, ts, tt = dict(boundary_weight=2.0, maximum_error=0.5), 60, 60
    rs, rt = R.decimate(sv, sf, ts, attrs=colours, **kw), R.decimate(tv, tf, tt, **kw)
    assert got["files"] == 2 and got["method"] == "quadric" and got["rounds"] == max(rs["info"]["rounds"], rt["info"]["rounds"])
    assert got["collapses"] == rs["info"]["collapses"] + rt["info"]["collapses"]
    assert got["faces_in"] == sf.shape[0] + tf.shape[0] and got["faces_out"] == rs["faces"].shape[0] + rt["faces"].shape[0]
    assert got["vertices_out"] == rs["verts"].shape[0] + rt["verts"].shape[0]
    assert got["open_edge_fraction_in"] == 0.0 and got["open_edge_fraction_out"] == 0.0
    (ov, of, oc), (tov, tof, toc) = _load(tmp_path / "out" / "a" / "sphere.ply"), _load(tmp_path / "out" / "b" / "torus.ply")
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy()) and oc is not None
    assert np.array_equal(tov.view(np.int32), rt["verts"].numpy().view(np.int32)) and np.array_equal(tof, rt["faces"].numpy()) and toc is None


def test_mesh_clean_cli_decimates_by_fraction(hip, tmp_path):
    (sv, sf, colours), (tv, tf) = _tree(tmp_path)
    base = [sys.executable, "-m", "bdm_amd.mesh_clean", "--mesh_dir", str(tmp_path / "mesh"), "--taubin-iters", "0", "--min-fraction", "0", "--min-faces", "0"]
    out = subprocess.run(base + ["--out_dir", str(tmp_path / "on"), "--decimate-fraction", "0.25"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    rs, rt = R.decimate(sv, sf, int(0.25 * sf.shape[0]), attrs=colours), R.decimate(tv, tf, int(0.25 * tf.shape[0]))
    assert got["faces_out"] == rs["faces"].shape[0] + rt["faces"].shape[0] and got["vertices_out"] == rs["verts"].shape[0] + rt["verts"].shape[0]
    assert got["decimate_collapses"] == rs["info"]["collapses"] + rt["info"]["collapses"]
    assert got["decimate_rounds"] == max(rs["info"]["rounds"], rt["info"]["rounds"])
    ov, of, _ = _load(tmp_path / "on" / "a" / "sphere.ply")
    assert np.array_equal(ov.view(np.int32), rs["verts"].numpy().view(np.int32)) and np.array_equal(of, rs["faces"].numpy())
    both = subprocess.run(base + ["--out_dir", str(tmp_path / "both"), "--decimate-fraction", "0.25", "--decimate-resolution", "16"], cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert both.returncode != 0


# ---- behind the mesher ------------------------------------------------------------------------------------------------------------------
def _sphere_cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, 3, generator=g, dtype=torch.float64)
    p = (p / p.norm(dim=1, keepdim=True)).float()
    return p * 0.5, p.clone()


def _poisson(points, normals, resolution):
    from bdm_amd.surface import reconstruct_surface
    out = reconstruct_surface(points.cuda()[None], normals.cuda()[None], resolution=resolution, method="poisson")
    return out[0][0], out[1][0]


def _disagree(v, f):
    from bdm_amd.mesh_voxel import voxelize_meshes
    return int(voxelize_meshes(([v], [f]), resolution=32, return_info=True)[1]["counts"]["disagree"][0])


def test_a_poisson_sphere_decimated_to_a_quarter_is_still_closed(hip):
    """The 512-point sphere meshed at 32^3, then a quarter of its faces: no open edge, the Euler characteristic of before, and a solid
    voxelisation on which the three ray directions agree.  The same mesh through simplify_vertex_clustering is printed for contrast."""
    from bdm_amd import mesh_decimate as MD
    v, f = _poisson(*_sphere_cloud(512, 5), 32)
    before = R.topology(f.cpu())
    assert before["open_edges"] == 0 and before["inconsistent_edges"] == 0 and f.shape[0] > 400
    (ov,), (of,), (info,) = MD.simplify_quadric_decimation(([v], [f]), target_fraction=0.25, return_info=True)
    after = R.topology(of.cpu())
    print("quadric:", info, after)
    assert of.shape[0] <= f.shape[0] // 4 and info["stop_reason"] == "target"
    assert after["open_edges"] == 0 and after["inconsistent_edges"] == 0 and after["multi_edges"] == 0 and after["duplicate_faces"] == 0
    assert after["euler"] == before["euler"]
    assert R.signed_volume(ov.cpu(), of.cpu()) * R.signed_volume(v.cpu(), f.cpu()) > 0
    assert _disagree(ov, of) == 0
    for res in (6, 8, 12):
        (cv,), (cf,) = MD.simplify_vertex_clustering(([v], [f]), resolution=res)
        c = R.topology(cf.cpu())
        print(f"clustering at {res}: {cf.shape[0]} faces", c, "disagree", _disagree(cv, cf))


def _mean_sqdist(points, v, f):
    from bdm_amd.mesh_metrics import point_mesh_sqdist
    sq, _ = point_mesh_sqdist(([v], [f]), points[None])
    return float(sq.double().mean())


def _torus_cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.rand(n, generator=g, dtype=torch.float64) * 2 * np.pi, torch.rand(n, generator=g, dtype=torch.float64) * 2 * np.pi
    nrm = torch.stack([torch.cos(b) * torch.cos(a), torch.cos(b) * torch.sin(a), torch.sin(b)], 1)
    ctr = torch.stack([torch.cos(a), torch.sin(a), torch.zeros_like(a)], 1) * 0.35
    return (ctr + 0.15 * nrm).float(), nrm.float()


@pytest.mark.parametrize("which", ["ico4", "poisson_torus"])
def test_quadric_decimation_is_closer_to_the_surface_than_clustering_with_no_fewer_faces(hip, which):
    """The mean squared distance from the original vertices to the decimated surface: QEM at N faces against vertex clustering at the
    coarsest resolution of the ladder that still leaves at least N faces (so clustering never has fewer faces to spend)."""
    from bdm_amd import mesh_decimate as MD
    if which == "ico4":
        v, f = (x.cuda() for x in R.icosphere(4))
    else:
        v, f = _poisson(*_torus_cloud(2048, 11), 48)
    (qv,), (qf,) = MD.simplify_quadric_decimation(([v], [f]), target_fraction=0.1)
    n = qf.shape[0]
    for res in range(4, 65):
        (cv,), (cf,) = MD.simplify_vertex_clustering(([v], [f]), resolution=res)
        if cf.shape[0] >= n:
            break
    assert cf.shape[0] >= n
    dq, dc = _mean_sqdist(v, qv, qf), _mean_sqdist(v, cv, cf)
    print(f"{which}: {f.shape[0]} faces; quadric {n} faces, mean squared distance {dq:.3e}; clustering at {res}: {cf.shape[0]} faces, {dc:.3e}")
    assert dq < dc
