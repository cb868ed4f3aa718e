"""bdm_knn_points and bdm_knn_interpolate (csrc/knn.hip) and their Python surface on the GPU against the CPU restatement
tests/knn_ref.py: every output with torch.equal, floats compared as bits, in every case; the pins of the launch path, the error
paths, and the feature end to end (a coloured sphere through normals -> surface -> colour transfer, the mesh_color command line, the
renderer's vert_albedo).

Every float operation of the rule is rounded on its own, so nothing here has a tolerance except the end-to-end colour of the sphere,
whose bound is derived in its test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_ref as K

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


def _pack(rows_list, width=3):
    """Packed device rows; an empty side still gets one (unread) row: no NULL among the inputs."""
    n = sum(t.shape[0] for t in rows_list)
    return torch.cat(rows_list).float().cuda().contiguous() if n else torch.zeros(1, width, device="cuda")


def _first(rows_list):
    return torch.tensor([0] + [t.shape[0] for t in rows_list], dtype=torch.int64).cumsum(0)


def _call_knn(q_list, r_list, k, outputs=("idx", "d2"), expect=0):
    """One ABI call on guarded outputs and a workspace pre-filled with 0xA5 -> [(idx int64, d2 float32)] per entry on the host (None
    for an output passed as NULL)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    B, np_ = len(q_list), [t.shape[0] for t in q_list]
    q_first, r_first = _first(q_list), _first(r_list)
    sum_p = int(q_first[-1])
    nbytes = lib.bdm_knn_points_workspace_bytes(B, sum_p, k)
    assert nbytes >= 16 * (B + 1) and nbytes % 16 == 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {"idx": _guarded(sum_p * k, torch.int32), "d2": _guarded(sum_p * k, torch.float32)}
    q, r = _pack(q_list), _pack(r_list)
    ptr = lambda name: L.ptr(bufs[name][1]) if name in outputs else None   # noqa: E731
    rc = lib.bdm_knn_points(B, k, L.ptr(q), L.ptr(r), q_first.data_ptr(), r_first.data_ptr(), ptr("idx"), ptr("d2"), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(whole, body=name not in outputs) for name, (whole, _) in bufs.items()), "sentinels around (or a NULL) output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    idx = bufs["idx"][1].view(sum_p, k).cpu().long().split(np_) if "idx" in outputs else [None] * B
    d2 = bufs["d2"][1].view(sum_p, k).cpu().split(np_) if "d2" in outputs else [None] * B
    return list(zip(idx, d2))


def _assert_equal(name, got, want):
    for e, ((gi, gd), (wi, wd)) in enumerate(zip(got, want)):
        if gi is not None:
            bad = gi != wi
            assert torch.equal(gi, wi), f"{name} entry {e}: idx differs at {int(bad.sum())} of {gi.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"
        if gd is not None:
            bad = K.bits(gd) != K.bits(wd)
            assert torch.equal(K.bits(gd), K.bits(wd)), f"{name} entry {e}: d2 differs at {int(bad.sum())} of {gd.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"


# ---- the search -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_cases_equal_the_restatement(hip, name):
    c, want = K.case(name), K.case_ref(name)
    got = _call_knn(c["q"], c["r"], c["k"])
    print(f"{name}: k = {c['k']}, (P, R) = {[(q.shape[0], r.shape[0]) for q, r in zip(c['q'], c['r'])]}")
    _assert_equal(name, got, want)


def test_entries_alone_have_their_bits_of_the_batch_and_calls_repeat(hip):
    c = K.case("ragged")
    whole, again = _call_knn(c["q"], c["r"], c["k"]), _call_knn(c["q"], c["r"], c["k"])
    _assert_equal("repeat", again, whole)
    for j in (2, 0, 3, 1):
        _assert_equal(f"entry {j} alone", _call_knn(c["q"][j:j + 1], c["r"][j:j + 1], c["k"]), whole[j:j + 1])


@pytest.mark.parametrize("b", [31, 32, 33, 65])
def test_offsets_cross_the_launch_boundary_of_the_upload(hip, b):
    """The b + 1 offsets of each array travel 32 per launch (csrc/ragged.hip): b + 1 = 32, 33, 34 and 66 are one launch exactly full,
    one entry and two entries into a second launch, and two entries into a third.  A wrong or missing entry of a later launch
    mis-addresses every entry behind it.  Entry i: 1 + i % 3 queries and 1 + (i * 7) % 4 reference rows (none for every fifth entry)
    on the lattice of the "ties" case, whose squared distances are exact in float32."""
    lattice = K.case("ties")["q"][0][:64]
    rows = lambda start, n: lattice[(start + torch.arange(n)) % 64]   # noqa: E731
    q = [rows(3 * i, 1 + i % 3) for i in range(b)]
    r = [rows(11 * i + 1, 0 if i % 5 == 4 else 1 + (i * 7) % 4) for i in range(b)]
    _assert_equal(f"b = {b}", _call_knn(q, r, 2), K.knn_batch(q, r, 2))


def test_optional_outputs_may_be_null(hip):
    c, want = K.case("edges_k3"), K.case_ref("edges_k3")
    for kept in (("idx",), ("d2",), ()):
        _assert_equal(f"only {kept}", _call_knn(c["q"], c["r"], c["k"], outputs=kept), want)


def test_same_set_equals_knn_self(hip):
    """p1 == p2: the two-set search and the normals kernel's self search share knn_list.h, and must give the same indices."""
    from bdm_amd.knn import knn_points
    from bdm_amd.normals import knn_self
    x = torch.stack([K.cloud(300, 900), K.cloud(300, 901)]).cuda()
    assert torch.equal(knn_points(x, x, K=16).idx, knn_self(x, 16))


def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    c = K.case("ragged")
    B, k, c_attr = 4, 3, 3
    q, r = _pack(c["q"]), _pack(c["r"])
    qf, rf = _first(c["q"]), _first(c["r"])
    sum_p, sum_r = int(qf[-1]), int(rf[-1])
    attr = torch.rand(sum_r, c_attr, device="cuda")
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = {"idx": _guarded(sum_p * k, torch.int32), "d2": _guarded(sum_p * k, torch.float32), "out": _guarded(sum_p * c_attr, torch.float32)}
    p = {name: L.ptr(body) for name, (_, body) in bufs.items()}
    good_idx = torch.zeros(sum_p, k, dtype=torch.int32, device="cuda")
    good_d2 = torch.ones(sum_p, k, device="cuda")
    good_s = dict(b=B, k=k, queries=L.ptr(q), refs=L.ptr(r), q_first=qf.data_ptr(), r_first=rf.data_ptr(), idx=p["idx"], d2=p["d2"],
                  ws=L.ptr(ws), stream=L.stream())
    good_i = dict(b=B, k=k, c=c_attr, mode=1, eps=1e-8, fill=0.5, attr=L.ptr(attr), idx=L.ptr(good_idx), d2=L.ptr(good_d2),
                  q_first=qf.data_ptr(), r_first=rf.data_ptr(), out=p["out"], ws=L.ptr(ws), stream=L.stream())
    assert lib.bdm_knn_points(*good_s.values()) == 0 and lib.bdm_knn_interpolate(*good_i.values()) == 0
    torch.cuda.synchronize()
    for _, body in bufs.values():
        body.fill_(I_SENTINEL if body.dtype == torch.int32 else F_SENTINEL)
    down = qf.clone()
    down[2] = down[1] - 1
    late = rf + 1
    huge = torch.tensor([0, 1 << 31, 1 << 31, 1 << 31, 1 << 31])
    many = torch.tensor([0, 1 << 26, 1 << 26, 1 << 26, 1 << 26])          # 2^26 queries of 64 neighbours reach 2^31 entries
    bad_s = [dict(k=0), dict(k=65), dict(b=-1), dict(b=65536), dict(queries=None), dict(refs=None), dict(q_first=None), dict(r_first=None),
             dict(ws=None), dict(ws=L.ptr(ws) + 8), dict(q_first=down.data_ptr()), dict(r_first=late.data_ptr()), dict(q_first=huge.data_ptr()),
             dict(r_first=huge.data_ptr()), dict(q_first=many.data_ptr(), k=64), dict(idx=L.ptr(q)), dict(d2=L.ptr(r)), dict(d2=p["idx"]),
             dict(ws=p["d2"]), dict(ws=L.ptr(q))]
    for change in bad_s:
        assert lib.bdm_knn_points(*dict(good_s, **change).values()) == 1, change
        assert lib.bdm_last_error()
    bad_i = [dict(k=0), dict(k=65), dict(c=0), dict(c=17), dict(mode=2), dict(mode=-1), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")),
             dict(b=-1), dict(b=65536), dict(attr=None), dict(idx=None), dict(d2=None), dict(out=None), dict(q_first=None), dict(r_first=None),
             dict(ws=None), dict(ws=L.ptr(ws) + 4), dict(q_first=down.data_ptr()), dict(r_first=late.data_ptr()), dict(q_first=huge.data_ptr()),
             dict(out=L.ptr(attr)), dict(out=L.ptr(good_idx)), dict(out=L.ptr(good_d2)), dict(ws=p["out"]), dict(ws=L.ptr(attr))]
    for change in bad_i:
        assert lib.bdm_knn_interpolate(*dict(good_i, **change).values()) == 1, change
        assert lib.bdm_last_error()
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values()), "a refused call wrote to an output"
    # nothing to do: 0, and nothing is touched (not even NULL pointers are looked at)
    zero = torch.zeros(5, dtype=torch.int64)
    assert lib.bdm_knn_points(*dict(good_s, b=0, queries=None, q_first=None).values()) == 0
    assert lib.bdm_knn_points(*dict(good_s, q_first=zero.data_ptr(), queries=None, ws=None).values()) == 0
    assert lib.bdm_knn_interpolate(*dict(good_i, b=0, attr=None, r_first=None).values()) == 0
    assert lib.bdm_knn_interpolate(*dict(good_i, q_first=zero.data_ptr(), out=None, ws=None).values()) == 0
    torch.cuda.synchronize()
    assert all(_untouched(whole, body=True) for whole, _ in bufs.values())
    assert bool((ws[256:] == 0xA5).all())
    wb = lib.bdm_knn_points_workspace_bytes
    assert wb(-1, 10, 3) == 0 and wb(65536, 10, 3) == 0 and wb(1, 10, 0) == 0 and wb(1, 10, 65) == 0 and wb(1, 1 << 31, 1) == 0
    assert wb(1, 1 << 26, 64) == 0 and wb(1, -1, 3) == 0 and wb(65535, 10, 64) == 16 * 65536 and wb(0, 0, 1) == 16
    assert lib.bdm_knn_interpolate_workspace_bytes(-1) == 0 and lib.bdm_knn_interpolate_workspace_bytes(65536) == 0
    assert lib.bdm_knn_interpolate_workspace_bytes(4) == 80


# ---- the interpolation ----------------------------------------------------------------------------------------------------------------
def _call_interp(c, mode, fill, expect=0):
    from bdm_amd import _lib as L
    lib = L.lib()
    ic = K.interp_case()
    B, k = len(ic["np"]), ic["k"]
    q_first = torch.tensor([0] + ic["np"], dtype=torch.int64).cumsum(0)
    r_first = torch.tensor([0] + ic["nr"], dtype=torch.int64).cumsum(0)
    sum_p = int(q_first[-1])
    nbytes = lib.bdm_knn_interpolate_workspace_bytes(B)
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    whole, out = _guarded(sum_p * c, torch.float32)
    attr, idx, d2 = ic["attr"][c].cuda().contiguous(), ic["idx"].int().cuda().contiguous(), ic["d2"].cuda().contiguous()
    rc = lib.bdm_knn_interpolate(B, k, c, mode, K.EPS, fill, L.ptr(attr), L.ptr(idx), L.ptr(d2), q_first.data_ptr(), r_first.data_ptr(),
                                 L.ptr(out), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert _untouched(whole) and bool((ws[nbytes:] == 0xA5).all())
    return out.view(sum_p, c).cpu()


@pytest.mark.parametrize("c", K.INTERP_C)
@pytest.mark.parametrize("mode", (0, 1))
def test_interpolation_equals_the_restatement(hip, mode, c):
    for fill in (float("nan"), 0.5):
        got, want = _call_interp(c, mode, fill), K.interp_ref(c, mode, fill)
        bad = K.bits(got) != K.bits(want)
        assert torch.equal(K.bits(got), K.bits(want)), f"mode {mode}, c = {c}, fill = {fill}: {int(bad.sum())} entries differ, first {torch.nonzero(bad)[:3].tolist()}"
    assert bool((got[0] == 0.5).all()) and bool((got[12:] == 0.5).all())            # m == 0: the fill
    if mode == 0:
        ic = K.interp_case()
        assert torch.equal(got[1], ic["attr"][c][ic["idx"][1, 0]]) and torch.equal(got[2], ic["attr"][c][4])   # bit for bit


# ---- through Python -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_mesh(hip):
    """A 4096-point unit sphere through the chain: visibility-oriented normals -> surface nets."""
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import reconstruct_surface
    g = torch.Generator().manual_seed(0)
    pts = torch.nn.functional.normalize(torch.randn(1, 4096, 3, generator=g), dim=-1).cuda()
    verts, faces = reconstruct_surface(pts, estimate_pointcloud_normals(pts, 50, "visibility"))
    assert faces[0].shape[0] > 1000
    return pts[0], verts[0], faces[0]


def test_python_surface_equals_the_restatement(hip):
    from bdm_amd.knn import knn_packed, knn_points, transfer_point_attributes
    c, want = K.case("ragged"), K.case_ref("ragged")
    got = knn_packed([q.cuda() for q in c["q"]], [r.cuda() for r in c["r"]], c["k"])
    assert all(i.dtype == torch.int64 and i.is_cuda for i, _ in got)
    _assert_equal("knn_packed", [(i.cpu(), d.cpu()) for i, d in got], want)
    # the padded form with lengths: the same entries cut out of padded tensors
    P, R = 33, 1025
    p1, p2 = torch.zeros(4, P, 3), torch.zeros(4, R, 3)
    for j in range(4):
        p1[j, :c["q"][j].shape[0]], p2[j, :c["r"][j].shape[0]] = c["q"][j], c["r"][j]
    l1, l2 = torch.tensor([q.shape[0] for q in c["q"]]), torch.tensor([r.shape[0] for r in c["r"]])
    res = knn_points(p1.cuda(), p2.cuda(), l1, l2, K=3, return_nn=True)
    assert res.dists.shape == (4, P, 3) and res.idx.dtype == torch.int64 and res.knn.shape == (4, P, 3, 3)
    for j in range(4):
        wi, wd = want[j]
        n = wi.shape[0]
        assert torch.equal(res.idx[j, :n].cpu(), wi.clamp_min(0)) and torch.equal(res.dists[j, :n].cpu(), torch.where(wi < 0, torch.zeros(()), wd))
        assert int(res.idx[j, n:].abs().sum()) == 0 and float(res.dists[j, n:].abs().sum()) == 0.0
    assert torch.equal(res.knn[0, :17].cpu(), torch.where((want[0][0] >= 0)[..., None], c["r"][0][want[0][0].clamp_min(0)], torch.zeros(())))
    assert float(res.knn[2].abs().sum()) == 0.0 and float(res.knn[3, :5, 2].abs().sum()) == 0.0     # an empty set; a set of two at K = 3
    # the transfer: both kernels behind one call
    attrs = [torch.rand(r.shape[0], 3, generator=torch.Generator().manual_seed(7 + j)) for j, r in enumerate(c["r"])]
    for mode, m in (("nearest", 0), ("idw", 1)):
        outs = transfer_point_attributes([q.cuda() for q in c["q"]], [r.cuda() for r in c["r"]], [a.cuda() for a in attrs], K=3, mode=mode, fill=0.25)
        for j in range(4):
            ref = K.interpolate(attrs[j], want[j][0], want[j][1], m, K.EPS, 0.25)
            assert torch.equal(K.bits(outs[j].cpu()), K.bits(ref)), (mode, j)


def test_colours_of_a_reconstructed_sphere_follow_the_affine_map(hip, sphere_mesh):
    """The cloud is coloured by c = (p + 1) / 2, a map with Lipschitz constant 0.5 (per channel, in the Euclidean norm of p).  A
    vertex colour is a convex combination (weights w_l / W >= 0 that add up to 1) of the colours of its K = 3 neighbours, which lie
    no farther from the vertex than sqrt(max_l d2_l): so it is within 0.5 * sqrt(max_l d2_l) of (v + 1) / 2, plus the rounding of the
    float32 evaluation, four ulp (of 1, the largest colour).  Derived, not tuned."""
    from bdm_amd.knn import transfer_point_attributes
    pts, verts, _ = sphere_mesh
    outs, knn = transfer_point_attributes([verts], [pts], [(pts + 1.0) / 2.0], K=3, mode="idw", return_knn=True)
    idx, d2 = knn[0]
    assert outs[0].shape == (verts.shape[0], 3) and bool((idx >= 0).all())
    bound = 0.5 * d2.double().max(dim=1).values.sqrt() + 4 * 2.0 ** -23
    err = (outs[0].double() - (verts.double() + 1.0) / 2.0).abs().max(dim=1).values
    print(f"{verts.shape[0]} vertices: largest colour error {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}, "
          f"mean nearest distance {float(d2[:, 0].sqrt().mean()):.4f}")
    assert bool((err <= bound).all())
    ri, rd = K.knn(verts.cpu(), pts.cpu(), 3)
    assert torch.equal(idx.cpu(), ri) and torch.equal(K.bits(d2.cpu()), K.bits(rd))
    assert torch.equal(K.bits(outs[0].cpu()), K.bits(K.interpolate(((pts + 1.0) / 2.0).cpu(), ri, rd, 1)))


def test_cli_colours_a_tree_and_prints_the_composed_json(hip, sphere_mesh, tmp_path):
    """python -m bdm_amd.mesh_color in a child process on two meshes with coloured clouds (one of them empty) and one mesh without: the
    JSON line is the one composed by hand from the restatement, and the files carry the restatement's colours."""
    from bdm_amd import mesh_color as MC
    from bdm_amd.io import load_mesh_ply, load_pointcloud_ply, save_mesh_ply, save_pointcloud_ply_rgb
    pts, verts, faces = (t.cpu() for t in sphere_mesh)
    small_v, small_f = verts[:200], faces[(faces < 200).all(1)]
    save_mesh_ply(small_v.numpy(), small_f.numpy(), tmp_path / "mesh" / "a" / "sphere.ply")
    save_mesh_ply((small_v[:50] * 0.5).numpy(), small_f[(small_f < 50).all(1)].numpy(), tmp_path / "mesh" / "b" / "half.ply")
    save_mesh_ply(small_v.numpy(), small_f.numpy(), tmp_path / "mesh" / "c" / "unmatched.ply")
    save_pointcloud_ply_rgb(pts[:1500].numpy(), ((pts[:1500] + 1.0) / 2.0).numpy(), tmp_path / "col" / "a" / "sphere.ply")
    save_pointcloud_ply_rgb(np.zeros((0, 3)), np.zeros((0, 3)), tmp_path / "col" / "b" / "half.ply")
    out = subprocess.run([sys.executable, "-m", "bdm_amd.mesh_color", "--mesh_dir", str(tmp_path / "mesh"), "--color_dir", str(tmp_path / "col"),
                          "--out_dir", str(tmp_path / "out")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    cloud, colours = (torch.from_numpy(x) for x in load_pointcloud_ply(tmp_path / "col" / "a" / "sphere.ply", with_colors=True))
    idx, d2 = K.knn(small_v, cloud, 3)
    want = MC.compose_result(2, 250, 50, float(d2[:, 0].double().sqrt().sum()))
    print(out.stdout.strip().splitlines()[-1])
    assert got == want and got["mean_nearest_distance"] < 0.1
    assert sorted(str(p.relative_to(tmp_path / "out")) for p in (tmp_path / "out").rglob("*.ply")) == ["a/sphere.ply", "b/half.ply"]
    v, f, c = load_mesh_ply(tmp_path / "out" / "a" / "sphere.ply", with_colors=True)
    ref = K.interpolate(colours, idx, d2, 1, K.EPS, MC.GREY)
    assert np.array_equal(v, small_v.numpy()) and np.array_equal(f, small_f.numpy())
    assert np.array_equal(c, np.rint(np.clip(ref.double().numpy(), 0.0, 1.0) * 255.0).astype(np.float32) / np.float32(255.0))
    _, _, grey = load_mesh_ply(tmp_path / "out" / "b" / "half.ply", with_colors=True)
    assert np.array_equal(grey, np.full((50, 3), np.float32(128.0) / np.float32(255.0)))


def test_vert_albedo_equals_the_restatement_fed_the_same_colours(hip):
    """render_mesh_batch(shading="smooth" / "flat", vert_albedo=...) equals tests/mesh_render_ref.py fed the per-vertex (per-face)
    colours composed from the same albedo, normals and camera by shade_by_normals.  The vertex normals are pinned (an icosphere's are
    its normalised vertices): Meshes.verts_normals_packed sums in an order that is not fixed."""
    import mesh_render_ref as M
    from bdm_amd.cameras import Meshes
    from bdm_amd.render import BACKGROUND, render_mesh_batch, shade_by_normals
    v, f = M.icosphere(2, 0.4)
    cam = M._persp()
    H = W = 48
    meshes = Meshes([v.cuda()], [f.cuda()])
    normals = torch.nn.functional.normalize(v, dim=-1).cuda()
    meshes.verts_normals_packed = lambda: normals
    albedo = ((v / 0.4 + 1.0) / 2.0).cuda()
    smooth = render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="smooth", vert_albedo=albedo).cpu()[0]
    colours = shade_by_normals(v.cuda()[None], normals[None], cam.to("cuda"), albedo=albedo, two_sided=False)[0].float().cpu()
    want = M.render(v, f, cam.packed()[0], H, W, vert_features=colours, background=BACKGROUND)
    covered = want["pix_to_face"] >= 0
    assert int(covered.sum()) > 200 and torch.equal(smooth, want["image"])
    grey = render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="smooth").cpu()[0]
    assert not torch.equal(grey, smooth) and float((smooth[covered].max(0).values - smooth[covered].min(0).values).max()) > 0.2
    assert torch.equal(render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="smooth", vert_albedo=torch.full_like(albedo, 0.8)).cpu()[0], grey)
    flat = render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="flat", vert_albedo=albedo).cpu()[0]
    a = albedo[f.cuda()]
    face_albedo = ((a[:, 0] + a[:, 1]) + a[:, 2]) / 3.0
    tri = v.cuda()[f.cuda()]
    fcol = shade_by_normals(tri.mean(1)[None], meshes.faces_normals_packed()[None], cam.to("cuda"), albedo=face_albedo, two_sided=False)[0].float().cpu()
    assert torch.equal(flat, M.render(v, f, cam.packed()[0], H, W, face_features=fcol, background=BACKGROUND)["image"])
