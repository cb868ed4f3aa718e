"""bdm_render_meshes (csrc/mesh_render.hip) and its Python surface on the GPU against the CPU restatement tests/mesh_render_ref.py:
pix_to_face, zbuf, bary (as bits) and the image with torch.equal in every case, the bit-exact pins, the error paths, and the feature
end to end.

Coverage is integer and every float operation of the rule is rounded on its own, so nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_render_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
I_SENTINEL, F_SENTINEL = -7777, 1234.5
OUTPUTS = ("pix_to_face", "zbuf", "bary", "image")


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * PAD,), I_SENTINEL if dtype == torch.int32 else F_SENTINEL, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + numel]


def _untouched(whole, body=False):
    s = I_SENTINEL if whole.dtype == torch.int32 else F_SENTINEL
    part = whole if body else torch.cat([whole[:PAD], whole[-PAD:]])
    return bool((part == s).all())


def _inputs(c):
    """Device and host arrays of a case in the ABI's form; an empty side still gets one (unread) row: no NULL among the inputs."""
    nv, nf = [v.shape[0] for v in c["verts"]], [f.shape[0] for f in c["faces"]]
    verts = torch.cat(c["verts"]).cuda() if sum(nv) else torch.zeros(1, 3, device="cuda")
    faces = torch.cat(c["faces"]).int().cuda() if sum(nf) else torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    return {"b": len(nv), "verts": verts.contiguous(), "faces": faces.contiguous(), "vert_first": torch.tensor([0] + nv).cumsum(0),
            "face_first": torch.tensor([0] + nf).cumsum(0), "cams": c["cams"].cuda().contiguous(), "sum_v": sum(nv), "sum_f": sum(nf)}


def _call(c, channels=3, vert_features=None, face_features=None, outputs=OUTPUTS, cull=None, expect=0):
    """One ABI call on guarded outputs and a workspace pre-filled with 0xA5 -> the dict of mesh_render_ref.render_batch (host)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    a = _inputs(c)
    B, H, W = a["b"], c["H"], c["W"]
    nbytes = lib.bdm_render_meshes_workspace_bytes(B, a["sum_v"], a["sum_f"], H, W)
    assert nbytes >= 8 * B * H * W + 16 * a["sum_v"]
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    shapes = {"pix_to_face": ((B, H, W), torch.int32), "zbuf": ((B, H, W), torch.float32), "bary": ((B, H, W, 3), torch.float32),
              "image": ((B, H, W, channels), torch.float32)}
    bufs = {k: _guarded(int(np.prod(s)), dt) for k, (s, dt) in shapes.items()}
    vf = None if vert_features is None else vert_features.cuda().contiguous()
    ff = None if face_features is None else face_features.cuda().contiguous()
    bg = torch.tensor(M.BACKGROUND[:channels], device="cuda")
    ptr = lambda k: L.ptr(bufs[k][1]) if k in outputs else None   # noqa: E731
    rc = lib.bdm_render_meshes(B, H, W, channels, int(c["ortho"]), int(c["cull"] if cull is None else cull), L.ptr(a["verts"]), L.ptr(a["faces"]),
                               a["vert_first"].data_ptr(), a["face_first"].data_ptr(), L.ptr(a["cams"]), L.ptr(vf), L.ptr(ff), L.ptr(bg),
                               ptr("pix_to_face"), ptr("zbuf"), ptr("bary"), ptr("image"), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, lib.bdm_last_error()
    assert all(_untouched(whole, body=k not in outputs) for k, (whole, _) in bufs.items()), "sentinels around (or a NULL) output were overwritten"
    assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were overwritten"
    return {k: (bufs[k][1].view(shapes[k][0]).cpu() if k in outputs else None) for k in OUTPUTS}


def _assert_equal(name, got, want, keys=OUTPUTS):
    for k in keys:
        g, w = got[k], want[k]
        if g is None and w is None:
            continue
        gb, wb = (g.view(torch.int32), w.view(torch.int32)) if g.dtype == torch.float32 else (g, w)
        bad = gb != wb
        assert torch.equal(gb, wb), f"{name}: {k} differs at {int(bad.sum())} of {g.numel()} entries, first {torch.nonzero(bad)[:3].tolist()}"


@pytest.mark.parametrize("name", list(M.CASES))
def test_cases_equal_the_restatement(hip, name):
    c = M.case(name)
    want = dict(M.case_ref(name))
    want["image"] = torch.where((want["pix_to_face"] >= 0)[..., None], torch.zeros(3), torch.tensor(M.BACKGROUND[:3]))   # no features: zeros
    got = _call(c)
    print(f"{name}: {int((want['pix_to_face'] >= 0).sum())} covered pixels, at most {int(want['count'].max())} fragments in one")
    _assert_equal(name, got, want)


def test_batch_rows_equal_single_calls_and_calls_repeat(hip):
    c = M.case("batch3_24x40")
    whole, again = _call(c), _call(c)
    _assert_equal("repeat", again, whole)
    for j in (2, 0, 1):
        alone = dict(c, verts=c["verts"][j:j + 1], faces=c["faces"][j:j + 1], cams=c["cams"][j:j + 1])
        _assert_equal(f"mesh {j} alone", _call(alone), {k: whole[k][j:j + 1] for k in OUTPUTS})


def _blank_image(want):
    """The restatement's fragments plus the image of a call without features: zeros where a face shows, the background elsewhere."""
    return dict(want, image=torch.where((want["pix_to_face"] >= 0)[..., None], torch.zeros(3), torch.tensor(M.BACKGROUND[:3])))


def _boxes_16_and_17():
    """Four right triangles with their vertices ON pixel centres of a 32 x 32 image, legs along the axes: boxes of 16 x 16, 17 x 16,
    16 x 17 and 17 x 17 pixel centres, wound alternately, each at its own depth (they share pixel column 15 and row 15)."""
    corners = [((0, 0), (15, 0), (0, 15)), ((31, 0), (15, 0), (31, 15)), ((0, 31), (0, 15), (15, 31)), ((31, 31), (31, 15), (15, 31))]
    verts = torch.cat([M.on_centres(list(tri), 32, 32, z=0.1 * k) for k, tri in enumerate(corners)])
    faces = torch.tensor([[0, 1, 2], [3, 5, 4], [6, 8, 7], [9, 10, 11]])
    return M._case([verts], [faces], M.ortho_pixel_camera(), 32, 32)


def _box_sizes(c, mesh=0):
    """(columns, rows) of pixel centres 256 i + 128 inside each face's bounding box, from the snapped coordinates, clamped to the image."""
    sx, sy, _, usable = M.project(c["verts"][mesh], c["cams"][mesh], c["H"], c["W"], c["ortho"])
    assert bool(usable.all())
    sizes = []
    for f in c["faces"][mesh]:
        n = []
        for s, size in ((sx[f], c["W"]), (sy[f], c["H"])):
            first, last = max(-((128 - int(s.min())) // 256), 0), min((int(s.max()) - 128) // 256, size - 1)
            n.append(last - first + 1)
        sizes.append(tuple(n))
    return sizes


def test_boxes_of_16_centres_are_walked_by_a_lane_and_boxes_of_17_by_the_wave(hip):
    """The threshold between the two walks of tri_walk_boxes, both kinds in one call; the restatement knows of neither."""
    c = _boxes_16_and_17()
    assert _box_sizes(c) == [(16, 16), (17, 16), (16, 17), (17, 17)]
    want = M.render_batch(c["verts"], c["faces"], c["cams"], 32, 32, True, False)
    assert sorted(set(want["pix_to_face"].flatten().tolist())) == [-1, 0, 1, 2, 3]
    for mutant in ("own_never", "own_always"):   # centres lie ON the legs: the tie rule decides pixels here
        assert not torch.equal(M.render_batch(c["verts"], c["faces"], c["cams"], 32, 32, True, False, mutant=mutant)["pix_to_face"], want["pix_to_face"])
    _assert_equal("boxes of 16 and 17", _call(c), _blank_image(want))


def _two_meshes_with_a_large_face_each():
    """Two meshes of three small faces and one triangle over the whole 32 x 32 image each: eight packed rows, so both large faces sit
    in the first wave, with different meshes.  The small faces lie nearer to the camera than the large one of their mesh."""
    from bdm_amd.cameras import join_cameras
    small = [[(3, 3), (9, 4), (5, 10)], [(20, 6), (27, 5), (24, 12)], [(8, 20), (15, 22), (10, 28)]]
    large = [[(-2, -2), (70, -2), (-2, 70)], [(33, 33), (-70, 33), (33, -70)]]
    verts, faces = [], []
    for m in range(2):
        sv = torch.cat([M.on_centres([(i + 2 * m, j + m) for i, j in tri], 32, 32, z=-0.5 + 0.1 * k) for k, tri in enumerate(small)])
        lv = M.on_centres(large[m], 32, 32)
        lv[:, 2] = torch.tensor([0.0, 0.3, 0.6]) + 0.05 * m
        verts.append(torch.cat([sv, lv]))
        faces.append(torch.tensor([[0, 1, 2], [3, 5, 4], [6, 7, 8], [9, 10, 11] if m == 0 else [9, 11, 10]]))
    cam = M.ortho_pixel_camera()
    return M._case(verts, faces, join_cameras([cam, cam]), 32, 32)


def test_two_large_faces_of_different_meshes_share_a_wave(hip):
    """The raster kernel's grid runs over the packed faces, so one wave holds faces of several meshes: what is broadcast for a large
    face has to carry its mesh."""
    c = _two_meshes_with_a_large_face_each()
    assert sum(f.shape[0] for f in c["faces"]) == 8
    for m in range(2):
        sizes = _box_sizes(c, m)
        assert sizes[3] == (32, 32) and all(max(s) <= 16 for s in sizes[:3])
    want = M.render_batch(c["verts"], c["faces"], c["cams"], 32, 32, True, False)
    for m in range(2):
        shown = want["pix_to_face"][m]
        assert int((shown == 3).sum()) > 900 and int((shown >= 0).sum()) == 1024 and all(int((shown == k).sum()) > 5 for k in range(3))
    assert not torch.equal(want["zbuf"][0], want["zbuf"][1])
    whole = _call(c)
    _assert_equal("two meshes", whole, _blank_image(want))
    for j in (1, 0):
        alone = dict(c, verts=c["verts"][j:j + 1], faces=c["faces"][j:j + 1], cams=c["cams"][j:j + 1])
        _assert_equal(f"mesh {j} alone", _call(alone), {k: whole[k][j:j + 1] for k in OUTPUTS})


def test_a_face_with_a_repeated_index_is_no_face(hip):
    """Faces (0, 1, 1) and (2, 2, 2) around a good face: the good face keeps its index 1 and its pixels, the others show nowhere."""
    verts = M.on_centres([[2, 8], [13, 8], [7, 2]], 16, 16)
    faces = torch.tensor([[0, 1, 1], [0, 1, 2], [2, 2, 2]])
    cam = M.ortho_pixel_camera()
    trio, alone = M._case([verts], [faces], cam, 16, 16), M._case([verts], [faces[1:2]], cam, 16, 16)
    got, single = _call(trio), _call(alone)
    assert int((single["pix_to_face"] == 0).sum()) > 10
    assert torch.equal(got["pix_to_face"], torch.where(single["pix_to_face"] >= 0, 1, -1).int())
    _assert_equal("good face alone", got, single, keys=("zbuf", "bary", "image"))
    _assert_equal("repeated indices", got, _blank_image(M.render_batch(trio["verts"], trio["faces"], trio["cams"], 16, 16, True, False)))


@pytest.mark.parametrize("per", ["vert", "face"])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_images_from_features(hip, channels, per):
    c = M.case(M.FEATURE_CASE)
    feats = M.case_features(M.FEATURE_CASE, channels, per)
    kw = {f"{per}_features": feats}
    want = M.render_batch(c["verts"], c["faces"], c["cams"], c["H"], c["W"], c["ortho"], c["cull"], background=M.BACKGROUND[:channels], **kw)
    assert int((want["pix_to_face"] >= 0).sum()) > 100
    _assert_equal(f"{per} features, c = {channels}", _call(c, channels, **kw), want)
    batch = M.case("batch3_24x40")
    feats = M.case_features("batch3_24x40", channels, per)
    kw = {f"{per}_features": feats}
    want = M.render_batch(batch["verts"], batch["faces"], batch["cams"], 24, 40, False, False, background=M.BACKGROUND[:channels], **kw)
    _assert_equal(f"batch, {per} features, c = {channels}", _call(batch, channels, **kw), want)


def test_every_output_may_be_null(hip):
    c = M.case("sphere_24x40_ortho_cull0")
    vf = M.case_features("sphere_24x40_ortho_cull0", 3, "vert")
    full = _call(c, vert_features=vf)
    for leave_out in OUTPUTS:
        kept = tuple(k for k in OUTPUTS if k != leave_out)
        _assert_equal(f"without {leave_out}", _call(c, vert_features=vf, outputs=kept), full, kept)
    for only in OUTPUTS:
        _assert_equal(f"only {only}", _call(c, vert_features=vf, outputs=(only,)), full, (only,))
    _call(c, vert_features=vf, outputs=())


def test_every_documented_limit_returns_1_and_launches_nothing(hip):
    from bdm_amd import _lib as L
    lib = L.lib()
    c = M.case("batch3_24x40")
    a = _inputs(c)
    H, W, B = 24, 40, 3
    ws = torch.zeros(lib.bdm_render_meshes_workspace_bytes(4, a["sum_v"], a["sum_f"], 64, 64), dtype=torch.uint8, device="cuda")
    vf, ff = torch.rand(a["sum_v"], 4, device="cuda"), torch.rand(a["sum_f"], 4, device="cuda")
    bg = torch.zeros(4, device="cuda")
    bufs = {"pix_to_face": _guarded(4 * 64 * 64, torch.int32), "zbuf": _guarded(4 * 64 * 64, torch.float32),
            "bary": _guarded(4 * 64 * 64 * 3, torch.float32), "image": _guarded(4 * 64 * 64 * 4, torch.float32)}
    good = dict(b=B, h=H, w=W, c=3, ortho=0, cull=0, verts=L.ptr(a["verts"]), faces=L.ptr(a["faces"]), vert_first=a["vert_first"].data_ptr(),
                face_first=a["face_first"].data_ptr(), cams=L.ptr(a["cams"]), vf=L.ptr(vf), ff=None, bg=L.ptr(bg),
                pix_to_face=L.ptr(bufs["pix_to_face"][1]), zbuf=L.ptr(bufs["zbuf"][1]), bary=L.ptr(bufs["bary"][1]), image=L.ptr(bufs["image"][1]),
                ws=L.ptr(ws))
    order = list(good)

    def call(**kw):
        p = {**good, **kw}
        rc = lib.bdm_render_meshes(*[p[k] for k in order], L.stream())
        torch.cuda.synchronize()
        return rc

    dec_v, dec_f, late = a["vert_first"].clone(), a["face_first"].clone(), a["vert_first"].clone()
    dec_v[1], dec_f[2], late[0] = dec_v[2] + 1, dec_f[1] - 1, 1
    huge = torch.tensor([0, 2 ** 31, 2 ** 31, 2 ** 31])
    as_f = lambda t: t.view(torch.float32)   # noqa: E731
    bad = {"b < 0": dict(b=-1), "h = 0": dict(h=0), "w = 0": dict(w=0), "h = 4097": dict(h=4097), "w = 4097": dict(w=4097), "c = 0": dict(c=0),
           "c = 5": dict(c=5), "ortho = 2": dict(ortho=2), "cull = -1": dict(cull=-1), "b h w = 2^31": dict(b=128, h=4096, w=4096),
           "both features": dict(ff=L.ptr(ff)), "vertex offsets decrease": dict(vert_first=dec_v.data_ptr()),
           "face offsets decrease": dict(face_first=dec_f.data_ptr()), "offsets start at 1": dict(vert_first=late.data_ptr()),
           "sum V = 2^31": dict(vert_first=huge.data_ptr()), "sum F = 2^31": dict(face_first=huge.data_ptr()),
           "image without background": dict(bg=None),
           **{f"no {k}": {k: None} for k in ("verts", "faces", "vert_first", "face_first", "cams", "ws")},
           "zbuf = verts": dict(zbuf=L.ptr(a["verts"])), "pix_to_face = faces": dict(pix_to_face=L.ptr(a["faces"])),
           "image = features": dict(image=L.ptr(vf)), "bary = cameras": dict(bary=L.ptr(a["cams"])), "image = background": dict(image=L.ptr(bg)),
           "workspace = verts": dict(ws=L.ptr(a["verts"])), "workspace = zbuf": dict(ws=L.ptr(bufs["zbuf"][1])),
           "zbuf inside bary": dict(zbuf=L.ptr(bufs["bary"][1][8:])), "image inside the workspace": dict(image=L.ptr(as_f(ws[1024:])))}
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc == 1 and lib.bdm_last_error(), what
        assert all(_untouched(whole, body=True) for whole, _ in bufs.values()), what
        assert bool((ws == 0).all()), what
    assert lib.bdm_render_meshes_workspace_bytes(-1, 10, 10, 16, 16) == 0 and lib.bdm_render_meshes_workspace_bytes(1, 2 ** 31, 10, 16, 16) == 0
    assert lib.bdm_render_meshes_workspace_bytes(1, 10, 10, 4097, 16) == 0 and lib.bdm_render_meshes_workspace_bytes(128, 10, 10, 4096, 4096) == 0
    assert lib.bdm_render_meshes_workspace_bytes(16, 100000, 200000, 224, 224) >= 16 * 224 * 224 * 8 + 1600000
    assert lib.bdm_render_meshes(0, H, W, 3, 0, 0, *([None] * 13), L.stream()) == 0
    assert call() == 0                                                                 # the good call is good
    assert not _untouched(bufs["zbuf"][0], body=True) and _untouched(bufs["zbuf"][0])


# ---- through the public interface -----------------------------------------------------------------------------------------------------
def test_python_fragments_and_images(hip):
    from bdm_amd.cameras import Meshes
    from bdm_amd.render import rasterize_meshes, render_mesh_batch
    c = M.case("batch3_24x40")
    want = M.case_ref("batch3_24x40")
    meshes = Meshes([v.cuda() for v in c["verts"]], [f.cuda() for f in c["faces"]])
    frag = rasterize_meshes(c["camera"].to("cuda"), meshes, image_size=(24, 40))
    assert frag.pix_to_face.dtype == torch.int64 and frag.pix_to_face.shape == (3, 24, 40, 1) and frag.bary_coords.shape == (3, 24, 40, 1, 3)
    assert torch.equal(frag.pix_to_face[..., 0].cpu().int(), want["pix_to_face"]) and torch.equal(frag.zbuf[..., 0].cpu(), want["zbuf"])
    assert torch.equal(frag.bary_coords[:, :, :, 0].cpu(), want["bary"])
    cols = M.case_features("batch3_24x40", 3, "vert")
    img = render_mesh_batch(c["camera"].to("cuda"), meshes, image_size=(24, 40), shading="none", vert_colors=cols.cuda(), background_color=M.BACKGROUND[:3])
    ref = M.render_batch(c["verts"], c["faces"], c["cams"], 24, 40, vert_features=cols, background=M.BACKGROUND[:3])
    assert torch.equal(img.cpu(), ref["image"])
    black = render_mesh_batch(c["camera"].to("cuda"), meshes, image_size=(24, 40), shading="none", background_color=M.BACKGROUND[:3]).cpu()
    assert torch.equal(black, torch.where((want["pix_to_face"] >= 0)[..., None], torch.zeros(3), torch.tensor(M.BACKGROUND[:3])))
    sphere = M.case("sphere_64x64_persp_cull1")
    one = Meshes([sphere["verts"][0].cuda()], [sphere["faces"][0].cuda()])
    culled = rasterize_meshes(sphere["camera"].to("cuda"), one, image_size=64, cull_backfaces=True)
    assert torch.equal(culled.pix_to_face[..., 0].cpu().int(), M.case_ref("sphere_64x64_persp_cull1")["pix_to_face"])
    empty = render_mesh_batch(sphere["camera"].to("cuda"), Meshes([torch.zeros(0, 3, device="cuda")], [torch.zeros(0, 3, dtype=torch.int64, device="cuda")]),
                              image_size=8).cpu()
    from bdm_amd.render import BACKGROUND
    assert torch.equal(empty, torch.tensor(BACKGROUND).expand(1, 8, 8, 3))                # no face anywhere: the default background


def test_face_indices_beyond_int32_are_invalid_not_wrapped(hip):
    """Face 1 is given as int64 2^32 + (0, 1, 3): cast to int32 it would wrap onto (0, 1, 3), which lies below the side it shares with
    face 0, nearer to the camera, over pixel centres face 0 does not cover.  It is no face of the mesh: no pixel shows it, and the
    covered set is that of face 0 alone."""
    from bdm_amd.cameras import Meshes
    from bdm_amd.render import rasterize_meshes
    verts = M.on_centres([[2, 8], [13, 8], [7, 2], [7, 14]], 16, 16)
    verts[3, 2] = -0.5
    faces = torch.tensor([[0, 1, 2], [2 ** 32, 2 ** 32 + 1, 2 ** 32 + 3]])
    assert faces.dtype == torch.int64 and faces[1].int().tolist() == [0, 1, 3]
    cam = M.ortho_pixel_camera()
    wrapped = M.render(verts, torch.tensor([[0, 1, 3]]), cam.packed()[0], 16, 16, ortho=True)["pix_to_face"] >= 0

    def pix_to_face(f):
        return rasterize_meshes(cam.to("cuda"), Meshes([verts.cuda()], [f.cuda()]), image_size=16).pix_to_face[0, :, :, 0].cpu()
    got, alone = pix_to_face(faces), pix_to_face(faces[:1])
    assert int((alone >= 0).sum()) > 10 and int((wrapped & (alone < 0)).sum()) > 10   # both triangles are visible, on different pixels
    assert not bool((got == 1).any()) and torch.equal(got >= 0, alone >= 0)


def test_reconstructed_sphere_flat_and_smooth(hip):
    """reconstruct_surface on the 4096-point sphere, drawn: "flat" equals the restatement fed the same face colours; "smooth" is
    checked by what does not depend on the order of the vertex-normal sum: the covered mask, and the range of the colours,
    [ambient * albedo, albedo] widened by 8 ulp of albedo -- a barycentric sum of three values of that range with weights that add up
    to 1 within 4 float32 roundings, after a Lambert term whose unit vectors are unit within a few ulp."""
    import surface_ref as S
    from bdm_amd.cameras import Meshes
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.render import BACKGROUND, rasterize_meshes, render_mesh_batch, shade_by_normals
    from bdm_amd.surface import reconstruct_surface
    pts, _ = S.sphere(torch.Generator().manual_seed(3206), 4096)
    dev = pts[None].cuda()
    verts, faces = reconstruct_surface(dev, estimate_pointcloud_normals(dev, 16, "visibility"))
    meshes = Meshes(verts, faces)
    assert faces[0].shape[0] > 2000
    cam = M._persp()
    H = W = 96
    flat = render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="flat").cpu()
    tri = verts[0][faces[0]]
    colours = shade_by_normals(tri.mean(1)[None], meshes.faces_normals_packed()[None], cam.to("cuda"), two_sided=False)[0].float().cpu()
    want = M.render(verts[0].cpu(), faces[0].cpu(), cam.packed()[0], H, W, face_features=colours, background=BACKGROUND)
    covered = want["pix_to_face"] >= 0
    print(f"reconstructed sphere: {faces[0].shape[0]} faces, {int(covered.sum())} covered pixels of {H * W}")
    assert int(covered.sum()) > 1000 and torch.equal(flat[0], want["image"])
    frag = rasterize_meshes(cam.to("cuda"), meshes, image_size=H)
    assert torch.equal(frag.pix_to_face[0, :, :, 0].cpu().int(), want["pix_to_face"]) and torch.equal(frag.zbuf[0, :, :, 0].cpu(), want["zbuf"])
    smooth = render_mesh_batch(cam.to("cuda"), meshes, image_size=H, shading="smooth", ambient=0.3).cpu()[0]
    bg = torch.tensor(BACKGROUND)
    assert torch.equal(smooth[~covered], bg.expand(int((~covered).sum()), 3))
    assert bool((smooth[covered] != bg).any(-1).all())                               # the covered mask is pix_to_face >= 0
    slack = 8 * float(np.spacing(np.float32(0.8)))
    lo, hi = float(smooth[covered].min()), float(smooth[covered].max())
    print(f"smooth shading: covered values in [{lo:.6f}, {hi:.6f}], allowed [{0.3 * 0.8 - slack:.6f}, {0.8 + slack:.6f}]")
    assert 0.3 * 0.8 - slack <= lo and hi <= 0.8 + slack and hi - lo > 0.2


def test_orbit_of_a_mesh(hip, tmp_path):
    from bdm_amd.cameras import Meshes, OrthographicCameras, look_at_view_transform
    from bdm_amd.render import BACKGROUND, render_mesh_batch, visualize_mesh_batch
    from PIL import Image
    v, f = M.icosphere(2, 3.0)                                        # the orbit's focal length of 0.25 makes this 18 pixels at 48 x 48
    v = v * torch.tensor([1.0, 0.6, 0.4])
    meshes = Meshes([v.cuda(), (v * 0.5).cuda()], [f.cuda(), f.cuda()])
    grids = visualize_mesh_batch(meshes, output_file_image=str(tmp_path / "o" / "x.png"), num_frames=3, shading="flat", image_size=48)
    assert grids.shape == (3, 3, 2 * 50 + 2, 50 + 2) and sorted(os.listdir(tmp_path / "o")) == ["x-0.png", "x-1.png", "x-2.png"]
    Rm, T = look_at_view_transform(10.0, 30, [0, 120, 240])
    for fr in (0, 2):
        cam = OrthographicCameras(focal_length=0.25, R=Rm[fr:fr + 1], T=T[fr:fr + 1], device="cuda")
        for b in range(2):
            one = render_mesh_batch(cam, Meshes(meshes.verts_list()[b:b + 1], meshes.faces_list()[b:b + 1]), image_size=48, shading="flat").cpu()[0]
            assert torch.equal(grids[fr][:, 2 + b * 50:2 + b * 50 + 48, 2:50].permute(1, 2, 0), one)
            ref = M.render(meshes.verts_list()[b].cpu(), f, cam.packed()[0].cpu(), 48, 48, ortho=True)
            assert torch.equal((one != torch.tensor(BACKGROUND)).any(-1), ref["pix_to_face"] >= 0) and int((ref["pix_to_face"] >= 0).sum()) > 20
            assert float(one[ref["pix_to_face"] >= 0].max()) > 0.7                    # lit from the viewer's side: not the ambient 0.24 alone
        png = np.asarray(Image.open(tmp_path / "o" / f"x-{fr}.png"))
        assert np.array_equal(png, (grids[fr].numpy() * 255.0).astype(np.uint8).transpose(1, 2, 0))
    single = visualize_mesh_batch(meshes, output_file_image=str(tmp_path / "single.png"), image_size=48)
    assert single.shape == (1, 3, 102, 52) and (tmp_path / "single.png").exists()


def test_command_line_draws_the_mesh_tree(hip, tmp_path):
    """main_render.py dataset=synthetic on a tiny sample directory with a pred_mesh tree, in a fresh child process: renders/mesh and
    renders/mesh_orbit hold one picture per mesh (and frame), of the right size, with pixels that are not background."""
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    from PIL import Image
    batch = next(iter(SyntheticShapes(range(2), 2, seed=42, image_size=224, num_points=1024)))
    names = list(batch.sequence_name)
    v, f = M.icosphere(2, 0.3)
    for j, name in enumerate(names):
        save_mesh_ply((v * (1.0 + 0.3 * j)).numpy(), f.numpy(), tmp_path / "pred_mesh" / "chair" / f"{name}.ply")
        save_pointcloud_ply(v.numpy(), tmp_path / "pred" / "chair" / f"{name}.ply")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "main_render.py"), "dataset=synthetic", "dataset.max_points=1024", "dataset.num_shapes=2",
                          "dataloader.batch_size=2", f"run.render_sample_dir={tmp_path}", "run.render_num_frames=2"], capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "renders" / "mesh" / "chair")) == [f"{n}.png" for n in names]
    assert sorted(os.listdir(tmp_path / "renders" / "mesh_orbit" / "chair")) == [f"{n}-{k}.png" for n in names for k in range(2)]
    assert sorted(os.listdir(tmp_path / "renders" / "pred" / "chair")) == [f"{n}.png" for n in names]
    bg = int(0.78431373 * 255.0)
    for png in [tmp_path / "renders" / "mesh" / "chair" / f"{names[0]}.png", tmp_path / "renders" / "mesh_orbit" / "chair" / f"{names[1]}-1.png"]:
        px = np.asarray(Image.open(png))
        lit = (px != bg).any(-1)
        assert px.shape == (224, 224, 3) and 100 < int(lit.sum()) < 224 * 224 and int(px[lit].max()) > 100, png
    # the entry's own camera: the restatement's silhouette of mesh 0
    ref = M.render(v, f, batch.camera[0].packed()[0], 224, 224)
    px = np.asarray(Image.open(tmp_path / "renders" / "mesh" / "chair" / f"{names[0]}.png"))
    lit, inside = (px != bg).any(-1), (ref["pix_to_face"] >= 0).numpy()
    # (a Lambert term near 0.977 gives the grey level of the background, 200: such pixels are inside and do not count as lit)
    assert not (lit & ~inside).any() and int(lit.sum()) > 0.9 * int(inside.sum()) and bool((px[inside & ~lit] == bg).all())
