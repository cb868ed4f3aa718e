"""Rendering of point clouds on the HIP path: the reference's `render_pointcloud_batch_pytorch3d` and
`visualize_pointcloud_batch_pytorch3d` (experiments/diffusion_utils.py:185-295, called from experiments/main.py:418-430) with
their names, keyword arguments and defaults, over bdm_render_points (csrc/render.hip).

The reference renders with pytorch3d's PointsRasterizer + NormWeightedCompositor / AlphaCompositor and tiles the images with
torchvision's make_grid.  Neither package is installed here, so both are restated from their published behaviour ("parity
unpinned", as oracle/ref_sampler.py says of the conditioning rasteriser).  Two documented departures from pytorch3d
(DESIGN.md section 12): `Fragments.idx` is the index of the point WITHIN its cloud (pytorch3d: within the packed batch), and for
H != W each image axis spans NDC [-1, 1] (pytorch3d scales the longer axis by the aspect ratio).

The mesh half of that package (MeshRasterizer plus a shader) follows further down: rasterize_meshes, render_mesh_batch and
visualize_mesh_batch over bdm_render_meshes (csrc/mesh_render.hip)."""
import math
import os
from collections import namedtuple

import torch

from . import _lib as L
from . import ops
from .cameras import OrthographicCameras, Pointclouds, join_cameras, look_at_view_transform
from .ragged import pack_meshes

Fragments = namedtuple("Fragments", ["idx", "zbuf", "dists"])
COMPOSITORS = {"norm_weighted": 0, "alpha": 1}
BACKGROUND = (0.78431373, 0.78431373, 0.78431373)


def _image_hw(image_size):
    return (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))


def _render(cameras, points, image_size, radius, points_per_pixel, features=None, background=None, compositor=None, fragments=True):
    """One bdm_render_points call: (Fragments or None, image (B, H, W, C) or None)."""
    cameras = join_cameras(cameras)
    points = L.f32(points)
    B, N, _ = points.shape
    H, W = _image_hw(image_size)
    K = int(points_per_pixel)
    dev = points.device
    if len(cameras) != B:
        raise ValueError(f"{len(cameras)} cameras for {B} clouds")
    cams = cameras.packed().to(dev)
    idx = zbuf = dists = image = bg = None
    C = 3
    if fragments:
        idx = torch.empty(B, H, W, K, dtype=torch.int32, device=dev)
        zbuf = torch.empty(B, H, W, K, dtype=torch.float32, device=dev)
        dists = torch.empty(B, H, W, K, dtype=torch.float32, device=dev)
    if compositor is not None:
        if compositor not in COMPOSITORS:
            raise ValueError(compositor)
        bg = torch.as_tensor(background, dtype=torch.float32).reshape(-1).to(dev)
        C = bg.shape[0]
        if features is not None:
            features = L.f32(features)
            if tuple(features.shape) != (B, N, C):
                raise ValueError(f"features {tuple(features.shape)} do not match {B} clouds of {N} points and a {C}-channel background")
        image = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_render_workspace_bytes(B, N, H, W, L.c_float(radius)), dev, "render")
    L.check(lib.bdm_render_points(B, N, H, W, K, C, L.c_float(radius), int(cameras.orthographic), COMPOSITORS.get(compositor, 0),
                                  L.ptr(points), L.ptr(cams), L.ptr(features), L.ptr(bg), L.ptr(idx), L.ptr(zbuf), L.ptr(dists),
                                  L.ptr(image), L.ptr(ws), L.stream()), "render_points")
    return (Fragments(idx.long(), zbuf, dists) if fragments else None), image


def rasterize_points(cameras, points, image_size=224, radius=0.01, points_per_pixel=10):
    """pytorch3d's PointsRasterizer (naive rule) on a padded batch: points (B, N, 3) world coordinates -> Fragments of
    idx (B, H, W, K) int64 (index within the cloud, -1 = empty), zbuf (view depth, -1) and dists (squared NDC distance, -1):
    per pixel the K points nearest in depth among those with dx^2 + dy^2 < radius^2 and z >= 0, ascending (z, index)."""
    return _render(cameras, points, image_size, radius, points_per_pixel)[0]


@torch.no_grad()
def render_pointcloud_batch_pytorch3d(cameras, pointclouds, image_size=224, radius=0.01, points_per_pixel=10,
                                      background_color=BACKGROUND, compositor="norm_weighted"):
    """diffusion_utils.py:185-226: images (B, H, W, C) of the clouds seen from `cameras` (Perspective- or OrthographicCameras, or
    a list of single cameras).  A cloud without features renders with zero colours (ensure_point_cloud_has_colors)."""
    if compositor not in COMPOSITORS:
        raise ValueError(compositor)
    return _render(cameras, pointclouds.points_padded(), image_size, radius, points_per_pixel, pointclouds.features_padded(),
                   background_color, compositor, fragments=False)[1]


def shade_by_normals(points, normals, cameras, ambient=0.3, albedo=(0.8, 0.8, 0.8), two_sided=True):
    """Features (B, N, 3) that light an uncoloured cloud from its cameras: albedo * (ambient + (1 - ambient) |n . v|), v the unit
    vector from the point to the camera centre (perspective) or the view axis (orthographic).  Two-sided, so the picture does
    not depend on the sign rule of the normals; two_sided=False is one-sided Lambert, max(n . v, 0) in place of |n . v|, for
    normals whose signs can be trusted (normals.orient_normals_by_visibility): a surface seen from behind gets the ambient term
    alone.  Elementwise torch on whatever device the points live on: not a hot path."""
    cameras = join_cameras(cameras)
    if len(cameras) != points.shape[0]:
        raise ValueError(f"{len(cameras)} cameras for {points.shape[0]} clouds")
    R, T = cameras.R.to(points), cameras.T.to(points)
    if cameras.orthographic:
        v = R[:, :, 2][:, None, :].expand_as(points)                 # X_view = X_world R + T: the view z axis in world coordinates
    else:
        centre = -torch.bmm(T[:, None, :], R.transpose(1, 2))        # X_view = 0  <=>  X_world = -T R^T
        v = centre - points
        v = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    lambert = (normals.to(points) * v).sum(-1, keepdim=True)
    lambert = lambert.abs() if two_sided else lambert.clamp_min(0.0)
    return torch.as_tensor(albedo, dtype=points.dtype, device=points.device) * (ambient + (1.0 - ambient) * lambert)


# ---- triangle meshes ---------------------------------------------------------------------------------------------------------------
# pytorch3d's MeshRasterizer (faces_per_pixel = 1, blur_radius = 0) and a Gouraud / flat shader over bdm_render_meshes
# (csrc/mesh_render.hip; the rule is stated in include/bdm_hip.h section 13 and DESIGN.md section 17).  Departures from pytorch3d,
# beside the two above: `pix_to_face` counts WITHIN the mesh (pytorch3d: within the packed batch), K is fixed at 1, there is no
# `dists` (no blur radius, so pytorch3d's would only hold the signed distance to the winning face's edges), and a pixel centre on
# a shared edge belongs to exactly one face by a half-plane rule (pytorch3d decides by floating-point signs).
MeshFragments = namedtuple("MeshFragments", ["pix_to_face", "zbuf", "bary_coords"])
MESH_SHADINGS = ("smooth", "flat", "none")
MESH_MAX_SIDE, MESH_MAX_C = 4096, 4   # limits of bdm_render_meshes


def _check_mesh_args(cameras, meshes, image_size):
    """The argument checks that need no device -> (joined cameras, H, W)."""
    if not hasattr(meshes, "verts_list") or not hasattr(meshes, "faces_list"):
        raise ValueError(f"expected a Meshes, got {type(meshes).__name__}")
    cameras = join_cameras(cameras)
    if len(cameras) != len(meshes):
        raise ValueError(f"{len(cameras)} cameras for {len(meshes)} meshes")
    H, W = _image_hw(image_size)
    if not (1 <= H <= MESH_MAX_SIDE and 1 <= W <= MESH_MAX_SIDE):
        raise ValueError(f"image size {H} x {W} is outside 1..{MESH_MAX_SIDE}")
    if len(meshes) * H * W >= 2 ** 31:
        raise ValueError(f"{len(meshes)} images of {H} x {W} pixels reach 2^31: split the batch")
    return cameras, H, W


def _render_meshes(cameras, meshes, image_size, cull_backfaces=False, vert_features=None, face_features=None, background=None,
                   fragments=True):
    """One bdm_render_meshes call: (MeshFragments or None, image (B, H, W, C) or None; an image is made iff `background` is given)."""
    cameras, H, W = _check_mesh_args(cameras, meshes, image_size)
    if vert_features is not None and face_features is not None:
        raise ValueError("vertex features and face features are exclusive")
    B = len(meshes)
    verts_list, faces_list = meshes.verts_list(), meshes.faces_list()
    sum_v, sum_f = sum(int(v.shape[0]) for v in verts_list), sum(int(f.shape[0]) for f in faces_list)
    bg, C = None, 3
    if background is not None:
        bg = torch.as_tensor(background, dtype=torch.float32).reshape(-1)
        C = int(bg.shape[0])
        if not 1 <= C <= MESH_MAX_C:
            raise ValueError(f"{C} background channels are outside 1..{MESH_MAX_C}")
    for name, feats, rows in (("vertex", vert_features, sum_v), ("face", face_features, sum_f)):
        if feats is not None and (background is None or tuple(feats.shape) != (rows, C)):
            raise ValueError(f"{name} features {tuple(feats.shape)} do not match ({rows}, {C}) and a {C}-channel background")
    if B == 0:
        dev = cameras.device
        frag = MeshFragments(torch.zeros(0, H, W, 1, dtype=torch.int64, device=dev), torch.zeros(0, H, W, 1, device=dev),
                             torch.zeros(0, H, W, 1, 3, device=dev)) if fragments else None
        return frag, (None if bg is None else torch.zeros(0, H, W, C, device=dev))
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    dev = verts.device
    cams = cameras.packed().to(dev)
    pix = zbuf = bary = image = None
    if fragments:
        pix = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        zbuf = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        bary = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    if bg is not None:
        bg = bg.to(dev)
        image = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        vert_features = None if vert_features is None else L.f32(vert_features)
        face_features = None if face_features is None else L.f32(face_features)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_render_meshes_workspace_bytes(B, sum_v, sum_f, H, W), dev, "render_meshes")
    L.check(lib.bdm_render_meshes(B, H, W, C, int(cameras.orthographic), int(bool(cull_backfaces)), L.ptr(verts), L.ptr(faces),
                                  vert_first.data_ptr(), face_first.data_ptr(), L.ptr(cams), L.ptr(vert_features), L.ptr(face_features),
                                  L.ptr(bg), L.ptr(pix), L.ptr(zbuf), L.ptr(bary), L.ptr(image), L.ptr(ws), L.stream()), "render_meshes")
    frag = MeshFragments(pix.long()[..., None], zbuf[..., None], bary[:, :, :, None, :]) if fragments else None
    return frag, image


def rasterize_meshes(cameras, meshes, image_size=224, cull_backfaces=False):
    """pytorch3d's MeshRasterizer at faces_per_pixel = 1, blur_radius = 0 -> MeshFragments of pix_to_face (B, H, W, 1) int64 (the
    face index WITHIN the mesh, -1 = empty), zbuf (B, H, W, 1) (view depth, -1) and bary_coords (B, H, W, 1, 3) (perspective-correct
    under a perspective camera, in the face's own vertex order, -1).  cull_backfaces drops the faces whose geometric normal
    (v1 - v0) x (v2 - v0) points away from the camera.  There is no near-plane clipping: a face with a vertex at or behind the
    camera plane is dropped whole."""
    return _render_meshes(cameras, meshes, image_size, cull_backfaces)[0]


@torch.no_grad()
def render_mesh_batch(cameras, meshes, image_size=224, shading="smooth", vert_colors=None, background_color=BACKGROUND, ambient=0.3,
                      cull_backfaces=False, vert_albedo=None):
    """Images (B, H, W, 3) of the meshes seen from `cameras` (Perspective- or OrthographicCameras, or a list of single cameras).
    shading="smooth": shade_by_normals(..., two_sided=False) on the vertices and their normals (Meshes.verts_normals_packed),
    Gouraud colours the kernel interpolates; "flat": the same on face centroids and face normals, one colour per face; "none":
    `vert_colors` (sum V, 3) interpolated, or zeros.  vert_albedo (sum V, 3): under "smooth" and "flat" it replaces the constant
    albedo of shade_by_normals, per vertex; a face's albedo under "flat" is the mean of its three vertices, ((a0 + a1) + a2) / 3.
    Bad arguments raise ValueError before any launch."""
    if shading not in MESH_SHADINGS:
        raise ValueError(f"shading={shading!r}: expected one of {MESH_SHADINGS}")
    if vert_colors is not None and shading != "none":
        raise ValueError("vert_colors need shading='none'")
    if vert_albedo is not None:
        if shading == "none":
            raise ValueError("vert_albedo needs a lit shading ('smooth' or 'flat'); unlit colours are vert_colors")
        sum_v = sum(int(v.shape[0]) for v in meshes.verts_list()) if hasattr(meshes, "verts_list") else -1
        if not torch.is_tensor(vert_albedo) or not vert_albedo.is_floating_point() or tuple(vert_albedo.shape) != (sum_v, 3):
            raise ValueError(f"vert_albedo must be a floating-point ({sum_v}, 3) tensor")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError(f"ambient={ambient} is outside 0..1")
    cameras, _, _ = _check_mesh_args(cameras, meshes, image_size)
    vert_features = face_features = None
    if shading == "none":
        vert_features = vert_colors
    elif len(meshes) and sum(int(f.shape[0]) for f in meshes.faces_list()):
        verts = meshes.verts_packed()
        if shading == "smooth":
            where, normals, sizes = verts, meshes.verts_normals_packed(), [int(v.shape[0]) for v in meshes.verts_list()]
        else:
            where, normals = verts[meshes.faces_packed().to(verts.device)].mean(dim=1), meshes.faces_normals_packed()
            sizes = [int(f.shape[0]) for f in meshes.faces_list()]
        albedos = [(0.8, 0.8, 0.8)] * len(sizes)   # shade_by_normals' default
        if vert_albedo is not None:
            albedo = vert_albedo.to(verts)
            if shading == "flat":
                a = albedo[meshes.faces_packed().to(verts.device)]
                albedo = ((a[:, 0] + a[:, 1]) + a[:, 2]) / 3.0
            albedos = torch.split(albedo, sizes)
        if cameras.orthographic:
            # one-sided, shade_by_normals lights an orthographic view along R[:, :, 2], the view axis INTO the screen (pinned by
            # tests/test_orient_host.py): a surface that faces the viewer has n . axis < 0, so the normals go in negated
            normals = -normals
        # shade_by_normals works on (B, n, 3) with one camera per row: one row per mesh, each with its own camera
        colours = [shade_by_normals(p[None], n[None], _camera_row(cameras, i), ambient=ambient, albedo=al, two_sided=False)[0]
                   for i, (p, n, al) in enumerate(zip(torch.split(where, sizes), torch.split(normals, sizes), albedos))]
        colours = torch.cat(colours).float().contiguous()
        vert_features, face_features = (colours, None) if shading == "smooth" else (None, colours)
    return _render_meshes(cameras, meshes, image_size, cull_backfaces, vert_features, face_features, background_color, fragments=False)[1]


def _camera_row(cameras, i):
    return type(cameras)(cameras.focal_length[i:i + 1], cameras.principal_point[i:i + 1], cameras.R[i:i + 1], cameras.T[i:i + 1],
                         device=cameras.device)


@torch.no_grad()
def visualize_mesh_batch(meshes, output_file_image=None, num_frames=1, elev=30, scale_factor=1.0, shading="smooth", image_size=224,
                         cull_backfaces=False, vert_albedo=None):
    """The orbit of visualize_pointcloud_batch_pytorch3d for meshes: `num_frames` orthographic cameras (focal 0.25 * scale_factor)
    at distance 10 and elevation `elev`, every frame lit from its own camera, tiled with make_grid(nrow=int(sqrt(B)), pad_value=1);
    one frame goes to `output_file_image`, with num_frames > 1 frame f goes to <stem>-<f>.png beside it.  Returns the grids
    (F, C, H', W') on the host.  vert_albedo (sum V, 3) is forwarded to render_mesh_batch for every frame."""
    from .cameras import Meshes
    from .io import save_image_png
    F = int(num_frames)
    if F < 1 or 360 % F:
        raise ValueError("num_frames must divide 360")
    B = len(meshes)
    if B == 0:
        raise ValueError("no mesh to draw")
    device = meshes.device
    R, T = look_at_view_transform(dist=10.0, elev=elev, azim=list(range(0, 360, 360 // F)), degrees=True, device=device)
    cameras = OrthographicCameras(focal_length=0.25 * scale_factor, device=device, R=R.repeat_interleave(B, dim=0), T=T.repeat_interleave(B, dim=0))
    images = render_mesh_batch(cameras, Meshes(meshes.verts_list() * F, meshes.faces_list() * F), image_size, shading, cull_backfaces=cull_backfaces,
                               vert_albedo=None if vert_albedo is None else vert_albedo.repeat(F, 1))
    frames = images.reshape(F, B, *images.shape[1:]).permute(0, 1, 4, 2, 3)
    grids = torch.stack([make_grid(f, nrow=int(math.sqrt(B)), pad_value=1) for f in frames], dim=0).detach().cpu()
    if output_file_image is not None:
        if F == 1:
            save_image_png(grids[0].numpy(), output_file_image)
        else:
            stem, ext = os.path.splitext(str(output_file_image))
            for f in range(F):
                save_image_png(grids[f].numpy(), f"{stem}-{f}{ext or '.png'}")
    return grids


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid (restated; torchvision is absent) for a (B, C, H, W) batch with its defaults normalize=False,
    scale_each=False: single-channel images are repeated to three channels, ONE image is returned as it is (no border), otherwise
    min(nrow, B) images per row, each cell (H + padding, W + padding) and a border of `padding`, filled with pad_value."""
    if tensor.dim() != 4:
        raise ValueError("make_grid restates the (B, C, H, W) case only")
    if tensor.shape[1] == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.shape[0] == 1:
        return tensor[0]
    nmaps = tensor.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.shape[2] + padding), int(tensor.shape[3] + padding)
    grid = tensor.new_full((tensor.shape[1], height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width] = tensor[k]
            k += 1
    return grid


@torch.no_grad()
def visualize_pointcloud_batch_pytorch3d(pointclouds, output_file_video=None, output_file_image=None, cameras=None,
                                         scale_factor=1.0, num_frames=1, elev=30):
    """diffusion_utils.py:229-295: renders the batch from `cameras`, or (cameras=None) from `num_frames` orthographic cameras
    (focal 0.25 * scale_factor) orbiting at distance 10 and elevation `elev`, tiles each frame with
    make_grid(nrow=int(sqrt(B)), pad_value=1) and saves it: one frame to `output_file_image`; with num_frames > 1 frame f goes to
    <stem>-<f>.png beside it.  The reference's video writer is commented out (imageio is absent here too): output_file_video must
    stay None.  Returns the grids (F, C, H', W') on the host."""
    from .io import save_image_png
    if output_file_video is not None:
        raise NotImplementedError("video output: the reference's writer is commented out; frames are written as <stem>-<f>.png")
    assert 360 % num_frames == 0, "please select a better number of frames"
    points, features, F = pointclouds.points_padded(), pointclouds.features_padded(), int(num_frames)
    B, device = points.shape[0], points.device
    if cameras is None:
        R, T = look_at_view_transform(dist=10.0, elev=elev, azim=list(range(0, 360, 360 // F)), degrees=True, device=device)
        R, T = R.repeat_interleave(B, dim=0), T.repeat_interleave(B, dim=0)
        cameras = OrthographicCameras(focal_length=0.25 * scale_factor, device=device, R=R, T=T)
        points = points.tile(F, 1, 1)
        features = torch.zeros_like(points) if features is None else features.tile(F, 1, 1)
    elif F != 1:
        raise ValueError("several frames need the orbiting cameras (cameras=None)")
    images = render_pointcloud_batch_pytorch3d(cameras, Pointclouds(points, features))
    frames = images.reshape(F, B, *images.shape[1:]).permute(0, 1, 4, 2, 3)
    grids = torch.stack([make_grid(f, nrow=int(math.sqrt(B)), pad_value=1) for f in frames], dim=0).detach().cpu()
    if output_file_image is not None:
        if F == 1:
            save_image_png(grids[0].numpy(), output_file_image)
        else:
            stem, ext = os.path.splitext(str(output_file_image))
            for f in range(F):
                save_image_png(grids[f].numpy(), f"{stem}-{f}{ext or '.png'}")
    return grids
