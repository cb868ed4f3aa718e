"""Rendering of point clouds on the HIP path: the reference's `render_pointcloud_batch_pytorch3d` and
`visualize_pointcloud_batch_pytorch3d` (experiments/diffusion_utils.py:185-295, called from experiments/main.py:418-430) with
their names, keyword arguments and defaults, over bdm_render_points (csrc/render.hip).

The reference renders with pytorch3d's PointsRasterizer + NormWeightedCompositor / AlphaCompositor and tiles the images with
torchvision's make_grid.  Neither package is installed here, so both are restated from their published behaviour ("parity
unpinned", as oracle/ref_sampler.py says of the conditioning rasteriser).  Two documented departures from pytorch3d
(DESIGN.md section 12): `Fragments.idx` is the index of the point WITHIN its cloud (pytorch3d: within the packed batch), and for
H != W each image axis spans NDC [-1, 1] (pytorch3d scales the longer axis by the aspect ratio)."""
import math
import os
from collections import namedtuple

import torch

from . import _lib as L
from . import ops
from .cameras import OrthographicCameras, Pointclouds, join_cameras, look_at_view_transform

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
