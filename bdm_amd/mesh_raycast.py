"""Rays against triangle meshes on the HIP path: a linear BVH per mesh (csrc/mesh_bvh.hip), the closest hit, the occlusion flag and
the crossing count of arbitrary rays (csrc/mesh_raycast.hip), and what is composed of them: pixel rays of a camera, visibility of
points from a viewpoint, ambient occlusion baked per vertex.  The rule is stated in include/bdm_hip.h section 24 and DESIGN.md
section 28; Open3D's RaycastingScene (cast_rays, test_occlusions, count_intersections) by name and meaning.

    python -m bdm_amd.mesh_raycast --mesh_dir D/pred_mesh_clean --out_dir D/pred_mesh_ao [--samples 32] [--max-distance x]

writes the tree of mesh .ply files again with uchar vertex colours albedo * ao (the file's own colours are the albedo, white without)
and prints one JSON line; `main_render.py run.render_colored_mesh_subdir=pred_mesh_ao` draws the result through the colored_mesh route.

A ray through a shared edge or vertex is accepted by every face that touches it, so count_intersections over-counts there:
voxelize_meshes stays the tool for exact parity.  Nothing here takes gradients."""
import argparse
import collections
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ragged import first, mesh_lists, pack_meshes

MAX_B = 65535   # limit of bdm_hip.h section 24
MODES = {"closest": 0, "any": 1, "count": 2}
COUNT_KEYS = ("rays_valid", "rays_invalid", "rays_hit", "faces_used", "faces_dropped")

RayHits = collections.namedtuple("RayHits", "t face_idx bary back counts")


class MeshBVH:
    """A packed batch of meshes and its hierarchy on the device: build once, query many times.  counts: {"faces_used",
    "faces_dropped"} -> int64 (B,) host tensors."""

    def __init__(self, verts, faces, vert_first, face_first, buffer, counts):
        self.verts, self.faces, self.vert_first, self.face_first, self.buffer, self.counts = verts, faces, vert_first, face_first, buffer, counts

    def __len__(self):
        return int(self.vert_first.shape[0]) - 1

    @property
    def device(self):
        return self.verts.device


class _PackedOnly(MeshBVH):
    """A packed batch without a hierarchy: what the exhaustive form needs."""

    def __init__(self, verts, faces, vert_first, face_first):
        super().__init__(verts, faces, vert_first, face_first, None, None)


def _packed(meshes):
    """-> (verts, faces, vert_first, face_first), checked against the limits; an empty batch is refused by the callers."""
    verts_list, faces_list = mesh_lists(meshes)
    if len(verts_list) == 0:
        raise ValueError("an empty batch of meshes has no rays to answer")
    if len(verts_list) > MAX_B:
        raise ValueError(f"{len(verts_list)} meshes exceed {MAX_B}: split the batch")
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    if int(vert_first[-1]) >= 2 ** 31 - 1 or 3 * int(face_first[-1]) >= 2 ** 31 - 1:
        raise ValueError("the batch reaches 2^31 vertices or face corners: split it")
    return verts, faces, vert_first, face_first


@torch.no_grad()
def build_bvh(meshes):
    """The hierarchy of a Meshes or a (verts_list, faces_list) pair -> MeshBVH.  Two calls into the library with one stable
    torch.sort of the int64 face keys between them."""
    verts, faces, vert_first, face_first = _packed(meshes)
    B, dev = int(vert_first.shape[0]) - 1, verts.device
    sum_v, sum_f = int(vert_first[-1]), int(face_first[-1])
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_bvh_workspace_bytes(B, sum_v, sum_f), dev, "mesh_bvh")
    keys = torch.empty(max(sum_f, 1), dtype=torch.int64, device=dev)
    args = (B, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr())
    L.check(lib.bdm_mesh_bvh_keys(*args, L.ptr(keys), L.ptr(ws), L.stream()), "mesh_bvh_keys")
    if sum_f:
        keys, order = torch.sort(keys[:sum_f], stable=True)
    else:
        order = torch.zeros(1, dtype=torch.int64, device=dev)
    buffer = torch.empty(lib.bdm_mesh_bvh_bytes(B, sum_f), dtype=torch.uint8, device=dev)
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    L.check(lib.bdm_mesh_bvh_build(*args, L.ptr(keys.contiguous()), L.ptr(order.contiguous()), L.ptr(counts), L.ptr(buffer), L.ptr(ws), L.stream()),
            "mesh_bvh_build")
    rows = counts.cpu().long()
    return MeshBVH(verts, faces, vert_first, face_first, buffer, {"faces_used": rows[:, 0].clone(), "faces_dropped": rows[:, 1].clone()})


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def _ray_lists(B, origins, directions, tmin, tmax, dev):
    """-> (rays (max(sum R, 1), 8) float32 on dev, ray_first, shape): origins and directions as a list of (R_i, 3) tensors or one padded
    (B, R, 3) tensor; tmin and tmax numbers, or of the rays' form without the last axis.  shape: None for lists, (B, R) for padded."""
    def rows(x, what):
        if torch.is_tensor(x):
            if x.dim() != 3 or x.shape[0] != B or x.shape[2] != 3:
                raise ValueError(f"{what} of shape {tuple(x.shape)} are not (B = {B}, R, 3)")
            return list(x), (B, int(x.shape[1]))
        if isinstance(x, (list, tuple)):
            if len(x) != B:
                raise ValueError(f"{len(x)} tensors of {what} for {B} meshes")
            for t in x:
                if not torch.is_tensor(t):
                    raise TypeError(f"{what} must be tensors, got {type(t).__name__}")
                if t.dim() != 2 or t.shape[1] != 3:
                    raise ValueError(f"{what} of shape {tuple(t.shape)} are not (R, 3)")
            return list(x), None
        raise TypeError(f"{what} must be a list of (R, 3) tensors or a (B, R, 3) tensor, got {type(x).__name__}")
    o, shape = rows(origins, "origins")
    d, shape_d = rows(directions, "directions")
    if shape != shape_d or any(a.shape != b.shape for a, b in zip(o, d)):
        raise ValueError("origins and directions differ in form or shape")
    for t in o + d:
        if not t.is_floating_point():
            raise TypeError(f"rays must be floating point, got {t.dtype}")
    counts = [int(t.shape[0]) for t in o]
    if sum(counts) >= 2 ** 31 - 1:
        raise ValueError("the rays reach 2^31: split them")

    def bounds(x, what):
        if isinstance(x, bool) or (not isinstance(x, (int, float)) and not torch.is_tensor(x) and not isinstance(x, (list, tuple))):
            raise TypeError(f"{what} must be a number, a tensor or a list of tensors, got {type(x).__name__}")
        if isinstance(x, (int, float)):
            x = float(x)
            if math.isnan(x) or (what == "tmin" and math.isinf(x)):
                raise ValueError(f"{what}={x} must be {'finite' if what == 'tmin' else 'a number or an infinity'}")
            return None, x
        parts = list(x) if not torch.is_tensor(x) or x.dim() == 2 else None
        if parts is None or len(parts) != B or any((not torch.is_tensor(p)) or p.dim() != 1 or p.shape[0] != c for p, c in zip(parts, counts)):
            raise ValueError(f"{what} does not have the rays' form without its last axis")
        return parts, None
    lo_parts, lo = bounds(tmin, "tmin")
    hi_parts, hi = bounds(tmax, "tmax")
    if lo is not None and hi is not None and lo > hi:
        raise ValueError(f"tmin={lo} exceeds tmax={hi}")
    if hi is not None and hi == float("-inf"):
        raise ValueError("tmax=-inf lies below every finite tmin")
    given = o + d + (lo_parts or []) + (hi_parts or [])
    for t in given:
        L.ptr(t)   # host tensors are refused, after every check of form
    for t in given:
        if t.device != dev:
            raise ValueError(f"rays on {t.device} for meshes on {dev}: nothing is copied between devices")
    total = sum(counts)
    rays = torch.zeros(max(total, 1), 8, dtype=torch.float32, device=dev)
    if total:
        rays[:total, 0:3] = torch.cat([t.float() for t in o]).to(dev)
        rays[:total, 3:6] = torch.cat([t.float() for t in d]).to(dev)
        rays[:total, 6] = lo if lo_parts is None else torch.cat([p.float() for p in lo_parts]).to(dev)
        rays[:total, 7] = hi if hi_parts is None else torch.cat([p.float() for p in hi_parts]).to(dev)
    return rays, first(counts), shape


def _cast(mode, target, origins, directions, tmin, tmax, exhaustive):
    """One call -> (dict of the mode's per-ray outputs as packed device tensors, counts dict, ray_first, shape)."""
    if not isinstance(exhaustive, bool):
        raise TypeError("exhaustive must be a bool")
    bvh = target if isinstance(target, MeshBVH) else None
    if bvh is None:   # the checks of the meshes' and the rays' form come before anything touches the device
        verts_list, _ = mesh_lists(target)
        if len(verts_list) == 0:
            raise ValueError("an empty batch of meshes has no rays to answer")
        B, dev = len(verts_list), verts_list[0].device
    else:
        B, dev = len(bvh), bvh.device
    rays, ray_first, shape = _ray_lists(B, origins, directions, tmin, tmax, dev)
    if bvh is None:
        bvh = _PackedOnly(*_packed(target)) if exhaustive else build_bvh(target)
    total = int(ray_first[-1])
    n = max(total, 1)
    out = {"t": None, "face": None, "bary": None, "back": None, "occluded": None, "crossings": None}
    if mode == "closest":
        out.update(t=torch.empty(n, dtype=torch.float32, device=dev), face=torch.empty(n, dtype=torch.int32, device=dev),
                   bary=torch.empty(n, 2, dtype=torch.float32, device=dev), back=torch.empty(n, dtype=torch.uint8, device=dev))
    elif mode == "any":
        out.update(occluded=torch.empty(n, dtype=torch.uint8, device=dev))
    else:
        out.update(crossings=torch.empty(n, dtype=torch.int32, device=dev))
    counts = torch.empty(B, len(COUNT_KEYS), dtype=torch.int32, device=dev)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_raycast_workspace_bytes(B), dev, "mesh_raycast")
    head = (MODES[mode], B, L.ptr(bvh.verts), L.ptr(bvh.faces), bvh.vert_first.data_ptr(), bvh.face_first.data_ptr())
    tail = (L.ptr(rays), ray_first.data_ptr(), *(L.ptr(out[k]) for k in ("t", "face", "bary", "back", "occluded", "crossings")),
            L.ptr(counts), L.ptr(ws), L.stream())
    if exhaustive:
        L.check(lib.bdm_mesh_raycast_exhaustive(*head, *tail), "mesh_raycast_exhaustive")
    else:
        L.check(lib.bdm_mesh_raycast(*head, L.ptr(bvh.buffer), *tail), "mesh_raycast")
    rows = counts.cpu().long()
    return ({k: v[:total] for k, v in out.items() if v is not None}, {k: rows[:, i].clone() for i, k in enumerate(COUNT_KEYS)}, ray_first, shape)


def _unpack(x, ray_first, shape):
    """Packed per-ray rows -> the form the rays came in: a list per mesh, or (B, R, ...)."""
    if shape is not None:
        return x.reshape(*shape, *x.shape[1:])
    return [x[int(ray_first[m]):int(ray_first[m + 1])] for m in range(ray_first.shape[0] - 1)]


@torch.no_grad()
def cast_rays(bvh_or_meshes, origins, directions, tmin=0.0, tmax=float("inf"), exhaustive=False):
    """The closest hit of every ray -> RayHits(t float32 (+inf: a miss), face_idx int32 (inside its mesh; -1), bary float32 (.., 2):
    the weights of the face's corners 1 and 2, back bool: the ray runs along the face's normal, counts: name -> int64 (B,) host
    tensors, the COUNT_KEYS).  Rays: a list of (R_i, 3) device tensors per mesh, or (B, R, 3); the outputs take the same form.
    directions need not be unit: t is in their units.  exhaustive=True tests every face without the tree: the same bits, slower.
    The rule's face interval is widened by a factor only: a face flat along an axis whose corners lie at more than about a hundred
    times the hit's t along the ray starts to lose hits."""
    out, counts, ray_first, shape = _cast("closest", bvh_or_meshes, origins, directions, tmin, tmax, exhaustive)
    un = lambda x: _unpack(x, ray_first, shape)   # noqa: E731
    return RayHits(un(out["t"]), un(out["face"]), un(out["bary"]), un(out["back"].bool()), counts)


@torch.no_grad()
def test_occlusions(bvh_or_meshes, origins, directions, tmin=0.0, tmax=float("inf"), exhaustive=False):
    """Whether any face is hit in [tmin, tmax] -> bool per ray, in the rays' form."""
    out, _, ray_first, shape = _cast("any", bvh_or_meshes, origins, directions, tmin, tmax, exhaustive)
    return _unpack(out["occluded"].bool(), ray_first, shape)


test_occlusions.__test__ = False   # not a test, whatever the name says to a collector


@torch.no_grad()
def count_intersections(bvh_or_meshes, origins, directions, tmin=0.0, tmax=float("inf"), exhaustive=False):
    """The number of faces hit in [tmin, tmax] -> int32 per ray, in the rays' form.  A ray through a shared edge or vertex counts
    every face that touches it."""
    out, _, ray_first, shape = _cast("count", bvh_or_meshes, origins, directions, tmin, tmax, exhaustive)
    return _unpack(out["crossings"], ray_first, shape)


def camera_rays(cameras, image_size):
    """The rays through the pixel centres of PerspectiveCameras / OrthographicCameras in world space -> (origins, directions), each
    (B, H W, 3) float32 on the cameras' device, row-major over (y, x).  render.py's conventions: pixel (y, x) has its centre at ndc
    u = 1 - (2 x + 1) / W, v = 1 - (2 y + 1) / H; X_view = X_world R + T; ndc = focal * X_view.xy (/ X_view.z) + principal point.  The
    view-space direction has z = 1, so t is the view depth."""
    if not (hasattr(cameras, "R") and hasattr(cameras, "focal_length") and hasattr(cameras, "principal_point")):
        raise TypeError(f"expected PerspectiveCameras or OrthographicCameras, got {type(cameras).__name__}")
    if isinstance(image_size, bool) or not (isinstance(image_size, int) or (isinstance(image_size, (tuple, list)) and len(image_size) == 2)):
        raise TypeError("image_size must be an int or (H, W)")
    H, W = (image_size, image_size) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
    if H < 1 or W < 1:
        raise ValueError(f"image_size={image_size!r} is not positive")
    dev = cameras.device
    u = 1.0 - (2.0 * torch.arange(W, dtype=torch.float32, device=dev) + 1.0) / W
    v = 1.0 - (2.0 * torch.arange(H, dtype=torch.float32, device=dev) + 1.0) / H
    uu, vv = u[None, :].expand(H, W).reshape(1, -1), v[:, None].expand(H, W).reshape(1, -1)
    f, pp = cameras.focal_length.float(), cameras.principal_point.float()
    x, y = (uu - pp[:, 0:1]) / f[:, 0:1], (vv - pp[:, 1:2]) / f[:, 1:2]   # (B, H W)
    zero, one = torch.zeros_like(x), torch.ones_like(x)
    if getattr(cameras, "orthographic", False):
        o_view, d_view = torch.stack([x, y, zero], dim=2), torch.stack([zero, zero, one], dim=2)
    else:
        o_view, d_view = torch.stack([zero, zero, zero], dim=2), torch.stack([x, y, one], dim=2)
    Rt = cameras.R.float().transpose(1, 2)
    origins = torch.bmm(o_view - cameras.T.float()[:, None, :], Rt)
    return origins.contiguous(), torch.bmm(d_view, Rt).contiguous()


def _diagonals(verts_list):
    """The length of the bounding-box diagonal of the finite vertices of every mesh -> float32 (B,) on the meshes' device (0 without
    one)."""
    rows = []
    for v in verts_list:
        v = v.float().reshape(-1, 3)
        fin = torch.isfinite(v).all(dim=1, keepdim=True)
        zero = v.new_zeros(1, 3)
        lo = torch.cat([torch.where(fin, v, torch.full_like(v, float("inf"))), v.new_full((1, 3), float("inf"))]).amin(dim=0)
        hi = torch.cat([torch.where(fin, v, torch.full_like(v, float("-inf"))), v.new_full((1, 3), float("-inf"))]).amax(dim=0)
        ext = torch.where(torch.isfinite(hi - lo), hi - lo, zero[0])
        rows.append((ext * ext).sum().sqrt())
    return torch.stack(rows)


@torch.no_grad()
def points_visible(meshes, points_list, eyes=None, directions=None, offset=1e-4):
    """Per point whether the segment from it to the viewer is free of the mesh -> list of bool (P_i,).  Exactly one of eyes (B, 3), the
    viewpoints of a perspective view, or directions (B, 3), pointing from the scene TOWARDS the viewer of a parallel view.  A point is
    first moved `offset` times the bounding-box diagonal of its mesh towards the viewer, so that a point on the surface does not hide
    itself.  Elementwise torch around one test_occlusions call."""
    if (eyes is None) == (directions is None):
        raise ValueError("give exactly one of eyes (perspective) and directions (parallel)")
    if isinstance(offset, bool) or not isinstance(offset, (int, float)) or not (0 <= offset < float("inf")):
        raise ValueError(f"offset={offset!r} is not a finite number >= 0")
    bvh = meshes if isinstance(meshes, MeshBVH) else None
    verts_list = mesh_lists(meshes)[0] if bvh is None else [bvh.verts[int(bvh.vert_first[m]):int(bvh.vert_first[m + 1])] for m in range(len(bvh))]
    B = len(verts_list)
    if not isinstance(points_list, (list, tuple)) or len(points_list) != B:
        raise ValueError(f"points_list must hold one (P, 3) tensor per mesh ({B})")
    view = eyes if eyes is not None else directions
    if not torch.is_tensor(view):
        raise TypeError("eyes / directions must be a (B, 3) tensor")
    if view.shape != (B, 3):
        raise ValueError(f"eyes / directions of shape {tuple(view.shape)} are not ({B}, 3)")
    for p in points_list:
        if not torch.is_tensor(p):
            raise TypeError("points must be tensors")
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError(f"points of shape {tuple(p.shape)} are not (P, 3)")
    lift = _diagonals(verts_list) * offset
    origins, dirs = [], []
    for m, p in enumerate(points_list):
        p, e = p.float(), view[m].float().to(p.device)
        towards = (e[None, :] - p) if eyes is not None else e[None, :].expand_as(p)
        unit = towards / towards.norm(dim=1, keepdim=True).clamp_min(1e-30)
        o = p + lift[m].to(p.device) * unit
        origins.append(o)
        dirs.append((e[None, :] - o) if eyes is not None else unit.contiguous())
    hidden = test_occlusions(meshes, origins, dirs, 0.0, 1.0 if eyes is not None else float("inf"))
    return [~h for h in hidden]


def fibonacci_sphere(n):
    """n unit vectors spread over the sphere, computed in float64 on the host and rounded once to float32 -> (n, 3) host tensor."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return torch.from_numpy(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32))


@torch.no_grad()
def vertex_ambient_occlusion(meshes, num_samples=32, max_distance=None, directions=None, offset=1e-4, return_info=False):
    """Ambient occlusion per vertex -> list of (V_i,) float32 in [0, 1], 1 = open.  Every vertex casts one ray per direction of the
    (S, 3) table of unit vectors (default: fibonacci_sphere(num_samples), passed in as data: no sine or cosine runs on the device)
    from the vertex lifted `offset` bounding-box diagonals along its normal (Meshes.verts_normals_packed); a direction on the far
    side of the normal is negated.  ao = 1 - sum(w occluded) / sum(w), w = |d . n|, accumulated direction after direction with
    elementwise operations; a vertex without a normal gets 1.  max_distance: rays end there (None: never).  return_info: also a dict
    with "rays", "occluded" (numbers) and "faces_dropped" (int64 (B,))."""
    from .cameras import Meshes
    if directions is None:
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 1 <= num_samples <= 4096:
            raise ValueError(f"num_samples={num_samples!r} is not an integer in 1..4096")
        directions = fibonacci_sphere(num_samples)
    if not torch.is_tensor(directions):
        raise TypeError("directions must be an (S, 3) tensor")
    if directions.dim() != 2 or directions.shape[1] != 3 or directions.shape[0] < 1 or not bool(torch.isfinite(directions).all()):
        raise ValueError(f"directions of shape {tuple(directions.shape)} are not (S, 3) finite vectors")
    if max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or not max_distance > 0):
        raise ValueError(f"max_distance={max_distance!r} is not a positive number")
    if isinstance(offset, bool) or not isinstance(offset, (int, float)) or not (0 <= offset < float("inf")):
        raise ValueError(f"offset={offset!r} is not a finite number >= 0")
    verts_list, faces_list = mesh_lists(meshes)
    if len(verts_list) == 0:
        return ([], {"rays": 0, "occluded": 0, "faces_dropped": torch.zeros(0, dtype=torch.int64)}) if return_info else []
    bvh = build_bvh((list(verts_list), list(faces_list)))
    dev, S = bvh.device, int(directions.shape[0])
    table = directions.float().to(dev)
    safe = [torch.where((f >= 0) & (f < v.shape[0]), f, torch.zeros_like(f)) if v.shape[0] else f[:0] for v, f in zip(verts_list, faces_list)]
    normals = Meshes([torch.nan_to_num(v.float(), nan=0.0, posinf=0.0, neginf=0.0) for v in verts_list], safe).verts_normals_packed()
    lift = _diagonals(verts_list) * offset
    origins, dirs, weights, start = [], [], [], 0
    for m, v in enumerate(verts_list):
        n = normals[start:start + v.shape[0]]
        start += v.shape[0]
        s = (n[:, None, 0] * table[None, :, 0] + n[:, None, 1] * table[None, :, 1]) + n[:, None, 2] * table[None, :, 2]   # (V, S)
        d = torch.where((s < 0)[:, :, None], -table[None], table[None].expand(v.shape[0], S, 3))
        o = v.float() + lift[m] * n
        origins.append(o[:, None, :].expand(-1, S, -1).reshape(-1, 3))
        dirs.append(d.reshape(-1, 3))
        weights.append(s.abs())
    hidden = test_occlusions(bvh, origins, dirs, 0.0, float("inf") if max_distance is None else float(max_distance))
    result, occluded = [], 0
    for w, h in zip(weights, hidden):
        h = h.reshape(w.shape).float()
        num, den = torch.zeros_like(w[:, 0]), torch.zeros_like(w[:, 0])
        for k in range(S):   # in the table's order: no reduction whose order is left open
            num, den = num + w[:, k] * h[:, k], den + w[:, k]
        result.append(torch.where(den > 0, 1.0 - num / den.clamp_min(1e-30), torch.ones_like(den)))
        occluded += int(h.sum())
    if not return_info:
        return result
    return result, {"rays": sum(int(w.numel()) for w in weights), "occluded": occluded, "faces_dropped": bvh.counts["faces_dropped"]}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def bake_ao_dirs(mesh_dir, out_dir, samples=32, max_distance=None, batch_size=16, device=None):
    """Walk mesh_dir for mesh .ply files in sorted path order and write each again under out_dir with uchar vertex colours
    albedo * ao -> {"meshes", "rays", "occluded_fraction", "faces_dropped"}."""
    from .io import load_mesh_ply, save_mesh_ply
    mesh_dir, out_dir = Path(mesh_dir), Path(out_dir)
    if device is None:
        if not torch.cuda.is_available():
            raise L.BdmHipError("bdm_amd.mesh_raycast needs a HIP device (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    items = [(path.relative_to(mesh_dir), path) for path in sorted(mesh_dir.rglob("*.ply"))]
    rays = occluded = dropped = 0
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        loaded = [load_mesh_ply(path, with_colors=True) for _, path in chunk]
        verts, faces = [torch.from_numpy(v).to(device) for v, _, _ in loaded], [torch.from_numpy(f).to(device) for _, f, _ in loaded]
        ao, info = vertex_ambient_occlusion((verts, faces), samples, max_distance, return_info=True)
        rays, occluded, dropped = rays + info["rays"], occluded + info["occluded"], dropped + int(info["faces_dropped"].sum())
        for (rel, _), (v, f, albedo), a in zip(chunk, loaded, ao):
            shade = a.cpu().numpy()[:, None]
            colors = shade * (albedo if albedo is not None else np.ones((v.shape[0], 3), dtype=np.float32))
            save_mesh_ply(v, f, out_dir / rel, colors=colors)
    return {"meshes": len(items), "rays": rays, "occluded_fraction": occluded / rays if rays else 0.0, "faces_dropped": dropped}


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_raycast", description="bake ambient occlusion into the vertex colours of a tree of meshes")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--out_dir", required=True, help="the same tree, written with vertex colours albedo * ao")
    ap.add_argument("--samples", type=int, default=32, help="rays per vertex, 1..4096")
    ap.add_argument("--max-distance", type=float, default=None, help="occluders beyond this distance are ignored")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if not 1 <= args.samples <= 4096:
        ap.error("--samples must be in 1..4096")
    if args.max_distance is not None and not args.max_distance > 0:
        ap.error("--max-distance must be positive")
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    result = bake_ao_dirs(args.mesh_dir, args.out_dir, args.samples, args.max_distance, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
