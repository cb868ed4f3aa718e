"""Solid voxelisation of triangle meshes and the volumetric IoU of two meshes on the HIP path, over bdm_mesh_voxelize
(csrc/mesh_voxel.hip; the rule is stated in include/bdm_hip.h section 21 and DESIGN.md section 25).

    python -m bdm_amd.mesh_voxel --mesh_dir D/pred_mesh_clean --gt_dir D/gt_mesh [--resolution 32] [--mode vote|x|y|z]
                                 [--out_dir D/pred_voxels] [--batch-size 16]

walks the mesh .ply files of mesh_dir in sorted order and scores each against the ground truth of the same relative path under
gt_dir: a `.binvox` file of the same stem (its own dim, translate and scale are the frame), or a mesh .ply (the frame is the bounding
cube of the pair).  It prints one JSON line; --out_dir writes every mesh's grid as .binvox.

A cell is inside when a ray from its centre crosses the surface an odd number of times; three rays are cast, one along each axis, and
by default a cell is occupied when two of them agree.  A closed mesh gives the same answer along all three; the number of cells on
which they differ ("disagree") says how far a mesh is from closed.  Nothing here repairs a mesh, aligns a pair or takes gradients."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ragged import mesh_lists, pack_meshes

MAX_B, MAX_R = 65535, 512   # limits of bdm_hip.h section 21
MODES = {"vote": 0, "x": 1, "y": 2, "z": 3}
COUNT_KEYS = ("faces_used", "faces_dropped", "occupied_x", "occupied_y", "occupied_z", "occupied", "disagree", "reserved")


def _check_resolution(resolution, B=1):
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not 1 <= resolution <= MAX_R:
        raise ValueError(f"resolution={resolution!r} is not an integer in 1..{MAX_R}")
    if B > MAX_B:
        raise ValueError(f"{B} meshes exceed {MAX_B}: split the batch")
    if B * resolution ** 3 >= 2 ** 31:
        raise ValueError(f"{B} grids of {resolution}^3 cells reach 2^31: split the batch")


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode={mode!r} is none of {list(MODES)}")


def _given_frame(origin, cell_size, B):
    """Both or neither -> None, or (origin (B, 3) float32, cell (B,) float32) numpy arrays, checked."""
    if (origin is None) != (cell_size is None):
        raise ValueError("give both origin and cell_size, or neither (the bounding cube is then the frame)")
    if origin is None:
        return None
    o = np.asarray(origin.cpu() if torch.is_tensor(origin) else origin, dtype=np.float64)
    h = np.asarray(cell_size.cpu() if torch.is_tensor(cell_size) else cell_size, dtype=np.float64)
    if o.shape == (3,):
        o = np.broadcast_to(o, (B, 3))
    if h.shape == ():
        h = np.broadcast_to(h, (B,))
    if o.shape != (B, 3) or h.shape != (B,):
        raise ValueError(f"origin of shape {o.shape} and cell_size of shape {h.shape} do not fit {B} meshes")
    o, h = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(h, dtype=np.float32)
    if not (np.isfinite(o).all() and np.isfinite(h).all() and (h > 0).all()):
        raise ValueError("every origin must be finite and every cell_size positive and finite as a float32")
    return o, h


def _bounds(verts_list):
    """Per mesh the per-axis minimum and maximum over its finite vertices -> float32 (B, 2, 3) on the host, from one read-back; a mesh
    without a finite vertex gives (+inf, -inf)."""
    rows = []
    for v in verts_list:
        v = v.float().reshape(-1, 3)
        fin = torch.isfinite(v).all(dim=1, keepdim=True)
        lo = torch.where(fin, v, torch.full_like(v, float("inf")))
        hi = torch.where(fin, v, torch.full_like(v, float("-inf")))
        pad_lo, pad_hi = v.new_full((1, 3), float("inf")), v.new_full((1, 3), float("-inf"))
        rows.append(torch.stack([torch.cat([lo, pad_lo]).amin(dim=0), torch.cat([hi, pad_hi]).amax(dim=0)]))
    return torch.stack(rows).cpu().numpy()


def _cube_frame(bounds, resolution):
    """bounds (B, 2, 3) float32 -> (origin (B, 3), cell (B,)) float32: o the minimum, h = the largest extent / R in float32, the side
    1 where that extent is zero or not finite (no finite vertex: origin 0)."""
    B = bounds.shape[0]
    origin, cell = np.zeros((B, 3), dtype=np.float32), np.empty(B, dtype=np.float32)
    for m in range(B):
        lo, hi = bounds[m, 0], bounds[m, 1]
        side = np.float32(1)
        if np.isfinite(lo).all():
            origin[m] = lo
            with np.errstate(over="ignore"):
                ext = np.float32((hi - lo).max())
            if ext > 0 and np.isfinite(ext):
                side = ext
        cell[m] = np.float32(side / np.float32(resolution))
    return origin, cell


def _voxelize(verts_list, faces_list, resolution, origin, cell, mode, with_axes):
    """One bdm_mesh_voxelize call -> (occupancy uint8 (B, R, R, R), axes uint8 or None, counts int32 (B, 8)) on the device."""
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, R, dev = len(verts_list), resolution, verts.device
    sum_v, sum_f = int(vert_first[-1]), int(face_first[-1])
    if sum_v >= 2 ** 31 - 1 or 3 * sum_f >= 2 ** 31 - 1:
        raise ValueError("the batch reaches 2^31 vertices or face corners: split it")
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_voxelize_workspace_bytes(B, sum_v, sum_f, R), dev, "mesh_voxel")
    occ = torch.empty(B, R, R, R, dtype=torch.uint8, device=dev)
    axes = torch.empty(B, R, R, R, dtype=torch.uint8, device=dev) if with_axes else None
    counts = torch.empty(B, len(COUNT_KEYS), dtype=torch.int32, device=dev)
    o, h = torch.from_numpy(np.ascontiguousarray(origin, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(cell, dtype=np.float32))
    L.check(lib.bdm_mesh_voxelize(B, R, MODES[mode], o.data_ptr(), h.data_ptr(), L.ptr(verts), L.ptr(faces), vert_first.data_ptr(),
                                  face_first.data_ptr(), L.ptr(occ), L.ptr(axes), L.ptr(counts), L.ptr(ws), L.stream()), "mesh_voxelize")
    return occ, axes, counts


@torch.no_grad()
def voxelize_meshes(meshes, resolution=32, *, origin=None, cell_size=None, mode="vote", return_info=False):
    """The solid occupancy grids of a batch of meshes -> bool (B, R, R, R) indexed [mesh][ix][iy][iz] on the meshes' device.  Cell i
    of an axis has its centre at origin + (i + 0.5) cell_size.  origin ((3,) or (B, 3)) and cell_size (a number or (B,)) are given
    together; without them every mesh is voxelised in its own bounding cube: origin = the per-axis minimum of its finite vertices,
    cell_size = its largest extent / R in float32 (an extent of zero or a mesh without finite vertices: side 1), computed on the host
    from one read-back.  mode: "vote" (at least two of the three axis-aligned rays say inside) or one axis "x", "y", "z".  Faces with an
    index out of range or repeated, a non-finite vertex or a vertex beyond 2048 cells from the origin are dropped and counted.
    return_info: also a dict with "counts" (name -> int64 (B,) host tensor, the COUNT_KEYS), "axes" (uint8 (B, R, R, R): bit 0, 1, 2 =
    inside along x, y, z), "origin" (B, 3) and "cell_size" (B,) float32 host tensors.  Bad arguments raise ValueError before any
    launch; host tensors are refused."""
    _check_mode(mode)
    verts_list, faces_list = mesh_lists(meshes)
    B = len(verts_list)
    _check_resolution(resolution, B)
    frame = _given_frame(origin, cell_size, B)
    R = resolution
    if B == 0:
        empty = torch.zeros(0, R, R, R, dtype=torch.bool)
        info = {"counts": {k: torch.zeros(0, dtype=torch.int64) for k in COUNT_KEYS}, "axes": torch.zeros(0, R, R, R, dtype=torch.uint8),
                "origin": torch.zeros(0, 3), "cell_size": torch.zeros(0)}
        return (empty, info) if return_info else empty
    for t in list(verts_list) + list(faces_list):
        L.ptr(t)
    o, h = frame if frame is not None else _cube_frame(_bounds(verts_list), R)
    occ, axes, counts = _voxelize(verts_list, faces_list, R, o, h, mode, return_info)
    if not return_info:
        return occ.bool()
    rows = counts.cpu().long()
    info = {"counts": {k: rows[:, i].clone() for i, k in enumerate(COUNT_KEYS)}, "axes": axes, "origin": torch.from_numpy(o.copy()),
            "cell_size": torch.from_numpy(h.copy())}
    return occ.bool(), info


def voxel_iou(a, b):
    """Two occupancy grids (..., R, R, R) of one shape -> (iou float64, intersection int64, union int64), each of the leading shape:
    exact integer sums, one float64 division; an empty union gives nan."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape or a.dim() < 3:
        raise ValueError(f"grids of shapes {tuple(a.shape)} and {tuple(b.shape)} cannot be compared")
    a, b = a != 0, b != 0
    inter, union = (a & b).sum(dim=(-3, -2, -1)), (a | b).sum(dim=(-3, -2, -1))
    iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.full_like(inter, float("nan"), dtype=torch.float64))
    return iou, inter, union


@torch.no_grad()
def volumetric_iou(meshes_a, meshes_b, resolution=32, *, origin=None, cell_size=None, mode="vote", return_info=False):
    """The IoU of the solid occupancy grids of mesh i of the one batch and mesh i of the other, both voxelised in ONE frame ->
    float64 (B,) on the meshes' device.  Without a given frame it is the bounding cube of each pair (voxelize_meshes' rule over the
    vertices of both meshes).  return_info: also a dict with "intersection", "union" (int64 (B,)), "a" and "b" (voxelize_meshes' info
    of either side) and the grids "voxels_a", "voxels_b".  Nothing aligns the pair: run bdm_amd.alignment first where that is wanted."""
    _check_mode(mode)
    va, fa = mesh_lists(meshes_a)
    vb, fb = mesh_lists(meshes_b)
    if len(va) != len(vb):
        raise ValueError(f"{len(va)} meshes against {len(vb)}")
    B = len(va)
    _check_resolution(resolution, B)
    frame = _given_frame(origin, cell_size, B)
    if B and frame is None:
        both = _bounds(list(va) + list(vb))
        pair = np.stack([np.minimum(both[:B, 0], both[B:, 0]), np.maximum(both[:B, 1], both[B:, 1])], axis=1)
        frame = _cube_frame(pair, resolution)
    kw = dict(mode=mode, return_info=True)
    if B:
        kw.update(origin=frame[0], cell_size=frame[1])
    ga, ia = voxelize_meshes((list(va), list(fa)), resolution, **kw)
    gb, ib = voxelize_meshes((list(vb), list(fb)), resolution, **kw)
    iou, inter, union = voxel_iou(ga, gb)
    if not return_info:
        return iou
    return iou, {"intersection": inter, "union": union, "a": ia, "b": ib, "voxels_a": ga, "voxels_b": gb}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def compose_result(ious, disagree_fractions, faces_dropped):
    """The dictionary evaluate_voxel_dirs returns: `iou` is the mean over the pairs with a non-empty union (None without one), `empty`
    the number of pairs with an empty union, `disagree_fraction` the mean over the meshes of disagreeing cells over cells."""
    scored = [x for x in ious if x == x]
    return {"num": len(ious), "iou": sum(scored) / len(scored) if scored else None, "empty": len(ious) - len(scored),
            "disagree_fraction": sum(disagree_fractions) / len(disagree_fractions) if disagree_fractions else 0.0,
            "faces_dropped": int(faces_dropped)}


def _ground_truth(gt_dir, rel):
    """-> ("binvox", voxels, origin, cell) or ("mesh", verts, faces)."""
    from .io import load_binvox, load_mesh_ply
    vox_path, ply_path = (gt_dir / rel).with_suffix(".binvox"), gt_dir / rel
    if vox_path.exists():
        vox, translate, scale = load_binvox(vox_path)
        return "binvox", torch.from_numpy(vox), translate.astype(np.float32), np.float32(np.float32(scale) / np.float32(vox.shape[0]))
    if not ply_path.exists():
        raise FileNotFoundError(f"no ground truth for {rel}: neither {vox_path} nor {ply_path}")
    try:
        v, f = load_mesh_ply(ply_path)
    except ValueError as e:
        if "face element" not in str(e):
            raise
        f = np.zeros((0, 3), dtype=np.int64)
    if f.shape[0] == 0:
        raise ValueError(f"{ply_path} is a cloud without faces and has no volume: mesh the ground-truth clouds first with "
                         "`python -m bdm_amd.surface`, or give .binvox files")
    return "mesh", torch.from_numpy(v), torch.from_numpy(f)


def evaluate_voxel_dirs(mesh_dir, gt_dir, resolution=32, mode="vote", batch_size=16, out_dir=None, device=None):
    """Walk mesh_dir for mesh .ply files in sorted path order and score each against gt_dir/<same relative path>: a .binvox of the
    same stem (the frame is its own: origin = translate, cell = scale / dim, R = dim) or a mesh .ply (R = resolution, the frame the
    bounding cube of the pair).  A ground-truth cloud without faces is refused.  out_dir: every mesh's grid is written there as
    .binvox, in the frame it was scored in.  -> compose_result's dictionary."""
    from .io import load_mesh_ply, save_binvox
    mesh_dir, gt_dir = Path(mesh_dir), Path(gt_dir)
    _check_resolution(resolution)
    _check_mode(mode)
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("batch_size must be a positive integer")
    if device is None:
        if not torch.cuda.is_available():
            raise L.BdmHipError("bdm_amd.mesh_voxel needs a HIP device (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    items = [(path.relative_to(mesh_dir), path) for path in sorted(mesh_dir.rglob("*.ply"))]
    ious, fractions, dropped = [], [], 0
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        meshes = [tuple(torch.from_numpy(x) for x in load_mesh_ply(path)) for _, path in chunk]
        truths = [_ground_truth(gt_dir, rel) for rel, _ in chunk]
        groups = {}   # the resolution (None: a mesh pair) -> the chunk's rows scored together
        for at, gt in enumerate(truths):
            groups.setdefault(int(gt[1].shape[0]) if gt[0] == "binvox" else None, []).append(at)
        scored = {}
        for R, rows in groups.items():
            verts, faces = [meshes[at][0].to(device) for at in rows], [meshes[at][1].to(device) for at in rows]
            if R is None:
                gv, gf = [truths[at][1].to(device) for at in rows], [truths[at][2].to(device) for at in rows]
                iou, info = volumetric_iou((verts, faces), (gv, gf), resolution, mode=mode, return_info=True)
                grids, pred, cells = info["voxels_a"], info["a"], resolution ** 3
                dropped += int(info["b"]["counts"]["faces_dropped"].sum())
            else:
                origin, cell = np.stack([truths[at][2] for at in rows]), np.stack([truths[at][3] for at in rows])
                grids, pred = voxelize_meshes((verts, faces), R, origin=origin, cell_size=cell, mode=mode, return_info=True)
                iou, _, _ = voxel_iou(grids.cpu(), torch.stack([truths[at][1] for at in rows]))
                cells = R ** 3
            dropped += int(pred["counts"]["faces_dropped"].sum())
            for k, at in enumerate(rows):
                scored[at] = (float(iou[k]), int(pred["counts"]["disagree"][k]) / cells, grids[k].cpu(), pred["origin"][k], pred["cell_size"][k])
        for at, (rel, _) in enumerate(chunk):
            iou, fraction, grid, origin, cell = scored[at]
            ious.append(iou), fractions.append(fraction)
            if out_dir is not None:
                side = float(np.float32(cell) * np.float32(grid.shape[0]))
                save_binvox(grid.numpy(), (Path(out_dir) / rel).with_suffix(".binvox"), origin.tolist(), side)
    return compose_result(ious, fractions, dropped)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_voxel",
                                 description="volumetric IoU of a tree of triangle meshes against ground-truth meshes or .binvox grids")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--gt_dir", required=True, help="the same tree of ground-truth mesh .ply or .binvox files")
    ap.add_argument("--resolution", type=int, default=32, help=f"cells per axis for mesh ground truth, 1..{MAX_R} (a .binvox brings its own)")
    ap.add_argument("--mode", choices=list(MODES), default="vote")
    ap.add_argument("--out_dir", default=None, help="write every mesh's grid here as .binvox")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    try:
        _check_resolution(args.resolution)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    result = evaluate_voxel_dirs(args.mesh_dir, args.gt_dir, args.resolution, args.mode, args.batch_size, out_dir=args.out_dir)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
