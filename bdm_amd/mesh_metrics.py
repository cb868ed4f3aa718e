"""Scoring triangle meshes on the HIP path: area-weighted surface samples (pytorch3d's sample_points_from_meshes) and the squared
distance from points to the nearest face (the point-to-face half of pytorch3d's point_mesh_face_distance), restated from their
published behaviour (bdm_mesh_sample_points / bdm_point_mesh_distance, csrc/mesh_metrics.hip; the rule is stated in
include/bdm_hip.h section 14 and DESIGN.md section 18), and the reconstruction metrics of a tree of meshes built on the two.

    python -m bdm_amd.mesh_metrics --mesh_dir D --gt_dir D [--num-samples S] [--seed K] [--batch-size 16] [--two-sided]

samples every mesh .ply of mesh_dir that has a ground-truth cloud at the same relative path of gt_dir and prints one JSON line:
CD x 1e3 and F1@0.01 of the samples against the ground truth (bdm_amd.evaluation's protocol), and the distance from the ground-truth
points to the mesh itself, which is free of sampling noise.  --two-sided adds the other direction, from the faces of the mesh to the
ground-truth points (bdm_face_point_distance, csrc/face_point.hip; bdm_hip.h section 17): how much of the mesh
lies where the ground truth has nothing, and pytorch3d's symmetric point_mesh_face_distance."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from . import ops, rng
from .ragged import first, mesh_lists, pack_meshes, pack_rows

MAX_FACES, MAX_B = 1 << 24, 65535   # limits of bdm_hip.h section 14
FORMS = {None: 0, "exhaustive": 1}   # the culled form is not built (no margin keeps its bits: DESIGN.md section 18)
FACE_FORMS = {None: 0, "resident": 1, "split": 2}   # bdm_hip.h section 17
FACE_THREADS, MAX_CHUNKS = 256, 65535


def _check_sizes(verts_list, faces_list):
    """The limits of bdm_hip.h section 14 on a batch, before anything is packed."""
    nv, nf = [int(v.shape[0]) for v in verts_list], [int(f.shape[0]) for f in faces_list]
    if len(nv) > MAX_B:
        raise ValueError(f"{len(nv)} meshes exceed {MAX_B}: split the batch")
    if nf and max(nf) > MAX_FACES:
        raise ValueError(f"a mesh of {max(nf)} faces exceeds {MAX_FACES}")
    if sum(nv) >= 2 ** 31 or sum(nf) >= 2 ** 31:
        raise ValueError("the batch reaches 2^31 vertices or faces: split it")


@torch.no_grad()
def sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, *, seed=0, first_index=0, return_face_idx=False):
    """pytorch3d's sample_points_from_meshes: `num_samples` area-weighted surface points per mesh -> (B, S, 3) on the meshes' device,
    then the unit face normals (B, S, 3) if return_normals, then the face index within the mesh (B, S) int64 if return_face_idx.
    Mesh m draws from the Philox stream keyed rng.shape_key(seed, first_index + m), purpose rng.MESH: its samples do not depend on
    its batch slot.  A mesh without a valid face yields zeros (and face index -1), as pytorch3d does for empty meshes.
    Bad arguments raise ValueError before any launch."""
    verts_list, faces_list = mesh_lists(meshes)
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"num_samples={num_samples} is not positive")
    B = len(verts_list)
    if B * S >= 2 ** 31:
        raise ValueError(f"{B} meshes of {S} samples reach 2^31: split the batch")
    if B == 0:
        out = (torch.zeros(0, S, 3),) + ((torch.zeros(0, S, 3),) if return_normals else ()) + \
            ((torch.zeros(0, S, dtype=torch.int64),) if return_face_idx else ())
        return out if len(out) > 1 else out[0]
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    dev, max_f = verts.device, int((face_first[1:] - face_first[:-1]).max())
    keys = [rng.shape_key(seed, int(first_index) + m) for m in range(B)]
    keys = torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in keys], dtype=torch.int64).to(dev)
    points = torch.empty(B, S, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(B, S, 3, dtype=torch.float32, device=dev) if return_normals else None
    face_idx = torch.empty(B, S, dtype=torch.int32, device=dev) if return_face_idx else None
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_sample_workspace_bytes(B, int(face_first[-1]), max_f), dev, "mesh_sample")
    L.check(lib.bdm_mesh_sample_points(B, S, max_f, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), L.ptr(keys), 0,
                                       rng.MESH, L.ptr(points), L.ptr(face_idx), L.ptr(normals), L.ptr(ws), L.stream()), "mesh_sample_points")
    out = (points,) + ((normals,) if return_normals else ()) + ((face_idx.long(),) if return_face_idx else ())
    return out if len(out) > 1 else out[0]


def morton_order(points, bits=10):
    """(B, P) int32 permutation: every cloud's points in Morton order of their coordinates quantised to `bits` bits per axis over the
    cloud's bounding box (torch integer operations and one sort on the points' device)."""
    p = torch.nan_to_num(points.float(), nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = p.min(dim=1, keepdim=True).values, p.max(dim=1, keepdim=True).values
    top = (1 << bits) - 1
    cell = ((p - lo) / (hi - lo).clamp_min(1e-30) * top).long().clamp(0, top)
    code = torch.zeros(cell.shape[:2], dtype=torch.int64, device=points.device)
    for b in range(bits):
        for axis in range(3):
            code |= ((cell[..., axis] >> b) & 1) << (3 * b + axis)
    return torch.sort(code, dim=1, stable=True).indices.int()


@torch.no_grad()
def point_mesh_sqdist(meshes, points, *, form=None, order=None):
    """(sqdist (B, P) float32, face_idx (B, P) int64): for every point of `points` ((B, P, 3) or a Pointclouds of equal sizes) the
    squared distance to the nearest valid face of mesh b and that face's index within the mesh (the lowest among equal distances).
    A point with a non-finite coordinate, and every point of a mesh without a valid face, gets (+inf, -1).
    form: None (the chooser) or "exhaustive".  order: None (natural), "morton", or a (B, P) integer permutation -- which thread takes
    which point; the result does not depend on it.  Bad arguments raise ValueError before any launch."""
    verts_list, faces_list = mesh_lists(meshes)
    if hasattr(points, "points_padded"):
        points = points.points_padded()
    if form not in FORMS:
        raise ValueError(f"form={form!r} is none of {list(FORMS)} (the culled form is not built)")
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3 or not points.is_floating_point():
        raise ValueError("expected a Pointclouds or a floating-point (B, P, 3) tensor")
    B, P, _ = points.shape
    if B != len(verts_list):
        raise ValueError(f"{B} clouds for {len(verts_list)} meshes")
    if B * P >= 2 ** 31:
        raise ValueError(f"{B} clouds of {P} points reach 2^31: split the batch")
    if torch.is_tensor(order) and (tuple(order.shape) != (B, P) or order.is_floating_point() or order.dtype == torch.bool):
        raise ValueError(f"order must be a (B, P) = ({B}, {P}) integer permutation")
    if order is not None and not torch.is_tensor(order) and order != "morton":
        raise ValueError(f"order={order!r} is none of None, 'morton', a (B, P) integer tensor")
    if B == 0 or P == 0:
        return torch.zeros(B, P, device=points.device), torch.zeros(B, P, dtype=torch.int64, device=points.device)
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    dev = verts.device
    points = L.f32(points.float().to(dev))
    if isinstance(order, str):
        order = morton_order(points)
    sqdist = torch.full((B, P), float("inf"), dtype=torch.float32, device=dev)   # (an order that is no permutation leaves these)
    face_idx = torch.full((B, P), -1, dtype=torch.int32, device=dev)
    order = None if order is None else L.i32(order.to(dev))
    lib = L.lib()
    ws = ops.workspace(lib.bdm_point_mesh_distance_workspace_bytes(B, int(face_first[-1])), dev, "mesh_distance")
    L.check(lib.bdm_point_mesh_distance(B, P, FORMS[form], L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(),
                                        L.ptr(points), L.ptr(order), L.ptr(sqdist), L.ptr(face_idx), L.ptr(ws), L.stream()),
            "point_mesh_distance")
    return sqdist, face_idx.long()


def _cloud_list(points, count):
    """A (B, P, 3) tensor, a Pointclouds or a list of (P_i, 3) tensors -> the list, checked against `count` meshes."""
    if hasattr(points, "points_list"):
        points = points.points_list()
    elif torch.is_tensor(points):
        if points.dim() != 3:
            raise ValueError(f"expected a (B, P, 3) tensor, a Pointclouds or a list of (P, 3) tensors, got shape {tuple(points.shape)}")
        points = list(points)
    if not isinstance(points, (list, tuple)):
        raise ValueError(f"expected a (B, P, 3) tensor, a Pointclouds or a list of (P, 3) tensors, got {type(points).__name__}")
    for t in points:
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or not t.is_floating_point():
            raise ValueError("every cloud must be a floating-point (P, 3) tensor")
    if len(points) != count:
        raise ValueError(f"{len(points)} clouds for {count} meshes")
    if sum(int(t.shape[0]) for t in points) >= 2 ** 31:
        raise ValueError("the clouds reach 2^31 points: split the batch")
    return list(points)


@torch.no_grad()
def face_point_sqdist(meshes, points, *, form=None, chunks=None):
    """(sqdist_list, point_idx_list), one float32 (F_m) and one int64 (F_m) tensor per mesh: for every face of mesh m the squared
    distance to the nearest point of cloud m and that point's index within the cloud (the lowest among equal distances).  An invalid
    face, every face of a mesh whose cloud is empty, and a face no point is at a finite distance of get (+inf, -1); a point with a
    non-finite coordinate is nobody's nearest point.  points: a (B, P, 3) tensor, a Pointclouds or a list of (P_i, 3) tensors.
    form: None (the chooser), "resident" or "split"; chunks (split only): over how many workgroups a cloud is divided, None for the
    chooser's count.  Neither changes a bit of the result.  Bad arguments raise ValueError before any launch."""
    verts_list, faces_list = mesh_lists(meshes)
    if form not in FACE_FORMS:
        raise ValueError(f"form={form!r} is none of {list(FACE_FORMS)}")
    if chunks is not None and (isinstance(chunks, bool) or not isinstance(chunks, int) or not 1 <= chunks <= MAX_CHUNKS):
        raise ValueError(f"chunks={chunks!r} is not an integer in 1 .. {MAX_CHUNKS}")
    if chunks is not None and form != "split" and not (form == "resident" and chunks == 1):
        raise ValueError("only form='split' takes a chunk count")
    clouds = _cloud_list(points, len(verts_list))
    B = len(verts_list)
    if B == 0:
        return [], []
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    dev, sum_f = verts.device, int(face_first[-1])
    pts = pack_rows([c.to(dev) for c in clouds], 3, dev)
    point_first = first(c.shape[0] for c in clouds)
    sqdist = torch.full((max(sum_f, 1),), float("inf"), dtype=torch.float32, device=dev)
    point_idx = torch.full((max(sum_f, 1),), -1, dtype=torch.int32, device=dev)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_face_point_distance_workspace_bytes(B, sum_f), dev, "face_point")
    L.check(lib.bdm_face_point_distance(B, FACE_FORMS[form], chunks or 0, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(),
                                        face_first.data_ptr(), L.ptr(pts), point_first.data_ptr(), L.ptr(sqdist), L.ptr(point_idx), L.ptr(ws),
                                        L.stream()), "face_point_distance")
    cuts = face_first.tolist()
    return ([sqdist[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [point_idx[a:b].long() for a, b in zip(cuts[:-1], cuts[1:])])


def symmetric_distance(point_sq, face_sq):
    """The value of point_mesh_face_distance from the two kernels' outputs: lists (one entry per mesh) of the squared distances of
    the cloud's points and of the mesh's faces -> sum_m mean(point_sq[m]) / B + sum_m mean(face_sq[m]) / B, every mean and sum in
    float64 (a Python float)."""
    B = len(point_sq)
    mean = lambda t: float(torch.as_tensor(t).double().mean())   # noqa: E731
    return sum(mean(t) for t in point_sq) / B + sum(mean(t) for t in face_sq) / B


@torch.no_grad()
def point_mesh_face_distance(meshes, pcls, min_triangle_area=None):
    """pytorch3d's point_mesh_face_distance, by name and argument order: sum_m mean_p d(p, mesh_m) / B + sum_m mean_f d(f, cloud_m) / B,
    d(p, mesh) the squared distance from a point to the nearest face (point_mesh_sqdist) and d(f, cloud) from a face to the nearest
    point (face_point_sqdist) -> a 0-dim float64 tensor on the meshes' device.  Each mean is formed in float64 from the float32 kernel
    outputs.  EVERY face of a mesh takes part in the second mean, as in pytorch3d: an invalid face (indices out of range, non-finite
    or collinear vertices) contributes +inf, and so does a point with a non-finite coordinate to the first; a mean over no points or
    no faces is NaN.  min_triangle_area must stay None: this rule has no area floor (the departure of DESIGN.md section 8) -- a
    face takes part as soon as its computed squared normal is positive.  Bad arguments raise ValueError before any launch."""
    if min_triangle_area is not None:
        raise ValueError("min_triangle_area is not supported: the rule of bdm_hip.h section 14 has no area floor (DESIGN.md section 8); "
                         "a face is valid as soon as its squared normal is positive")
    verts_list, faces_list = mesh_lists(meshes)
    clouds = _cloud_list(pcls, len(verts_list))
    if not verts_list:
        raise ValueError("an empty batch has no distance")
    _check_sizes(verts_list, faces_list)
    face_sq, _ = face_point_sqdist((verts_list, faces_list), clouds)
    if len({int(c.shape[0]) for c in clouds}) == 1:
        point_sq = list(point_mesh_sqdist((verts_list, faces_list), torch.stack(clouds))[0])
    else:   # the point side takes clouds of one size: ragged clouds go mesh by mesh
        point_sq = [point_mesh_sqdist(([v], [f]), c[None])[0][0] for v, f, c in zip(verts_list, faces_list, clouds)]
    return torch.tensor(symmetric_distance(point_sq, face_sq), dtype=torch.float64, device=verts_list[0].device)


def face_areas(verts, faces, valid):
    """Areas of the faces of one mesh in float64 on the host, 0 where `valid` is False: verts (V, 3) and faces (F, 3) numpy arrays or
    host tensors, valid (F) bool."""
    v, f, valid = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64), np.asarray(valid, dtype=bool)
    area = np.zeros(f.shape[0], dtype=np.float64)
    if valid.any():
        t = v[f[valid]]
        area[valid] = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    return area


def compose_scores(rows, two_sided=None):
    """[(cd_x1000, f1, gt sqdist (n,) float64 array) or None for an empty mesh] -> the dictionary evaluate_mesh_dirs returns.
    Two-sided rows carry two more entries: the face-to-point squared distances of ALL faces (F,) float64 (+inf for an invalid face)
    and the faces' float64 areas (F,), 0 for an invalid face; the dictionary then gains "surface_to_gt_x1000", "surface_within_0.01"
    and "face_distance_x1000".  two_sided: None = as the rows are."""
    kept = [r for r in rows if r is not None]
    nan = float("nan")
    out = {"num": len(rows), "cd_x1000": float(np.mean([r[0] for r in kept])) if kept else nan,
           "f1_at_0.01": float(np.mean([r[1] for r in kept])) if kept else nan,
           "gt_to_surface_x1000": float(np.mean([r[2].mean() for r in kept])) * 1000.0 if kept else nan,
           "gt_within_0.01": float(np.mean([(r[2] < 0.01).mean() for r in kept])) if kept else nan, "empty": len(rows) - len(kept)}
    if two_sided is None:
        two_sided = any(len(r) > 3 for r in kept)
    if not two_sided:
        return out
    s2g, within, sym = [], [], []
    for _, _, gt_sq, face_sq, area in kept:
        ok = area > 0
        s2g.append(float((area[ok] * face_sq[ok]).sum() / area[ok].sum()) if ok.any() else nan)
        within.append(float(area[ok & (face_sq < 0.01)].sum() / area[ok].sum()) if ok.any() else nan)
        sym.append(float(gt_sq.mean()) + float(face_sq.mean()))
    out["surface_to_gt_x1000"] = float(np.mean(s2g)) * 1000.0 if kept else nan
    out["surface_within_0.01"] = float(np.mean(within)) if kept else nan
    out["face_distance_x1000"] = float(np.mean(sym)) * 1000.0 if kept else nan
    return out


def evaluate_mesh_dirs(mesh_dir, gt_dir, num_samples=None, seed=0, batch_size=16, device="cuda", two_sided=False):
    """For every mesh .ply under mesh_dir with a ground-truth cloud .ply at the same relative path under gt_dir (in sorted path
    order; file i samples from the stream of shape index i): as many surface samples as the ground truth has points (or
    num_samples), scored by evaluation.chamfer_distance_x1000 and evaluation.f1_score under evaluation.evaluate_dirs' centring.
    -> {"num", "cd_x1000", "f1_at_0.01", "gt_to_surface_x1000" (mean squared distance from the UNCENTRED ground-truth points to the mesh,
    x 1000), "gt_within_0.01" (share of ground-truth points with squared distance below 0.01), "empty" (meshes without a valid face:
    counted in num, left out of the means)}.
    two_sided=True adds the direction the ground truth cannot see, from every face of the mesh to the nearest (uncentred)
    ground-truth point: "surface_to_gt_x1000" (per mesh the area-weighted mean of that squared distance over its valid faces, x 1000;
    the areas in float64 on the host), "surface_within_0.01" (the area share of valid faces with squared distance below 0.01) and
    "face_distance_x1000" (point_mesh_face_distance of the file alone, x 1000), each averaged over the non-empty files."""
    from .evaluation import chamfer_distance_x1000, f1_score
    from .io import load_mesh_ply, load_pointcloud_ply
    mesh_dir, gt_dir = Path(mesh_dir), Path(gt_dir)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    if num_samples is not None and int(num_samples) < 1:
        raise ValueError(f"num_samples={num_samples} is not positive")
    items = []
    for path in sorted(mesh_dir.rglob("*.ply")):
        rel = path.relative_to(mesh_dir)
        if (gt_dir / rel).exists():
            items.append((len(items), path, gt_dir / rel))
    rows = [None] * len(items)
    groups = {}   # ground-truth point count -> items: one batch holds clouds of one size
    loaded = {}
    for i, path, gt_path in items:
        loaded[i] = (load_mesh_ply(path), load_pointcloud_ply(gt_path))
        groups.setdefault(loaded[i][1].shape[0], []).append(i)
    for n_gt, members in sorted(groups.items()):
        for lo in range(0, len(members), batch_size):
            # consecutive file indices form one call (first_index + m must be the file's index); others go alone
            chunk = members[lo:lo + batch_size]
            runs, run = [], [chunk[0]]
            for i in chunk[1:]:
                if i == run[-1] + 1:
                    run.append(i)
                else:
                    runs.append(run)
                    run = [i]
            runs.append(run)
            for run in runs:
                verts = [torch.from_numpy(loaded[i][0][0]).to(device) for i in run]
                faces = [torch.from_numpy(loaded[i][0][1]).to(device) for i in run]
                gt = torch.stack([torch.from_numpy(loaded[i][1]) for i in run]).to(device)
                S = n_gt if num_samples is None else int(num_samples)
                samples, fidx = sample_points_from_meshes((verts, faces), S, seed=seed, first_index=run[0], return_face_idx=True)
                sq, _ = point_mesh_sqdist((verts, faces), gt)
                sq, empty = sq.double().cpu().numpy(), (fidx < 0).all(dim=1).cpu().tolist()
                if two_sided:
                    face_sq, face_pt = face_point_sqdist((verts, faces), gt)
                for j, i in enumerate(run):
                    if empty[j]:
                        continue
                    # one cloud at a time: torch's mean (the centring) sums in an order that depends on the batch size, and a file's
                    # score must not depend on what it was batched with
                    s, g = samples[j:j + 1], gt[j:j + 1]
                    rows[i] = (float(chamfer_distance_x1000(s, g)[0]),
                               float(f1_score(s - s.mean(1, keepdim=True), g - g.mean(1, keepdim=True))[0]), sq[j])
                    if two_sided:
                        rows[i] += (face_sq[j].double().cpu().numpy(), face_areas(*loaded[i][0], (face_pt[j] >= 0).cpu().numpy()))
    return compose_scores(rows, two_sided=bool(two_sided))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_metrics",
                                 description="CD x 1e3, F1@0.01 and point-to-surface distance of mesh .ply trees against gt cloud trees")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--gt_dir", required=True, help="directory tree of ground-truth .ply clouds with the same relative paths")
    ap.add_argument("--num-samples", type=int, default=None, help="surface samples per mesh (default: as many as the ground truth has points)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--two-sided", action="store_true",
                    help="also score the faces of every mesh against the ground-truth points: surface_to_gt_x1000, surface_within_0.01, "
                         "face_distance_x1000")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or (args.num_samples is not None and args.num_samples < 1):
        ap.error("--batch-size and --num-samples must be positive")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_metrics needs a HIP device (no CPU fallback)")
    result = evaluate_mesh_dirs(args.mesh_dir, args.gt_dir, args.num_samples, args.seed, args.batch_size, two_sided=args.two_sided)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
