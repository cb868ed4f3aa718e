"""Point-cloud normals on the HIP path: pytorch3d's `estimate_pointcloud_normals` (ops/points_normals.py) with its name,
argument order and defaults, and the self K-nearest-neighbour search underneath it, over bdm_estimate_normals
(csrc/normals.hip; the rule is stated in include/bdm_hip.h section 10 and DESIGN.md section 14).  pytorch3d is not installed, so
the function is restated from its published behaviour ("parity unpinned", as for the renderer).

    python -m bdm_amd.normals --in_dir <tree of .ply> --out_dir <tree> [--neighborhood-size 50] [--batch-size 16]
                              [--orient {neighbours,canonical,visibility}] [--no-disambiguate]

writes every cloud again under the same relative path with nx, ny, nz per vertex and prints one JSON line.

The three sign rules of the estimator are local.  `orient_normals_by_visibility` (bdm_orient_normals, csrc/orient.hip; the rule is
stated in include/bdm_hip.h section 11 and DESIGN.md section 15) makes the signs agree over the whole surface, pointing outwards:
what screened Poisson or ball pivoting need.  `estimate_pointcloud_normals(..., disambiguate_directions="visibility")` and
`--orient visibility` run it behind the estimator."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

from . import _lib as L
from . import ops

K_MIN, K_MAX = 3, 64
ORIENT_CANONICAL, ORIENT_NEIGHBOURS, ORIENT_VIEWPOINT = 0, 1, 2
# limits of bdm_orient_normals (bdm_hip.h section 11)
ORIENT_N_MAX, ORIENT_VIEWS_MAX, ORIENT_RESOLUTION_MAX, ORIENT_SPLAT_MAX, ORIENT_ROUNDS_MAX, ORIENT_EPS_MAX = 32768, 256, 128, 4, 32, 65535
VISIBILITY_K = 16   # neighbours orient_normals_by_visibility looks up itself when it is given none


def _points_of(pointclouds):
    points = pointclouds.points_padded() if hasattr(pointclouds, "points_padded") else pointclouds
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"expected a Pointclouds or a (B, N, 3) tensor, got {tuple(points.shape)}")
    return points


def _check_k(n, k):
    if n <= k:   # pytorch3d's check and message
        raise ValueError("The neighborhood_size argument has to be" + " strictly smaller than the number of points in the cloud.")
    if not K_MIN <= k <= K_MAX:
        raise ValueError(f"neighborhood_size={k} is outside {K_MIN}..{K_MAX} (the kernel holds one neighbour per lane of a wave)")


def _estimate(points, k, orient, viewpoint=None, want_idx=False, want_curvatures=False):
    """One bdm_estimate_normals call: (normals (B, N, 3), knn_idx (B, N, k) int32 or None, curvatures (B, N, 3) or None)."""
    k = int(k)
    _check_k(points.shape[1], k)
    points = L.f32(points)
    L.ptr(points)   # refuses host tensors before anything is allocated
    B, N, _ = points.shape
    dev = points.device
    if B * N * k >= 2 ** 31:
        raise ValueError(f"{B} clouds of {N} points with {k} neighbours exceed 2^31 indices: split the batch")
    normals = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev) if want_idx else None
    curv = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if want_curvatures else None
    lib = L.lib()
    nbytes = lib.bdm_estimate_normals_workspace_bytes(B, N, k)
    ws = ops.workspace(nbytes, dev, "normals") if nbytes else None
    L.check(lib.bdm_estimate_normals(B, N, k, orient, L.ptr(points), L.ptr(viewpoint), L.ptr(idx), L.ptr(normals), L.ptr(curv),
                                     L.ptr(ws), L.stream()), "estimate_normals")
    return normals, idx, curv


@torch.no_grad()
def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True, *, use_symeig_workaround=True,
                                viewpoint=None, return_curvatures=False):
    """Normals (B, N, 3) of a `Pointclouds` or a (B, N, 3) tensor: the unit eigenvector of the smallest eigenvalue of the
    covariance of every point's `neighborhood_size` nearest neighbours (the point itself included).
    disambiguate_directions=True: pytorch3d's rule (the normal points to the side where most neighbours lie); False: the
    component of largest magnitude is positive; "visibility": the canonical estimate, then orient_normals_by_visibility with its
    defaults on the same neighbour lists (outward, consistent over the surface); any other string is refused.
    viewpoint (B, 3) or (3,): the normals point towards it instead (not together with "visibility").
    use_symeig_workaround is accepted for signature parity and ignored (there is one eigen-solver).
    return_curvatures=True: (normals, curvatures (B, N, 3)), the eigenvalues ascending.  Rows of non-finite points are NaN."""
    points = _points_of(pointclouds)
    if isinstance(disambiguate_directions, str):
        if disambiguate_directions != "visibility":
            raise ValueError(f"disambiguate_directions={disambiguate_directions!r}: expected True, False or 'visibility'")
        if viewpoint is not None:
            raise ValueError("disambiguate_directions='visibility' and a viewpoint are two sign rules: pass one")
        normals, idx, curv = _estimate(points, neighborhood_size, ORIENT_CANONICAL, want_idx=True, want_curvatures=return_curvatures)
        normals = orient_normals_by_visibility(points, normals, idx)
        return (normals, curv) if return_curvatures else normals
    orient = ORIENT_NEIGHBOURS if disambiguate_directions else ORIENT_CANONICAL
    if viewpoint is not None:
        viewpoint = torch.as_tensor(viewpoint, dtype=torch.float32)
        if viewpoint.shape not in ((3,), (points.shape[0], 3)):
            raise ValueError(f"viewpoint must be (3,) or ({points.shape[0]}, 3), got {tuple(viewpoint.shape)}")
        viewpoint = viewpoint.expand(points.shape[0], 3).contiguous().to(points.device)
        orient = ORIENT_VIEWPOINT
    normals, _, curv = _estimate(points, neighborhood_size, orient, viewpoint, want_curvatures=return_curvatures)
    return (normals, curv) if return_curvatures else normals


@torch.no_grad()
def knn_self(points, K):
    """(B, N, K) int64: for every point the indices, within its cloud, of the K points with the smallest (squared distance,
    index), ascending, the point itself included; -1 rows for non-finite points."""
    return _estimate(_points_of(points), K, ORIENT_CANONICAL, want_idx=True)[1].long()


def fibonacci_views(num_views):
    """(num_views, 3, 3) float32 on the host: per view the rows u, w, d of bdm_orient_normals.  d runs over the Fibonacci sphere
    (z = 1 - (2 i + 1) / V, azimuth i pi (3 - sqrt 5)); u = e x d normalised with e the coordinate axis d is least aligned with
    (the lowest among equals), w = d x u.  Formed in float64, rounded to float32."""
    num_views = int(num_views)
    if not 1 <= num_views <= ORIENT_VIEWS_MAX:
        raise ValueError(f"num_views={num_views} is outside 1..{ORIENT_VIEWS_MAX}")
    i = torch.arange(num_views, dtype=torch.float64)
    z = 1.0 - (2.0 * i + 1.0) / num_views
    rad = torch.sqrt((1.0 - z * z).clamp_min(0.0))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    d = torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), z], dim=1)
    d = d / d.norm(dim=1, keepdim=True)
    e = torch.nn.functional.one_hot(d.abs().argmin(dim=1), 3).double()
    u = torch.linalg.cross(e, d)
    u = u / u.norm(dim=1, keepdim=True)
    w = torch.linalg.cross(d, u)
    return torch.stack([u, w, d], dim=1).float()


def _check_orient_args(points, normals, knn_idx, resolution, splat, depth_tolerance_px, fallback_k, fallback_rounds, views):
    """Argument checks of orient_normals_by_visibility that need no device -> (eps, views (v, 3, 3) float32 host or device)."""
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"expected (B, N, 3) points, got {tuple(points.shape)}")
    if tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f"normals {tuple(normals.shape)} do not match points {tuple(points.shape)}")
    B, N, _ = points.shape
    if not 1 <= N <= ORIENT_N_MAX:
        raise ValueError(f"{N} points per cloud are outside 1..{ORIENT_N_MAX}")
    resolution, splat, fallback_k, fallback_rounds = int(resolution), int(splat), int(fallback_k), int(fallback_rounds)
    if not 1 <= resolution <= ORIENT_RESOLUTION_MAX:
        raise ValueError(f"resolution={resolution} is outside 1..{ORIENT_RESOLUTION_MAX} (the z-buffer lives in one workgroup's LDS)")
    if not 0 <= splat <= ORIENT_SPLAT_MAX:
        raise ValueError(f"splat={splat} is outside 0..{ORIENT_SPLAT_MAX}")
    if not 0 <= fallback_rounds <= ORIENT_ROUNDS_MAX:
        raise ValueError(f"fallback_rounds={fallback_rounds} is outside 0..{ORIENT_ROUNDS_MAX}")
    if not (depth_tolerance_px >= 0 and math.isfinite(depth_tolerance_px)):
        raise ValueError(f"depth_tolerance_px={depth_tolerance_px} must be finite and not negative")
    eps = int(round(depth_tolerance_px * 65536 / resolution))
    if eps > ORIENT_EPS_MAX:
        raise ValueError(f"depth_tolerance_px={depth_tolerance_px} at resolution {resolution} gives eps={eps} above {ORIENT_EPS_MAX}")
    if knn_idx is not None:
        if knn_idx.dim() != 3 or tuple(knn_idx.shape[:2]) != (B, N) or knn_idx.shape[2] < 1:
            raise ValueError(f"knn_idx must be ({B}, {N}, k), got {tuple(knn_idx.shape)}")
        if knn_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"knn_idx must hold int32 or int64 indices, got {knn_idx.dtype}")
        k = knn_idx.shape[2]
    else:
        k = min(VISIBILITY_K, N - 1)
        if k < K_MIN:
            raise ValueError(f"{N} points are too few to look neighbours up: pass knn_idx")
    if not 1 <= fallback_k <= k:
        raise ValueError(f"fallback_k={fallback_k} is outside 1..{k} (the width of the neighbour lists)")
    if B * N * k >= 2 ** 31:
        raise ValueError(f"{B} clouds of {N} points with {k} neighbours exceed 2^31 indices: split the batch")
    if views is not None:
        views = torch.as_tensor(views)
        if views.dim() != 3 or tuple(views.shape[1:]) != (3, 3) or not 1 <= views.shape[0] <= ORIENT_VIEWS_MAX:
            raise ValueError(f"views must be (v, 3, 3) with v in 1..{ORIENT_VIEWS_MAX}, got {tuple(views.shape)}")
        views = views.float()
    return eps, views


@torch.no_grad()
def orient_normals_by_visibility(points, normals, knn_idx=None, *, num_views=32, resolution=128, splat=2, depth_tolerance_px=2.0,
                                 fallback_k=8, fallback_rounds=8, views=None, return_info=False):
    """Normals (B, N, 3) with signs that agree over the whole surface and point outwards (bdm_hip.h section 11): the cloud is
    looked at from the `views` (default: num_views Fibonacci-sphere directions); a point that survives a z-buffer test of
    resolution x resolution pixels, splatted by `splat` pixels, with a depth tolerance of depth_tolerance_px pixel widths, votes
    for the side of its normal that faces the viewer.  Points no view decided take the sign of the first fallback_k neighbours of
    knn_idx (B, N, k) (None: knn_self with 16 neighbours), in at most fallback_rounds rounds.  The output carries the input's
    bits or their negation; where a sign was decided it does not depend on the input's signs.
    return_info=True: (normals, {"votes" (B, N) int32, "seen" (B, N) int32, "undecided" (B,) int32})."""
    eps, views = _check_orient_args(points, normals, knn_idx, resolution, splat, depth_tolerance_px, fallback_k, fallback_rounds, views)
    if views is None:
        views = fibonacci_views(num_views)
    points, normals = L.f32(points), L.f32(normals)
    L.ptr(points), L.ptr(normals)   # refuses host tensors before anything is allocated
    dev = points.device
    B, N, _ = points.shape
    if knn_idx is None:
        knn_idx = _estimate(points, min(VISIBILITY_K, N - 1), ORIENT_CANONICAL, want_idx=True)[1]
    knn_idx = L.i32(knn_idx)
    views = views.to(dev).contiguous()
    k, V = knn_idx.shape[2], views.shape[0]
    out = torch.empty_like(points)
    votes = torch.empty(B, N, dtype=torch.int32, device=dev) if return_info else None
    seen = torch.empty(B, N, dtype=torch.int32, device=dev) if return_info else None
    undecided = torch.empty(B, dtype=torch.int32, device=dev) if return_info else None
    if B == 0:
        return (out, {"votes": votes, "seen": seen, "undecided": undecided}) if return_info else out
    lib = L.lib()
    ws = ops.workspace(lib.bdm_orient_normals_workspace_bytes(B, N, V), dev, "orient")
    L.check(lib.bdm_orient_normals(B, N, k, V, int(resolution), int(splat), eps, int(fallback_k), int(fallback_rounds), L.ptr(points),
                                   L.ptr(normals), L.ptr(knn_idx), L.ptr(views), L.ptr(out), L.ptr(votes), L.ptr(seen),
                                   L.ptr(undecided), L.ptr(ws), L.stream()), "orient_normals")
    return (out, {"votes": votes, "seen": seen, "undecided": undecided}) if return_info else out


# ---- command line ------------------------------------------------------------------------------------------------------------------
ORIENT_CHOICES = ("neighbours", "canonical", "visibility")


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.normals", description="write a tree of .ply clouds again with normals")
    ap.add_argument("--in_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--neighborhood-size", type=int, default=50)
    ap.add_argument("--orient", choices=ORIENT_CHOICES, default=None,
                    help="sign rule: pytorch3d's neighbour majority (default), the canonical sign, or visibility voting (outward, "
                         "consistent over the surface)")
    ap.add_argument("--no-disambiguate", action="store_true", help="the same as --orient canonical")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not K_MIN <= args.neighborhood_size <= K_MAX:
        ap.error(f"--neighborhood-size must lie in {K_MIN}..{K_MAX}")
    if args.no_disambiguate and args.orient not in (None, "canonical"):
        ap.error(f"--no-disambiguate means --orient canonical, not --orient {args.orient}")
    if args.orient is None:
        args.orient = "canonical" if args.no_disambiguate else "neighbours"
    return args


def process_tree(in_dir, out_dir, estimate_fn, batch_size=16):
    """Walk in_dir for .ply files, batch those of equal point count (up to batch_size per call, in sorted path order), call
    estimate_fn(points (B, N, 3) float32 host tensor) -> (normals (B, N, 3), curvatures (B, N, 3)) host tensors, and write
    out_dir/<same relative path> with normals.  -> {"files", "points", "mean_surface_variation"}; the surface variation
    l0 / (l0 + l1 + l2) is averaged over the points where it is finite.  An estimate_fn that returns a third value, the number
    of points whose sign stayed undecided, adds "undecided_fraction" (of all points)."""
    from .io import load_pointcloud_ply, save_pointcloud_ply_normals
    in_dir, out_dir = Path(in_dir), Path(out_dir)
    groups = {}   # point count -> [(relative path, points)]
    for path in sorted(in_dir.rglob("*.ply")):
        pts = load_pointcloud_ply(path)
        groups.setdefault(pts.shape[0], []).append((path.relative_to(in_dir), pts))
    files = points = counted = 0
    variation, undecided = 0.0, None
    for _, items in sorted(groups.items()):
        for lo in range(0, len(items), batch_size):
            chunk = items[lo:lo + batch_size]
            normals, curv, *rest = estimate_fn(torch.stack([torch.from_numpy(p) for _, p in chunk]))
            if rest:
                undecided = (undecided or 0) + int(rest[0])
            sv = (curv[..., 0] / curv.sum(-1)).double()
            good = torch.isfinite(sv)
            variation += float(sv[good].sum())
            counted += int(good.sum())
            for (rel, pts), nrm in zip(chunk, normals):
                save_pointcloud_ply_normals(pts, nrm.numpy(), out_dir / rel)
                files += 1
                points += pts.shape[0]
    result = {"files": files, "points": points, "mean_surface_variation": variation / counted if counted else float("nan")}
    if undecided is not None:
        result["undecided_fraction"] = undecided / points if points else 0.0
    return result


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    device = torch.device("cuda", torch.cuda.current_device())

    def estimate_fn(points):
        points = points.to(device)
        if args.orient == "visibility":
            normals, idx, curv = _estimate(points, args.neighborhood_size, ORIENT_CANONICAL, want_idx=True, want_curvatures=True)
            normals, info = orient_normals_by_visibility(points, normals, idx, return_info=True)
            return normals.cpu(), curv.cpu(), int(info["undecided"].sum())
        normals, curv = estimate_pointcloud_normals(points, args.neighborhood_size, args.orient == "neighbours", return_curvatures=True)
        return normals.cpu(), curv.cpu()

    result = process_tree(args.in_dir, args.out_dir, estimate_fn, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
