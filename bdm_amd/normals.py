"""Point-cloud normals on the HIP path: pytorch3d's `estimate_pointcloud_normals` (ops/points_normals.py) with its name,
argument order and defaults, and the self K-nearest-neighbour search underneath it, over bdm_estimate_normals
(csrc/normals.hip; the rule is stated in include/bdm_hip.h section 10 and DESIGN.md section 14).  pytorch3d is not installed, so
the function is restated from its published behaviour ("parity unpinned", as for the renderer).

    python -m bdm_amd.normals --in_dir <tree of .ply> --out_dir <tree> [--neighborhood-size 50] [--no-disambiguate] [--batch-size 16]

writes every cloud again under the same relative path with nx, ny, nz per vertex and prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

import torch

from . import _lib as L
from . import ops

K_MIN, K_MAX = 3, 64
ORIENT_CANONICAL, ORIENT_NEIGHBOURS, ORIENT_VIEWPOINT = 0, 1, 2


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
    component of largest magnitude is positive.  viewpoint (B, 3) or (3,): the normals point towards it instead.
    use_symeig_workaround is accepted for signature parity and ignored (there is one eigen-solver).
    return_curvatures=True: (normals, curvatures (B, N, 3)), the eigenvalues ascending.  Rows of non-finite points are NaN."""
    points = _points_of(pointclouds)
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


# ---- command line ------------------------------------------------------------------------------------------------------------------
def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.normals", description="write a tree of .ply clouds again with normals")
    ap.add_argument("--in_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--neighborhood-size", type=int, default=50)
    ap.add_argument("--no-disambiguate", action="store_true", help="canonical sign instead of pytorch3d's neighbour-majority rule")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not K_MIN <= args.neighborhood_size <= K_MAX:
        ap.error(f"--neighborhood-size must lie in {K_MIN}..{K_MAX}")
    return args


def process_tree(in_dir, out_dir, estimate_fn, batch_size=16):
    """Walk in_dir for .ply files, batch those of equal point count (up to batch_size per call, in sorted path order), call
    estimate_fn(points (B, N, 3) float32 host tensor) -> (normals (B, N, 3), curvatures (B, N, 3)) host tensors, and write
    out_dir/<same relative path> with normals.  -> {"files", "points", "mean_surface_variation"}; the surface variation
    l0 / (l0 + l1 + l2) is averaged over the points where it is finite."""
    from .io import load_pointcloud_ply, save_pointcloud_ply_normals
    in_dir, out_dir = Path(in_dir), Path(out_dir)
    groups = {}   # point count -> [(relative path, points)]
    for path in sorted(in_dir.rglob("*.ply")):
        pts = load_pointcloud_ply(path)
        groups.setdefault(pts.shape[0], []).append((path.relative_to(in_dir), pts))
    files = points = counted = 0
    variation = 0.0
    for _, items in sorted(groups.items()):
        for lo in range(0, len(items), batch_size):
            chunk = items[lo:lo + batch_size]
            normals, curv = estimate_fn(torch.stack([torch.from_numpy(p) for _, p in chunk]))
            sv = (curv[..., 0] / curv.sum(-1)).double()
            good = torch.isfinite(sv)
            variation += float(sv[good].sum())
            counted += int(good.sum())
            for (rel, pts), nrm in zip(chunk, normals):
                save_pointcloud_ply_normals(pts, nrm.numpy(), out_dir / rel)
                files += 1
                points += pts.shape[0]
    return {"files": files, "points": points, "mean_surface_variation": variation / counted if counted else float("nan")}


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    device = torch.device("cuda", torch.cuda.current_device())

    def estimate_fn(points):
        normals, curv = estimate_pointcloud_normals(points.to(device), args.neighborhood_size, not args.no_disambiguate,
                                                    return_curvatures=True)
        return normals.cpu(), curv.cpu()

    result = process_tree(args.in_dir, args.out_dir, estimate_fn, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
