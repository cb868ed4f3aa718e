"""Colouring the reconstructed meshes: every vertex of a mesh takes the colour of the coloured cloud around it, through the two-set
K-nearest-neighbour search and the interpolation kernel of bdm_amd.knn (bdm_hip.h section 15).

    python -m bdm_amd.mesh_color --mesh_dir D/pred_mesh --color_dir D/colored --out_dir D/colored_mesh [--k 3] [--mode idw]
                                 [--batch-size 16]

walks the mesh .ply files of mesh_dir that have a coloured cloud at the same relative path of color_dir, writes every mesh again
under out_dir with uchar red, green, blue per vertex, and prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

import torch

from . import _lib as L
from .knn import K_MAX, MODES, transfer_point_attributes

GREY = 0.5   # the colour of a vertex without a neighbour (an empty or all-non-finite cloud, a non-finite vertex)


def compose_result(files, vertices, unmatched, nearest_sum):
    """The dictionary process_tree returns, from its four sums (nearest_sum: the float64 sum of the nearest distances of the matched
    vertices)."""
    matched = vertices - unmatched
    return {"files": files, "vertices": vertices, "unmatched": unmatched,
            "mean_nearest_distance": nearest_sum / matched if matched else float("nan")}


def process_tree(mesh_dir, color_dir, out_dir, color_fn, batch_size=16):
    """Walk mesh_dir for mesh .ply files that have a coloured cloud .ply at the same relative path under color_dir, in sorted path
    order, up to batch_size files per call of color_fn(verts_list, points_list, colors_list; float32 host tensors of ragged sizes)
    -> (colours per mesh [(V_i, 3)], nearest squared distance per vertex [(V_i,)], has a neighbour [(V_i,) bool]; host tensors), and write
    out_dir/<same relative path> as a mesh with vertex colours; a vertex without a neighbour is mid-grey.
    -> {"files", "vertices", "unmatched" (vertices without a neighbour), "mean_nearest_distance" (from a matched vertex to the
    nearest point of its cloud, the mean of the square roots in float64)}."""
    from .io import load_mesh_ply, load_pointcloud_ply, save_mesh_ply
    mesh_dir, color_dir, out_dir = Path(mesh_dir), Path(color_dir), Path(out_dir)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    items = [(path.relative_to(mesh_dir), path) for path in sorted(mesh_dir.rglob("*.ply"))
             if (color_dir / path.relative_to(mesh_dir)).exists()]
    files = vertices = unmatched = 0
    nearest_sum = 0.0
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        meshes = [load_mesh_ply(path) for _, path in chunk]
        clouds = [load_pointcloud_ply(color_dir / rel, with_colors=True) for rel, _ in chunk]
        colours, nearest, matched = color_fn([torch.from_numpy(v) for v, _ in meshes], [torch.from_numpy(p) for p, _ in clouds],
                                    [torch.from_numpy(c) for _, c in clouds])
        for (rel, _), (verts, faces), col, d2, has in zip(chunk, meshes, colours, nearest, matched):
            lost = ~has
            col = torch.where(lost[:, None], torch.full((), GREY), col)
            save_mesh_ply(verts, faces, out_dir / rel, colors=col.numpy())
            files += 1
            vertices += verts.shape[0]
            unmatched += int(lost.sum())
            nearest_sum += float(d2[~lost].double().sqrt().sum())
    return compose_result(files, vertices, unmatched, nearest_sum)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_color",
                                 description="write a tree of triangle meshes again with vertex colours taken from coloured clouds")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--color_dir", required=True, help="directory tree of coloured .ply clouds with the same relative paths")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--mode", choices=sorted(MODES), default="idw")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not 1 <= args.k <= K_MAX:
        ap.error(f"--k must lie in 1..{K_MAX}")
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_color needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())

    def color_fn(verts_list, points_list, colors_list):
        outs, knn = transfer_point_attributes([v.to(device) for v in verts_list], [p.to(device) for p in points_list],
                                              [c.to(device) for c in colors_list], K=args.k, mode=args.mode, fill=GREY, return_knn=True)
        return [o.cpu() for o in outs], [d2[:, 0].cpu() for _, d2 in knn], [(idx[:, 0] >= 0).cpu() for idx, _ in knn]

    result = process_tree(args.mesh_dir, args.color_dir, args.out_dir, color_fn, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
