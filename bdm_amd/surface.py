"""Triangle meshes from oriented point clouds on the HIP path: the cloud is accumulated into a signed-distance grid (implicit moving
least squares with a compact polynomial weight, in fixed point) and the grid is meshed by surface nets, one vertex per sign-change
cell and one quad per sign-change edge (bdm_surface_grid / bdm_surface_extract, csrc/surface.hip; the rule is stated in
include/bdm_hip.h section 12 and DESIGN.md section 16).

    python -m bdm_amd.surface --in_dir <tree of .ply> --out_dir <tree> [--resolution R] [--support 3] [--neighborhood-size 50]
                              [--batch-size 16] [--method imls|poisson] [--cycles C] [--trim-density x]

writes every cloud again under the same relative path as a triangle mesh and prints one JSON line.  Files with nx, ny, nz are
meshed as they are; the others get estimate_pointcloud_normals(..., disambiguate_directions="visibility") first.

The method has no hole filling: where the grid is finer than the sampling, nodes stay undefined and the quads next to them are
left out; `skipped_quads` and `open_edge_fraction` report it.  bdm_amd.mesh_fill.fill_holes closes the small holes afterwards.

method="poisson" (bdm_surface_poisson_grid, csrc/surface_poisson.hip; bdm_hip.h section 22) closes by
construction: the normals are splatted into a vector field, Laplace(phi) = div V is solved on every node of the grid by a fixed
number of multigrid V-cycles, and the level set through the samples goes to the same surface nets.  No quad is skipped and every
edge has an even number of faces; what the field invents across an open boundary has a low density and trim_by_density cuts it."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

from . import _lib as L
from . import ops

# limits of bdm_surface_grid (bdm_hip.h section 12)
N_MAX, R_MIN, R_MAX, S_MIN, S_MAX = 65536, 16, 256, 2, 4
# bdm_surface_poisson_grid (section 22): the resolutions that halve to a side of at most 8, and the V-cycles
POISSON_RESOLUTIONS = (16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256)
DEFAULT_CYCLES, CYCLES_MAX = 12, 32   # 12: where the vertices stop moving against a converged solve
METHODS = ("imls", "poisson")


def default_resolution(n):
    """8 * round(sqrt(n / 4) / 8) clamped to [16, 256]: 16 at 1024 points, 32 at 4096, 64 at 16384."""
    return min(R_MAX, max(R_MIN, 8 * round(math.sqrt(n / 4) / 8)))


def nearest_poisson_resolution(R):
    """The accepted resolution nearest to R (the smaller of two equally near)."""
    return min(POISSON_RESOLUTIONS, key=lambda a: (abs(a - R), a))


def _check_poisson(n, resolution, min_weight, cycles):
    """What method="poisson" adds to the argument checks -> (R, cycles)."""
    if float(min_weight) != 0.0:
        raise ValueError(f"min_weight={min_weight} has no meaning with method='poisson' (every node is defined): leave it at 0")
    R = nearest_poisson_resolution(default_resolution(n)) if resolution is None else int(resolution)
    if R not in POISSON_RESOLUTIONS:
        raise ValueError(f"resolution={R} is not accepted by method='poisson' (it must halve to a side of at most 8); "
                         f"the nearest accepted one is {nearest_poisson_resolution(R)}")
    cycles = DEFAULT_CYCLES if cycles is None else int(cycles)
    if not 1 <= cycles <= CYCLES_MAX:
        raise ValueError(f"cycles={cycles} is outside 1..{CYCLES_MAX}")
    return R, cycles


def _check_args(points, normals, resolution, support, min_weight):
    """The argument checks that need no device -> (R, s, min_weight)."""
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"expected a Pointclouds or a (B, n, 3) tensor, got {tuple(points.shape)}")
    if normals is None or tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f"normals {None if normals is None else tuple(normals.shape)} do not match points {tuple(points.shape)}")
    B, n, _ = points.shape
    if not 1 <= n <= N_MAX:
        raise ValueError(f"{n} points per cloud are outside 1..{N_MAX}")
    R = default_resolution(n) if resolution is None else int(resolution)
    s = int(support)
    if not R_MIN <= R <= R_MAX:
        raise ValueError(f"resolution={R} is outside {R_MIN}..{R_MAX}")
    if not S_MIN <= s <= S_MAX:
        raise ValueError(f"support={s} is outside {S_MIN}..{S_MAX}")
    min_weight = float(min_weight)
    if not 0.0 <= min_weight <= 1.0:
        raise ValueError(f"min_weight={min_weight} is outside 0..1")
    if B * R ** 3 >= 2 ** 31:
        raise ValueError(f"{B} grids of {R}^3 nodes exceed 2^31 nodes: split the batch")
    return R, s, min_weight


@torch.no_grad()
def reconstruct_surface(points, normals=None, *, resolution=None, support=3, min_weight=0.0, return_info=False, return_grid=False,
                        method="imls", cycles=None, return_density=False):
    """(verts_list, faces_list) of a `Pointclouds` or a (B, n, 3) tensor with outward normals (B, n, 3): per cloud verts (V, 3)
    float32 and faces (F, 3) int64 on the input's device (the argument convention of pytorch3d's Meshes).  A Pointclouds carries
    its normals as its features when `normals` is None.
    resolution: grid nodes per axis (None: default_resolution(n)); support: the weight's radius in voxels (2..4); min_weight: a node
    is defined when its summed weight reaches max(1, rint(4096 min_weight)) / 4096.
    method: "imls" (section 12: holes where the grid is finer than the sampling) or "poisson" (section 22: closed).  With "poisson"
    the resolution must be one of POISSON_RESOLUTIONS (None: the one nearest to default_resolution(n)), min_weight must stay 0 and
    cycles (None: DEFAULT_CYCLES) is the number of multigrid V-cycles; return_density=True appends the list of per-vertex densities
    (V,) float32, the summed weight of the samples around the vertex (what trim_by_density takes).
    return_info=True appends {"counts" (B, 4) int32 on the host: V, F, skipped quads, valid points; "resolution"; "support"} and with
    "poisson" also "border_raised" (B,) int32, "iso" (B,) float32, "cycles"; return_grid=True appends (SW, SU), each (B, R, R, R)
    int32, return_grid="all" with "poisson" (SW, SU, phi), phi float32.  Bad arguments raise ValueError before any launch."""
    if method not in METHODS:
        raise ValueError(f"method={method!r} is not one of {METHODS}")
    poisson = method == "poisson"
    if not poisson and (cycles is not None or return_density or return_grid == "all"):
        raise ValueError("cycles, return_density and return_grid='all' belong to method='poisson'")
    if hasattr(points, "points_padded"):
        if normals is None:
            normals = points.features_padded()
        points = points.points_padded()
    if poisson and points.dim() == 3:
        resolution, cycles = _check_poisson(points.shape[1], resolution, min_weight, cycles)
    R, s, min_weight = _check_args(points, normals, resolution, support, min_weight)
    points, normals = L.f32(points), L.f32(normals)
    L.ptr(points), L.ptr(normals)   # refuses host tensors before anything is allocated
    dev = points.device
    B, n, _ = points.shape
    extras = []
    if B == 0:
        if return_density:
            extras.append([])
        if return_info:
            info = {"counts": torch.zeros(0, 4, dtype=torch.int32), "resolution": R, "support": s}
            if poisson:
                info.update(border_raised=torch.zeros(0, dtype=torch.int32), iso=torch.zeros(0), cycles=cycles)
            extras.append(info)
        if return_grid:
            grids = (torch.zeros(0, R, R, R, dtype=torch.int32, device=dev),) * 2
            extras.append(grids + (torch.zeros(0, R, R, R, device=dev),) if return_grid == "all" else grids)
        return ([], [], *extras)
    lib = L.lib()
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    if poisson:
        ws = ops.workspace(lib.bdm_surface_poisson_workspace_bytes(B, n, R, s), dev, "surface")
        pinfo = torch.empty(B, 3, dtype=torch.int32, device=dev)
        L.check(lib.bdm_surface_poisson_grid(B, n, R, s, cycles, L.ptr(points), L.ptr(normals), L.ptr(counts), L.ptr(pinfo), L.ptr(ws),
                                             L.stream()), "surface_poisson_grid")
    else:
        ws = ops.workspace(lib.bdm_surface_workspace_bytes(B, n, R, s), dev, "surface")
        L.check(lib.bdm_surface_grid(B, n, R, s, min_weight, L.ptr(points), L.ptr(normals), L.ptr(counts), L.ptr(ws), L.stream()), "surface_grid")
    host = counts.cpu()   # the one synchronisation: the sizes of the outputs
    nv, nf = host[:, 0].long(), host[:, 1].long()
    offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).to(dev)
    verts = torch.empty(int(nv.sum()), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(int(nf.sum()), 3, dtype=torch.int32, device=dev)
    if verts.numel():
        face_buf = faces if faces.numel() else faces.new_empty(1, 3)   # vertices without faces (every quad skipped): no NULL
        L.check(lib.bdm_surface_extract(B, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(face_buf), L.ptr(ws), L.stream()),
                "surface_extract")
    verts_list = list(torch.split(verts, nv.tolist()))
    faces_list = [f.long() for f in torch.split(faces, nf.tolist())]
    if return_density:
        density = torch.empty(int(nv.sum()), dtype=torch.float32, device=dev)
        if density.numel():
            L.check(lib.bdm_surface_poisson_density(B, R, L.ptr(offsets[0]), L.ptr(density), L.ptr(ws), L.stream()), "surface_poisson_density")
        extras.append(list(torch.split(density, nv.tolist())))
    if return_info:
        info = {"counts": host, "resolution": R, "support": s}
        if poisson:
            pi = pinfo.cpu()
            info.update(border_raised=pi[:, 0].clone(), iso=pi[:, 1].clone().view(torch.float32), cycles=cycles)
        extras.append(info)
    if return_grid:
        r3 = B * R ** 3 * 4
        grids = ws[:2 * r3].view(torch.int32).view(2, B, R, R, R)
        out = (grids[0].clone(), grids[1].clone())
        if return_grid == "all":   # section 22: behind the section-12 layout W, Vx, Vy, Vz, D, phi
            at = lib.bdm_surface_workspace_bytes(B, n, R, s) + 5 * r3
            out += (ws[at:at + r3].view(torch.float32).view(B, R, R, R).clone(),)
        extras.append(out)
    return (verts_list, faces_list, *extras)


def trim_by_density(verts, faces, densities, min_density):
    """One mesh without the vertices of density below min_density and the faces that use one (torch ops; any device): what the Poisson
    field invents across an open boundary lies far from every sample and has a low density.  -> (verts, faces, densities) of the kept
    vertices and faces in their old order, the faces renumbered."""
    verts, faces, densities = torch.as_tensor(verts), torch.as_tensor(faces).long(), torch.as_tensor(densities)
    if densities.shape != verts.shape[:1]:
        raise ValueError(f"densities {tuple(densities.shape)} do not match {verts.shape[0]} vertices")
    keep = densities >= min_density
    new_id = torch.cumsum(keep.long(), 0) - 1
    kept_faces = faces[keep[faces].all(dim=1)] if faces.numel() else faces
    return verts[keep], new_id[kept_faces], densities[keep]


def mesh_stats(verts, faces):
    """Bookkeeping of one triangle mesh (torch ops; any device): vertices, faces, edges (undirected), open_edges (edges not shared by
    exactly two faces), inconsistent_edges (directed edges used more than once: two faces wound against each other),
    euler_characteristic V - E + F, signed_volume (positive when the triangle normals point outwards), area."""
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces).long()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F == 0:
        return {"vertices": V, "faces": 0, "edges": 0, "open_edges": 0, "inconsistent_edges": 0, "euler_characteristic": V,
                "signed_volume": 0.0, "area": 0.0}
    a, b = faces.flatten(), faces.roll(-1, dims=1).flatten()
    span = max(V, int(faces.max()) + 1)
    _, shared = torch.unique(torch.minimum(a, b) * span + torch.maximum(a, b), return_counts=True)
    _, directed = torch.unique(a * span + b, return_counts=True)
    tri = verts.double()[faces]
    cross = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    edges = int(shared.numel())
    return {"vertices": V, "faces": F, "edges": edges, "open_edges": int((shared != 2).sum()), "inconsistent_edges": int((directed > 1).sum()),
            "euler_characteristic": V - edges + F, "signed_volume": float((tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum() / 6.0),
            "area": float(cross.norm(dim=1).sum() / 2.0)}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.surface", description="write a tree of .ply clouds again as triangle meshes")
    ap.add_argument("--in_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--resolution", type=int, default=None, help="grid nodes per axis (default: from the number of points)")
    ap.add_argument("--support", type=int, default=3)
    ap.add_argument("--neighborhood-size", type=int, default=50, help="for the normals of files that carry none")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--method", choices=METHODS, default="imls", help="poisson: closed meshes (multigrid Poisson solve on the grid)")
    ap.add_argument("--cycles", type=int, default=None, help=f"V-cycles of --method poisson (default {DEFAULT_CYCLES})")
    ap.add_argument("--trim-density", type=float, default=None, help="with --method poisson: drop vertices of a lower density")
    args = ap.parse_args(argv)
    if args.method != "poisson" and (args.cycles is not None or args.trim_density is not None):
        ap.error("--cycles and --trim-density need --method poisson")
    if args.cycles is not None and not 1 <= args.cycles <= CYCLES_MAX:
        ap.error(f"--cycles must lie in 1..{CYCLES_MAX}")
    if args.method == "poisson" and args.resolution is not None and args.resolution not in POISSON_RESOLUTIONS:
        ap.error(f"--resolution {args.resolution} is not accepted by --method poisson; the nearest accepted one is "
                 f"{nearest_poisson_resolution(args.resolution)}")
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if args.resolution is not None and not R_MIN <= args.resolution <= R_MAX:
        ap.error(f"--resolution must lie in {R_MIN}..{R_MAX}")
    if not S_MIN <= args.support <= S_MAX:
        ap.error(f"--support must lie in {S_MIN}..{S_MAX}")
    return args


def process_tree(in_dir, out_dir, mesh_fn, batch_size=16):
    """Walk in_dir for .ply files, batch those of equal point count that agree on carrying normals (up to batch_size per call, in
    sorted path order), call mesh_fn(points (B, n, 3), normals (B, n, 3) or None; float32 host tensors) -> (verts_list, faces_list,
    counts (B, 4)[, border_raised (B,)]) and write out_dir/<same relative path> as a mesh.  -> {"files", "vertices", "faces",
    "skipped_quads", "open_edge_fraction"} (open edges over all edges of all meshes; "vertices" and "faces" count what is written)
    and "border_raised" when mesh_fn returns it."""
    from .io import load_pointcloud_ply, save_mesh_ply
    in_dir, out_dir = Path(in_dir), Path(out_dir)
    groups = {}   # (point count, has normals) -> [(relative path, points, normals or None)]
    for path in sorted(in_dir.rglob("*.ply")):
        try:
            pts, nrm = load_pointcloud_ply(path, with_normals=True)
        except ValueError:
            pts, nrm = load_pointcloud_ply(path), None
        groups.setdefault((pts.shape[0], nrm is not None), []).append((path.relative_to(in_dir), pts, nrm))
    result = {"files": 0, "vertices": 0, "faces": 0, "skipped_quads": 0}
    edges = open_edges = 0
    for (_, has_normals), items in sorted(groups.items()):
        for lo in range(0, len(items), batch_size):
            chunk = items[lo:lo + batch_size]
            points = torch.stack([torch.from_numpy(p) for _, p, _ in chunk])
            normals = torch.stack([torch.from_numpy(nr) for _, _, nr in chunk]) if has_normals else None
            verts_list, faces_list, counts, *raised = mesh_fn(points, normals)
            if raised:
                result["border_raised"] = result.get("border_raised", 0) + int(raised[0].sum())
            for (rel, _, _), verts, faces, row in zip(chunk, verts_list, faces_list, counts.tolist()):
                save_mesh_ply(verts.cpu().numpy(), faces.cpu().numpy(), out_dir / rel)
                stats = mesh_stats(verts.cpu(), faces.cpu())
                edges, open_edges = edges + stats["edges"], open_edges + stats["open_edges"]
                result["files"] += 1
                result["vertices"] += int(verts.shape[0])
                result["faces"] += int(faces.shape[0])
                result["skipped_quads"] += row[2]
    result["open_edge_fraction"] = open_edges / edges if edges else 0.0
    return result


def main(argv=None, device=None):
    from .normals import estimate_pointcloud_normals
    args = parse_args(sys.argv[1:] if argv is None else argv)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def mesh_fn(points, normals):
        points = points.to(device)
        normals = estimate_pointcloud_normals(points, args.neighborhood_size, "visibility") if normals is None else normals.to(device)
        if args.method == "imls":
            verts_list, faces_list, info = reconstruct_surface(points, normals, resolution=args.resolution, support=args.support, return_info=True)
            return verts_list, faces_list, info["counts"]
        verts_list, faces_list, density, info = reconstruct_surface(points, normals, resolution=args.resolution, support=args.support,
                                                                    method="poisson", cycles=args.cycles, return_density=True, return_info=True)
        if args.trim_density is not None:
            trimmed = [trim_by_density(v, f, d, args.trim_density)[:2] for v, f, d in zip(verts_list, faces_list, density)]
            verts_list, faces_list = [m[0] for m in trimmed], [m[1] for m in trimmed]
        return verts_list, faces_list, info["counts"], info["border_raised"]

    result = process_tree(args.in_dir, args.out_dir, mesh_fn, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
