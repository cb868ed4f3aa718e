"""Decimation of the reconstructed meshes on the HIP path: vertex clustering, Open3D's simplify_vertex_clustering by name and meaning,
over bdm_mesh_cluster / bdm_mesh_decimate (csrc/mesh_decimate.hip; the rule is stated in include/bdm_hip.h section 20 and DESIGN.md
section 24).

    python -m bdm_amd.mesh_decimate --mesh_dir D/pred_mesh --out_dir D/pred_mesh_small (--resolution R | --voxel-size x)
                                    [--contraction average|first] [--batch-size 16]

walks the mesh .ply files of mesh_dir in sorted order, decimates every mesh, writes it under out_dir at the same relative path
(vertex colours are carried along) and prints one JSON line.

The vertices of a mesh that fall into one cell of a regular grid become one vertex; faces that lose a corner that way are dropped,
and of several faces over the same three new vertices the first stays.  The grid of cell size h is anchored at lo, the per-axis
minimum of the mesh's finite vertices: not at the origin, and not half a cell below lo as Open3D's is, so the cells differ from
Open3D's by that half cell.  Clustering can leave non-manifold edges and change the genus; surface.mesh_stats reports that and
nothing here repairs it.  Edge-collapse decimation is not offered."""
import argparse
import json
import sys
from pathlib import Path

import torch

from . import _lib as L
from . import ops
from .mesh_fill import _check_colors, _round_uint8
from .ragged import first, mesh_lists, pack_meshes

MAX_B, MAX_V, MAX_R, MAX_C = 65535, 2 ** 21, 1024, 16   # limits of bdm_hip.h section 20
CONTRACTIONS = {"average": 0, "first": 1}
COLLAPSED, DUPLICATE, BAD = -1, -2, -3   # face_map of a dropped face
INFO_KEYS = ("new_vertices", "new_faces", "collapsed_faces", "duplicate_faces", "bad_faces", "nonfinite_vertices", "largest_cluster",
             "merged_vertices")


def _check_grid(voxel_size, resolution, B):
    """Exactly one of the two -> (resolution or 0, the per-mesh float32 cell sizes on the host or None)."""
    if (voxel_size is None) == (resolution is None):
        raise ValueError("give exactly one of voxel_size and resolution")
    if resolution is not None:
        if isinstance(resolution, bool) or not isinstance(resolution, int) or not 1 <= resolution <= MAX_R:
            raise ValueError(f"resolution={resolution!r} is not an integer in 1..{MAX_R}")
        return resolution, None
    if isinstance(voxel_size, (list, tuple)) or torch.is_tensor(voxel_size):
        sizes = [float(x) for x in (voxel_size.tolist() if torch.is_tensor(voxel_size) else voxel_size)]
        if len(sizes) != B:
            raise ValueError(f"{len(sizes)} voxel sizes for {B} meshes")
    elif isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float)):
        raise ValueError(f"voxel_size={voxel_size!r} is neither a number nor one number per mesh")
    else:
        sizes = [float(voxel_size)] * B
    h = torch.tensor(sizes, dtype=torch.float64).float()
    if not bool((torch.isfinite(h) & (h > 0)).all()):
        raise ValueError("every voxel_size must be positive and finite as a float32")
    return 0, h


def _check_contraction(contraction):
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction={contraction!r} is none of {list(CONTRACTIONS)}")


def _check_sizes(verts_list, faces_list):
    """The limits of bdm_hip.h section 20 on a batch, before anything is packed."""
    if len(verts_list) > MAX_B:
        raise ValueError(f"{len(verts_list)} meshes exceed {MAX_B}: split the batch")
    if any(int(v.shape[0]) >= MAX_V for v in verts_list):
        raise ValueError(f"a mesh reaches {MAX_V} vertices")
    sum_v, sum_f = sum(int(v.shape[0]) for v in verts_list), sum(int(f.shape[0]) for f in faces_list)
    if sum_v >= 2 ** 31 - 1 or 3 * sum_f >= 2 ** 31 - 1:
        raise ValueError("the batch reaches 2^31 vertices or face corners: split it")


def _cluster(verts, faces, vert_first, face_first, resolution, sizes, contraction):
    """One bdm_mesh_cluster call -> (vert_map (sum V), face_map (sum F), mesh_counts (B, 8), workspace): int32 device tensors as the ABI
    writes them; the workspace holds the plan for bdm_mesh_decimate."""
    B, sum_v, sum_f, dev = vert_first.numel() - 1, int(vert_first[-1]), int(face_first[-1]), verts.device
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_decimate_workspace_bytes(B, sum_v, sum_f), dev, "mesh_decimate")
    vert_map = torch.zeros(max(sum_v, 1), dtype=torch.int32, device=dev)
    face_map = torch.zeros(max(sum_f, 1), dtype=torch.int32, device=dev)
    counts = torch.zeros(B, len(INFO_KEYS), dtype=torch.int32, device=dev)
    L.check(lib.bdm_mesh_cluster(B, resolution, None if sizes is None else sizes.data_ptr(), CONTRACTIONS[contraction], L.ptr(verts), L.ptr(faces),
                                 vert_first.data_ptr(), face_first.data_ptr(), L.ptr(vert_map), L.ptr(face_map), L.ptr(counts), L.ptr(ws),
                                 L.stream()), "mesh_cluster")
    return vert_map[:sum_v], face_map[:sum_f], counts, ws


@torch.no_grad()
def cluster_vertices(meshes, voxel_size=None, resolution=None):
    """-> (vert_map_list, face_map_list, info).  vert_map (V,) int64: the new index of every vertex's cluster, clusters numbered by
    their smallest member.  face_map (F,) int64: the new index of a kept face, -1 for a face that collapsed, -2 for a duplicate of an
    earlier face (same three new vertices, orientation ignored), -3 for a face with an index out of range or repeated.  info: per
    mesh the INFO_KEYS.  The grid is anchored at the per-axis minimum of the mesh's finite vertices (see the module text)."""
    verts_list, faces_list = mesh_lists(meshes)
    resolution, sizes = _check_grid(voxel_size, resolution, len(verts_list))
    if not verts_list:
        return [], [], []
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    vert_map, face_map, counts, _ = _cluster(verts, faces, vert_first, face_first, resolution, sizes, "average")
    nv, nf = [int(v.shape[0]) for v in verts_list], [int(f.shape[0]) for f in faces_list]
    info = [dict(zip(INFO_KEYS, row)) for row in counts.cpu().tolist()]
    return [x.long() for x in vert_map.split(nv)], [x.long() for x in face_map.split(nf)], info


@torch.no_grad()
def simplify_vertex_clustering(meshes, voxel_size=None, resolution=None, contraction="average", colors_list=None, return_info=False):
    """Thin every mesh by vertex clustering -> (verts_list, faces_list[, colors_list][, info]).  Exactly one of voxel_size (a float, or
    one per mesh) and resolution (an integer R in 1..1024: the cell is the mesh's largest extent over R) is given.  The vertices of one
    cell become one vertex: their mean (contraction="average"; an order-free fixed-point mean, bit-reproducible) or the one of the
    lowest index ("first"); a vertex alone in its cell keeps its bits, and so does a non-finite vertex, which is never merged.  The
    new vertices are ordered by the lowest old index of their cell.  Faces with an index out of range or repeated, faces that lose a
    corner, and later faces over the same three new vertices are dropped; the others keep their order and winding.  colors_list
    ((V_i, C) per mesh, uint8 or floating point, C <= 16 the same everywhere) is carried along the same way: averaged (correctly
    rounded and clamped for uint8; a floating-point channel with a non-finite member gives NaN) or taken from the first.  The grid is
    anchored at the per-axis minimum of the mesh's finite vertices, not at the origin and not half a cell below the minimum as
    Open3D's is.  info: per mesh the INFO_KEYS.  Bad arguments raise ValueError before any launch; host tensors are refused."""
    _check_contraction(contraction)
    verts_list, faces_list = mesh_lists(meshes)
    resolution, sizes = _check_grid(voxel_size, resolution, len(verts_list))
    C = 0 if colors_list is None else _check_colors(colors_list, verts_list)
    if not verts_list:
        return ([], []) + (([],) if colors_list is not None else ()) + (([],) if return_info else ())
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, dev = len(verts_list), verts.device
    if C:
        for c in colors_list:
            L.ptr(c)
        attrs = L.f32(torch.cat([c.float() for c in colors_list] + [torch.zeros(1, C, device=dev)]))   # one unread row: never empty
    else:
        attrs = torch.zeros(1, 1, dtype=torch.float32, device=dev)
    _, _, counts, ws = _cluster(verts, faces, vert_first, face_first, resolution, sizes, contraction)
    counts = counts.cpu()   # the one read-back: it sizes the outputs
    new_v, new_f = counts[:, 0].tolist(), counts[:, 1].tolist()
    out_vert_first, out_face_first = first(new_v), first(new_f)
    verts_out = torch.zeros(max(int(out_vert_first[-1]), 1), 3, dtype=torch.float32, device=dev)
    attrs_out = torch.zeros(max(int(out_vert_first[-1]), 1), max(C, 1), dtype=torch.float32, device=dev)
    faces_out = torch.zeros(max(int(out_face_first[-1]), 1), 3, dtype=torch.int32, device=dev)
    lib = L.lib()
    L.check(lib.bdm_mesh_decimate(B, resolution, None if sizes is None else sizes.data_ptr(), CONTRACTIONS[contraction], C, L.ptr(verts),
                                  L.ptr(attrs), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), out_vert_first.data_ptr(),
                                  out_face_first.data_ptr(), L.ptr(verts_out), L.ptr(attrs_out), L.ptr(faces_out), L.ptr(ws), L.stream()),
            "mesh_decimate")
    out_v, out_f, out_c = [], [], []
    for m in range(B):
        v0, f0 = int(out_vert_first[m]), int(out_face_first[m])
        out_v.append(verts_out[v0:v0 + new_v[m]])
        out_f.append(faces_out[f0:f0 + new_f[m]].to(faces_list[m].dtype))
        if C:
            rows = attrs_out[v0:v0 + new_v[m]]
            out_c.append(_round_uint8(rows) if colors_list[m].dtype == torch.uint8 else rows.to(colors_list[m].dtype))
        elif colors_list is not None:
            out_c.append(colors_list[m].new_zeros(new_v[m], 0))
    info = [dict(zip(INFO_KEYS, row)) for row in counts.tolist()]
    return (out_v, out_f) + ((out_c,) if colors_list is not None else ()) + ((info,) if return_info else ())


# ---- command line ------------------------------------------------------------------------------------------------------------------
def decimate_batch(verts_list, faces_list, colors_list, device, voxel_size=None, resolution=None, contraction="average"):
    """Host tensors of ragged sizes (a colour entry None for a file that carries none) -> (verts_list, faces_list, colors_list, info) on
    the host, through simplify_vertex_clustering.  Files without colours ride along with zero rows of the batch's colour width."""
    verts, faces = [v.to(device) for v in verts_list], [f.to(device) for f in faces_list]
    have = [c for c in colors_list if c is not None]
    if have:
        like = have[0]
        cols = [like.new_zeros(v.shape[0], like.shape[1]).to(device) if c is None else c.to(device) for c, v in zip(colors_list, verts)]
        verts, faces, cols, info = simplify_vertex_clustering((verts, faces), voxel_size, resolution, contraction, colors_list=cols, return_info=True)
    else:
        verts, faces, info = simplify_vertex_clustering((verts, faces), voxel_size, resolution, contraction, return_info=True)
        cols = [None] * len(verts)
    return ([v.cpu() for v in verts], [f.cpu() for f in faces], [None if c0 is None else c.cpu() for c, c0 in zip(cols, colors_list)], info)


def compose_result(files, info_sums, vertices_in, faces_in, vertices_out, faces_out, edges_in, open_in, edges_out, open_out):
    """The dictionary process_tree returns: the file count, the summed info, the sizes and the open edges over all edges of all meshes
    before and after."""
    out = {"files": files}
    out.update(info_sums)
    out.update(vertices_in=vertices_in, faces_in=faces_in, vertices_out=vertices_out, faces_out=faces_out)
    out["open_edge_fraction_in"] = open_in / edges_in if edges_in else 0.0
    out["open_edge_fraction_out"] = open_out / edges_out if edges_out else 0.0
    return out


def _stats(v, f):
    """mesh_stats of the faces whose indices are all in range (it looks every index up)."""
    from .surface import mesh_stats
    f = f.long()
    ok = ((f >= 0) & (f < v.shape[0])).all(dim=1) if f.numel() else torch.zeros(0, dtype=torch.bool)
    return mesh_stats(v, f[ok])


def process_tree(mesh_dir, out_dir, decimate_fn, batch_size=16):
    """Walk mesh_dir for mesh .ply files in sorted path order, up to batch_size files per call of decimate_fn(verts_list, faces_list,
    colors_list) -> (verts_list, faces_list, colors_list, info; host tensors), and write out_dir/<same relative path>."""
    from .io import load_mesh_ply, save_mesh_ply
    mesh_dir, out_dir = Path(mesh_dir), Path(out_dir)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    items = [(path.relative_to(mesh_dir), path) for path in sorted(mesh_dir.rglob("*.ply"))]
    sums, sizes, edges = {k: 0 for k in INFO_KEYS}, [0, 0, 0, 0], [0, 0, 0, 0]
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        loaded = [load_mesh_ply(path, with_colors=True) for _, path in chunk]
        verts, faces, colors, info = decimate_fn([torch.from_numpy(v) for v, _, _ in loaded], [torch.from_numpy(f) for _, f, _ in loaded],
                                                 [None if c is None else torch.from_numpy(c) for _, _, c in loaded])
        for (rel, _), (v_in, f_in, _), v, f, c, i in zip(chunk, loaded, verts, faces, colors, info):
            save_mesh_ply(v.numpy(), f.numpy(), out_dir / rel, colors=None if c is None else c.numpy())
            before, after = _stats(torch.from_numpy(v_in), torch.from_numpy(f_in)), _stats(v, f)
            for k, add in enumerate((before["edges"], before["open_edges"], after["edges"], after["open_edges"])):
                edges[k] += add
            for k, add in enumerate((v_in.shape[0], f_in.shape[0], v.shape[0], f.shape[0])):
                sizes[k] += int(add)
            for k in INFO_KEYS:
                sums[k] = max(sums[k], int(i[k])) if k == "largest_cluster" else sums[k] + int(i[k])
    return compose_result(len(items), sums, *sizes, *edges)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_decimate",
                                 description="write a tree of triangle meshes again, thinned by vertex clustering")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--out_dir", required=True)
    grid = ap.add_mutually_exclusive_group(required=True)
    grid.add_argument("--resolution", type=int, help=f"cells along the mesh's largest extent, 1..{MAX_R}")
    grid.add_argument("--voxel-size", type=float, help="the cell size")
    ap.add_argument("--contraction", choices=sorted(CONTRACTIONS), default="average")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    try:
        _check_grid(args.voxel_size, args.resolution, 1)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_decimate needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    result = process_tree(args.mesh_dir, args.out_dir,
                          lambda v, f, c: decimate_batch(v, f, c, device, args.voxel_size, args.resolution, args.contraction), args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
