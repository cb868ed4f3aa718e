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
nothing here repairs it.

    python -m bdm_amd.mesh_decimate --mesh_dir D/pred_mesh --out_dir D/pred_mesh_small --method quadric
                                    (--target-faces N | --target-fraction f) [--max-error x] [--boundary-weight w]

thins by quadric edge collapses instead (simplify_quadric_decimation, Open3D's simplify_quadric_decimation by name and meaning, over
bdm_mesh_qem_init / _rounds / _finish, csrc/mesh_qem.hip; bdm_hip.h section 23): a closed manifold mesh stays
closed and manifold, and the faces go where the curvature is.  Its JSON line carries the method, the sizes, the open-edge fractions,
the rounds (the maximum over the files) and the collapses."""
import argparse
import json
import sys

import torch

from . import _lib as L
from . import ops
from .mesh_batch import MAX_C, _check_colors, _round_uint8   # noqa: F401  (their names here are part of the module)
from .mesh_batch import alloc_outputs, mesh_tuple, run_on_host_batch, split_outputs, stage_attrs, walk_tree
from .ragged import first, mesh_lists, pack_meshes

MAX_B, MAX_V, MAX_R = 65535, 2 ** 21, 1024   # limits of bdm_hip.h section 20 (with mesh_batch.MAX_C)
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
        return mesh_tuple([], [], [], colors_list) + (([],) if return_info else ())
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, dev = len(verts_list), verts.device
    attrs = stage_attrs(colors_list, C, dev)
    _, _, counts, ws = _cluster(verts, faces, vert_first, face_first, resolution, sizes, contraction)
    counts = counts.cpu()   # the one read-back: it sizes the outputs
    new_v, new_f = counts[:, 0].tolist(), counts[:, 1].tolist()
    out_vert_first, out_face_first = first(new_v), first(new_f)
    verts_out, attrs_out, faces_out = alloc_outputs(out_vert_first, out_face_first, C, dev)
    lib = L.lib()
    L.check(lib.bdm_mesh_decimate(B, resolution, None if sizes is None else sizes.data_ptr(), CONTRACTIONS[contraction], C, L.ptr(verts),
                                  L.ptr(attrs), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), out_vert_first.data_ptr(),
                                  out_face_first.data_ptr(), L.ptr(verts_out), L.ptr(attrs_out), L.ptr(faces_out), L.ptr(ws), L.stream()),
            "mesh_decimate")
    out = split_outputs(verts_out, attrs_out, faces_out, out_vert_first, out_face_first, faces_list, colors_list, C)
    return out + (([dict(zip(INFO_KEYS, row)) for row in counts.tolist()],) if return_info else ())


# ---- quadric edge collapse (bdm_hip.h section 23) -------------------------------------------------------------------------------------
QEM_INFO_KEYS = ("stop", "rounds", "collapses", "faces_in", "faces_out", "vertices_in", "vertices_out", "locked_vertices", "bad_faces",
                 "max_cost_bits", "selected", "candidates", "rejected_nonmanifold", "rejected_locked", "rejected_cost", "rejected_link",
                 "rejected_boundary", "rejected_valence", "rejected_flip", "target")
QEM_STOPS = ("running", "target", "no_edge", "max_rounds")
QEM_MAX_ROUNDS = 2 ** 20
QEM_ROUNDS_PER_CALL = 8   # rounds between two reads of the number of meshes still running


def _per_mesh(value, B, name):
    if isinstance(value, (list, tuple)) or torch.is_tensor(value):
        out = list(value.tolist() if torch.is_tensor(value) else value)
        if len(out) != B:
            raise ValueError(f"{len(out)} values of {name} for {B} meshes")
        return out
    return [value] * B


def _check_targets(target_number_of_triangles, target_fraction, faces_list):
    """Exactly one of the two, a number or one per mesh -> the per-mesh face targets (Python ints)."""
    if (target_number_of_triangles is None) == (target_fraction is None):
        raise ValueError("give exactly one of target_number_of_triangles and target_fraction")
    B = len(faces_list)
    if target_fraction is not None:
        out = []
        for f, faces in zip(_per_mesh(target_fraction, B, "target_fraction"), faces_list):
            if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 < float(f) <= 1.0:
                raise ValueError(f"target_fraction={f!r} is not a number in (0, 1]")
            out.append(int(float(f) * int(faces.shape[0])))
        return out
    out = _per_mesh(target_number_of_triangles, B, "target_number_of_triangles")
    for n in out:
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n < 2 ** 31 - 1:
            raise ValueError(f"target_number_of_triangles={n!r} is not an integer in 0..2^31-2")
    return out


def _check_qem(maximum_error, boundary_weight, max_rounds):
    for name, x in (("maximum_error", maximum_error), ("boundary_weight", boundary_weight)):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not float(x) >= 0.0:
            raise ValueError(f"{name}={x!r} is not a number >= 0")
    if float(boundary_weight) == float("inf"):
        raise ValueError("boundary_weight must be finite")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or not 1 <= max_rounds <= QEM_MAX_ROUNDS:
        raise ValueError(f"max_rounds={max_rounds!r} is not an integer in 1..{QEM_MAX_ROUNDS}")


def qem_info(row):
    """One row of mesh_counts -> the info dictionary: QEM_INFO_KEYS, and stop_reason and max_cost decoded."""
    out = dict(zip(QEM_INFO_KEYS, (int(x) for x in row)))
    out["stop_reason"] = QEM_STOPS[out["stop"]]
    out["max_cost"] = float(torch.tensor(out["max_cost_bits"], dtype=torch.int32).view(torch.float32))
    return out


@torch.no_grad()
def simplify_quadric_decimation(meshes, target_number_of_triangles=None, target_fraction=None, maximum_error=float("inf"), boundary_weight=1.0,
                                colors_list=None, return_info=False, return_maps=False, max_rounds=256):
    """Thin every mesh by quadric edge collapses -> (verts_list, faces_list[, colors_list][, info][, (vert_map_list, face_map_list)]).
    Exactly one of target_number_of_triangles (an integer, or one per mesh) and target_fraction (in (0, 1], or one per mesh: the target
    is int(fraction * faces)) is given.  Collapses happen in rounds: every edge that is the cheapest of its two-hop neighbourhood and
    passes the validity checks (link condition, no flipped face, bdm_hip.h section 23) collapses at once, the vertex of the lower
    index surviving at the quadric's optimum.  Rounds are applied whole, so the final face count lies in (target - the last round's
    removals, target]; it is not exact.  A mesh stops when it has reached its target, when a round finds no valid edge (or none within
    maximum_error), or after max_rounds rounds; info[m]["stop_reason"] says which.  A closed, consistently wound manifold stays one,
    with its Euler characteristic; an open sheet keeps its boundary loops; non-manifold edges, non-finite vertices and faces with a bad
    index are left locked in place and counted.  Surviving vertices keep their order, surviving faces their order and winding.
    colors_list ((V_i, C) per mesh, uint8 or floating point, C <= 16) is carried along: a vertex nothing merged into keeps its row,
    another takes the order-free fixed-point mean of the old vertices mapped to it, as simplify_vertex_clustering does.  The maps:
    vert_map (V,) int64 old -> new index, face_map (F,) int64 the new index, -1 for a collapsed face, -3 for a bad one.  Everything is
    bit-reproducible and a mesh's result does not depend on its batch.  Not Open3D's heap order, and no attribute-aware quadrics.
    Bad arguments raise ValueError before any launch; host tensors are refused."""
    verts_list, faces_list = mesh_lists(meshes)
    targets = _check_targets(target_number_of_triangles, target_fraction, faces_list)
    _check_qem(maximum_error, boundary_weight, max_rounds)
    C = 0 if colors_list is None else _check_colors(colors_list, verts_list)
    if not verts_list:
        return mesh_tuple([], [], [], colors_list) + (([],) if return_info else ()) + ((([], []),) if return_maps else ())
    if len(verts_list) > MAX_B:
        raise ValueError(f"{len(verts_list)} meshes exceed {MAX_B}: split the batch")
    nv, nf = [int(v.shape[0]) for v in verts_list], [int(f.shape[0]) for f in faces_list]
    if sum(nv) >= 2 ** 31 - 1 or 6 * sum(nf) >= 2 ** 31 - 1:
        raise ValueError("the batch reaches 2^31 vertices or incidence records (six per face): split it")
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, dev, sum_v, sum_f = len(verts_list), verts.device, sum(nv), sum(nf)
    attrs = stage_attrs(colors_list, C, dev)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_qem_workspace_bytes(B, sum_v, sum_f), dev, "mesh_qem")
    counts = torch.zeros(B, len(QEM_INFO_KEYS), dtype=torch.int32, device=dev)
    active = torch.zeros(1, dtype=torch.int32, device=dev)
    want = torch.tensor(targets, dtype=torch.int64)
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()
    L.check(lib.bdm_mesh_qem_init(B, float(boundary_weight), want.data_ptr(), L.ptr(verts), L.ptr(faces), vf, ff, L.ptr(counts), L.ptr(ws),
                                  L.stream()), "mesh_qem_init")
    done = 0
    while True:
        L.check(lib.bdm_mesh_qem_rounds(B, QEM_ROUNDS_PER_CALL, max_rounds, float(maximum_error), vf, ff, L.ptr(counts), L.ptr(active), L.ptr(ws),
                                        L.stream()), "mesh_qem_rounds")
        done += QEM_ROUNDS_PER_CALL
        if int(active.item()) == 0 or done >= max_rounds + QEM_ROUNDS_PER_CALL:   # the one small read-back per call
            break
    rows = counts.cpu()
    new_v, new_f = rows[:, 6].tolist(), rows[:, 4].tolist()
    out_vert_first, out_face_first = first(new_v), first(new_f)
    verts_out, attrs_out, faces_out = alloc_outputs(out_vert_first, out_face_first, C, dev)
    vert_map = torch.zeros(max(sum_v, 1), dtype=torch.int32, device=dev)
    face_map = torch.zeros(max(sum_f, 1), dtype=torch.int32, device=dev)
    L.check(lib.bdm_mesh_qem_finish(B, C, L.ptr(attrs), vf, ff, out_vert_first.data_ptr(), out_face_first.data_ptr(), L.ptr(verts_out),
                                    L.ptr(attrs_out), L.ptr(faces_out), L.ptr(vert_map), L.ptr(face_map), L.ptr(ws), L.stream()), "mesh_qem_finish")
    out = split_outputs(verts_out, attrs_out, faces_out, out_vert_first, out_face_first, faces_list, colors_list, C)
    if return_info:
        out += ([qem_info(row) for row in rows.tolist()],)
    if return_maps:
        out += (([x.long() for x in vert_map[:sum_v].split(nv)], [x.long() for x in face_map[:sum_f].split(nf)]),)
    return out


# ---- command line ------------------------------------------------------------------------------------------------------------------
def decimate_batch(verts_list, faces_list, colors_list, device, voxel_size=None, resolution=None, contraction="average"):
    """Host tensors of ragged sizes (a colour entry None for a file that carries none) -> (verts_list, faces_list, colors_list, info) on
    the host, through simplify_vertex_clustering.  Files without colours ride along with zero rows of the batch's colour width."""
    return run_on_host_batch(simplify_vertex_clustering, verts_list, faces_list, colors_list, device, voxel_size, resolution, contraction)


QEM_CLI_KEYS = ("rounds", "collapses", "locked_vertices", "bad_faces")   # of the quadric method's JSON line: sums, rounds the maximum


def quadric_batch(verts_list, faces_list, colors_list, device, target_faces=None, target_fraction=None, maximum_error=float("inf"),
                  boundary_weight=1.0):
    """decimate_batch for simplify_quadric_decimation."""
    return run_on_host_batch(simplify_quadric_decimation, verts_list, faces_list, colors_list, device, target_number_of_triangles=target_faces,
                             target_fraction=target_fraction, maximum_error=maximum_error, boundary_weight=boundary_weight)


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


def process_tree(mesh_dir, out_dir, decimate_fn, batch_size=16, info_keys=INFO_KEYS, max_keys=("largest_cluster",)):
    """Walk mesh_dir for mesh .ply files in sorted path order, up to batch_size files per call of decimate_fn(verts_list, faces_list,
    colors_list) -> (verts_list, faces_list, colors_list, info; host tensors), and write out_dir/<same relative path>.  info_keys are
    summed over the files, those in max_keys take the maximum."""
    sums, sizes, edges = {k: 0 for k in info_keys}, [0, 0, 0, 0], [0, 0, 0, 0]

    def visit(v_in, f_in, v, f, i):
        before, after = _stats(torch.from_numpy(v_in), torch.from_numpy(f_in)), _stats(v, f)
        for k, add in enumerate((before["edges"], before["open_edges"], after["edges"], after["open_edges"])):
            edges[k] += add
        for k, add in enumerate((v_in.shape[0], f_in.shape[0], v.shape[0], f.shape[0])):
            sizes[k] += int(add)
        for k in info_keys:
            sums[k] = max(sums[k], int(i[k])) if k in max_keys else sums[k] + int(i[k])
    return compose_result(walk_tree(mesh_dir, out_dir, decimate_fn, batch_size, visit), sums, *sizes, *edges)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_decimate",
                                 description="write a tree of triangle meshes again, thinned by vertex clustering or by quadric edge collapses")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--method", choices=("clustering", "quadric"), default="clustering",
                    help="clustering: --resolution or --voxel-size; quadric (keeps a closed mesh closed): --target-faces or --target-fraction")
    grid = ap.add_mutually_exclusive_group()
    grid.add_argument("--resolution", type=int, help=f"cells along the mesh's largest extent, 1..{MAX_R}")
    grid.add_argument("--voxel-size", type=float, help="the cell size")
    grid.add_argument("--target-faces", type=int, help="quadric: the face count to reach, per mesh")
    grid.add_argument("--target-fraction", type=float, help="quadric: the share of its faces a mesh keeps, in (0, 1]")
    ap.add_argument("--contraction", choices=sorted(CONTRACTIONS), default="average")
    ap.add_argument("--max-error", type=float, default=float("inf"), help="quadric: no collapse above this quadric error")
    ap.add_argument("--boundary-weight", type=float, default=1.0, help="quadric: the weight of the planes that hold a boundary in place")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    try:
        if args.method == "quadric":
            if args.resolution is not None or args.voxel_size is not None:
                ap.error("--method quadric takes --target-faces or --target-fraction, not a grid")
            _check_targets(args.target_faces, args.target_fraction, [torch.zeros(0, 3)])
            _check_qem(args.max_error, args.boundary_weight, 256)
        else:
            if args.target_faces is not None or args.target_fraction is not None:
                ap.error("--target-faces and --target-fraction belong to --method quadric")
            _check_grid(args.voxel_size, args.resolution, 1)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_decimate needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    if args.method == "quadric":
        result = process_tree(args.mesh_dir, args.out_dir,
                              lambda v, f, c: quadric_batch(v, f, c, device, args.target_faces, args.target_fraction, args.max_error,
                                                            args.boundary_weight), args.batch_size, QEM_CLI_KEYS, ("rounds",))
        result = {"files": result.pop("files"), "method": "quadric", **result}
    else:
        result = process_tree(args.mesh_dir, args.out_dir,
                              lambda v, f, c: decimate_batch(v, f, c, device, args.voxel_size, args.resolution, args.contraction), args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
