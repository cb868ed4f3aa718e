"""Filling the holes of the reconstructed meshes on the HIP path: the boundary loops of a packed batch of triangle meshes, and one new
vertex with a fan of new faces over every loop that is small, simple and finite, over bdm_mesh_boundary_loops / bdm_mesh_fill_holes
(csrc/mesh_fill.hip; the rule is stated in include/bdm_hip.h section 19 and DESIGN.md section 23).

    python -m bdm_amd.mesh_fill --mesh_dir D/pred_mesh --out_dir D/pred_mesh_filled [--max-hole-edges 32] [--batch-size 16]

walks the mesh .ply files of mesh_dir in sorted order, fills the holes of every mesh, writes it under out_dir at the same relative
path (vertex colours are carried along, a new vertex takes the mean colour of its loop) and prints one JSON line.

Left out, and counted in the returned info: a loop of more than max_hole_edges edges (a hole cannot be told from the rim of an open
sheet other than by size; a lone fragment with a short rim is closed into a pillow, so remove the islands first), a loop that passes
through a vertex twice ("pinched"), a loop with a non-finite vertex, and boundary edges next to a fin or to two faces wound the same
way ("blocked").  The patch is the plain centroid fan: no refinement, no fairing (Taubin smoothing afterwards relaxes it), no
gradients.  max_hole_edges = 32 is an interface default (MeshLab's close-holes default is 30 edges), documented, not tuned."""
import argparse
import json
import sys

import torch

from . import _lib as L
from . import ops
from .mesh_batch import MAX_C, _check_colors, _round_uint8   # noqa: F401  (their names here are part of the module)
from .mesh_batch import alloc_outputs, mesh_tuple, run_on_host_batch, split_outputs, stage_attrs, walk_tree
from .ragged import first, mesh_lists, pack_meshes

MAX_B, MAX_EDGES = 65535, 65535   # limits of bdm_hip.h section 19 (with mesh_batch.MAX_C)
FILLED, TOO_LARGE, PINCHED, NONFINITE = 1, 2, 4, 8   # loop flags
INFO_KEYS = ("boundary_edges", "loops", "filled_loops", "too_large_loops", "pinched_loops", "nonfinite_loops", "blocked_edges", "new_vertices",
             "new_faces")


def _check_cap(max_hole_edges):
    if isinstance(max_hole_edges, bool) or not isinstance(max_hole_edges, int) or not 3 <= max_hole_edges <= MAX_EDGES:
        raise ValueError(f"max_hole_edges={max_hole_edges!r} is not an integer in 3..{MAX_EDGES}")


def _check_sizes(verts_list, faces_list):
    """The limits of bdm_hip.h section 19 on a batch, before anything is packed."""
    if len(verts_list) > MAX_B:
        raise ValueError(f"{len(verts_list)} meshes exceed {MAX_B}: split the batch")
    sum_v, sum_f = sum(int(v.shape[0]) for v in verts_list), sum(int(f.shape[0]) for f in faces_list)
    if 6 * sum_f >= 2 ** 31 or sum_v + sum_f >= 2 ** 31 - 1:
        raise ValueError("the batch reaches 2^31 corner records (six per face) or vertex indices: split it")


def _loops(verts, faces, vert_first, face_first, max_hole_edges):
    """One bdm_mesh_boundary_loops call -> (halfedge_loop, loop_size, loop_flags (3 sum F each), mesh_counts (B, 9), workspace): int32
    device tensors as the ABI writes them; the workspace holds the loops for bdm_mesh_fill_holes."""
    B, sum_v, sum_f, dev = vert_first.numel() - 1, int(vert_first[-1]), int(face_first[-1]), verts.device
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_fill_workspace_bytes(B, sum_v, sum_f), dev, "mesh_fill")
    loop = torch.full((max(3 * sum_f, 1),), -1, dtype=torch.int32, device=dev)
    size, flags = torch.zeros_like(loop), torch.zeros_like(loop)
    counts = torch.zeros(B, len(INFO_KEYS), dtype=torch.int32, device=dev)
    L.check(lib.bdm_mesh_boundary_loops(B, int(max_hole_edges), L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(),
                                        L.ptr(loop), L.ptr(size), L.ptr(flags), L.ptr(counts), L.ptr(ws), L.stream()), "mesh_boundary_loops")
    return loop[:3 * sum_f], size[:3 * sum_f], flags[:3 * sum_f], counts, ws


@torch.no_grad()
def boundary_loops(meshes, max_hole_edges=32):
    """Per mesh (halfedge_loop (F, 3) int64, loop_sizes (L,) int64, loop_flags (L,) int64).  halfedge_loop[f, k] is the label of the loop
    that half-edge 3 f + k (faces[f, k] -> faces[f, (k + 1) % 3]) lies on, the loop's smallest half-edge index; -1 for a half-edge that
    is not on the boundary, -2 for a blocked one.  The L loops are listed in ascending label (torch.unique(halfedge_loop[halfedge_loop
    >= 0]) gives the labels); flags: 1 fillable, 2 more than max_hole_edges edges, 4 pinched, 8 a non-finite vertex."""
    _check_cap(max_hole_edges)
    verts_list, faces_list = mesh_lists(meshes)
    if not verts_list:
        return []
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    loop, size, flags, _, _ = _loops(verts, faces, vert_first, face_first, max_hole_edges)
    n3 = [3 * int(f.shape[0]) for f in faces_list]
    out = []
    for hl, ls, lf in zip(loop.split(n3), size.split(n3), flags.split(n3)):
        at = ls > 0
        out.append((hl.long().view(-1, 3), ls[at].long(), lf[at].long()))
    return out


@torch.no_grad()
def fill_holes(meshes, max_hole_edges=32, colors_list=None, return_info=False):
    """Close the small holes of every mesh -> (verts_list, faces_list[, colors_list][, info]).  Every boundary loop of at most
    max_hole_edges edges that is neither pinched nor non-finite gets one new vertex, the mean of its vertices, and one new face per
    edge, wound like the faces around it.  Old vertices and faces keep their place, order and bits (faces that take no part, with an
    index out of range or repeated, too); new vertices follow in ascending loop label and new faces in ascending half-edge index.
    colors_list ((V_i, C) per mesh, uint8 or floating point, C <= 16 the same everywhere) is carried along: a new row is the mean of its
    loop's rows, correctly rounded and clamped for uint8; a floating-point channel with a non-finite value gives NaN.  info: per mesh
    {"boundary_edges", "loops", "filled_loops", "too_large_loops", "pinched_loops", "nonfinite_loops", "blocked_edges", "new_vertices",
    "new_faces"}.  Bad arguments raise ValueError before any launch; host tensors are refused."""
    _check_cap(max_hole_edges)
    verts_list, faces_list = mesh_lists(meshes)
    C = 0 if colors_list is None else _check_colors(colors_list, verts_list)
    if not verts_list:
        return mesh_tuple([], [], [], colors_list) + (([],) if return_info else ())
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, dev = len(verts_list), verts.device
    attrs = stage_attrs(colors_list, C, dev)
    _, _, _, counts, ws = _loops(verts, faces, vert_first, face_first, max_hole_edges)
    counts = counts.cpu()   # the one read-back: it sizes the outputs
    new_v, new_f = counts[:, 7].tolist(), counts[:, 8].tolist()
    nv, nf = [int(v.shape[0]) for v in verts_list], [int(f.shape[0]) for f in faces_list]
    out_vert_first, out_face_first = first(a + b for a, b in zip(nv, new_v)), first(a + b for a, b in zip(nf, new_f))
    verts_out, attrs_out, faces_out = alloc_outputs(out_vert_first, out_face_first, C, dev)
    lib = L.lib()
    L.check(lib.bdm_mesh_fill_holes(B, C, L.ptr(verts), L.ptr(attrs), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(),
                                    out_vert_first.data_ptr(), out_face_first.data_ptr(), L.ptr(verts_out), L.ptr(attrs_out), L.ptr(faces_out),
                                    L.ptr(ws), L.stream()), "mesh_fill_holes")
    out = split_outputs(verts_out, attrs_out, faces_out, out_vert_first, out_face_first, faces_list, colors_list, C, old_verts=verts_list)
    return out + (([dict(zip(INFO_KEYS, row)) for row in counts.tolist()],) if return_info else ())   # the old rows keep their bits


# ---- command line ------------------------------------------------------------------------------------------------------------------
def fill_batch(verts_list, faces_list, colors_list, device, max_hole_edges=32):
    """Host tensors of ragged sizes (a colour entry None for a file that carries none) -> (verts_list, faces_list, colors_list, info) on
    the host, through fill_holes.  Files without colours ride along with zero rows of the batch's colour width."""
    return run_on_host_batch(fill_holes, verts_list, faces_list, colors_list, device, max_hole_edges)


def compose_result(files, info_sums, edges_in, open_in, edges_out, open_out):
    """The dictionary process_tree returns: the file count, the summed info, and the open edges over all edges of all meshes before
    and after."""
    out = {"files": files}
    out.update(info_sums)
    out["open_edge_fraction_in"] = open_in / edges_in if edges_in else 0.0
    out["open_edge_fraction_out"] = open_out / edges_out if edges_out else 0.0
    return out


def process_tree(mesh_dir, out_dir, fill_fn, batch_size=16):
    """Walk mesh_dir for mesh .ply files in sorted path order, up to batch_size files per call of fill_fn(verts_list, faces_list,
    colors_list) -> (verts_list, faces_list, colors_list, info; host tensors), and write out_dir/<same relative path>."""
    from .surface import mesh_stats
    sums, edges = {k: 0 for k in INFO_KEYS}, [0, 0, 0, 0]

    def visit(v_in, f_in, v, f, i):
        before, after = mesh_stats(torch.from_numpy(v_in), torch.from_numpy(f_in)), mesh_stats(v, f)
        for k, add in enumerate((before["edges"], before["open_edges"], after["edges"], after["open_edges"])):
            edges[k] += add
        for k in INFO_KEYS:
            sums[k] += int(i[k])
    return compose_result(walk_tree(mesh_dir, out_dir, fill_fn, batch_size, visit), sums, *edges)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_fill", description="write a tree of triangle meshes again with their small holes filled")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--max-hole-edges", type=int, default=32, help="a boundary loop of more edges stays open")
    ap.add_argument("--batch-size", type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    try:
        _check_cap(args.max_hole_edges)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_fill needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    result = process_tree(args.mesh_dir, args.out_dir, lambda v, f, c: fill_batch(v, f, c, device, args.max_hole_edges), args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
