"""Cleaning the reconstructed meshes on the HIP path: the vertex adjacency of a packed batch of triangle meshes, its connected
components, the removal of small floating islands, and pytorch3d's `taubin_smoothing` (ops/mesh_filtering.py) with its name, argument
order and defaults, over bdm_mesh_adjacency / bdm_mesh_components_* / bdm_mesh_taubin (csrc/mesh_clean.hip; the rule is stated in
include/bdm_hip.h section 16 and DESIGN.md section 20).  pytorch3d is not installed, so the smoothing is restated from its published
behaviour ("parity unpinned", as for the normals).

    python -m bdm_amd.mesh_clean --mesh_dir D/pred_mesh --out_dir D/pred_mesh_clean [--min-fraction 0.1] [--min-faces 1]
                                 [--keep-largest] [--taubin-iters 10] [--lambd 0.53] [--mu -0.34] [--weights inverse_length]
                                 [--batch-size 16] [--fill-holes 0] [--decimate-resolution 0 | --decimate-fraction 0]

walks the mesh .ply files of mesh_dir in sorted order, removes the small components of every mesh, smooths what is left, writes it
under out_dir at the same relative path (vertex colours are carried along) and prints one JSON line.  --fill-holes N > 0 closes the
boundary loops of at most N edges between the two steps (bdm_amd.mesh_fill.fill_holes: islands, then holes, then smoothing) and adds
the summed fill counts to the JSON line; 0, the default, leaves files and JSON as they are without the option.
--decimate-resolution R > 0 thins every mesh by vertex clustering at R cells along its largest extent
(bdm_amd.mesh_decimate.simplify_vertex_clustering, contraction "average") after islands and holes and before the smoothing, which
relaxes the clustered triangles, and adds its counts to the JSON line as decimate_<count> (sums; the maximum for largest_cluster); 0,
the default, leaves files and JSON as they are without the option.  --decimate-fraction f in (0, 1] thins in the same place by
quadric edge collapses down to the share f of every mesh's faces instead (bdm_amd.mesh_decimate.simplify_quadric_decimation, which
keeps a closed mesh closed) and adds decimate_rounds (the maximum), decimate_collapses and decimate_locked_vertices (sums); the two
options exclude each other.

Departures from pytorch3d: a vertex without neighbours keeps its position (pytorch3d forms 0 / 0), `weights="uniform"` is an
extension, no gradients."""
import argparse
import json
import math
import sys

import torch

from . import _lib as L
from . import ops
from .mesh_fill import INFO_KEYS as FILL_KEYS   # what a clean_fn that fills holes adds to the info of a mesh (mesh_fill imports nothing of this module)
from .mesh_decimate import INFO_KEYS as DECIMATE_KEYS   # likewise for one that decimates, under "decimate_" + key
QEM_KEYS = ("rounds", "collapses", "locked_vertices")   # and for one that decimates by quadrics (sums; the maximum for rounds)
from .mesh_batch import walk_tree, with_padded_colors
from .ragged import mesh_lists, pack_meshes

MAX_B, MAX_ITER = 65535, 10000   # limits of bdm_hip.h section 16
WEIGHTS = {"inverse_length": 0, "uniform": 1}
ROUNDS_PER_CALL = 8   # label rounds between two reads of the `changed` flag


def _check_sizes(verts_list, faces_list):
    """The limits of bdm_hip.h section 16 on a batch, before anything is packed."""
    if len(verts_list) > MAX_B:
        raise ValueError(f"{len(verts_list)} meshes exceed {MAX_B}: split the batch")
    if sum(int(v.shape[0]) for v in verts_list) >= 2 ** 31 - 1 or 6 * sum(int(f.shape[0]) for f in faces_list) >= 2 ** 31:
        raise ValueError("the batch reaches 2^31 vertices or neighbour entries (six per face): split it")


def _adjacency(faces, vert_first, face_first):
    """One bdm_mesh_adjacency call -> (nbr_first (sum V + 1) int32, nbr (max(6 sum F, 1)) int32, -1 past nbr_first[-1])."""
    B, sum_v, sum_f, dev = vert_first.numel() - 1, int(vert_first[-1]), int(face_first[-1]), faces.device
    nbr_first = torch.zeros(sum_v + 1, dtype=torch.int32, device=dev)
    nbr = torch.full((max(6 * sum_f, 1),), -1, dtype=torch.int32, device=dev)
    if B == 0 or sum_v == 0:
        return nbr_first, nbr
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_adjacency_workspace_bytes(B, sum_v, sum_f), dev, "mesh_adjacency")
    L.check(lib.bdm_mesh_adjacency(B, L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), L.ptr(nbr_first), L.ptr(nbr), L.ptr(ws),
                                   L.stream()), "mesh_adjacency")
    return nbr_first, nbr


def _components(faces, vert_first, face_first, nbr_first, nbr, rounds_per_call=None):
    """init, rounds until the flag is clear, finish -> (vert_comp, face_comp, comp_count, comp_verts, comp_faces, calls); packed int32
    device tensors as the ABI writes them."""
    B, sum_v, sum_f, dev = vert_first.numel() - 1, int(vert_first[-1]), int(face_first[-1]), faces.device
    vert_comp = torch.zeros(sum_v, dtype=torch.int32, device=dev)
    face_comp = torch.full((sum_f,), -1, dtype=torch.int32, device=dev)
    comp_count = torch.zeros(B, dtype=torch.int32, device=dev)
    comp_verts, comp_faces = torch.zeros_like(vert_comp), torch.zeros_like(vert_comp)
    if B == 0 or sum_v == 0:
        return vert_comp, face_comp, comp_count, comp_verts, comp_faces, 0
    rounds = ROUNDS_PER_CALL if rounds_per_call is None else int(rounds_per_call)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_components_workspace_bytes(B, sum_v), dev, "mesh_components")
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()
    L.check(lib.bdm_mesh_components_init(B, vf, ff, L.ptr(ws), L.stream()), "mesh_components_init")
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    bound = int((vert_first[1:] - vert_first[:-1]).max())   # a round of plain propagation fixes at least one more vertex
    calls = 0
    while True:
        L.check(lib.bdm_mesh_components_rounds(B, rounds, vf, ff, L.ptr(nbr_first), L.ptr(nbr), L.ptr(changed), L.ptr(ws), L.stream()),
                "mesh_components_rounds")
        calls += 1
        if int(changed.item()) == 0:   # the only synchronisation: one read per call
            break
        if calls * rounds > bound + 1:
            raise L.BdmHipError(f"connected components: labels still change after {calls * rounds} rounds on meshes of at most {bound} vertices")
    fc = face_comp if sum_f else torch.zeros(1, dtype=torch.int32, device=dev)   # no NULL among the outputs
    L.check(lib.bdm_mesh_components_finish(B, L.ptr(faces), vf, ff, L.ptr(vert_comp), L.ptr(fc), L.ptr(comp_count), L.ptr(comp_verts),
                                           L.ptr(comp_faces), L.ptr(ws), L.stream()), "mesh_components_finish")
    return vert_comp, face_comp, comp_count, comp_verts, comp_faces, calls


@torch.no_grad()
def vertex_adjacency(meshes):
    """The vertex adjacency of a batch as a CSR over the packed vertices -> (nbr_first (sum V + 1) int32, nbr int32): the neighbours of
    packed vertex g are nbr[nbr_first[g] : nbr_first[g + 1]], ascending indices WITHIN its mesh, each once.  nbr has the upper bound of
    six entries per face (no read-back sizes it); the entries from nbr_first[-1] on are -1.  Only faces whose three indices are in range
    and pairwise different take part."""
    verts_list, faces_list = mesh_lists(meshes)
    if not verts_list:
        return torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    _check_sizes(verts_list, faces_list)
    _, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    return _adjacency(faces, vert_first, face_first)


@torch.no_grad()
def connected_components(meshes):
    """Per mesh (vert_comp (V,) int64, face_comp (F,) int64, comp_verts (C,) int64, comp_faces (C,) int64): the component of every vertex
    and face (-1 for a face that takes no part: an index out of range or repeated), components ranked by their smallest vertex index,
    and the vertex and face counts of the C components.  A vertex no face uses is a component of its own."""
    verts_list, faces_list = mesh_lists(meshes)
    if not verts_list:
        return []
    _check_sizes(verts_list, faces_list)
    _, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    nbr_first, nbr = _adjacency(faces, vert_first, face_first)
    vert_comp, face_comp, comp_count, comp_verts, comp_faces, _ = _components(faces, vert_first, face_first, nbr_first, nbr)
    counts = comp_count.cpu().tolist()   # the one read-back
    nv, nf = (vert_first[1:] - vert_first[:-1]).tolist(), (face_first[1:] - face_first[:-1]).tolist()
    return [(vc.long(), fc.long(), cv[:c].long(), cf[:c].long())
            for vc, fc, cv, cf, c in zip(vert_comp.split(nv), face_comp.split(nf), comp_verts.split(nv), comp_faces.split(nv), counts)]


def select_components(comp_faces, min_fraction=0.1, min_faces=1, keep_largest=False):
    """(C,) bool: which components of ONE mesh stay.  A component stays iff comp_faces >= max(min_faces, ceil(min_fraction * the largest
    comp_faces)); with keep_largest only the component of the most faces stays, the lower rank among equals."""
    cf = torch.as_tensor(comp_faces).long()
    if cf.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=cf.device)
    top = int(cf.max())
    if keep_largest:
        keep = torch.zeros_like(cf, dtype=torch.bool)
        keep[int((cf == top).nonzero()[0])] = True
        return keep
    return cf >= max(int(min_faces), math.ceil(min_fraction * top))


def compact_mesh(verts, faces, vert_comp, face_comp, keep, colors=None):
    """The kept vertices and the kept connected faces of one mesh in their original order, re-indexed (a boolean mask and a cumsum:
    integer torch plumbing on the tensors' device) -> (verts, faces, colors or None)."""
    vmask = keep[vert_comp] if keep.numel() else torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    fmask = face_comp >= 0
    fmask[fmask.clone()] = keep[face_comp[fmask]]
    new_index = torch.cumsum(vmask.long(), 0) - 1
    return verts[vmask], new_index[faces[fmask].long()].to(faces.dtype), (None if colors is None else colors[vmask])


def _check_selection(min_fraction, min_faces):
    if not (isinstance(min_fraction, (int, float)) and 0.0 <= min_fraction <= 1.0):
        raise ValueError(f"min_fraction={min_fraction!r} is outside 0..1")
    if isinstance(min_faces, bool) or int(min_faces) != min_faces or min_faces < 0:
        raise ValueError(f"min_faces={min_faces!r} is not a non-negative integer")


@torch.no_grad()
def remove_small_components(meshes, min_fraction=0.1, min_faces=1, keep_largest=False, colors_list=None, return_info=False):
    """Drop the small floating islands of every mesh -> (verts_list, faces_list[, colors_list][, info]).  A component is kept iff its
    face count is >= max(min_faces, ceil(min_fraction * the largest face count of its mesh)); keep_largest keeps the component of the
    most faces only (the lower rank on a tie).  Kept vertices and faces stay in their original order and are re-indexed; faces with an
    index out of range or repeated are always dropped; colors_list ((V_i, C) per mesh) is carried along.  A mesh that loses everything
    becomes a legal empty mesh.  info: per mesh {"components", "removed_components", "removed_vertices", "removed_faces"}."""
    _check_selection(min_fraction, min_faces)
    verts_list, faces_list = mesh_lists(meshes)
    if colors_list is not None:
        if not isinstance(colors_list, (list, tuple)) or len(colors_list) != len(verts_list):
            raise ValueError("colors_list must be a list with one (V_i, C) tensor per mesh")
        for c, v in zip(colors_list, verts_list):
            if not torch.is_tensor(c) or c.dim() != 2 or c.shape[0] != v.shape[0]:
                raise ValueError(f"a colour tensor is not ({v.shape[0]}, C)")
    out_v, out_f, out_c, info = [], [], [], []
    comps = connected_components((verts_list, faces_list))
    for m, (verts, faces, (vert_comp, face_comp, _, comp_faces)) in enumerate(zip(verts_list, faces_list, comps)):
        keep = select_components(comp_faces.cpu(), min_fraction, min_faces, keep_largest).to(verts.device)
        v, f, c = compact_mesh(verts, faces, vert_comp, face_comp, keep, None if colors_list is None else colors_list[m])
        out_v.append(v), out_f.append(f), out_c.append(c)
        info.append({"components": int(keep.numel()), "removed_components": int((~keep).sum()), "removed_vertices": int(verts.shape[0] - v.shape[0]),
                     "removed_faces": int(faces.shape[0] - f.shape[0])})
    out = (out_v, out_f) + ((out_c,) if colors_list is not None else ()) + ((info,) if return_info else ())
    return out


def _check_taubin(lambd, mu, num_iter, weights):
    if weights not in WEIGHTS:
        raise ValueError(f"weights={weights!r} is none of {list(WEIGHTS)}")
    if isinstance(num_iter, bool) or int(num_iter) != num_iter or not 0 <= num_iter <= MAX_ITER:
        raise ValueError(f"num_iter={num_iter!r} is outside 0..{MAX_ITER}")
    if not (math.isfinite(lambd) and math.isfinite(mu)):
        raise ValueError("lambd and mu must be finite")


@torch.no_grad()
def taubin_smoothing(meshes, lambd=0.53, mu=-0.34, num_iter=10, *, weights="inverse_length"):
    """pytorch3d's taubin_smoothing: num_iter times a Laplacian step with factor lambd, then one with factor mu, each the mean of the
    neighbours weighted by the inverse edge length (pytorch3d's norm_laplacian) or, weights="uniform", equally -> Meshes with the
    same faces.  A vertex without neighbours keeps its position.  Bad arguments raise ValueError before any launch."""
    from .cameras import Meshes
    _check_taubin(lambd, mu, num_iter, weights)
    verts_list, faces_list = mesh_lists(meshes)
    if not verts_list:
        return Meshes([], [])
    _check_sizes(verts_list, faces_list)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    B, sum_v, dev = len(verts_list), int(vert_first[-1]), verts.device
    if sum_v == 0:
        return Meshes([v.float() for v in verts_list], list(faces_list))
    nbr_first, nbr = _adjacency(faces, vert_first, face_first)
    out = torch.empty(sum_v, 3, dtype=torch.float32, device=dev)
    lib = L.lib()
    ws = ops.workspace(lib.bdm_mesh_taubin_workspace_bytes(B, sum_v), dev, "mesh_taubin")
    L.check(lib.bdm_mesh_taubin(B, int(num_iter), WEIGHTS[weights], float(lambd), float(mu), L.ptr(verts), vert_first.data_ptr(),
                                L.ptr(nbr_first), L.ptr(nbr), L.ptr(out), L.ptr(ws), L.stream()), "mesh_taubin")
    return Meshes(list(out.split((vert_first[1:] - vert_first[:-1]).tolist())), list(faces_list))


# ---- command line ------------------------------------------------------------------------------------------------------------------
def compose_result(files, vertices_in, faces_in, vertices_out, faces_out, components, removed_components):
    """The dictionary process_tree returns, from its seven sums."""
    return {"files": files, "vertices_in": vertices_in, "faces_in": faces_in, "vertices_out": vertices_out, "faces_out": faces_out,
            "components": components, "removed_components": removed_components}


def process_tree(mesh_dir, out_dir, clean_fn, batch_size=16):
    """Walk mesh_dir for mesh .ply files in sorted path order, up to batch_size files per call of clean_fn(verts_list, faces_list,
    colors_list; host tensors of ragged sizes, a colour entry None for a file that carries none) -> (verts_list, faces_list,
    colors_list, info as remove_small_components returns it; host tensors), and write out_dir/<same relative path>."""
    sums, fill_sums, decimate_sums = [0] * 7, {}, {}

    def visit(v_in, f_in, v, f, i):
        for k, add in enumerate((1, v_in.shape[0], f_in.shape[0], v.shape[0], f.shape[0], i["components"], i["removed_components"])):
            sums[k] += int(add)
        for k in FILL_KEYS:
            if k in i:   # clean_fn filled holes as well
                fill_sums[k] = fill_sums.get(k, 0) + int(i[k])
        for k in DECIMATE_KEYS + QEM_KEYS:
            if "decimate_" + k in i:   # clean_fn decimated as well
                combine = max if k in ("largest_cluster", "rounds") else int.__add__
                decimate_sums["decimate_" + k] = combine(decimate_sums.get("decimate_" + k, 0), int(i["decimate_" + k]))
    walk_tree(mesh_dir, out_dir, clean_fn, batch_size, visit)
    result = compose_result(*sums)
    result.update(fill_sums)
    result.update(decimate_sums)
    return result


def clean_batch(verts_list, faces_list, colors_list, device, min_fraction=0.1, min_faces=1, keep_largest=False, taubin_iters=10, lambd=0.53,
                mu=-0.34, weights="inverse_length", fill_holes=0, decimate_resolution=0, decimate_fraction=0.0):
    """process_tree's clean_fn on the HIP path: islands first, then (fill_holes > 0) the holes of at most fill_holes edges, then
    (decimate_resolution > 0) vertex clustering at that resolution or (decimate_fraction > 0; not both) quadric edge collapses down to
    that share of the faces, smoothing last (taubin_iters == 0 skips it)."""
    verts, faces = [v.to(device) for v in verts_list], [f.to(device) for f in faces_list]
    V = [v.shape[0] for v in verts]
    # files without colours ride along with a zero-width colour tensor, so that one call compacts all of them
    cols = [torch.zeros(n, 0, device=device) if c is None else c.to(device) for c, n in zip(colors_list, V)]
    verts, faces, cols, info = remove_small_components((verts, faces), min_fraction, min_faces, keep_largest, colors_list=cols, return_info=True)
    if fill_holes:
        from . import mesh_fill
        verts, faces, cols, fill_info = with_padded_colors(mesh_fill.fill_holes, (verts, faces), cols, int(fill_holes))
        info = [{**i, **fi} for i, fi in zip(info, fill_info)]
    if decimate_resolution:
        from . import mesh_decimate
        verts, faces, cols, dec_info = with_padded_colors(mesh_decimate.simplify_vertex_clustering, (verts, faces), cols,
                                                          resolution=int(decimate_resolution))
        info = [{**i, **{"decimate_" + k: v for k, v in di.items()}} for i, di in zip(info, dec_info)]
    if decimate_fraction:
        from . import mesh_decimate
        if decimate_resolution:
            raise ValueError("decimate_resolution and decimate_fraction exclude each other")
        verts, faces, cols, dec_info = with_padded_colors(mesh_decimate.simplify_quadric_decimation, (verts, faces), cols,
                                                          target_fraction=float(decimate_fraction))
        info = [{**i, **{"decimate_" + k: di[k] for k in QEM_KEYS}} for i, di in zip(info, dec_info)]
    if taubin_iters:
        verts = taubin_smoothing((verts, faces), lambd, mu, taubin_iters, weights=weights).verts_list()
    return ([v.cpu() for v in verts], [f.cpu() for f in faces], [None if c0 is None else c.cpu() for c, c0 in zip(cols, colors_list)], info)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.mesh_clean",
                                 description="write a tree of triangle meshes again without small islands and Taubin-smoothed")
    ap.add_argument("--mesh_dir", required=True, help="directory tree of triangle-mesh .ply files")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--min-fraction", type=float, default=0.1, help="a component stays with at least this share of the largest one's faces")
    ap.add_argument("--min-faces", type=int, default=1)
    ap.add_argument("--keep-largest", action="store_true")
    ap.add_argument("--taubin-iters", type=int, default=10, help="0 skips the smoothing")
    ap.add_argument("--lambd", type=float, default=0.53)
    ap.add_argument("--mu", type=float, default=-0.34)
    ap.add_argument("--weights", choices=sorted(WEIGHTS), default="inverse_length")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--fill-holes", type=int, default=0, metavar="N",
                    help="after the islands, close the boundary loops of at most N edges (bdm_amd.mesh_fill); 0 = off")
    ap.add_argument("--decimate-resolution", type=int, default=0, metavar="R",
                    help="after islands and holes, thin the mesh by vertex clustering at R cells along its largest extent "
                         "(bdm_amd.mesh_decimate); 0 = off")
    ap.add_argument("--decimate-fraction", type=float, default=0.0, metavar="f",
                    help="in the same place, thin the mesh by quadric edge collapses down to the share f of its faces, which keeps a closed "
                         "mesh closed (bdm_amd.mesh_decimate.simplify_quadric_decimation); 0 = off; not together with --decimate-resolution")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not 0 <= args.decimate_resolution <= 1024:
        ap.error("--decimate-resolution must be 0 (off) or lie in 1..1024")
    if not 0.0 <= args.decimate_fraction <= 1.0:
        ap.error("--decimate-fraction must be 0 (off) or lie in (0, 1]")
    if args.decimate_fraction and args.decimate_resolution:
        ap.error("--decimate-fraction and --decimate-resolution exclude each other")
    if args.fill_holes != 0 and not 3 <= args.fill_holes <= 65535:
        ap.error("--fill-holes must be 0 (off) or lie in 3..65535")
    try:
        _check_selection(args.min_fraction, args.min_faces)
        _check_taubin(args.lambd, args.mu, args.taubin_iters, args.weights)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.mesh_clean needs a HIP device (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())

    def clean_fn(verts_list, faces_list, colors_list):
        return clean_batch(verts_list, faces_list, colors_list, device, args.min_fraction, args.min_faces, args.keep_largest, args.taubin_iters,
                           args.lambd, args.mu, args.weights, args.fill_holes, args.decimate_resolution, args.decimate_fraction)

    result = process_tree(args.mesh_dir, args.out_dir, clean_fn, args.batch_size)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
