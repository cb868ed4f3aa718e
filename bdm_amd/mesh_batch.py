"""The tail that the operators which write new meshes share on the Python side (mesh_fill.fill_holes, mesh_decimate's two simplifiers
and their command lines; the front is ragged.py, the device side csrc/mesh_emit.h): the checks on the colour
tensors, their staging as float32 attribute rows, the packed outputs and their split back into per-mesh tensors, the wrapping that
lets host files with and without colours share one call, and the walk over a tree of mesh files."""
from pathlib import Path

import torch

from . import _lib as L

MAX_C = 16   # attribute channels (bdm_hip.h sections 19, 20 and 23)


def _check_colors(colors_list, verts_list):
    """-> C.  One (V_i, C) tensor per mesh, uint8 or floating point, the same C <= 16 everywhere."""
    if not isinstance(colors_list, (list, tuple)) or len(colors_list) != len(verts_list):
        raise ValueError("colors_list must be a list with one (V_i, C) tensor per mesh")
    C = None
    for c, v in zip(colors_list, verts_list):
        if not torch.is_tensor(c) or c.dim() != 2 or c.shape[0] != v.shape[0]:
            raise ValueError(f"a colour tensor is not ({v.shape[0]}, C)")
        if c.dtype != torch.uint8 and not c.dtype.is_floating_point:
            raise ValueError(f"a colour tensor is {c.dtype}, neither uint8 nor floating point")
        C = c.shape[1] if C is None else C
        if c.shape[1] != C:
            raise ValueError("the colour tensors differ in their number of channels")
    if C is not None and C > MAX_C:
        raise ValueError(f"{C} colour channels exceed {MAX_C}")
    return C or 0


def _round_uint8(rows):
    """float32 means of uint8 values -> uint8: to nearest, halves to even, clamped; a NaN (it cannot come from uint8 sources) -> 0."""
    return torch.nan_to_num(rows, nan=0.0).round().clamp(0, 255).to(torch.uint8)


def stage_attrs(colors_list, C, device):
    """The checked colour tensors of a non-empty batch (C channels; colors_list is not read at C = 0) -> the packed float32 attribute
    rows the ABI reads.  Host tensors raise BdmHipError before anything is allocated."""
    if not C:
        return torch.zeros(1, 1, dtype=torch.float32, device=device)
    for c in colors_list:
        L.ptr(c)
    return L.f32(torch.cat([c.float() for c in colors_list] + [torch.zeros(1, C, device=device)]))   # one unread row: never empty


def alloc_outputs(out_vert_first, out_face_first, C, device):
    """-> (verts_out, attrs_out, faces_out) for the two host offset arrays of the outputs, zeroed and never empty."""
    rows_v, rows_f = max(int(out_vert_first[-1]), 1), max(int(out_face_first[-1]), 1)
    return (torch.zeros(rows_v, 3, dtype=torch.float32, device=device), torch.zeros(rows_v, max(C, 1), dtype=torch.float32, device=device),
            torch.zeros(rows_f, 3, dtype=torch.int32, device=device))


def mesh_tuple(out_v, out_f, out_c, colors_list):
    """(verts_list, faces_list[, colors_list]): the colours are returned iff they were given."""
    return (out_v, out_f) + ((out_c,) if colors_list is not None else ())


def split_outputs(verts_out, attrs_out, faces_out, out_vert_first, out_face_first, faces_list, colors_list, C, old_verts=None):
    """The packed outputs -> mesh_tuple of per-mesh tensors: faces in the dtype of faces_list, colours (if given) in the dtype of
    colors_list, uint8 rounded and clamped, zero-width when they were given with C = 0.  With old_verts (fill_holes) a mesh's outputs
    begin with its old rows: float32 vertices, faces and colours keep the input's rows as they were given, and only the rows behind them
    are taken from the outputs."""
    out_v, out_f, out_c = [], [], []
    first_v, first_f = out_vert_first.tolist(), out_face_first.tolist()
    for m, f_old in enumerate(faces_list):
        v0, v1, f0, f1 = first_v[m], first_v[m + 1], first_f[m], first_f[m + 1]
        skip_v, skip_f = (int(old_verts[m].shape[0]), int(f_old.shape[0])) if old_verts is not None else (0, 0)
        if old_verts is not None and old_verts[m].dtype == torch.float32:
            out_v.append(torch.cat([old_verts[m], verts_out[v0 + skip_v:v1]]))
        else:
            out_v.append(verts_out[v0:v1])
        f_new = faces_out[f0 + skip_f:f1].to(f_old.dtype)
        out_f.append(f_new if old_verts is None else torch.cat([f_old, f_new]))
        if colors_list is not None:
            c_old = colors_list[m]
            if C:
                rows = attrs_out[v0 + skip_v:v1]
                c_new = _round_uint8(rows) if c_old.dtype == torch.uint8 else rows.to(c_old.dtype)
            else:
                c_new = c_old.new_zeros(v1 - v0 - skip_v, 0)
            out_c.append(c_new if old_verts is None else torch.cat([c_old, c_new]))
    return mesh_tuple(out_v, out_f, out_c, colors_list)


def with_padded_colors(fn, meshes, cols, *args, **kw):
    """fn(meshes, *args, colors_list=..., return_info=True, **kw) for colour tensors of mixed widths (zero-width: a mesh without
    colours): the narrower ones ride along as zero rows of the batch's width and come back zero-width."""
    width = max((c.shape[1] for c in cols), default=0)
    padded = [c if c.shape[1] == width else c.new_zeros(c.shape[0], width) for c in cols]
    verts, faces, out, info = fn(meshes, *args, colors_list=padded, return_info=True, **kw)
    return verts, faces, [o if c.shape[1] == width else o[:, :0] for o, c in zip(out, cols)], info


def run_on_host_batch(fn, verts_list, faces_list, colors_list, device, *args, **kw):
    """Host tensors of ragged sizes (a colour entry None for a file that carries none) -> (verts_list, faces_list, colors_list, info) on
    the host, through fn(meshes, *args[, colors_list=...], return_info=True, **kw) on `device`.  Files without colours ride along with
    zero rows of the batch's colour width and come back as None."""
    verts, faces = [v.to(device) for v in verts_list], [f.to(device) for f in faces_list]
    if any(c is not None for c in colors_list):
        cols = [torch.zeros(v.shape[0], 0, device=device) if c is None else c.to(device) for c, v in zip(colors_list, verts)]
        verts, faces, cols, info = with_padded_colors(fn, (verts, faces), cols, *args, **kw)
    else:
        verts, faces, info = fn((verts, faces), *args, return_info=True, **kw)
        cols = [None] * len(verts)
    return ([v.cpu() for v in verts], [f.cpu() for f in faces], [None if c0 is None else c.cpu() for c, c0 in zip(cols, colors_list)], info)


def walk_tree(mesh_dir, out_dir, batch_fn, batch_size, visit):
    """Walk mesh_dir for mesh .ply files in sorted path order, up to batch_size files per call of batch_fn(verts_list, faces_list,
    colors_list; host tensors of ragged sizes, a colour entry None for a file that carries none) -> (verts_list, faces_list,
    colors_list, info; host tensors), write out_dir/<same relative path> and call visit(v_in, f_in (numpy, as loaded), v, f, info
    entry) per file -> the number of files."""
    from .io import load_mesh_ply, save_mesh_ply
    mesh_dir, out_dir = Path(mesh_dir), Path(out_dir)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    items = [(path.relative_to(mesh_dir), path) for path in sorted(mesh_dir.rglob("*.ply"))]
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        loaded = [load_mesh_ply(path, with_colors=True) for _, path in chunk]
        verts, faces, colors, info = batch_fn([torch.from_numpy(v) for v, _, _ in loaded], [torch.from_numpy(f) for _, f, _ in loaded],
                                              [None if c is None else torch.from_numpy(c) for _, _, c in loaded])
        for (rel, _), (v_in, f_in, _), v, f, c, i in zip(chunk, loaded, verts, faces, colors, info):
            save_mesh_ply(v.numpy(), f.numpy(), out_dir / rel, colors=None if c is None else c.numpy())
            visit(v_in, f_in, v, f, i)
    return len(items)
