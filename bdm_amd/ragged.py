"""The ragged-batch conventions of the mesh and kNN operators, stated once (the device side is
csrc/ragged.h).  A batch travels as packed rows -- the rows of all entries, entry after entry, on the device -- and one host int64
array of b + 1 "first row" offsets per side, which the call reads before it returns.  An empty side still gets one (unread) row, so
that no input is NULL.  Batch and sum limits differ per operator and stay with the callers."""
import torch

from . import _lib as L


def first(counts):
    """Per-entry row counts -> the host int64 (len + 1,) array of first rows; its last entry is the sum."""
    return torch.tensor([0] + list(counts), dtype=torch.int64).cumsum(0)


def pack_rows(rows_list, width, device):
    """(n_i, width) device tensors -> packed float32 rows on `device`.  Host tensors raise BdmHipError before anything is allocated."""
    for t in rows_list:
        L.ptr(t)
    if sum(int(t.shape[0]) for t in rows_list) == 0:
        return torch.zeros(1, width, dtype=torch.float32, device=device)
    return L.f32(torch.cat([t.float() for t in rows_list]))


def mesh_lists(meshes):
    """A Meshes or a (verts_list, faces_list) pair -> (verts_list, faces_list), checked as cameras.Meshes checks them."""
    from .cameras import Meshes
    if hasattr(meshes, "verts_list") and hasattr(meshes, "faces_list"):
        return meshes.verts_list(), meshes.faces_list()
    if isinstance(meshes, (tuple, list)) and len(meshes) == 2 and isinstance(meshes[0], (list, tuple)):
        m = Meshes(list(meshes[0]), list(meshes[1]))   # raises ValueError for float or bool faces and bad shapes
        return m.verts_list(), m.faces_list()
    raise ValueError(f"expected a Meshes or a (verts_list, faces_list) pair, got {type(meshes).__name__}")


def faces_as_int32(f):
    """Vertex indices as int32.  An int64 index outside [0, 2^31) cannot be a vertex index: it becomes -1, an invalid face under every
    operator's rule, instead of wrapping around.  Pure torch: works on host tensors too."""
    if f.dtype == torch.int64:
        f = torch.where((f >= 0) & (f < 2 ** 31), f, -1)
    return f.int()


def pack_meshes(verts_list, faces_list):
    """A non-empty batch of meshes on one device -> (verts (sum V, 3) float32, faces (sum F, 3) int32, vert_first, face_first)."""
    for f in faces_list:
        L.ptr(f)   # host faces are refused here and host vertices by pack_rows, both before anything is allocated
    dev = verts_list[0].device
    verts = pack_rows(verts_list, 3, dev)
    if sum(int(f.shape[0]) for f in faces_list) == 0:
        faces = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    else:
        faces = torch.cat([faces_as_int32(f) for f in faces_list]).contiguous().to(dev)
    return verts, faces, first(v.shape[0] for v in verts_list), first(f.shape[0] for f in faces_list)
