"""K nearest neighbours between two point sets on the HIP path: pytorch3d's `knn_points` / `knn_gather` (ops/knn.py) with their
names, argument order and defaults, the ragged form the mesh code uses, and the transfer of per-point attributes through the
neighbour lists, over bdm_knn_points / bdm_knn_interpolate (csrc/knn.hip; the rule is stated in include/bdm_hip.h section 15 and
DESIGN.md section 19).  pytorch3d is not installed, so the functions are restated from their published behaviour ("parity
unpinned", as for the normals).

Departures from pytorch3d: D = 3 only, K <= 64, no gradients; `version` and `return_sorted` are accepted and ignored (there is one
kernel, and its result is always sorted)."""
from collections import namedtuple

import torch

from . import _lib as L
from . import ops
from .ragged import first, pack_rows

K_MAX, C_MAX, MAX_B = 64, 16, 65535   # limits of bdm_hip.h section 15
MODES = {"nearest": 0, "idw": 1}
KNN = namedtuple("KNN", "dists idx knn")


def _check_k(K):
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= K_MAX:
        raise ValueError(f"K={K!r} is outside 1..{K_MAX} (the kernel holds one neighbour per lane of a wave)")
    return int(K)


def _check_cloud_list(name, clouds):
    if not isinstance(clouds, (list, tuple)):
        raise ValueError(f"{name} must be a list of (n, 3) tensors, got {type(clouds).__name__}")
    for t in clouds:
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or not t.is_floating_point():
            raise ValueError(f"{name} must hold floating-point (n, 3) tensors (D = 3 only), got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")


def _check_sizes(np_, nr, K):
    if len(np_) != len(nr):
        raise ValueError(f"{len(np_)} query sets for {len(nr)} reference sets")
    if len(np_) > MAX_B:
        raise ValueError(f"{len(np_)} entries exceed {MAX_B}: split the batch")
    if sum(np_) >= 2 ** 31 or sum(nr) >= 2 ** 31 or sum(np_) * K >= 2 ** 31:
        raise ValueError("the batch reaches 2^31 rows or neighbour entries: split it")


def _search(queries, refs, q_first, r_first, K):
    """One bdm_knn_points call on packed device rows -> (idx (sum P, K) int32, d2 (sum P, K) float32)."""
    B, sum_p, dev = q_first.numel() - 1, int(q_first[-1]), queries.device
    idx = torch.empty(sum_p, K, dtype=torch.int32, device=dev)
    d2 = torch.empty(sum_p, K, dtype=torch.float32, device=dev)
    if B == 0 or sum_p == 0:
        return idx, d2
    lib = L.lib()
    ws = ops.workspace(lib.bdm_knn_points_workspace_bytes(B, sum_p, K), dev, "knn")
    L.check(lib.bdm_knn_points(B, K, L.ptr(queries), L.ptr(refs), q_first.data_ptr(), r_first.data_ptr(), L.ptr(idx), L.ptr(d2),
                               L.ptr(ws), L.stream()), "knn_points")
    return idx, d2


def _interpolate(attr, idx, d2, q_first, r_first, mode, eps, fill):
    """One bdm_knn_interpolate call -> out (sum P, c) float32."""
    B, sum_p, dev = q_first.numel() - 1, int(q_first[-1]), attr.device
    out = torch.empty(sum_p, attr.shape[1], dtype=torch.float32, device=dev)
    if B == 0 or sum_p == 0:
        return out
    lib = L.lib()
    ws = ops.workspace(lib.bdm_knn_interpolate_workspace_bytes(B), dev, "knn")
    L.check(lib.bdm_knn_interpolate(B, idx.shape[1], attr.shape[1], mode, float(eps), float(fill), L.ptr(attr), L.ptr(idx), L.ptr(d2),
                                    q_first.data_ptr(), r_first.data_ptr(), L.ptr(out), L.ptr(ws), L.stream()), "knn_interpolate")
    return out


@torch.no_grad()
def knn_packed(q_list, r_list, K):
    """The ragged form: for entry i the K nearest rows of r_list[i] ((R_i, 3)) to every row of q_list[i] ((P_i, 3)) ->
    [(idx (P_i, K) int64, d2 (P_i, K) float32)], the indices within r_list[i], ascending in (d2, index).  A row with fewer than K
    neighbours (a short or empty reference set, non-finite points) ends in idx = -1 and d2 = +inf.  All entries go through one call.
    Bad arguments raise ValueError before any launch; host tensors raise BdmHipError."""
    K = _check_k(K)
    _check_cloud_list("q_list", q_list)
    _check_cloud_list("r_list", r_list)
    np_, nr = [int(t.shape[0]) for t in q_list], [int(t.shape[0]) for t in r_list]
    _check_sizes(np_, nr, K)
    if not np_:
        return []
    for t in list(q_list) + list(r_list):
        L.ptr(t)   # refuses host tensors before anything is allocated
    dev = q_list[0].device
    idx, d2 = _search(pack_rows(q_list, 3, dev), pack_rows(r_list, 3, dev), first(np_), first(nr), K)
    return list(zip(idx.long().split(np_), d2.split(np_)))


@torch.no_grad()
def knn_gather(x, idx, lengths=None):
    """pytorch3d's knn_gather: x (N, M, U), idx (N, L, K) -> (N, L, K, U) with out[n, l, k] = x[n, idx[n, l, k]].  Rows where idx < 0,
    and neighbours k >= lengths[n] ((N,), the sizes of the sets idx points into), are zero.  Torch indexing: not a hot path."""
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError(f"expected x (N, M, U) and idx (N, L, K), got {tuple(x.shape)} and {tuple(idx.shape)}")
    if idx.is_floating_point() or idx.dtype == torch.bool:
        raise ValueError(f"idx must hold integers, got {idx.dtype}")
    N, M, U = x.shape
    K = idx.shape[2]
    if lengths is None:
        lengths = torch.full((N,), M, dtype=torch.int64, device=x.device)
    lengths = torch.as_tensor(lengths, device=x.device).long()
    if lengths.shape != (N,):
        raise ValueError(f"lengths must be ({N},), got {tuple(lengths.shape)}")
    idx = idx.long()
    absent = (idx < 0) | (idx >= M) | (torch.arange(K, device=x.device)[None, None, :] >= lengths[:, None, None])
    if M == 0:
        return torch.zeros(N, idx.shape[1], K, U, dtype=x.dtype, device=x.device)
    out = x[torch.arange(N, device=x.device)[:, None, None], idx.clamp(0, M - 1)]
    return torch.where(absent[..., None], torch.zeros((), dtype=x.dtype, device=x.device), out)


@torch.no_grad()
def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """pytorch3d's knn_points: for every point of p1 (N, P1, 3) the K nearest points of p2 (N, P2, 3) of the same batch entry ->
    KNN(dists (N, P1, K) float32 squared distances, idx (N, P1, K) int64, knn (N, P1, K, 3) if return_nn else None), ascending.
    lengths1 / lengths2 (N,): the number of valid points per cloud; rows past lengths1 and neighbours past lengths2 (and every
    other missing neighbour) come back zero-filled in both dists and idx, pytorch3d's documented padding (knn_packed shows the
    ABI's -1 / +inf).  version and return_sorted are accepted and ignored.  D = 3 only, K <= 64, no gradients."""
    K = _check_k(K)
    for name, p in (("p1", p1), ("p2", p2)):
        if not torch.is_tensor(p) or p.dim() != 3 or p.shape[2] != 3 or not p.is_floating_point():
            raise ValueError(f"{name} must be a floating-point (N, P, 3) tensor (D = 3 only)")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")   # pytorch3d's message
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]

    def counts(lengths, full, name):
        if lengths is None:
            return [full] * N
        lengths = torch.as_tensor(lengths)
        if lengths.shape != (N,) or lengths.is_floating_point() or lengths.dtype == torch.bool:
            raise ValueError(f"{name} must be ({N},) integers")
        c = [int(v) for v in lengths.tolist()]
        if c and (min(c) < 0 or max(c) > full):
            raise ValueError(f"{name} must lie in 0..{full}")
        return c
    n1, n2 = counts(lengths1, P1, "lengths1"), counts(lengths2, P2, "lengths2")
    _check_sizes(n1, n2, K)
    L.ptr(p1), L.ptr(p2)   # refuses host tensors before anything is allocated
    dev = p1.device
    dists = torch.zeros(N, P1, K, dtype=torch.float32, device=dev)
    idx = torch.zeros(N, P1, K, dtype=torch.int64, device=dev)
    if N and sum(n1):
        pi, pd = _search(pack_rows([p1[i, :n1[i]] for i in range(N)], 3, dev), pack_rows([p2[i, :n2[i]] for i in range(N)], 3, dev),
                         first(n1), first(n2), K)
        absent = pi < 0
        pi, pd = pi.long().masked_fill(absent, 0), pd.masked_fill(absent, 0.0)
        if n1 == [P1] * N:
            idx, dists = pi.view(N, P1, K), pd.view(N, P1, K)
        else:
            for i, (ri, rd) in enumerate(zip(pi.split(n1), pd.split(n1))):
                idx[i, :n1[i]], dists[i, :n1[i]] = ri, rd
    nn = knn_gather(p2, idx, torch.tensor(n2)) if return_nn else None
    return KNN(dists, idx, nn)


@torch.no_grad()
def transfer_point_attributes(query_list, ref_list, attr_list, K=3, mode="idw", eps=1e-8, fill=float("nan"), return_knn=False):
    """Attributes of reference points carried to query points: for entry i, attr_list[i] (R_i, C) of ref_list[i] (R_i, 3) ->
    (P_i, C) at query_list[i] (P_i, 3).  mode "nearest": the nearest reference row's attributes, bit for bit; "idw": the mean of
    the K nearest weighted by 1 / (d2 + eps).  A query without a neighbour gets `fill` in every channel.  1 <= C <= 16.
    return_knn=True: (outputs, knn_packed's list) of the same search.  One search and one interpolation launch for the batch."""
    K = _check_k(K)
    if mode not in MODES:
        raise ValueError(f"mode={mode!r} is none of {list(MODES)}")
    if mode == "idw" and not (eps > 0 and eps < float("inf")):
        raise ValueError(f"eps={eps} must be positive and finite")
    _check_cloud_list("query_list", query_list)
    _check_cloud_list("ref_list", ref_list)
    if not isinstance(attr_list, (list, tuple)) or len(attr_list) != len(ref_list):
        raise ValueError("attr_list must be a list with one (R_i, C) tensor per reference set")
    np_, nr = [int(t.shape[0]) for t in query_list], [int(t.shape[0]) for t in ref_list]
    _check_sizes(np_, nr, K)
    if not np_:
        return ([], []) if return_knn else []
    C = attr_list[0].shape[1] if torch.is_tensor(attr_list[0]) and attr_list[0].dim() == 2 else -1
    if not 1 <= C <= C_MAX:
        raise ValueError(f"attributes must be (R_i, C) tensors with C in 1..{C_MAX}")
    for a, n in zip(attr_list, nr):
        if not torch.is_tensor(a) or tuple(a.shape) != (n, C) or not a.is_floating_point():
            raise ValueError(f"an attribute tensor is not a floating-point ({n}, {C}) tensor")
    for t in list(query_list) + list(ref_list) + list(attr_list):
        L.ptr(t)   # refuses host tensors before anything is allocated
    dev = query_list[0].device
    q_first, r_first = first(np_), first(nr)
    idx, d2 = _search(pack_rows(query_list, 3, dev), pack_rows(ref_list, 3, dev), q_first, r_first, K)
    out = _interpolate(pack_rows(attr_list, C, dev), idx, d2, q_first, r_first, MODES[mode], eps if mode == "idw" else 1.0, fill)
    outs = list(out.split(np_))
    return (outs, list(zip(idx.long().split(np_), d2.split(np_)))) if return_knn else outs
