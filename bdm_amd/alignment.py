"""Rigid and similarity alignment of point clouds on the HIP path: pytorch3d's `iterative_closest_point` and
`corresponding_points_alignment` (ops/points_alignment.py) with their names, argument order and defaults, over bdm_similarity_apply /
bdm_corresponding_points_alignment / bdm_icp_* (csrc/align.hip; the rule is stated in include/bdm_hip.h section 18 and DESIGN.md
section 22).  pytorch3d is not installed, so the functions are restated from their published behaviour ("parity unpinned").

Departures from pytorch3d: D = 3 only; no reflections and no float weights (NotImplementedError; a 0/1 mask is accepted); no
gradients; every batch entry stops on its own, so `converged` is a bool tensor of N where pytorch3d has one bool, and an entry's
result does not depend on its batch-mates; identical clouds converge (mse == 0) where pytorch3d forms 0 / 0; `rmse` is, as in
pytorch3d, the mean SQUARED residual, here formed from the moments of the pairs and not by a second pass."""
from collections import namedtuple

import torch

from . import _lib as L
from . import ops
from .ragged import first, pack_rows

MAX_B, MAX_N, MAX_ITER = 65535, 2 ** 20, 10000   # limits of bdm_hip.h section 18
ROUNDS_PER_CALL = 4   # iterations between two reads of the `active` counter; the result does not depend on it
SimilarityTransform = namedtuple("SimilarityTransform", "R T s")
ICPSolution = namedtuple("ICPSolution", "converged rmse Xt RTs t_history")


def _clouds(name, X):
    """A padded (N, P, 3) tensor, a list of (P_i, 3) tensors or a Pointclouds -> (list of (P_i, 3) tensors, kind)."""
    if hasattr(X, "points_list") and hasattr(X, "points_padded"):
        return list(X.points_list()), "clouds"
    if torch.is_tensor(X):
        if X.dim() != 3 or X.shape[2] != 3 or not X.is_floating_point():
            raise ValueError(f"{name} must be a floating-point (N, P, 3) tensor (D = 3 only), got {tuple(X.shape)}")
        return list(X.unbind(0)), "padded"
    if isinstance(X, (list, tuple)):
        for t in X:
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or not t.is_floating_point():
                raise ValueError(f"{name} must hold floating-point (n, 3) tensors (D = 3 only)")
        return list(X), "list"
    raise ValueError(f"{name} must be an (N, P, 3) tensor, a list of (n, 3) tensors or a Pointclouds, got {type(X).__name__}")


def _check_sizes(xs, ys):
    if len(xs) != len(ys):
        raise ValueError(f"Point sets X and Y have to have the same number of batches: {len(xs)} and {len(ys)}")
    if len(xs) > MAX_B:
        raise ValueError(f"{len(xs)} entries exceed {MAX_B}: split the batch")
    np_, nr = [int(t.shape[0]) for t in xs], [int(t.shape[0]) for t in ys]
    if sum(np_) >= 2 ** 31 or sum(nr) >= 2 ** 31 or max(np_ + nr + [0]) > MAX_N:
        raise ValueError(f"the batch reaches 2^31 rows or an entry exceeds {MAX_N} points: split it")
    return np_, nr


def _check_common(estimate_scale, allow_reflection):
    if allow_reflection:
        raise NotImplementedError("allow_reflection=True is not offered: the solve (Horn's quaternion) always returns a proper rotation")
    if not isinstance(estimate_scale, (bool, int)):
        raise ValueError(f"estimate_scale={estimate_scale!r} is not a bool")


def _transform_rows(R, T, s, n, dev):
    """R (N, 3, 3), T (N, 3), s (N,) -> the (N, 13) float32 device rows of the ABI."""
    R, T, s = torch.as_tensor(R), torch.as_tensor(T), torch.as_tensor(s)
    if tuple(R.shape) != (n, 3, 3) or tuple(T.shape) != (n, 3) or tuple(s.shape) != (n,):
        raise ValueError(f"a transform of {n} entries is R ({n}, 3, 3), T ({n}, 3), s ({n},); got {tuple(R.shape)}, {tuple(T.shape)}, {tuple(s.shape)}")
    return L.f32(torch.cat([R.reshape(n, 9).float(), T.float(), s.reshape(n, 1).float()], dim=1).to(dev))


def _split_transform(rows):
    n = rows.shape[0]
    return SimilarityTransform(rows[:, :9].reshape(n, 3, 3).clone(), rows[:, 9:12].clone(), rows[:, 12].clone())


def _identity_rows(n, dev):
    rows = torch.zeros(n, 13, dtype=torch.float32, device=dev)
    rows[:, [0, 4, 8, 12]] = 1.0
    return rows


def _apply(x, x_first, rows):
    """One bdm_similarity_apply call on packed device rows."""
    B, sum_p = x_first.numel() - 1, int(x_first[-1])
    out = torch.empty(max(sum_p, 1), 3, dtype=torch.float32, device=x.device)
    if B and sum_p:
        lib = L.lib()
        ws = ops.workspace(lib.bdm_similarity_apply_workspace_bytes(B), x.device, "align")
        L.check(lib.bdm_similarity_apply(B, L.ptr(x), x_first.data_ptr(), L.ptr(rows), L.ptr(out), L.ptr(ws), L.stream()), "similarity_apply")
    return out


def _output(packed, counts, kind, like):
    """Packed rows back in the form the source came in."""
    parts = list(packed[:sum(counts)].split(counts))
    if kind == "padded":
        return torch.stack(parts).to(like.dtype) if parts else like.clone()
    if kind == "clouds":
        from .cameras import Pointclouds
        return Pointclouds(parts)
    return parts


@torch.no_grad()
def apply_similarity_transform(X, R, T, s):
    """xt = s (x @ R) + T per entry (pytorch3d's private _apply_similarity_transform, row-vector convention) on the device, every
    product and sum rounded on its own.  X: (N, P, 3), a list or a Pointclouds; the result has X's form."""
    xs, kind = _clouds("X", X)
    np_, _ = _check_sizes(xs, xs)
    rows = _transform_rows(R, T, s, len(xs), "cpu" if not xs else torch.as_tensor(R).device)   # the shapes are checked first
    if not xs:
        return _output(torch.zeros(0, 3), [], kind, X)
    for t in xs:
        L.ptr(t)   # refuses host tensors before anything is allocated
    dev = xs[0].device
    rows = rows.to(dev)
    x_first = first(np_)
    return _output(_apply(pack_rows(xs, 3, dev), x_first, rows), np_, kind, X)


def _mask_rows(xs, weights):
    """A 0/1 mask (N, P) or a list of (P_i,) masks: the rows with weight 0 become NaN rows, which no pair takes."""
    ws = list(weights.unbind(0)) if torch.is_tensor(weights) else list(weights)
    if len(ws) != len(xs) or any(tuple(w.shape) != (x.shape[0],) for w, x in zip(ws, xs)):
        raise ValueError("weights must give one value per point of X")
    for w in ws:
        if not bool(((w == 0) | (w == 1)).all()):
            raise NotImplementedError("float weights are not offered: weights must be a 0/1 mask")
    return [torch.where((w != 0)[:, None], x, torch.full((), float("nan"), dtype=x.dtype, device=x.device)) for x, w in zip(xs, ws)]


@torch.no_grad()
def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
    """pytorch3d's corresponding_points_alignment: the similarity transform (R, T, s) minimising sum |s x_i R + T - y_i|^2 over the
    pairs (x_i, y_i) of every entry -> SimilarityTransform(R (N, 3, 3), T (N, 3), s (N,)), s = 1 unless estimate_scale.  X and Y:
    (N, P, 3), lists of (P_i, 3) or Pointclouds with equal sizes per entry.  weights: None or a 0/1 mask; pairs with a non-finite
    member are left out; an entry without a pair gets the identity.  allow_reflection=True and float weights raise
    NotImplementedError.  No gradients."""
    _check_common(estimate_scale, allow_reflection)
    if not (eps >= 0 and eps < float("inf")):
        raise ValueError(f"eps={eps} must be finite and not negative")
    xs, _ = _clouds("X", X)
    ys, _ = _clouds("Y", Y)
    np_, nr = _check_sizes(xs, ys)
    if np_ != nr:
        raise ValueError("Point sets X and Y have to have the same number of points per entry.")
    if weights is not None:
        xs = _mask_rows(xs, weights)
    if not xs:
        return SimilarityTransform(torch.zeros(0, 3, 3), torch.zeros(0, 3), torch.zeros(0))
    for t in xs + ys:
        L.ptr(t)
    dev = xs[0].device
    rows, _ = _paired(pack_rows(xs, 3, dev), pack_rows(ys, 3, dev), first(np_), first(nr), bool(estimate_scale), float(eps))
    return _split_transform(rows)


def _paired(x, y, x_first, y_first, estimate_scale, eps):
    """One bdm_corresponding_points_alignment call -> (rows (B, 13), mse (B,))."""
    B, dev = x_first.numel() - 1, x.device
    rows, mse = _identity_rows(B, dev), torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    if B and int(x_first[-1]):
        lib = L.lib()
        ws = ops.workspace(lib.bdm_align_workspace_bytes(B), dev, "align")
        L.check(lib.bdm_corresponding_points_alignment(B, int(estimate_scale), eps, L.ptr(x), L.ptr(y), x_first.data_ptr(), y_first.data_ptr(),
                                                       L.ptr(rows), L.ptr(mse), L.ptr(ws), L.stream()), "corresponding_points_alignment")
    return rows, mse


def _icp(x, y, x_first, y_first, max_iterations, thr, estimate_scale, eps, rounds_per_call=None, history=True):
    """init, rounds until nobody is active, finish on packed device rows -> dict of device tensors: xt (sum P, 3), rows (B, 13),
    mse (B,), converged (B,) int32, iterations (B,) int32, history (B, max_iterations, 13) NaN-filled where no iteration wrote."""
    B, sum_p, dev = x_first.numel() - 1, int(x_first[-1]), x.device
    out = {"xt": x[:max(sum_p, 1)].clone(), "rows": _identity_rows(B, dev), "mse": torch.full((B,), float("nan"), dtype=torch.float32, device=dev),
           "converged": torch.zeros(B, dtype=torch.int32, device=dev), "iterations": torch.zeros(B, dtype=torch.int32, device=dev),
           "history": torch.full((B, max_iterations, 13), float("nan"), dtype=torch.float32, device=dev) if history else None, "calls": 0}
    if B == 0 or sum_p == 0:
        return out
    rounds = ROUNDS_PER_CALL if rounds_per_call is None else int(rounds_per_call)
    lib = L.lib()
    ws = torch.empty(max(lib.bdm_align_workspace_bytes(B), 16), dtype=torch.uint8, device=dev)   # stays untouched between the calls
    xf, yf = x_first.data_ptr(), y_first.data_ptr()
    L.check(lib.bdm_icp_init(B, L.ptr(x), L.ptr(y), xf, yf, None, L.ptr(ws), L.stream()), "icp_init")
    active = torch.zeros(1, dtype=torch.int32, device=dev)
    spent = 0
    while True:
        L.check(lib.bdm_icp_rounds(B, rounds, max_iterations, int(estimate_scale), thr, eps, L.ptr(x), L.ptr(y), xf, yf, L.ptr(out["history"]),
                                   L.ptr(active), L.ptr(ws), L.stream()), "icp_rounds")
        out["calls"] += 1
        spent += rounds
        if int(active.item()) == 0:   # the only synchronisation: one read per call
            break
        if spent >= max_iterations:
            raise L.BdmHipError(f"icp: {int(active.item())} entries still active after {spent} rounds with max_iterations={max_iterations}")
    L.check(lib.bdm_icp_finish(B, L.ptr(x), xf, yf, L.ptr(out["xt"]), L.ptr(out["rows"]), L.ptr(out["mse"]), L.ptr(out["converged"]),
                               L.ptr(out["iterations"]), L.ptr(ws), L.stream()), "icp_finish")
    return out


@torch.no_grad()
def icp_align_lists(x_list, y_list, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False):
    """The ragged form the evaluator uses: align every x_list[i] (P_i, 3) to y_list[i] (R_i, 3) in one batch ->
    (xt_list, converged (N,) bool, iterations (N,) int32, mse (N,) float32), device tensors."""
    sol_x, _ = _clouds("x_list", list(x_list))
    sol_y, _ = _clouds("y_list", list(y_list))
    np_, nr = _check_sizes(sol_x, sol_y)
    if not sol_x:
        return [], torch.zeros(0, dtype=torch.bool), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    for t in sol_x + sol_y:
        L.ptr(t)
    dev = sol_x[0].device
    res = _icp(pack_rows(sol_x, 3, dev), pack_rows(sol_y, 3, dev), first(np_), first(nr), int(max_iterations), float(relative_rmse_thr),
               bool(estimate_scale), 1e-9, history=False)
    return list(res["xt"][:sum(np_)].split(np_)), res["converged"].bool(), res["iterations"], res["mse"]


@torch.no_grad()
def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                            allow_reflection=False, verbose=False):
    """pytorch3d's iterative_closest_point: align the source clouds X to the target clouds Y by alternating the nearest-neighbour
    match of the transformed X in Y and the closed-form alignment of X to its partners -> ICPSolution(converged, rmse, Xt, RTs,
    t_history).  X and Y: (N, P, 3) tensors, lists of (P_i, 3) tensors or Pointclouds (lists give a list Xt, Pointclouds a Pointclouds).

    converged is a bool tensor of N, one per entry, where pytorch3d returns one bool for the batch: every entry stops on its own (when
    its mean squared residual is 0, or drops by no more than relative_rmse_thr relative to the previous iteration, or after
    max_iterations), and its result does not depend on its batch-mates.  rmse (N,) is pytorch3d's: the mean squared residual, NaN
    for an entry in which nothing matched.  RTs = SimilarityTransform(R (N, 3, 3), T (N, 3), s (N,)) maps the START cloud -- X after
    init_transform -- to Xt = s (X @ R) + T, as pytorch3d's does.  t_history lists the SimilarityTransform of every iteration that any
    entry ran; an entry that stopped earlier repeats its last transform.  init_transform: a SimilarityTransform (or an (R, T, s)
    tuple) applied first.  allow_reflection=True raises NotImplementedError.  No gradients; verbose prints one line."""
    _check_common(estimate_scale, allow_reflection)
    if isinstance(max_iterations, bool) or int(max_iterations) != max_iterations or not 1 <= max_iterations <= MAX_ITER:
        raise ValueError(f"max_iterations={max_iterations!r} is outside 1..{MAX_ITER}")
    if not relative_rmse_thr == relative_rmse_thr:
        raise ValueError("relative_rmse_thr is NaN")
    xs, kind = _clouds("X", X)
    ys, _ = _clouds("Y", Y)
    np_, nr = _check_sizes(xs, ys)
    N = len(xs)
    if init_transform is not None:
        if not isinstance(init_transform, (tuple, list)) or len(init_transform) != 3:
            raise ValueError("init_transform must be a SimilarityTransform (R, T, s)")
        R0, T0, s0 = (torch.as_tensor(t) for t in init_transform)
        if tuple(R0.shape) != (N, 3, 3) or tuple(T0.shape) != (N, 3) or tuple(s0.shape) != (N,):
            raise ValueError("The initial transformation init_transform has to be a named tuple of R (minibatch, 3, 3), T (minibatch, 3) "
                             "and s (minibatch,) tensors.")
    if N == 0:
        empty = SimilarityTransform(torch.zeros(0, 3, 3), torch.zeros(0, 3), torch.zeros(0))
        return ICPSolution(torch.zeros(0, dtype=torch.bool), torch.zeros(0), _output(torch.zeros(0, 3), [], kind, X), empty, [])
    for t in xs + ys:
        L.ptr(t)   # refuses host tensors before anything is allocated
    dev = xs[0].device
    x, y, x_first, y_first = pack_rows(xs, 3, dev), pack_rows(ys, 3, dev), first(np_), first(nr)
    if init_transform is not None:
        x = _apply(x, x_first, _transform_rows(R0, T0, s0, N, dev))   # the start cloud
    res = _icp(x, y, x_first, y_first, int(max_iterations), float(relative_rmse_thr), bool(estimate_scale), 1e-9)
    iters = res["iterations"].cpu()
    t_history = []
    for t in range(int(iters.max()) if N else 0):
        rows = torch.where((iters > t).to(dev)[:, None], res["history"][:, t], res["rows"])
        t_history.append(_split_transform(rows))
    sol = ICPSolution(res["converged"].bool(), res["mse"], _output(res["xt"], np_, kind, X), _split_transform(res["rows"]), t_history)
    if verbose:
        print(f"ICP: {int(sol.converged.sum())} of {N} entries converged, {int(iters.max())} iterations at most, "
              f"mean squared residual up to {float(torch.nan_to_num(sol.rmse, nan=0.0).max()):.3e}")
    return sol
