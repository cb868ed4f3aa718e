"""Quality-parity harness: the reference's acceptance metrics on `sample_*/{gt,pred}` directories
(experiments/evaluation/evaluation_cd.py:111-131: pytorch3d chamfer_distance x 1000 on mean-centred clouds;
experiments/evaluation/evaluation_f1.py:90-110: F1 with threshold 0.01 on SQUARED nearest-neighbour distances).
Nearest-neighbour search runs in HIP (bdm_nn_sqdist); the scalar reductions are host-side numpy.  On request also the
approximate-match EMD of every pred/gt pair with equal point counts (bdm_amd.metrics.paired_emd; the reference reports none).

    python -m bdm_amd.evaluation --pred_dir D --gt_dir D [--emd] [--icp] [--icp-scale]

With --icp the mean-centred pred is aligned to the mean-centred gt by iterative closest point (bdm_amd.alignment; --icp-scale also
estimates a scale) before the scores are taken, and the scores of the clouds as they lie are reported beside them.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import _lib as L
from .io import load_pointcloud_ply


def nn_sqdist(src, tgt):
    """src (B,N,3), tgt (B,M,3) on the GPU -> (B,N) squared distance to the nearest target point."""
    src, tgt = src.float().contiguous(), tgt.float().contiguous()
    B, N, _ = src.shape
    out = torch.empty(B, N, dtype=torch.float32, device=src.device)
    L.check(L.lib().bdm_nn_sqdist(B, N, tgt.shape[1], L.ptr(src), L.ptr(tgt), L.ptr(out), L.stream()), "nn_sqdist")
    return out


def chamfer_distance_x1000(pred, gt):
    """evaluation_cd.py: both clouds mean-centred; mean squared NN distance in both directions, summed, x 1000."""
    pred = pred - pred.mean(dim=1, keepdim=True)
    gt = gt - gt.mean(dim=1, keepdim=True)
    d_pg = nn_sqdist(pred, gt).double().cpu().numpy().mean(axis=1)
    d_gp = nn_sqdist(gt, pred).double().cpu().numpy().mean(axis=1)
    return (d_pg + d_gp) * 1000.0


def f1_score(pred, gt, thr=0.01):
    """evaluation_f1.py:90-110 (threshold on the squared distance, clamped at 1e-12, as the reference does)."""
    d1 = np.maximum(nn_sqdist(gt, pred).cpu().numpy(), 1e-12)
    d2 = np.maximum(nn_sqdist(pred, gt).cpu().numpy(), 1e-12)
    precision = (d1 < thr).mean(axis=1)
    recall = (d2 < thr).mean(axis=1)
    return 2 * recall * precision / (recall + precision + 1e-12)


def cd_x1000_as_is(pred, gt):
    """chamfer_distance_x1000 without the centring: for clouds that have been aligned."""
    d_pg = nn_sqdist(pred, gt).double().cpu().numpy().mean(axis=1)
    d_gp = nn_sqdist(gt, pred).double().cpu().numpy().mean(axis=1)
    return (d_pg + d_gp) * 1000.0


def align_batch(pred_list, gt_list, scale=False):
    """evaluate_dirs' alignment step on the HIP path: (P_i, 3) mean-centred device clouds -> (aligned pred list, converged (N,) bool,
    iterations (N,), mse (N,))."""
    from .alignment import icp_align_lists
    return icp_align_lists(pred_list, gt_list, estimate_scale=scale)


def _evaluate_dirs_aligned(pred_dir, gt_dir, device, emd, align_scale, batch_size):
    """evaluate_dirs with align="icp": the files go through align_batch in ragged batches of batch_size."""
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    pairs = []
    for root, _, files in os.walk(pred_dir):
        for f in sorted(files):
            rel = os.path.relpath(os.path.join(root, f), pred_dir)
            if f.endswith(".ply") and os.path.exists(os.path.join(gt_dir, rel)):
                pairs.append((os.path.join(root, f), os.path.join(gt_dir, rel)))
    pairs.sort()   # the batches do not depend on the order in which the tree is walked
    cds, f1s, emds, cds0, f1s0, conv, iters, mses = [], [], [], [], [], 0, [], []
    for lo in range(0, len(pairs), batch_size):
        chunk = pairs[lo:lo + batch_size]
        preds = [torch.from_numpy(load_pointcloud_ply(p)).float().to(device) for p, _ in chunk]
        gts = [torch.from_numpy(load_pointcloud_ply(g)).float().to(device) for _, g in chunk]
        preds, gts = [p - p.mean(0, keepdim=True) for p in preds], [g - g.mean(0, keepdim=True) for g in gts]
        aligned, converged, iterations, mse = align_batch(preds, gts, align_scale)
        conv += int(converged.sum())
        iters += [float(v) for v in iterations.cpu().tolist()]
        mses += [float(v) for v in mse.cpu().tolist()]
        for p, a, g in zip(preds, aligned, gts):
            p, a, g = p[None], a[None], g[None]
            cds0.append(float(cd_x1000_as_is(p, g)[0]))
            f1s0.append(float(f1_score(p, g)[0]))
            cds.append(float(cd_x1000_as_is(a, g)[0]))
            f1s.append(float(f1_score(a, g)[0]))
            if emd and a.shape[1] == g.shape[1]:
                from .metrics import paired_emd
                emds.append(float(paired_emd(a, g)[0]))
    mean = lambda v: float(np.mean(v)) if v else float("nan")   # noqa: E731
    out = {"num": len(cds), "cd_x1000": mean(cds), "f1_at_0.01": mean(f1s), "cd_x1000_unaligned": mean(cds0), "f1_at_0.01_unaligned": mean(f1s0),
           "icp_converged": conv, "icp_iterations_mean": mean(iters), "icp_mse_mean": float(np.nanmean(mses)) if np.isfinite(mses).any() else float("nan")}
    if emd:
        out.update(emd=mean(emds), emd_num=len(emds))
    return out


def evaluate_dirs(pred_dir, gt_dir, device="cuda", emd=False, align=None, align_scale=False, batch_size=16):
    """Mean CD x 1e3 and mean F1@0.01 over matching .ply files of two directory trees.  `emd=True` adds "emd", the mean
    approximate-match EMD (cost / points, pred against gt) of the mean-centred clouds over the pairs whose two clouds have equal
    point counts, and "emd_num", the number of such pairs.  align="icp": the mean-centred pred is aligned to the mean-centred gt by
    iterative closest point (align_scale: with a scale) before CD, F1 and EMD, in ragged batches of batch_size files; the result
    gains "cd_x1000_unaligned" and "f1_at_0.01_unaligned" (the scores as the clouds lie), "icp_converged" (a count),
    "icp_iterations_mean" and "icp_mse_mean" (over the entries in which something matched)."""
    if align is not None:
        if align != "icp":
            raise ValueError(f"align={align!r} is neither None nor 'icp'")
        return _evaluate_dirs_aligned(pred_dir, gt_dir, device, emd, align_scale, batch_size)
    cds, f1s, emds = [], [], []
    for root, _, files in os.walk(pred_dir):
        for f in sorted(files):
            if not f.endswith(".ply"):
                continue
            rel = os.path.relpath(os.path.join(root, f), pred_dir)
            gt_path = os.path.join(gt_dir, rel)
            if not os.path.exists(gt_path):
                continue
            p = torch.from_numpy(load_pointcloud_ply(os.path.join(root, f)))[None].to(device)
            g = torch.from_numpy(load_pointcloud_ply(gt_path))[None].to(device)
            cds.append(float(chamfer_distance_x1000(p, g)[0]))
            pc, gc = p - p.mean(1, keepdim=True), g - g.mean(1, keepdim=True)
            f1s.append(float(f1_score(pc, gc)[0]))
            if emd and pc.shape[1] == gc.shape[1]:
                from .metrics import paired_emd
                emds.append(float(paired_emd(pc, gc)[0]))
    out = {"num": len(cds), "cd_x1000": float(np.mean(cds)) if cds else float("nan"),
           "f1_at_0.01": float(np.mean(f1s)) if f1s else float("nan")}
    if emd:
        out.update(emd=float(np.mean(emds)) if emds else float("nan"), emd_num=len(emds))
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.evaluation", description="CD x 1e3, F1@0.01 (and EMD) of pred against gt .ply trees")
    ap.add_argument("--pred_dir", required=True, help="directory tree of predicted .ply clouds")
    ap.add_argument("--gt_dir", required=True, help="directory tree of ground-truth .ply clouds with the same relative paths")
    ap.add_argument("--emd", action="store_true", help="also the mean approximate-match EMD over the pairs with equal point counts")
    ap.add_argument("--icp", action="store_true", help="align the mean-centred pred to the mean-centred gt by ICP first; the unaligned scores stay in the output")
    ap.add_argument("--icp-scale", action="store_true", help="with --icp: estimate a scale as well")
    ap.add_argument("--batch-size", type=int, default=16, help="with --icp: files per ragged batch")
    args = ap.parse_args(argv)
    if args.icp_scale and not args.icp:
        ap.error("--icp-scale needs --icp")
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.evaluation needs a HIP device (no CPU fallback)")
    if args.icp:
        result = evaluate_dirs(args.pred_dir, args.gt_dir, emd=args.emd, align="icp", align_scale=args.icp_scale, batch_size=args.batch_size)
    else:
        result = evaluate_dirs(args.pred_dir, args.gt_dir, emd=args.emd)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
