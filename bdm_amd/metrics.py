"""Generation metrics for unconditional samples (e.g. `pvd.Model.gen_samples`): set-against-set measures built from the full
(S, R) matrix of cloud-to-cloud distances between S generated and R reference clouds -- minimum matching distance (MMD),
coverage (COV) and 1-nearest-neighbour accuracy (1-NNA), each under Chamfer distance (CD) and under the approximate-match earth
mover's distance (EMD) the point-cloud generation literature reports.

The distance matrices are HIP (csrc/metrics.hip: bdm_pairwise_chamfer, bdm_pairwise_emd_approx for clouds of up to 2048 points;
csrc/metrics_emd_large.hip: bdm_pairwise_emd_large for any size, all pairs or paired; device tensors only, no CPU path);
the reductions over the small matrices are host-side torch and work on CPU tensors too.

The Jensen-Shannon divergence (JSD) between the occupancy-grid distributions of the two sets, and the mean occupancy entropy of a
set, come from per-cell histograms (csrc/occupancy.hip: bdm_occupancy_grid; device tensors only); the function names are those of
the reference's experiments/pvd/utils/metrics.py, and the float64 arithmetic on the histograms works on CPU tensors and arrays.

    python -m bdm_amd.metrics --sample gen.npy --ref ref.npy [--metrics cd,emd] [--num-points K] [--normalize] [--batch-size N] [--jsd] [--jsd-resolution R]
"""
import argparse
import functools
import glob
import json
import os
import sys
import warnings

import numpy as np
import torch

from . import _lib as L
from .io import load_pointcloud_ply


def _clouds(t, name):
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[1] < 1:
        raise ValueError(f"{name}: expected (count, points >= 1, 3), got {tuple(t.shape)}")
    return L.f32(t)


def _chunks(r, batch_size):
    if batch_size is None or batch_size >= r:
        return [(0, r)]
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    return [(j, min(r, j + batch_size)) for j in range(0, r, batch_size)]


def pairwise_chamfer(a, b, batch_size=None, return_directions=False):
    """a (S, N, 3), b (R, M, 3) on the GPU -> (S, R): mean over a_i of the squared distance to the nearest point of b_j, plus the
    same with the roles swapped.  `return_directions=True` returns the two halves (a -> b, b -> a) instead of their sum.
    `batch_size` bounds the references per launch; the result does not depend on it, bit for bit."""
    a, b = _clouds(a, "a"), _clouds(b, "b")
    S, R = a.shape[0], b.shape[0]
    chunks = _chunks(R, batch_size)
    ab = torch.empty(S, R, dtype=torch.float32, device=a.device)
    ba = torch.empty(S, R, dtype=torch.float32, device=a.device)
    for j0, j1 in chunks:
        # one chunk (the default) writes the result itself; column chunks of a row-major matrix go through a contiguous piece
        o_ab, o_ba = (ab, ba) if len(chunks) == 1 else (torch.empty(2, S, j1 - j0, dtype=torch.float32, device=a.device))
        L.check(L.lib().bdm_pairwise_chamfer(S, j1 - j0, a.shape[1], b.shape[1], L.ptr(a), L.ptr(b[j0:j1]), L.ptr(o_ab), L.ptr(o_ba),
                                             L.stream()), "pairwise_chamfer")
        if len(chunks) > 1:
            ab[:, j0:j1], ba[:, j0:j1] = o_ab, o_ba
    return (ab, ba) if return_directions else ab + ba


def pairwise_emd(a, b, batch_size=None):
    """a (S, N, 3), b (R, N, 3) on the GPU -> (S, R): approximate-match EMD cost(a_i, b_j) / N (not symmetric in a, b)."""
    a, b = _clouds(a, "a"), _clouds(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"pairwise_emd needs equal-sized clouds, got {a.shape[1]} and {b.shape[1]} points")
    S, R = a.shape[0], b.shape[0]
    chunks = _chunks(R, batch_size)
    out = torch.empty(S, R, dtype=torch.float32, device=a.device)
    for j0, j1 in chunks:
        o = out if len(chunks) == 1 else torch.empty(S, j1 - j0, dtype=torch.float32, device=a.device)
        L.check(L.lib().bdm_pairwise_emd_approx(S, j1 - j0, a.shape[1], L.ptr(a), L.ptr(b[j0:j1]), L.ptr(o), L.stream()), "pairwise_emd")
        if len(chunks) > 1:
            out[:, j0:j1] = o
    return out


EMD_SMALL_MAX_POINTS = 2048   # what bdm_pairwise_emd_approx holds in one workgroup; compute_all_metrics routes above it


def _emd_large_call(a, b, paired, mode, out):
    """One bdm_pairwise_emd_large launch on a (S, N, 3), b (R, N, 3) into out ((S, R), or (S,) when paired), with its workspace."""
    S, R, n = a.shape[0], b.shape[0], a.shape[1]
    pairs = S if paired else S * R
    if pairs == 0:
        return out
    if pairs >= 2 ** 31:
        raise ValueError(f"pairwise_emd_large: {S} x {R} pairs exceed one launch; pass a batch_size")
    nbytes = int(L.lib().bdm_pairwise_emd_large_workspace_bytes(pairs, n))
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=a.device)   # 0 bytes (n out of range): the call reports it
    L.check(L.lib().bdm_pairwise_emd_large(S, R, n, int(paired), int(mode), L.ptr(a), L.ptr(b), L.ptr(ws), nbytes, L.ptr(out),
                                           L.stream()), "pairwise_emd_large")
    return out


def _equal_sized(a, b, what):
    a, b = _clouds(a, "a"), _clouds(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{what} needs equal-sized clouds, got {a.shape[1]} and {b.shape[1]} points")
    return a, b


def pairwise_emd_large(a, b, batch_size=None, mode=0):
    """a (S, N, 3), b (R, N, 3) on the GPU, any N >= 1 -> (S, R): approximate-match EMD cost(a_i, b_j) / N (not symmetric in a, b).
    The same measure as `pairwise_emd` on another kernel (csrc/metrics_emd_large.hip); its bits are its own.  `mode` 0 lets the
    library choose between its resident (N <= 4096) and streamed forms, 1 / 2 force them: all give the same bits, and so does any
    `batch_size` (references per launch)."""
    a, b = _equal_sized(a, b, "pairwise_emd_large")
    S, R = a.shape[0], b.shape[0]
    chunks = _chunks(R, batch_size)
    out = torch.empty(S, R, dtype=torch.float32, device=a.device)
    for j0, j1 in chunks:
        o = out if len(chunks) == 1 else torch.empty(S, j1 - j0, dtype=torch.float32, device=a.device)
        _emd_large_call(a, b[j0:j1], False, mode, o)
        if len(chunks) > 1:
            out[:, j0:j1] = o
    return out


def paired_emd(a, b, mode=0):
    """a, b (P, N, 3) on the GPU, any N >= 1 -> (P,): approximate-match EMD cost(a_i, b_i) / N, the diagonal of
    `pairwise_emd_large(a, b)` bit for bit without the other P^2 - P pairs."""
    a, b = _equal_sized(a, b, "paired_emd")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"paired_emd needs as many clouds in a as in b, got {a.shape[0]} and {b.shape[0]}")
    return _emd_large_call(a, b, True, mode, torch.empty(a.shape[0], dtype=torch.float32, device=a.device))


def emd_route(num_points):
    """The function `compute_all_metrics` takes its EMD matrices from at this cloud size."""
    return pairwise_emd if num_points <= EMD_SMALL_MAX_POINTS else pairwise_emd_large


def mmd_cov(dist):
    """dist (S, R), rows = samples, columns = references ->
    mmd: mean over references of the distance to the nearest sample; mmd_smp: mean over samples of the distance to the nearest
    reference; cov: share of the references that are some sample's nearest reference (lowest index on ties)."""
    dist = torch.as_tensor(dist)
    S, R = dist.shape
    min_over_ref, min_over_smp = dist.min(dim=1).values, dist.min(dim=0).values
    nearest_ref = _first_argmin(dist)
    return {"mmd": float(min_over_smp.double().mean()), "mmd_smp": float(min_over_ref.double().mean()),
            "cov": float(nearest_ref.unique().numel()) / float(R)}


def _first_argmin(m):
    """Index of each row's minimum, the lowest index among ties."""
    n = m.shape[1]
    is_min = m == m.min(dim=1, keepdim=True).values
    idx = torch.arange(n, device=m.device).expand_as(m)
    return torch.where(is_min, idx, torch.full_like(idx, n)).min(dim=1).values


def one_nn_accuracy(dxx, dxy, dyy):
    """Leave-one-out 1-NN classifier over samples (dxx (S, S)) and references (dyy (R, R)) with dxy (S, R) between them: each
    item's nearest OTHER item (lowest index on ties; samples come first) predicts its label.  acc over all S + R items,
    acc_sample over the samples, acc_ref over the references."""
    dxx, dxy, dyy = torch.as_tensor(dxx), torch.as_tensor(dxy), torch.as_tensor(dyy)
    S, R = dxy.shape
    full = torch.cat([torch.cat([dxx, dxy], dim=1), torch.cat([dxy.t(), dyy], dim=1)], dim=0).clone()
    full.fill_diagonal_(float("inf"))
    nearest = _first_argmin(full)
    pred_sample = nearest < S
    is_sample = torch.arange(S + R, device=full.device) < S
    correct = pred_sample == is_sample
    return {"acc": float(correct.double().mean()), "acc_sample": float(correct[:S].double().mean()),
            "acc_ref": float(correct[S:].double().mean())}


def metrics_from_matrices(dxy, dxx, dyy, suffix):
    """The six figures of one distance (`suffix` "cd" or "emd") from its three matrices."""
    mc, nn = mmd_cov(dxy), one_nn_accuracy(dxx, dxy, dyy)
    return {f"mmd-{suffix}": mc["mmd"], f"mmd_smp-{suffix}": mc["mmd_smp"], f"cov-{suffix}": mc["cov"],
            f"1nna-{suffix}": nn["acc"], f"1nna_sample-{suffix}": nn["acc_sample"], f"1nna_ref-{suffix}": nn["acc_ref"]}


def compute_all_metrics(sample, ref, metrics=("cd", "emd"), batch_size=None):
    """sample (S, N, 3), ref (R, N, 3) on the GPU -> flat dict of floats: mmd, mmd_smp, cov, 1nna, 1nna_sample, 1nna_ref, each
    suffixed -cd / -emd.  EMD matrices of clouds of up to 2048 points come from `pairwise_emd`, larger ones from `pairwise_emd_large`."""
    fns = {"cd": pairwise_chamfer, "emd": emd_route(sample.shape[1])}
    out = {}
    for name in metrics:
        if name not in fns:
            raise ValueError(f"unknown metric {name!r}: choose from cd, emd")
        fn = fns[name]
        dxy, dxx, dyy = (fn(p, q, batch_size=batch_size).cpu() for p, q in ((sample, ref), (sample, sample), (ref, ref)))
        out.update(metrics_from_matrices(dxy, dxx, dyy, name))
    return out


# ---- occupancy grid: JSD and occupancy entropy -------------------------------------------------------------------------------
def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """Centres of the resolution^3 cells of a grid over the unit cube [-0.5, 0.5]^3, float32 (resolution, resolution, resolution, 3),
    and the spacing 1 / (resolution - 1).  `clip_sphere` drops the cells whose centre lies outside radius 0.5 and returns (kept, 3)
    in row-major cell order.  Coordinate i is float32(i * spacing - 0.5) with the arithmetic in double."""
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution) * spacing - 0.5).astype(np.float32)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1)
    if clip_sphere:
        cells = grid.reshape(-1, 3)
        return cells[_centre_in_sphere(cells)], spacing
    return grid, spacing


def _centre_in_sphere(cells):
    """cells (M, 3) float32 -> bool (M): the float32 norm of the centre is at most 0.5."""
    return np.linalg.norm(cells, axis=1) <= 0.5


@functools.lru_cache(maxsize=8)
def _device_grid(resolution, in_sphere, device):
    """axis (r) float32, cell mask (r^3) uint8 and the flat indices of the kept cells, on `device`."""
    grid, _ = unit_cube_grid_point_cloud(resolution)
    flat = grid.reshape(-1, 3)
    mask = _centre_in_sphere(flat) if in_sphere else np.ones(len(flat), dtype=bool)
    axis = np.ascontiguousarray(grid[:, 0, 0, 0])
    return (torch.from_numpy(axis).to(device), torch.from_numpy(mask.astype(np.uint8)).to(device),
            torch.from_numpy(np.flatnonzero(mask)).to(device))


def occupancy_grid(clouds, resolution=28, in_sphere=True):
    """clouds (S, N, 3) on the GPU -> (hits, active), int64 over the kept cells of the resolution^3 grid in row-major order (with
    `in_sphere` the cells whose centre lies within radius 0.5, else all): hits[c] = points of all clouds whose nearest kept cell is
    c, active[c] = clouds with at least one such point.  Integer sums: the sum over any split of the clouds equals the whole."""
    if not torch.is_tensor(clouds) or not clouds.is_cuda:
        raise L.BdmHipError("occupancy_grid runs on a HIP device only; got a host array (no CPU fallback)")
    clouds = _clouds(clouds, "clouds")
    if resolution < 2:
        raise ValueError(f"occupancy_grid: resolution must be at least 2, got {resolution}")
    S, N = clouds.shape[0], clouds.shape[1]
    bound = 0.5 + 10e-4
    if S > 0:
        if abs(float(clouds.max())) > bound or abs(float(clouds.min())) > bound:
            warnings.warn("Point-clouds are not in unit cube.")
        if in_sphere and float((clouds ** 2).sum(dim=2).sqrt().max()) > bound:
            warnings.warn("Point-clouds are not in unit sphere.")
    axis, mask, kept = _device_grid(int(resolution), bool(in_sphere), clouds.device)
    out = torch.empty(2, int(resolution) ** 3, dtype=torch.int32, device=clouds.device)
    L.check(L.lib().bdm_occupancy_grid(S, N, int(resolution), L.ptr(clouds), L.ptr(axis), L.ptr(mask), L.ptr(out[0]), L.ptr(out[1]),
                                       L.stream()), "occupancy_grid")
    return out[0][kept].long(), out[1][kept].long()


def _host_f64(v):
    return v.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)


def _xlogx(p, log=np.log):
    """p log p elementwise with 0 log 0 = 0."""
    out = np.zeros_like(p)
    pos = p > 0
    out[pos] = p[pos] * log(p[pos])
    return out


def _occupancy_entropy(active, num_clouds):
    """Mean over the cells of the entropy in nats of the Bernoulli variable "a cloud hits this cell", whose probability is
    active / num_clouds; cells that no cloud or every cloud hits add 0."""
    p = _host_f64(active) / float(num_clouds)
    return float(-(_xlogx(p) + _xlogx(1.0 - p)).sum() / p.size)


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False):
    """pclouds (S, N, 3), a GPU tensor or a host array (copied to the GPU) -> (mean occupancy entropy in nats, hits per kept cell as
    a float64 array)."""
    if not torch.is_tensor(pclouds):
        pclouds = _to_device(np.ascontiguousarray(pclouds, dtype=np.float32))
    hits, active = occupancy_grid(pclouds, grid_resolution, in_sphere)
    return _occupancy_entropy(active, pclouds.shape[0]), _host_f64(hits)


def _jsd_kl_form(p, q, mix):
    """JSD in bits of two distributions as the mean of their Kullback-Leibler divergences from their mixture `mix`."""
    def kl_from_mix(a):
        pos = a > 0   # mix >= a / 2 > 0 there
        return float((a[pos] * np.log2(a[pos] / mix[pos])).sum())
    return 0.5 * (kl_from_mix(p) + kl_from_mix(q))


def jensen_shannon_divergence(P, Q):
    """JSD in base 2 (0 .. 1) between the distributions P / sum(P) and Q / sum(Q); float64 on the host, any array or tensor.
    Returned in the entropy form H(mix) - (H(p) + H(q)) / 2; the Kullback-Leibler form is evaluated beside it and a warning is
    raised when the two are more than 10e-5 apart."""
    counts = [_host_f64(P), _host_f64(Q)]
    if any((c < 0).any() for c in counts):
        raise ValueError("Negative values.")
    if len(counts[0]) != len(counts[1]):
        raise ValueError("Non equal size.")
    p, q = (c / c.sum() for c in counts)
    mix = 0.5 * (p + q)
    bits = lambda d: float(-_xlogx(d, np.log2).sum())
    jsd = bits(mix) - 0.5 * (bits(p) + bits(q))
    if abs(jsd - _jsd_kl_form(p, q, mix)) > 10e-5:
        warnings.warn("Numerical values of two JSD methods don't agree.")
    return jsd


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """JSD between the occupancy-grid distributions (sphere-clipped resolution^3 grid) of two sets of clouds (S, N, 3), (R, M, 3)."""
    hits = [entropy_of_occupancy_grid(clouds, resolution, in_sphere=True)[1] for clouds in (sample_pcs, ref_pcs)]
    return jensen_shannon_divergence(*hits)


def normalize_unit_sphere(clouds):
    """Centre every cloud on its mean and scale it so that its farthest point lies on the unit sphere."""
    clouds = clouds - clouds.mean(axis=1, keepdims=True)
    radius = np.sqrt((clouds ** 2).sum(axis=2)).max(axis=1)
    return (clouds / np.maximum(radius, 1e-30)[:, None, None]).astype(np.float32)


def load_clouds(path):
    """A .npy of shape (count, N, 3), or a directory of .ply files (sorted by name) with equal point counts -> float32 array."""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.ply")))
        if not files:
            raise ValueError(f"{path}: no .ply files")
        clouds = [load_pointcloud_ply(f) for f in files]
        sizes = {c.shape[0] for c in clouds}
        if len(sizes) != 1:
            raise ValueError(f"{path}: clouds of different sizes {sorted(sizes)}")
        arr = np.stack(clouds)
    else:
        arr = np.load(path)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"{path}: expected (count, N, 3), got {arr.shape}")
    return np.ascontiguousarray(arr, dtype=np.float32)


def subsample_fps(clouds, num_points):
    """clouds (S, N, 3) on the GPU -> (S, num_points, 3): every cloud's furthest-point sample (bdm_furthest_point_sampling, which
    starts at point 0), points in the order they were picked.  num_points > N is an error."""
    from .functional import furthest_point_sample
    clouds = _clouds(clouds, "clouds")
    if not 1 <= num_points <= clouds.shape[1]:
        raise ValueError(f"--num-points {num_points}: the clouds have {clouds.shape[1]} points")
    if clouds.shape[0] == 0 or num_points == clouds.shape[1]:
        return clouds
    return furthest_point_sample(clouds.transpose(1, 2).contiguous(), num_points).transpose(1, 2).contiguous()


def _to_device(array):
    if not torch.cuda.is_available():
        raise L.BdmHipError("bdm_amd.metrics needs a HIP device (no CPU fallback)")
    return torch.from_numpy(array).cuda()


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m bdm_amd.metrics", description="MMD / COV / 1-NNA (and JSD) of generated against reference clouds")
    ap.add_argument("--sample", required=True, help=".npy (count, N, 3) or a directory of .ply: generated clouds")
    ap.add_argument("--ref", required=True, help=".npy (count, N, 3) or a directory of .ply: reference clouds")
    ap.add_argument("--metrics", default="cd,emd", type=lambda s: tuple(m for m in s.split(",") if m), help="cd, emd or cd,emd")
    ap.add_argument("--normalize", action="store_true", help="centre and scale every cloud to the unit sphere first")
    ap.add_argument("--batch-size", type=int, default=None, help="references per launch")
    ap.add_argument("--num-points", type=int, default=None, help="score furthest-point samples of this many points per cloud (the literature's protocol is 2048); "
                    "taken before --normalize and everything else; more than the clouds have is an error")
    ap.add_argument("--jsd", action="store_true", help="also report the occupancy-grid JSD and the two sets' occupancy entropies; the grid spans radius 0.5, so pass clouds that lie "
                    "inside it (--normalize scales to radius 1: most points would then snap to the cells at the sphere's surface)")
    ap.add_argument("--jsd-resolution", type=int, default=28, help="cells per axis of the occupancy grid")
    args = ap.parse_args(argv)
    bad = [m for m in args.metrics if m not in ("cd", "emd")]
    if bad or not args.metrics:
        ap.error(f"--metrics: choose from cd, emd (got {','.join(bad) or 'nothing'})")
    if args.num_points is not None and args.num_points < 1:
        ap.error("--num-points must be positive")
    return args


def main(argv=None):
    args = parse_args(argv)
    sample, ref = load_clouds(args.sample), load_clouds(args.ref)
    if args.num_points is not None:
        if args.num_points > min(sample.shape[1], ref.shape[1]):
            raise ValueError(f"--num-points {args.num_points}: the clouds have {sample.shape[1]} and {ref.shape[1]} points")
        sample, ref = (subsample_fps(_to_device(c), args.num_points).cpu().numpy() for c in (sample, ref))
    if args.normalize:
        sample, ref = normalize_unit_sphere(sample), normalize_unit_sphere(ref)
    sample_dev, ref_dev = _to_device(sample), _to_device(ref)
    result = compute_all_metrics(sample_dev, ref_dev, metrics=args.metrics, batch_size=args.batch_size)
    if args.jsd:
        (ent_s, hits_s), (ent_r, hits_r) = (entropy_of_occupancy_grid(c, args.jsd_resolution, True) for c in (sample_dev, ref_dev))
        result.update({"jsd": float(jensen_shannon_divergence(hits_s, hits_r)), "occupancy_entropy_sample": float(ent_s),
                       "occupancy_entropy_ref": float(ent_r)})
    result.update(num_sample=int(sample.shape[0]), num_ref=int(ref.shape[0]), num_points=int(sample.shape[1]))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
