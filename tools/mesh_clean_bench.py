"""Times bdm_mesh_adjacency, the connected components (all rounds) and bdm_mesh_taubin.  Times as
tools/knn_bench.py takes them: the median of the timed calls, HIP events around each call, after warm-up, with the fastest and the
slowest of the timed calls beside it; the yardsticks are timed in the same run.

  Workload: B meshes from reconstruct_surface at 64^3 of 4096-point spheres (about 224 000 vertices at B = 16).
  Yardsticks: a torch composition on the same GPU of the same three (edges by torch.unique, label propagation by scatter_reduce,
    Laplacian by index_add_), and the mesher itself (bdm_surface_grid + bdm_surface_extract through reconstruct_surface).

    python tools/mesh_clean_bench.py [--batch 16] [--iters 10] [--repeats 30]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import mesh_clean as MC  # noqa: E402
from bdm_amd.ragged import pack_meshes  # noqa: E402


def timed_ms(fn, repeats, warmup=3):
    """{"median", "min", "max"} in milliseconds of `repeats` calls between HIP events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return {"median": round(times[len(times) // 2], 4), "min": round(times[0], 4), "max": round(times[-1], 4)}


def sphere_clouds(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, N, 3, generator=g)
    return (d / d.norm(dim=-1, keepdim=True) * (0.3 + 0.003 * torch.randn(B, N, 1, generator=g))).cuda()


# ---- the torch composition (packed indices: the meshes are disjoint, so one graph serves the batch) -------------------------------------
def torch_edges(faces_packed, sum_v):
    """Directed edges (src, dst) of the packed batch, each once, sorted: torch.unique of directed keys."""
    f = faces_packed
    a = torch.cat([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    c = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    keys = torch.unique(a * sum_v + c)
    return keys // sum_v, keys % sum_v


def torch_labels(src, dst, sum_v):
    """The same round (minimum over the neighbours, one pointer jump) by scatter_reduce, to the fixed point -> (labels, rounds)."""
    l = torch.arange(sum_v, device=src.device)
    rounds = 0
    while True:
        m = l.clone().scatter_reduce_(0, src, l[dst], "amin", include_self=True)
        new = l[m]
        rounds += 1
        if torch.equal(new, l):   # one read-back per round
            return l, rounds
        l = new


def torch_taubin(verts, src, dst, lambd, mu, iters):
    """norm_laplacian weights and index_add_ sums (the order of the sums is not fixed: close to the kernel, not equal to it)."""
    v = verts
    for _ in range(iters):
        for f in (lambd, mu):
            w = 1.0 / ((v[src] - v[dst]).norm(dim=1) + 1e-12)
            s = torch.zeros_like(v).index_add_(0, src, w[:, None] * v[dst])
            tot = torch.zeros(v.shape[0], device=v.device).index_add_(0, src, w)
            v = torch.where((tot > 0)[:, None], (1.0 - f) * v + f * s / tot[:, None], v)
    return v


def run(B, iters, repeats):
    from bdm_amd.normals import estimate_pointcloud_normals
    from bdm_amd.surface import reconstruct_surface
    pts = sphere_clouds(B, 4096, seed=1)
    normals = estimate_pointcloud_normals(pts, 50, "visibility")
    verts_list, faces_list = reconstruct_surface(pts, normals, resolution=64)
    mesher = timed_ms(lambda: reconstruct_surface(pts, normals, resolution=64), repeats)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    sum_v, sum_f, lib = int(vert_first[-1]), int(face_first[-1]), L.lib()
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()

    nbr_first = torch.empty(sum_v + 1, dtype=torch.int32, device="cuda")
    nbr = torch.empty(6 * sum_f, dtype=torch.int32, device="cuda")
    ws_a = torch.empty(lib.bdm_mesh_adjacency_workspace_bytes(B, sum_v, sum_f), dtype=torch.uint8, device="cuda")

    def adjacency():
        L.check(lib.bdm_mesh_adjacency(B, L.ptr(faces), vf, ff, L.ptr(nbr_first), L.ptr(nbr), L.ptr(ws_a), L.stream()), "mesh_adjacency")
    adj = timed_ms(adjacency, repeats)

    calls = []

    def components():
        out = MC._components(faces, vert_first, face_first, nbr_first, nbr)
        calls.append(out[-1])
        return out
    comp = timed_ms(components, repeats)
    comp_out = components()

    out = torch.empty(sum_v, 3, device="cuda")
    ws_t = torch.empty(lib.bdm_mesh_taubin_workspace_bytes(B, sum_v), dtype=torch.uint8, device="cuda")

    def taubin(mode):
        def call():
            L.check(lib.bdm_mesh_taubin(B, iters, mode, 0.53, -0.34, L.ptr(verts), vf, L.ptr(nbr_first), L.ptr(nbr), L.ptr(out), L.ptr(ws_t), L.stream()),
                    "mesh_taubin")
        return call
    tau = timed_ms(taubin(0), repeats)
    tau_uniform = timed_ms(taubin(1), repeats)
    taubin(0)()
    smoothed = out.clone()

    # the torch composition
    shift = torch.repeat_interleave(vert_first[:-1], face_first[1:] - face_first[:-1]).cuda()
    faces_packed = faces.long() + shift[:, None]
    t_edges = timed_ms(lambda: torch_edges(faces_packed, sum_v), repeats)
    src, dst = torch_edges(faces_packed, sum_v)
    t_rounds = []
    t_labels = timed_ms(lambda: t_rounds.append(torch_labels(src, dst, sum_v)[1]), repeats)
    t_taubin = timed_ms(lambda: torch_taubin(verts, src, dst, 0.53, -0.34, iters), repeats)
    labels = torch_labels(src, dst, sum_v)[0]
    same_components = int(torch.unique(labels).numel()) == int(comp_out[2].sum())
    degree_total = int(nbr_first[-1])
    half_step_bytes = sum_v * (16 + 16 + 8) + degree_total * (4 + 16)     # own row in and out, two offsets; per neighbour its index and its row
    return {"meshes": B, "vertices": sum_v, "faces": sum_f, "neighbour_entries": degree_total, "taubin_iterations": iters, "repeats": repeats,
            "adjacency_ms": adj, "components_ms": comp, "component_calls_of_%d_rounds" % MC.ROUNDS_PER_CALL: calls[-1],
            "taubin_ms": tau, "taubin_uniform_ms": tau_uniform, "taubin_half_step_us": round(tau["median"] * 1e3 / (2 * iters), 2),
            "taubin_gather_gb_per_s": round(half_step_bytes * 2 * iters / (tau["median"] * 1e-3) / 1e9, 1),
            "torch_unique_edges_ms": t_edges, "torch_scatter_labels_ms": t_labels, "torch_label_rounds": t_rounds[-1], "torch_index_add_taubin_ms": t_taubin,
            "torch_over_kernel": {"adjacency": round(t_edges["median"] / adj["median"], 2), "components": round(t_labels["median"] / comp["median"], 2),
                                  "taubin": round(t_taubin["median"] / tau["median"], 2)},
            "same_component_count_as_torch": same_components, "edges_equal_to_torch": bool(src.numel() == degree_total),
            "largest_difference_to_torch_taubin": float((smoothed - torch_taubin(verts, src, dst, 0.53, -0.34, iters)).abs().max()),
            "mesher_ms": mesher, "cleaning_over_mesher": round((adj["median"] + comp["median"] + tau["median"]) / mesher["median"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"device": torch.cuda.get_device_name(0)}
    out.update(run(args.batch, args.iters, args.repeats))
    print(json.dumps(out))
