"""Times simplify_quadric_decimation (bdm_mesh_qem_init, the rounds with one 4-byte read-back per 8 of them, bdm_mesh_qem_finish) beside
simplify_vertex_clustering, bdm_mesh_adjacency and the Poisson mesher that made the batch, all in one run.
Times as tools/mesh_decimate_bench.py takes them: the median of the timed calls, HIP events around each call, after warm-up, with the
fastest and the slowest beside it.  The time per round is the median over single-round calls, timed while a run is driven one round
at a time to its target; the collapses per round come from the same run, as counts and as a fraction of the live vertices.

  Workload: B Poisson meshes of 4096-point spheres at R = 64 and R = 128, each to 50 %, 25 % and 10 % of its faces.

    python tools/mesh_qem_bench.py [--batch 16] [--repeats 10] [--resolutions 64 128] [--fractions 0.5 0.25 0.1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import mesh_decimate as MD  # noqa: E402
from bdm_amd.ragged import pack_meshes  # noqa: E402
from tools.mesh_fill_bench import sphere_clouds, timed_ms  # noqa: E402


def per_round(verts, faces, vert_first, face_first, targets):
    """One run driven a round per call -> (ms per round, per round the collapses and live vertices summed over the batch, init ms)."""
    B, sum_v, sum_f, lib = vert_first.numel() - 1, int(vert_first[-1]), int(face_first[-1]), L.lib()
    ws = torch.empty(lib.bdm_mesh_qem_workspace_bytes(B, sum_v, sum_f), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(B, len(MD.QEM_INFO_KEYS), dtype=torch.int32, device="cuda")
    active = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = torch.tensor(targets, dtype=torch.int64)
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    L.check(lib.bdm_mesh_qem_init(B, 1.0, want.data_ptr(), L.ptr(verts), L.ptr(faces), vf, ff, L.ptr(counts), L.ptr(ws), L.stream()), "mesh_qem_init")
    t1.record()
    torch.cuda.synchronize()
    init_ms, times, rows = t0.elapsed_time(t1), [], []
    before = counts.cpu()
    for _ in range(1024):
        t0.record()
        L.check(lib.bdm_mesh_qem_rounds(B, 1, 1024, float("inf"), vf, ff, L.ptr(counts), L.ptr(active), L.ptr(ws), L.stream()), "mesh_qem_rounds")
        t1.record()
        torch.cuda.synchronize()
        now = counts.cpu()
        times.append(t0.elapsed_time(t1))
        rows.append({"collapses": int((now[:, 2] - before[:, 2]).sum()), "live_vertices": int(before[before[:, 0] == 0][:, 6].sum()),
                     "running": int((before[:, 0] == 0).sum())})
        before = now
        if int(active.item()) == 0:
            break
    return times, rows, init_ms


def run(B, N, resolution, fraction, repeats):
    from bdm_amd.surface import mesh_stats, reconstruct_surface
    pts, normals = sphere_clouds(B, N, seed=1)
    verts_list, faces_list = reconstruct_surface(pts, normals, resolution=resolution, method="poisson")
    mesher = timed_ms(lambda: reconstruct_surface(pts, normals, resolution=resolution, method="poisson"), repeats)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    sum_v, sum_f, lib = int(vert_first[-1]), int(face_first[-1]), L.lib()
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()
    nbr_first = torch.empty(sum_v + 1, dtype=torch.int32, device="cuda")
    nbr = torch.empty(6 * sum_f, dtype=torch.int32, device="cuda")
    ws_a = torch.empty(lib.bdm_mesh_adjacency_workspace_bytes(B, sum_v, sum_f), dtype=torch.uint8, device="cuda")

    def adjacency():
        L.check(lib.bdm_mesh_adjacency(B, L.ptr(faces), vf, ff, L.ptr(nbr_first), L.ptr(nbr), L.ptr(ws_a), L.stream()), "mesh_adjacency")
    adj = timed_ms(adjacency, repeats)
    whole = timed_ms(lambda: MD.simplify_quadric_decimation((verts_list, faces_list), target_fraction=fraction), repeats)
    out_v, out_f, info = MD.simplify_quadric_decimation((verts_list, faces_list), target_fraction=fraction, return_info=True)
    times, rows, init_ms = per_round(verts, faces, vert_first, face_first, [int(fraction * f.shape[0]) for f in faces_list])
    faces_out = sum(int(f.shape[0]) for f in out_f)
    cluster_R, cluster_faces = None, None
    for R in (8, 12, 16, 24, 32, 48, 64, 96, 128):   # the coarsest clustering of the ladder that leaves no fewer faces
        cf = MD.simplify_vertex_clustering((verts_list, faces_list), resolution=R)[1]
        if sum(int(f.shape[0]) for f in cf) >= faces_out:
            cluster_R, cluster_faces = R, sum(int(f.shape[0]) for f in cf)
            break
    cluster = timed_ms(lambda: MD.simplify_vertex_clustering((verts_list, faces_list), resolution=cluster_R), repeats) if cluster_R else None
    after = [mesh_stats(v.cpu(), f.cpu()) for v, f in zip(out_v, out_f)]
    share = [r["collapses"] / r["live_vertices"] for r in rows if r["live_vertices"]]
    return {"meshes": B, "points": N, "resolution": resolution, "fraction": fraction, "vertices": sum_v, "faces": sum_f, "faces_out": faces_out,
            "repeats": repeats, "rounds": [i["rounds"] for i in info], "stop": sorted({i["stop_reason"] for i in info}),
            "open_edges_after": sum(r["open_edges"] for r in after), "simplify_quadric_ms": whole, "init_ms": round(init_ms, 4),
            "round_ms": {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4), "n": len(times)},
            "collapses_per_round": [r["collapses"] for r in rows], "collapsed_share_of_live_vertices": [round(x, 4) for x in share],
            "collapsed_share_median": round(statistics.median(share), 4) if share else None,
            "rounds_times_round_ms_over_whole": round(len(times) * statistics.median(times) / whole["median"], 3),
            "clustering_resolution": cluster_R, "clustering_faces": cluster_faces, "simplify_clustering_ms": cluster, "adjacency_ms": adj,
            "mesher_ms": mesher, "round_over_adjacency": round(statistics.median(times) / adj["median"], 3),
            "quadric_over_mesher": round(whole["median"] / mesher["median"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.5, 0.25, 0.1])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"device": torch.cuda.get_device_name(0)}
    for R in args.resolutions:
        for frac in args.fractions:
            out[f"poisson_{args.points}_R{R}_to_{frac}"] = run(args.batch, args.points, R, frac, args.repeats)
            print(json.dumps({f"poisson_{args.points}_R{R}_to_{frac}": out[f"poisson_{args.points}_R{R}_to_{frac}"]}), flush=True)
    print(json.dumps(out))
