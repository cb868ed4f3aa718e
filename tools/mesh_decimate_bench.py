"""Times simplify_vertex_clustering (bdm_mesh_cluster + the read-back of the counts + bdm_mesh_decimate) and its two calls alone, beside
bdm_mesh_adjacency on the same batch, the mesher that made the batch, and point_mesh_sqdist against a 4096-point cloud per mesh before
and after the decimation.  Times as tools/mesh_fill_bench.py takes them: the median of the timed calls, HIP
events around each call, after warm-up, with the fastest and the slowest beside it, everything in one run.

  Workloads: B meshes from reconstruct_surface of 4096-point spheres at 64^3, support 3, and of 600-point spheres at 32^3, support 2,
  each decimated at the given resolutions.

    python tools/mesh_decimate_bench.py [--batch 16] [--repeats 30] [--resolutions 32 16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import mesh_decimate as MD  # noqa: E402
from bdm_amd.ragged import first, pack_meshes  # noqa: E402
from tools.mesh_fill_bench import sphere_clouds, timed_ms  # noqa: E402


def run(B, N, resolution, support, R, repeats):
    from bdm_amd.mesh_metrics import point_mesh_sqdist
    from bdm_amd.surface import mesh_stats, reconstruct_surface
    pts, normals = sphere_clouds(B, N, seed=1)
    verts_list, faces_list = reconstruct_surface(pts, normals, resolution=resolution, support=support)
    mesher = timed_ms(lambda: reconstruct_surface(pts, normals, resolution=resolution, support=support), repeats)
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    sum_v, sum_f, lib = int(vert_first[-1]), int(face_first[-1]), L.lib()
    vf, ff = vert_first.data_ptr(), face_first.data_ptr()

    nbr_first = torch.empty(sum_v + 1, dtype=torch.int32, device="cuda")
    nbr = torch.empty(6 * sum_f, dtype=torch.int32, device="cuda")
    ws_a = torch.empty(lib.bdm_mesh_adjacency_workspace_bytes(B, sum_v, sum_f), dtype=torch.uint8, device="cuda")

    def adjacency():
        L.check(lib.bdm_mesh_adjacency(B, L.ptr(faces), vf, ff, L.ptr(nbr_first), L.ptr(nbr), L.ptr(ws_a), L.stream()), "mesh_adjacency")
    adj = timed_ms(adjacency, repeats)

    whole = timed_ms(lambda: MD.simplify_vertex_clustering((verts_list, faces_list), resolution=R), repeats)
    cluster = timed_ms(lambda: MD._cluster(verts, faces, vert_first, face_first, R, None, "average"), repeats)
    _, _, counts, ws = MD._cluster(verts, faces, vert_first, face_first, R, None, "average")
    counts = counts.cpu()
    info = {k: (max(col) if k == "largest_cluster" else sum(col)) for k, col in zip(MD.INFO_KEYS, zip(*counts.tolist()))}
    ovf, off = first(counts[:, 0].tolist()), first(counts[:, 1].tolist())
    verts_out = torch.empty(int(ovf[-1]), 3, device="cuda")
    faces_out = torch.empty(max(int(off[-1]), 1), 3, dtype=torch.int32, device="cuda")
    attrs = torch.zeros(1, 1, device="cuda")
    attrs_out = torch.zeros(1, 1, device="cuda")

    def decimate():
        L.check(lib.bdm_mesh_decimate(B, R, None, 0, 0, L.ptr(verts), L.ptr(attrs), L.ptr(faces), vf, ff, ovf.data_ptr(), off.data_ptr(),
                                      L.ptr(verts_out), L.ptr(attrs_out), L.ptr(faces_out), L.ptr(ws), L.stream()), "mesh_decimate")
    decimate_only = timed_ms(decimate, repeats)

    out_v, out_f = MD.simplify_vertex_clustering((verts_list, faces_list), resolution=R)
    cloud = sphere_clouds(B, 4096, seed=2)[0]
    score_before = timed_ms(lambda: point_mesh_sqdist((verts_list, faces_list), cloud), repeats)
    score_after = timed_ms(lambda: point_mesh_sqdist((out_v, out_f), cloud), repeats)
    d_before, d_after = point_mesh_sqdist((verts_list, faces_list), cloud)[0], point_mesh_sqdist((out_v, out_f), cloud)[0]
    before = [mesh_stats(v.cpu(), f.cpu()) for v, f in zip(verts_list, faces_list)]
    after = [mesh_stats(v.cpu(), f.cpu()) for v, f in zip(out_v, out_f)]
    frac = lambda rows: round(sum(r["open_edges"] for r in rows) / max(sum(r["edges"] for r in rows), 1), 5)   # noqa: E731
    both = cluster["median"] + decimate_only["median"]
    return {"meshes": B, "points": N, "resolution": resolution, "support": support, "decimate_resolution": R, "vertices": sum_v, "faces": sum_f,
            "repeats": repeats, "info": info, "face_ratio": round(info["new_faces"] / max(sum_f, 1), 4),
            "vertex_ratio": round(info["new_vertices"] / max(sum_v, 1), 4),
            "open_edge_fraction_before": frac(before), "open_edge_fraction_after": frac(after),
            "mean_point_to_mesh_dist_before": float(d_before.sqrt().mean()), "mean_point_to_mesh_dist_after": float(d_after.sqrt().mean()),
            "simplify_ms": whole, "cluster_call_ms": cluster, "decimate_call_ms": decimate_only, "adjacency_ms": adj, "mesher_ms": mesher,
            "point_mesh_sqdist_before_ms": score_before, "point_mesh_sqdist_after_ms": score_after,
            "two_calls_over_adjacency": round(both / adj["median"], 3), "simplify_over_mesher": round(whole["median"] / mesher["median"], 3),
            "scorer_saved_ms": round(score_before["median"] - score_after["median"], 4),
            "scorer_saved_over_simplify": round((score_before["median"] - score_after["median"]) / whole["median"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[32, 16])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"device": torch.cuda.get_device_name(0)}
    for R in args.resolutions:
        out[f"spheres_4096_R64_s3_at_{R}"] = run(args.batch, 4096, 64, 3, R, args.repeats)
        out[f"spheres_600_R32_s2_at_{R}"] = run(args.batch, 600, 32, 2, R, args.repeats)
    print(json.dumps(out))
