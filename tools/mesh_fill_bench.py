"""Times fill_holes (bdm_mesh_boundary_loops + the read-back of the counts + bdm_mesh_fill_holes) and its two calls alone, beside
bdm_mesh_adjacency on the same batch (the same incidence work: count, scan, claim, sort per vertex) and the mesher that made the batch
(DESIGN.md section 23).  Times as tools/mesh_clean_bench.py takes them: the median of the timed calls, HIP events around each call,
after warm-up, with the fastest and the slowest beside it, everything in one run.

  Workloads: B meshes from reconstruct_surface of 4096-point spheres at 64^3, support 3 (few holes), and of 600-point spheres at 32^3,
  support 2 (hole-rich: about a quarter of the edges are open).

    python tools/mesh_fill_bench.py [--batch 16] [--repeats 30] [--max-hole-edges 32]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import mesh_fill as MF  # noqa: E402
from bdm_amd.ragged import first, pack_meshes  # noqa: E402


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
    d = d / d.norm(dim=-1, keepdim=True)
    return (d * 0.4).cuda(), d.cuda()   # points and their analytic outward normals


def run(B, N, resolution, support, cap, repeats):
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

    whole = timed_ms(lambda: MF.fill_holes((verts_list, faces_list), cap), repeats)
    loops = timed_ms(lambda: MF._loops(verts, faces, vert_first, face_first, cap), repeats)
    _, _, _, counts, ws = MF._loops(verts, faces, vert_first, face_first, cap)
    counts = counts.cpu()
    info = dict(zip(MF.INFO_KEYS, counts.sum(0).tolist()))
    nv, nf = (vert_first[1:] - vert_first[:-1]).tolist(), (face_first[1:] - face_first[:-1]).tolist()
    ovf, off = first(a + b for a, b in zip(nv, counts[:, 7].tolist())), first(a + b for a, b in zip(nf, counts[:, 8].tolist()))
    verts_out = torch.empty(int(ovf[-1]), 3, device="cuda")
    faces_out = torch.empty(int(off[-1]), 3, dtype=torch.int32, device="cuda")
    attrs = torch.zeros(1, 1, device="cuda")
    attrs_out = torch.zeros(1, 1, device="cuda")

    def fill():
        L.check(lib.bdm_mesh_fill_holes(B, 0, L.ptr(verts), L.ptr(attrs), L.ptr(faces), vf, ff, ovf.data_ptr(), off.data_ptr(), L.ptr(verts_out),
                                        L.ptr(attrs_out), L.ptr(faces_out), L.ptr(ws), L.stream()), "mesh_fill_holes")
    fill_only = timed_ms(fill, repeats)

    out_v, out_f = MF.fill_holes((verts_list, faces_list), cap)
    before = [mesh_stats(v.cpu(), f.cpu()) for v, f in zip(verts_list, faces_list)]
    after = [mesh_stats(v.cpu(), f.cpu()) for v, f in zip(out_v, out_f)]
    frac = lambda rows: round(sum(r["open_edges"] for r in rows) / max(sum(r["edges"] for r in rows), 1), 5)   # noqa: E731
    return {"meshes": B, "points": N, "resolution": resolution, "support": support, "max_hole_edges": cap, "vertices": sum_v, "faces": sum_f,
            "repeats": repeats, "info": info, "open_edge_fraction_before": frac(before), "open_edge_fraction_after": frac(after),
            "doubling_rounds": lib.bdm_mesh_fill_variant(B, ff) & 255,
            "fill_holes_ms": whole, "boundary_loops_call_ms": loops, "fill_call_ms": fill_only, "adjacency_ms": adj, "mesher_ms": mesher,
            "loops_plus_fill_over_adjacency": round((loops["median"] + fill_only["median"]) / adj["median"], 3),
            "fill_holes_over_mesher": round(whole["median"] / mesher["median"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--max-hole-edges", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"device": torch.cuda.get_device_name(0),
           "spheres_4096_R64_s3": run(args.batch, 4096, 64, 3, args.max_hole_edges, args.repeats),
           "spheres_600_R32_s2": run(args.batch, 600, 32, 2, args.max_hole_edges, args.repeats)}
    print(json.dumps(out))
