"""Times the mesh metrics (bdm_mesh_sample_points, bdm_point_mesh_distance) on the mesher's own benchmark
shapes: B = 16 ellipsoid clouds of 4096 points meshed at R = 64 and of 16384 points at R = 128 (support 3), as many query points and
samples per mesh as the cloud has points, the queries in their given order and in Morton order.

HIP events around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows divided by the launches,
all candidates alternating in one run (the figures to compare against are the two same-run columns reconstruct_ms and nn_sqdist_ms:
the mesher that made the meshes, and the cloud-to-cloud nearest neighbour at n = P, m = the mean face count).  The ABI calls run on
preallocated outputs and workspaces; reconstruct_surface contains one host synchronisation per call.

The culled form of the distance is not built (no margin keeps its bits), so there is no culled column.  What culling by tile boxes
COULD skip is reported from host arithmetic instead: `skippable_tiles_*` = the share of (wave of 64 threads, tile of 256 faces)
pairs in which every lane's FINAL squared distance is below the exact squared distance to the tile's bounding box -- an upper bound
of what any such cull reaches, since a real one compares against the running best, not the final one.  One JSON line.

    python tools/mesh_metrics_bench.py [--repeats 7] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import evaluation as E  # noqa: E402
from bdm_amd import mesh_metrics as MM  # noqa: E402
from bdm_amd import rng  # noqa: E402
from bdm_amd import surface as S  # noqa: E402
from bdm_amd.ragged import pack_meshes  # noqa: E402

TILE, WAVE = 256, 64


def window_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def shapes(b, n, generator):
    """b ellipsoids of random axes with their analytic outward normals (tools/surface_bench.py's shapes)."""
    d = torch.nn.functional.normalize(torch.randn(b, n, 3, device="cuda", generator=generator), dim=-1)
    axes = 0.2 + 0.3 * torch.rand(b, 1, 3, device="cuda", generator=generator)
    return (d * axes).contiguous(), torch.nn.functional.normalize(d / axes, dim=-1).contiguous()


def skippable_share(verts_list, faces_list, points, sqdist, order):
    """Host arithmetic (float64 torch): see the module docstring."""
    skipped = total = 0
    for m, (v, f) in enumerate(zip(verts_list, faces_list)):
        F = f.shape[0]
        if F == 0:
            continue
        tri = v.double()[f]                                              # (F, 3, 3)
        pad = (-F) % TILE
        tri = torch.cat([tri, tri[-1:].expand(pad, 3, 3)]).reshape(-1, TILE * 3, 3)
        lo, hi = tri.min(dim=1).values, tri.max(dim=1).values             # (T, 3)
        idx = order[m].long()
        p, best = points[m].double()[idx], sqdist[m].double()[idx]
        gap = torch.maximum(torch.maximum(lo[None] - p[:, None], p[:, None] - hi[None]), torch.zeros((), dtype=torch.float64, device=p.device))
        box = (gap * gap).sum(dim=2)                                      # (P, T)
        can = box > best[:, None]
        P = can.shape[0] - can.shape[0] % WAVE
        waves = can[:P].reshape(-1, WAVE, can.shape[1]).all(dim=1)
        skipped, total = skipped + int(waves.sum()), total + waves.numel()
    return skipped / max(total, 1)


def rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.lib()
    out = []
    for b, n, R, s in ((16, 4096, 64, 3), (16, 16384, 128, 3)):
        pts, nrm = shapes(b, n, gen)
        verts_list, faces_list = S.reconstruct_surface(pts, nrm, resolution=R, support=s)
        verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
        sum_f, max_f = int(face_first[-1]), int((face_first[1:] - face_first[:-1]).max())
        morton = MM.morton_order(pts).contiguous()
        natural = torch.arange(n, dtype=torch.int32, device="cuda").repeat(b, 1).contiguous()
        keys = torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in (rng.shape_key(0, m) for m in range(b))]).cuda()
        ws_s = torch.empty(lib.bdm_mesh_sample_workspace_bytes(b, sum_f, max_f), dtype=torch.uint8, device="cuda")
        ws_d = torch.empty(lib.bdm_point_mesh_distance_workspace_bytes(b, sum_f), dtype=torch.uint8, device="cuda")
        samples = torch.empty(b, n, 3, device="cuda")
        sq, fi = torch.empty(b, n, device="cuda"), torch.empty(b, n, dtype=torch.int32, device="cuda")
        targets = torch.rand(b, max(sum_f // b, 1), 3, device="cuda", generator=gen)

        def sample():
            L.check(lib.bdm_mesh_sample_points(b, n, max_f, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), L.ptr(keys),
                                               0, rng.MESH, L.ptr(samples), None, None, L.ptr(ws_s), L.stream()), "mesh_sample_points")

        def dist(order):
            L.check(lib.bdm_point_mesh_distance(b, n, 1, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), L.ptr(pts),
                                                L.ptr(order), L.ptr(sq), L.ptr(fi), L.ptr(ws_d), L.stream()), "point_mesh_distance")

        calls = {"sample": sample, "distance_exhaustive": lambda: dist(None), "distance_exhaustive_morton": lambda: dist(morton),
                 "reconstruct": lambda: S.reconstruct_surface(pts, nrm, resolution=R, support=s),
                 "nn_sqdist": lambda: E.nn_sqdist(pts, targets)}
        for name, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            print(f"[{b} x {n}, R = {R}, {sum_f} faces] warmed up {name}", file=sys.stderr, flush=True)
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():                         # alternating: all see the same machine
                times[name].append(window_ms(fn, args.launches))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        dist(None)
        torch.cuda.synchronize()
        pairs = n * sum_f                                          # every point of a mesh against every face of that mesh
        out.append({"meshes": b, "points": n, "resolution": R, "faces": sum_f, "max_faces": max_f,
                    **{f"{name}_ms": round(v, 4) for name, v in med.items()},
                    "distance_exhaustive_ms_min_max": [round(min(times["distance_exhaustive"]), 4), round(max(times["distance_exhaustive"]), 4)],
                    "pairs": pairs, "pairs_per_s": pairs / (med["distance_exhaustive"] * 1e-3),
                    "distance_over_reconstruct": round(med["distance_exhaustive"] / med["reconstruct"], 3),
                    "distance_over_nn_sqdist": round(med["distance_exhaustive"] / med["nn_sqdist"], 3),
                    "chooser_variant": int(lib.bdm_point_mesh_distance_variant(b, n, sum_f, 0)),
                    "skippable_tiles_natural": round(skippable_share(verts_list, faces_list, pts, sq, natural), 4),
                    "skippable_tiles_morton": round(skippable_share(verts_list, faces_list, pts, sq, morton), 4)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rows": rows(args)}))
