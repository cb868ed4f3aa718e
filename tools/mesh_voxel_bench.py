"""Times voxelize_meshes (the frame read-back + bdm_mesh_voxelize) and the bdm_mesh_voxelize call alone at several resolutions, beside
the mesher that made the batch and point_mesh_sqdist against a 4096-point cloud per mesh, everything in one run (DESIGN.md section
25).  Times as tools/mesh_fill_bench.py takes them: the median of the timed calls, HIP events around each call, after warm-up, with the
fastest and the slowest beside it.

  Workload: B meshes from reconstruct_surface of 4096-point spheres at 64^3, support 3.

    python tools/mesh_voxel_bench.py [--batch 16] [--repeats 30] [--resolutions 32 64 128]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import mesh_voxel as MV  # noqa: E402
from bdm_amd.ragged import pack_meshes  # noqa: E402
from tools.mesh_fill_bench import sphere_clouds, timed_ms  # noqa: E402


def run(B, N, resolution, support, resolutions, repeats):
    from bdm_amd.mesh_metrics import point_mesh_sqdist
    from bdm_amd.surface import reconstruct_surface
    pts, normals = sphere_clouds(B, N, seed=1)
    verts_list, faces_list = reconstruct_surface(pts, normals, resolution=resolution, support=support)
    mesher = timed_ms(lambda: reconstruct_surface(pts, normals, resolution=resolution, support=support), repeats)
    cloud = sphere_clouds(B, 4096, seed=2)[0]
    scorer = timed_ms(lambda: point_mesh_sqdist((verts_list, faces_list), cloud), repeats)
    out = {"meshes": B, "points": N, "resolution": resolution, "support": support, "vertices": sum(int(v.shape[0]) for v in verts_list),
           "faces": sum(int(f.shape[0]) for f in faces_list), "repeats": repeats, "mesher_ms": mesher, "point_mesh_sqdist_ms": scorer}
    verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
    sum_v, sum_f, lib = int(vert_first[-1]), int(face_first[-1]), L.lib()
    for R in resolutions:
        origin, cell = MV._cube_frame(MV._bounds(verts_list), R)
        whole = timed_ms(lambda: MV.voxelize_meshes((verts_list, faces_list), R), repeats)
        call = timed_ms(lambda: MV._voxelize(verts_list, faces_list, R, origin, cell, "vote", True), repeats)
        occ, axes = (torch.empty(B, R, R, R, dtype=torch.uint8, device="cuda") for _ in range(2))
        cnt = torch.empty(B, 8, dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.bdm_mesh_voxelize_workspace_bytes(B, sum_v, sum_f, R), dtype=torch.uint8, device="cuda")
        o, h = torch.from_numpy(origin), torch.from_numpy(cell)

        def bare():
            L.check(lib.bdm_mesh_voxelize(B, R, 0, o.data_ptr(), h.data_ptr(), L.ptr(verts), L.ptr(faces), vert_first.data_ptr(),
                                          face_first.data_ptr(), L.ptr(occ), L.ptr(axes), L.ptr(cnt), L.ptr(ws), L.stream()), "mesh_voxelize")
        abi = timed_ms(bare, repeats)
        _, info = MV.voxelize_meshes((verts_list, faces_list), R, return_info=True)
        counts = {k: int(v.sum()) for k, v in info["counts"].items()}
        assert torch.equal(cnt.cpu().long().sum(0), torch.tensor(list(counts.values())))
        out[f"voxelize_at_{R}"] = {"voxelize_meshes_ms": whole, "call_with_packing_ms": call, "abi_call_ms": abi, "counts": counts,
                                   "occupied_fraction": round(counts["occupied"] / (B * R ** 3), 5),
                                   "call_over_mesher": round(call["median"] / mesher["median"], 3),
                                   "call_over_scorer": round(call["median"] / scorer["median"], 3)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[32, 64, 128])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    result = {"device": torch.cuda.get_device_name(0), "spheres_4096_R64_s3": run(args.batch, 4096, 64, 3, args.resolutions, args.repeats)}
    print(json.dumps(result))
