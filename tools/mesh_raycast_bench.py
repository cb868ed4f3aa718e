"""Times the hierarchy build (build_bvh: keys, torch's stable sort, tree and boxes) and the three queries of bdm_amd/mesh_raycast.py on
two ray bundles, with the tree and exhaustively, beside rasterize_meshes at the same image size and point_mesh_sqdist on the same
meshes, everything in one run.  Times as tools/mesh_fill_bench.py takes them: the median of the timed calls,
HIP events around each call, after warm-up, with the fastest and the slowest beside it.

  Workload: B meshes from reconstruct_surface of 4096-point spheres at 64^3, support 3.
  Coherent bundle: the image x image pixel rays of one r2n2 camera per mesh (closest hit).
  Incoherent bundle: the ambient-occlusion rays, `samples` per vertex over the hemisphere of its normal (occlusion).

    python tools/mesh_raycast_bench.py [--batch 16] [--repeats 20] [--slow-repeats 3] [--image 224] [--samples 32]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import mesh_raycast as MR  # noqa: E402
from tools.mesh_fill_bench import sphere_clouds, timed_ms  # noqa: E402


def ao_rays(verts_list, faces_list, samples):
    """The rays vertex_ambient_occlusion casts, as lists."""
    from bdm_amd.cameras import Meshes
    table = MR.fibonacci_sphere(samples).cuda()
    normals = Meshes(verts_list, faces_list).verts_normals_packed()
    lift = MR._diagonals(verts_list) * 1e-4
    origins, dirs, start = [], [], 0
    for m, v in enumerate(verts_list):
        n = normals[start:start + v.shape[0]]
        start += v.shape[0]
        s = n @ table.t()
        d = torch.where((s < 0)[:, :, None], -table[None], table[None].expand(v.shape[0], samples, 3))
        origins.append((v + lift[m] * n)[:, None, :].expand(-1, samples, -1).reshape(-1, 3).contiguous())
        dirs.append(d.reshape(-1, 3).contiguous())
    return origins, dirs


def run(B, N, resolution, support, image, samples, repeats, slow_repeats):
    from bdm_amd.cameras import Meshes, join_cameras, r2n2_camera
    from bdm_amd.mesh_metrics import point_mesh_sqdist
    from bdm_amd.render import rasterize_meshes
    from bdm_amd.surface import reconstruct_surface
    pts, normals = sphere_clouds(B, N, seed=1)
    verts_list, faces_list = reconstruct_surface(pts, normals, resolution=resolution, support=support)
    meshes, drawn = (verts_list, faces_list), Meshes(list(verts_list), list(faces_list))
    cloud = sphere_clouds(B, 4096, seed=2)[0]
    cameras = join_cameras([r2n2_camera(30.0 + 20.0 * i, 25.0, 1.4) for i in range(B)]).to("cuda")
    out = {"meshes": B, "points": N, "resolution": resolution, "support": support, "vertices": sum(int(v.shape[0]) for v in verts_list),
           "faces": sum(int(f.shape[0]) for f in faces_list), "image": image, "samples": samples, "repeats": repeats, "slow_repeats": slow_repeats,
           "point_mesh_sqdist_ms": timed_ms(lambda: point_mesh_sqdist(meshes, cloud), repeats),
           "rasterize_meshes_ms": timed_ms(lambda: rasterize_meshes(cameras, drawn, image), repeats),
           "build_bvh_ms": timed_ms(lambda: MR.build_bvh(meshes), repeats)}
    bvh = MR.build_bvh(meshes)
    co, cd = MR.camera_rays(cameras, image)
    ao, ad = ao_rays(verts_list, faces_list, samples)
    for name, o, d, fn in (("camera", co, cd, MR.cast_rays), ("ao", ao, ad, MR.test_occlusions)):
        rays = int(o.shape[0] * o.shape[1]) if torch.is_tensor(o) else sum(int(x.shape[0]) for x in o)
        tree = timed_ms(lambda: fn(bvh, o, d), repeats)
        flat = timed_ms(lambda: fn(bvh, o, d, exhaustive=True), slow_repeats, warmup=1)
        a, b = fn(bvh, o, d), fn(bvh, o, d, exhaustive=True)
        if fn is MR.cast_rays:
            same = torch.equal(a.t, b.t) and torch.equal(a.face_idx, b.face_idx)
            hit = float((a.face_idx >= 0).float().mean())
        else:
            same = all(torch.equal(x, y) for x, y in zip(a, b))
            hit = float(torch.cat(a).float().mean())
        assert same, f"{name}: the tree changes an answer"
        out[f"{name}_rays"] = {"rays": rays, "tree_ms": tree, "exhaustive_ms": flat, "hit_fraction": round(hit, 5),
                               "mrays_per_s_tree": round(rays / tree["median"] / 1e3, 1),
                               "exhaustive_over_tree": round(flat["median"] / tree["median"], 1)}
    out["camera_tree_over_rasterize"] = round(out["camera_rays"]["tree_ms"]["median"] / out["rasterize_meshes_ms"]["median"], 3)
    out["ao_total_over_point_mesh_sqdist"] = round((out["build_bvh_ms"]["median"] + out["ao_rays"]["tree_ms"]["median"]) / out["point_mesh_sqdist_ms"]["median"], 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--slow-repeats", type=int, default=3, help="timed calls of the exhaustive forms")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--samples", type=int, default=32)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    result = {"device": torch.cuda.get_device_name(0),
              "spheres_4096_R64_s3": run(args.batch, 4096, 64, 3, args.image, args.samples, args.repeats, args.slow_repeats)}
    print(json.dumps(result))
