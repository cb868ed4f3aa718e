"""Times the mesh renderer (render_mesh_batch over bdm_render_meshes) at 224 x 224 beside the only renderer the
project had before it, render_pointcloud_batch_pytorch3d on the same meshes' vertices as a cloud:
  B = 16 meshes of reconstruct_surface from 4096-point ellipsoids at R = 64, B = 16 from 16384-point ellipsoids at R = 128, and 30
  orbit frames of one of the large meshes.

HIP events around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows divided by the launches,
the functions alternating in one run (the figure to read is the ratio in the same run).  Per row:
  mesh_smooth   render_mesh_batch(shading="smooth"): vertex normals and Lambert colours in torch, then the kernels, image only
  mesh_kernels  bdm_render_meshes alone on preallocated buffers with those colours, image only
  mesh_raster   the same call with every output NULL: offsets, key preset, vertex and raster kernels, no resolve
  points        render_pointcloud_batch_pytorch3d of the vertices (padded to the longest mesh by repeating a vertex), black points
`fragments` is 2 x the covered pixels: these shapes are closed and convex, so every covered pixel has one front and one back
fragment; the raster kernel skips the atomic of a fragment that has already lost, so fragments / mesh_raster time bounds the atomic
rate from above.  One JSON line.

    python tools/mesh_render_bench.py [--repeats 7] [--launches 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import render as R  # noqa: E402
from bdm_amd import surface as S  # noqa: E402
from bdm_amd.cameras import Meshes, OrthographicCameras, Pointclouds, join_cameras, look_at_view_transform, r2n2_camera  # noqa: E402

SIZE = 224


def window_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def ellipsoid_meshes(b, n, resolution, generator):
    """b ellipsoids of random axes with their analytic outward normals, meshed."""
    d = torch.nn.functional.normalize(torch.randn(b, n, 3, device="cuda", generator=generator), dim=-1)
    axes = 0.2 + 0.3 * torch.rand(b, 1, 3, device="cuda", generator=generator)
    verts, faces = S.reconstruct_surface((d * axes).contiguous(), torch.nn.functional.normalize(d / axes, dim=-1).contiguous(),
                                         resolution=resolution, support=3)
    return Meshes(verts, faces)


def row(name, meshes, cameras, args):
    lib = L.lib()
    B = len(meshes)
    cameras = join_cameras(cameras)
    verts, faces = torch.cat(meshes.verts_list()).contiguous(), L.i32(torch.cat(meshes.faces_list()))
    nv, nf = [int(v.shape[0]) for v in meshes.verts_list()], [int(f.shape[0]) for f in meshes.faces_list()]
    vert_first, face_first = torch.tensor([0] + nv).cumsum(0), torch.tensor([0] + nf).cumsum(0)
    normals = meshes.verts_normals_packed() * (-1.0 if cameras.orthographic else 1.0)   # as render_mesh_batch hands them over
    colours = torch.cat([R.shade_by_normals(v[None], n[None], R._camera_row(cameras, i), two_sided=False)[0]
                         for i, (v, n) in enumerate(zip(meshes.verts_list(), torch.split(normals, nv)))]).float().contiguous()
    cams, bg = cameras.packed().cuda(), torch.tensor(R.BACKGROUND, device="cuda")
    image = torch.empty(B, SIZE, SIZE, 3, device="cuda")
    ws = torch.empty(lib.bdm_render_meshes_workspace_bytes(B, sum(nv), sum(nf), SIZE, SIZE), dtype=torch.uint8, device="cuda")
    ortho = int(cameras.orthographic)

    def kernels(out=image):
        L.check(lib.bdm_render_meshes(B, SIZE, SIZE, 3, ortho, 0, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(),
                                      L.ptr(cams), L.ptr(colours), None, L.ptr(bg), None, None, None, L.ptr(out), L.ptr(ws), L.stream()), "render_meshes")

    longest = max(nv)
    cloud = Pointclouds(torch.stack([torch.cat([v, v[-1:].expand(longest - v.shape[0], 3)]) for v in meshes.verts_list()]).contiguous())
    calls = {"mesh_smooth": lambda: R.render_mesh_batch(cameras, meshes, SIZE), "mesh_kernels": kernels, "mesh_raster": lambda: kernels(None),
             "points": lambda: R.render_pointcloud_batch_pytorch3d(cameras, cloud, SIZE)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    covered = int((R.rasterize_meshes(cameras, meshes, SIZE).pix_to_face >= 0).sum())
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k, fn in calls.items():                                # alternating: all see the same machine
            times[k].append(window_ms(fn, args.launches))
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    return {"row": name, "meshes": B, "vertices": sum(nv), "faces": sum(nf), "covered_pixels": covered, "fragments": 2 * covered,
            **{f"{k}_ms": round(v, 4) for k, v in med.items()},
            "mesh_smooth_ms_min_max": [round(min(times["mesh_smooth"]), 4), round(max(times["mesh_smooth"]), 4)],
            "mesh_smooth_over_points": round(med["mesh_smooth"] / med["points"], 3), "mesh_kernels_over_points": round(med["mesh_kernels"] / med["points"], 3),
            "faces_per_s_raster": sum(nf) / (med["mesh_raster"] * 1e-3), "atomics_per_s_upper_bound": 2 * covered / (med["mesh_raster"] * 1e-3)}


def rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    out = []
    large = None
    for b, n, res in ((16, 4096, 64), (16, 16384, 128)):
        meshes = ellipsoid_meshes(b, n, res, gen)
        cameras = [r2n2_camera(20.0 * i, 25.0, 1.5).to("cuda") for i in range(b)]
        out.append(row(f"b{b}_n{n}_R{res}", meshes, cameras, args))
        large = meshes
    frames = 30
    Rm, T = look_at_view_transform(dist=10.0, elev=30, azim=list(range(0, 360, 360 // frames)), degrees=True, device="cuda")
    orbit = Meshes(large.verts_list()[:1] * frames, large.faces_list()[:1] * frames)
    out.append(row("orbit_30_frames_n16384_R128", orbit, OrthographicCameras(focal_length=1.0, R=Rm, T=T, device="cuda"), args))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "image": SIZE, "rows": rows(args)}))
