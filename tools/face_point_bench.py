"""Times the face-to-point distance (bdm_face_point_distance) on the mesh metrics' benchmark shapes -- B = 16
ellipsoid clouds of 4096 points meshed at R = 64 and of 16384 points at R = 128 (support 3), and 8192 points at R = 96 between them --
and on one small-mesh workload where the resident form leaves the chip empty: B = 2 clouds of 16384 points meshed at R = 16.  Every
mesh is scored against the cloud it was made from.

The resident form, the split form (at the chooser's count and at every power of two up to the tile count) and
bdm_point_mesh_distance on the same meshes and points alternate in one run: HIP events
around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows divided by the launches, with the
minimum and the maximum.  Both directions evaluate the same (point, face) pairs, so pairs per second compare directly.  The ABI
calls run on preallocated outputs and workspaces.  One JSON line.

    python tools/face_point_bench.py [--repeats 7] [--launches 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import surface as S  # noqa: E402
from bdm_amd.ragged import first, pack_meshes  # noqa: E402

TILE, THREADS = 1024, 256


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


def rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.lib()
    out = []
    for b, n, R, s in ((16, 4096, 64, 3), (16, 8192, 96, 3), (16, 16384, 128, 3), (2, 16384, 16, 3)):
        pts, nrm = shapes(b, n, gen)
        verts_list, faces_list = S.reconstruct_surface(pts, nrm, resolution=R, support=s)
        verts, faces, vert_first, face_first = pack_meshes(verts_list, faces_list)
        point_first = first([n] * b)
        sum_f = int(face_first[-1])
        workgroups = sum(-(-int(f.shape[0]) // THREADS) for f in faces_list)
        sizes = (b, sum_f, b * n, n, workgroups)
        variant, chooser_chunks = int(lib.bdm_face_point_distance_variant(*sizes)), int(lib.bdm_face_point_distance_chunks(*sizes))
        tiles = -(-n // TILE)
        ws_f = torch.empty(lib.bdm_face_point_distance_workspace_bytes(b, sum_f), dtype=torch.uint8, device="cuda")
        ws_p = torch.empty(lib.bdm_point_mesh_distance_workspace_bytes(b, sum_f), dtype=torch.uint8, device="cuda")
        fsq, fpt = torch.empty(sum_f, device="cuda"), torch.empty(sum_f, dtype=torch.int32, device="cuda")
        psq, pfi = torch.empty(b, n, device="cuda"), torch.empty(b, n, dtype=torch.int32, device="cuda")

        def face_side(form, chunks):
            L.check(lib.bdm_face_point_distance(b, form, chunks, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(),
                                                L.ptr(pts), point_first.data_ptr(), L.ptr(fsq), L.ptr(fpt), L.ptr(ws_f), L.stream()),
                    "face_point_distance")

        def point_side():
            L.check(lib.bdm_point_mesh_distance(b, n, 1, L.ptr(verts), L.ptr(faces), vert_first.data_ptr(), face_first.data_ptr(), L.ptr(pts),
                                                None, L.ptr(psq), L.ptr(pfi), L.ptr(ws_p), L.stream()), "point_mesh_distance")

        counts = sorted({2, chooser_chunks} | {c for c in (1, 2, 4, 8, 16) if c <= tiles})
        calls = {"resident": lambda: face_side(1, 0), "point_side": point_side}
        for c in counts:
            calls[f"split_{c}"] = lambda c=c: face_side(2, c)
        results = {}
        for name, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            if name != "point_side":
                results[name] = (fsq.clone(), fpt.clone())
            print(f"[{b} x {n}, R = {R}, {sum_f} faces] warmed up {name}", file=sys.stderr, flush=True)
        same_bits = all(torch.equal(r[0].view(torch.int32), results["resident"][0].view(torch.int32)) and torch.equal(r[1], results["resident"][1])
                        for r in results.values())
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():                         # alternating: all see the same machine
                times[name].append(window_ms(fn, args.launches))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        pairs = n * sum_f                                          # every point of a cloud against every face of its mesh
        out.append({"meshes": b, "points": n, "resolution": R, "faces": sum_f, "max_faces": max(int(f.shape[0]) for f in faces_list),
                    "resident_workgroups": workgroups, "tiles": tiles, "chooser": [variant, chooser_chunks], "forms_agree_bitwise": same_bits,
                    **{f"{name}_ms": [round(v, 4), round(min(times[name]), 4), round(max(times[name]), 4)] for name, v in med.items()},
                    "pairs": pairs, **{f"{name}_pairs_per_s": float(f"{pairs / (v * 1e-3):.4g}") for name, v in med.items()},
                    "resident_over_point_side": round(med["resident"] / med["point_side"], 3)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rows": rows(args)}))
