"""Times bdm_render_points on the GPU: image-only calls at B = 16, 224^2, k = 10 for N = 4096 and N = 16384,
and 30 orbit frames of one N = 16384 cloud (one call over 30 orthographic cameras).  Median of the timed repeats, HIP events around
each repeat, after warm-up.  Beside each time: the bytes the call MUST move (points, cameras, features in; the image out -- the
projected-point workspace and the per-tile re-reads of it are the implementation's own traffic and are not counted) and the
fraction of the 8 TB/s HBM figure DESIGN.md uses that this is at the measured time.

    python tools/render_bench.py [--repeats 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd.cameras import OrthographicCameras, join_cameras, look_at_view_transform, r2n2_camera  # noqa: E402
from bdm_amd.render import BACKGROUND, _render  # noqa: E402

HBM_PEAK = 8.0e12


def median_ms(fn, repeats, warmup=3):
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
    return sorted(times)[len(times) // 2]


def must_move_bytes(B, N, H, W, C=3):
    return 4 * (B * N * 3 + B * 16 + B * N * C + C + B * H * W * C)


def row(name, cams, pts, feats, repeats, size=224, k=10, radius=0.01):
    B, N = pts.shape[:2]
    ms = median_ms(lambda: _render(cams, pts, size, radius, k, feats, BACKGROUND, "norm_weighted", fragments=False), repeats)
    image = _render(cams, pts, size, radius, k, feats, BACKGROUND, "norm_weighted", fragments=False)[1]
    covered = float((image != torch.tensor(BACKGROUND, device=image.device)).any(-1).float().mean())
    nbytes = must_move_bytes(B, N, size, size)
    return {"case": name, "shapes": B, "points": N, "image": size, "k": k, "ms_per_call": round(ms, 4), "must_move_bytes": nbytes,
            "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), "covered_pixel_fraction": round(covered, 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for N in (4096, 16384):   # the synthetic shapes of bdm_amd/data.py: a Gaussian cloud of std 0.15 seen from an R2N2-style camera
        pts = torch.randn(16, N, 3, device="cuda", generator=gen) * 0.15
        feats = torch.rand(16, N, 3, device="cuda", generator=gen)
        cams = join_cameras([r2n2_camera(22.5 * i, 27.0, 1.4) for i in range(16)]).to("cuda")
        rows.append(row(f"image-only B=16 N={N}", cams, pts, feats, args.repeats))
    F = 30
    Rm, T = look_at_view_transform(dist=10.0, elev=30, azim=list(range(0, 360, 360 // F)))
    pts = (torch.randn(1, 16384, 3, device="cuda", generator=gen) * 0.8).tile(F, 1, 1)
    feats = torch.rand(1, 16384, 3, device="cuda", generator=gen).tile(F, 1, 1)
    rows.append(row("30 orbit frames N=16384", OrthographicCameras(focal_length=0.25, R=Rm, T=T).to("cuda"), pts, feats, args.repeats))
    for r in rows:
        print(json.dumps(r))
