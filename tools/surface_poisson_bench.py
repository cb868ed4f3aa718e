"""Times the Poisson mesher (reconstruct_surface(method="poisson"): bdm_surface_poisson_grid + bdm_surface_extract, DESIGN.md
section 26) beside the IMLS mesher of section 16 on B = 16 ellipsoids of N = 4096 points at R = 64 and of N = 16384 points at
R = 128, support 3, the default number of V-cycles.

HIP events around `--launches` back-to-back calls after a warm-up, the median of `--repeats` such windows divided by the launches,
all functions alternating in one run (the figure to read is the ratio in the same run).  Both reconstruct_surface forms read the
counts between their two ABI calls, so their windows contain one host synchronisation per call.  The Poisson grid call is also timed
alone and in its three parts (bdm_surface_poisson_grid_staged: splat = frame, memset, splat, divergence; solve; hand-over = maximum,
samples, level, hand-over, the two separation passes and the mark stage), and the solve with the LDS tail against the same solve run one launch per level and
operator; the two forms' phi are compared bit for bit first.  Every figure comes with its number of launches (memsets included).
One JSON line.

    python tools/surface_poisson_bench.py [--repeats 7] [--launches 10] [--cycles C]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import surface as S  # noqa: E402

TAIL_SIDE, COARSEST, SEPARATE = 20, 32, 2


def window_ms(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def shapes(b, n, generator):
    """b ellipsoids of random axes with their analytic outward normals."""
    d = torch.nn.functional.normalize(torch.randn(b, n, 3, device="cuda", generator=generator), dim=-1)
    axes = 0.2 + 0.3 * torch.rand(b, 1, 3, device="cuda", generator=generator)
    return (d * axes).contiguous(), torch.nn.functional.normalize(d / axes, dim=-1).contiguous()


def launch_counts(R, cycles):
    """Launches (memsets included) of the parts of one grid call, from the schedule of bdm_hip.h section 22."""
    sides = [R]
    while sides[-1] % 2 == 0 and sides[-1] > 4:
        sides.append(sides[-1] // 2)
    glob = sum(1 for m in sides if m > TAIL_SIDE)
    tail = cycles * (6 * glob + 1) if glob else 1
    per_level = cycles * (6 * (len(sides) - 1) + COARSEST)
    return {"splat": 4, "solve": tail, "solve_per_level": per_level, "handover": 8 + SEPARATE, "poisson_grid": 12 + SEPARATE + tail, "imls_grid": 7, "extract": 2}


def rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = L.lib()
    out = []
    for b, n, R, s in ((16, 4096, 64, 3), (16, 16384, 128, 3)):
        pts, nrm = shapes(b, n, gen)
        head = lib.bdm_surface_workspace_bytes(b, n, R, s)
        ws = torch.empty(lib.bdm_surface_poisson_workspace_bytes(b, n, R, s), dtype=torch.uint8, device="cuda")
        counts = torch.empty(b, 4, dtype=torch.int32, device="cuda")
        info = torch.empty(b, 3, dtype=torch.int32, device="cuda")
        r3 = 4 * b * R ** 3

        def staged(stages, per_level=0):
            L.check(lib.bdm_surface_poisson_grid_staged(b, n, R, s, args.cycles, stages, per_level, L.ptr(pts), L.ptr(nrm), L.ptr(counts), L.ptr(info),
                                                        L.ptr(ws), L.stream()), "surface_poisson_grid_staged")

        def phi():
            return ws[head + 5 * r3:head + 6 * r3].view(torch.int32).clone()

        staged(3, 1)
        per_level_phi = phi()
        staged(7, 0)
        same_bits = bool(torch.equal(per_level_phi, phi()))
        host = counts.cpu()
        nv, nf = host[:, 0].long(), host[:, 1].long()
        offsets = torch.stack([torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf]).cuda()
        verts = torch.empty(int(nv.sum()), 3, dtype=torch.float32, device="cuda")
        faces = torch.empty(int(nf.sum()), 3, dtype=torch.int32, device="cuda")

        def extract():
            L.check(lib.bdm_surface_extract(b, n, R, s, L.ptr(offsets[0]), L.ptr(offsets[1]), L.ptr(verts), L.ptr(faces), L.ptr(ws), L.stream()),
                    "surface_extract")

        imls_ws = torch.empty(head, dtype=torch.uint8, device="cuda")          # its own: the marks in `ws` stay the Poisson mesh's
        imls_counts = torch.empty(b, 4, dtype=torch.int32, device="cuda")

        def imls_grid():
            L.check(lib.bdm_surface_grid(b, n, R, s, 0.0, L.ptr(pts), L.ptr(nrm), L.ptr(imls_counts), L.ptr(imls_ws), L.stream()), "surface_grid")

        imls = S.reconstruct_surface(pts, nrm, resolution=R, support=s, return_info=True)
        # the solve's stages continue from the workspace: their arithmetic does not depend on the values, so the time does not either
        calls = {"imls_reconstruct": lambda: S.reconstruct_surface(pts, nrm, resolution=R, support=s),
                 "poisson_reconstruct": lambda: S.reconstruct_surface(pts, nrm, resolution=R, support=s, method="poisson", cycles=args.cycles),
                 "imls_grid": imls_grid, "poisson_grid": lambda: staged(7), "splat": lambda: staged(1), "solve": lambda: staged(2),
                 "solve_per_level": lambda: staged(2, 1), "handover": lambda: staged(4)}
        for fn in calls.values():
            fn()
        calls["extract"] = extract
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():                         # alternating: all see the same machine
                if name == "extract":
                    staged(7)       # the staged solves above moved phi on: the marks must again be those the offsets were read from
                times[name].append(window_ms(fn, args.launches))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        out.append({"clouds": b, "points": n, "resolution": R, "support": s, "cycles": args.cycles, "vertices": int(nv.sum()), "faces": int(nf.sum()),
                    "skipped_quads": int(host[:, 2].sum()), "imls_vertices": int(imls[2]["counts"][:, 0].sum()),
                    "imls_skipped_quads": int(imls[2]["counts"][:, 2].sum()), "per_level_phi_has_the_same_bits": same_bits,
                    **{f"{name}_ms": round(v, 4) for name, v in med.items()},
                    "min_max_ms": {name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
                    "launches": launch_counts(R, args.cycles),
                    "poisson_over_imls_reconstruct": round(med["poisson_reconstruct"] / med["imls_reconstruct"], 4),
                    "tail_over_per_level_solve": round(med["solve"] / med["solve_per_level"], 4)})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--cycles", type=int, default=S.DEFAULT_CYCLES)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "rows": rows(args)}))
