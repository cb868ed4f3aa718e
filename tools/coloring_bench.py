"""tools/coloring_bench.py -- the colouring model's transformer at B = 16, N = 4096: one forward (conditioned input -> colours), the
fused tail kernel alone (bdm_color_block_tail, colour-head form and next-norm form), and the same second half composed from
existing launches (bdm_simple_add, bdm_layer_norm_channels, two bdm_pointwise_conv, output projection + denormalisation) as the
yardstick.  Median of --iters single-launch timings between HIP events after a warm-up, one process.  Procedural weights.

    python tools/coloring_bench.py [--iters 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdm_amd import transformer as T  # noqa: E402
from bdm_amd.utils.procedural import fill_module_  # noqa: E402

B, N, E, C_IN = 16, 4096, 64, 390


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda")
    net = fill_module_(T.PointCloudTransformerModel(num_layers=max(a.layers, 2), in_channels=C_IN, out_channels=3, embed_dim=E).eval(),
                       seed=0).to(dev)
    one = fill_module_(T.PointCloudTransformerModel(num_layers=a.layers, in_channels=C_IN, out_channels=3, embed_dim=E).eval(),
                       seed=0).to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C_IN, N, generator=g)
    x[:, :3] *= 0.5
    x = x.to(dev).transpose(1, 2)   # the conditioning gather's channel-first tensor seen as (B, N, C)
    h, p = torch.randn(B, E, N, generator=g).to(dev), torch.randn(B, E, N, generator=g).to(dev)
    blk, head, nxt = net.blocks[0], (net.output_projection, 0.5, 0.5), net.blocks[1].norm0
    act = B * E * N * 4   # bytes of one (B, E, N) tensor
    res = {"B": B, "N": N, "layers": a.layers, "iters": a.iters}
    default = T.TAIL_IMPL
    for impl in ("fused", "composed"):
        T.TAIL_IMPL = impl
        res[f"forward_{impl}_ms"] = median_ms(lambda: one.forward_colors(x, 0.5, 0.5), a.iters)
        res[f"tail_{impl}_colors_ms"] = median_ms(lambda: blk.tail(h, p, head=head), a.iters)
        res[f"tail_{impl}_ln_next_ms"] = median_ms(lambda: blk.tail(h, p, next_norm=nxt), a.iters)
    T.TAIL_IMPL = default
    # bytes through HBM (activations; the 128 KB of weights stay in cache).  fused: read h, p; write y and ln_next | colours.
    # composed: add (2 r + 1 w), norm2 (1 + 1), fc1 (1 r + 4 w), fc2 (4 r + 1 r residual + 1 w), then norm (1 + 1) | head (1 r + colours x 3 passes)
    col = B * N * 3 * 4
    res["bytes_fused_colors"], res["bytes_fused_ln_next"] = 3 * act + col, 4 * act
    res["bytes_composed_colors"], res["bytes_composed_ln_next"] = 17 * act + 5 * col, 18 * act
    for k in ("colors", "ln_next"):
        res[f"fused_{k}_GBps"] = res[f"bytes_fused_{k}"] / res[f"tail_fused_{k}_ms"] * 1e-6
        res[f"fused_{k}_TFLOPs"] = 2.0 * B * N * 2 * E * 4 * E / res[f"tail_fused_{k}_ms"] * 1e-9
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
