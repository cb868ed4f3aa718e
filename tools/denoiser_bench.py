"""tools/denoiser_bench.py -- one denoiser forward of each PointCloudModel type at B = 16, N = 4096, S = 387 (device events, after
a warm-up), the fused simple layer kernel alone, and the simple model's layers composed of existing operators (pointwise_conv +
bdm_layer_norm_channels + torch pooling / gate) for comparison.  Procedural weights.

    python tools/denoiser_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bdm_amd import _lib as L  # noqa: E402
from bdm_amd import ops  # noqa: E402
from bdm_amd.model import PointCloudModel  # noqa: E402
from bdm_amd.utils.procedural import fill_module_  # noqa: E402

B, N, S = 16, 4096, 387
PEAK_TF = 157.3  # fp32 matrix peak of the MI355X (dense, TFLOP/s)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def composed_simple(net, x_in, t):
    """The same network from existing operators: the hidden layers (512 wide) go through memory."""
    pk = net._weight_packs()
    tp = net.timestep_projection
    te = ops.time_embedding(t, tp[0].weight, tp[0].bias, tp[2].weight, tp[2].bias)
    bb = ops.pointwise_conv(te[:, :, None], pk["w_t"], net.input_projection.bias)
    pe = [x_in[:, :3]]
    for f in net.positional_encoding.freq_bands:
        pe += [torch.sin(f * x_in[:, :3]), torch.cos(f * x_in[:, :3])]
    W = net.input_projection.weight
    kin = W.shape[1] - net.timestep_embed_dim
    x = ops.pointwise_conv(torch.cat([x_in] + pe, dim=1), W[:, :kin].contiguous(), batch_bias=bb)
    lib = L.lib()
    for ff in net.layers:
        xin = torch.cat([x, x.amax(dim=2, keepdim=True).expand_as(x), x.std(dim=2, keepdim=True).expand_as(x)], dim=1).contiguous()
        h = torch.empty_like(xin)
        L.check(lib.bdm_layer_norm_channels(B, xin.shape[1], N, L.ptr(xin), L.ptr(ff.layernorm.weight), L.ptr(ff.layernorm.bias),
                                            L.c_float(1e-5), L.ptr(h), L.stream()), "layer_norm_channels")
        g = F.silu(ops.pointwise_conv(h, ff.layer1.weight)) * ops.pointwise_conv(h, ff.linear_v.weight)
        x = ops.pointwise_conv(g, ff.layer2.weight, residual=x)
    return ops.pointwise_conv(x, net.output_projection.weight, net.output_projection.bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3 + S, N, generator=g)
    x[:, :3] *= 0.5
    x = x.to(dev)
    t = torch.arange(B, device=dev) * 60 + 7
    res = {"B": B, "N": N, "S": S, "iters": args.iters}
    nets = {}
    for kind in ("pvcnn", "simple", "pvcnnplusplus"):
        net = fill_module_(PointCloudModel(model_type=kind, in_channels=3 + S).eval(), seed=1).to(dev).model
        nets[kind] = net
        res[f"{kind}_forward_ms"] = round(timed(lambda: net(x, t), args.iters), 4)
    simple = nets["simple"]
    res["simple_composed_forward_ms"] = round(timed(lambda: composed_simple(simple, x, t), args.iters), 4)
    y_f, y_c = simple(x, t), composed_simple(simple, x, t)
    res["simple_composed_rel_l2"] = float((y_f - y_c).norm() / y_c.norm())
    # the fused layer kernel alone, for timing only: layer 0's operands on a random input xs, with the per-shape state of a
    # different input (the partials one forward left); the FLOP count is the folded form's, the prologue kernel is not counted
    simple(x, t)
    pk, lib = simple._weight_packs(), L.lib()
    part = ops.workspace(lib.bdm_simple_partials_bytes(B, N), dev, "simple_partials")
    state = torch.zeros(lib.bdm_simple_state_elems(B), device=dev)
    L.check(lib.bdm_simple_layer_prep(B, N, L.ptr(part), L.ptr(pk["layers"][0][3]), L.ptr(state), L.stream()), "prep")
    xs, ys = torch.randn(B, 128, N, device=dev), torch.empty(B, 128, N, device=dev)
    a1, av, a2, _, vec = pk["layers"][0]
    layer = lambda: L.check(lib.bdm_simple_layer(B, N, L.ptr(xs), L.ptr(state), L.ptr(a1), L.ptr(av), L.ptr(a2), L.ptr(vec),  # noqa: E731
                                                 L.ptr(ys), L.ptr(part), L.stream()), "layer")
    ms = timed(layer, args.iters)
    flop = 2.0 * B * N * (128 * 1024 + 512 * 128)   # the folded form the kernel executes
    res["simple_layer_kernel_ms"] = round(ms, 4)
    res["simple_layer_tflops"] = round(flop / ms / 1e9, 2)
    res["simple_layer_share_of_fp32_matrix_peak"] = round(flop / ms / 1e9 / PEAK_TF, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
