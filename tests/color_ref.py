"""TEST INFRASTRUCTURE: plain-torch restatement of the PC^2 colouring model's transformer (experiments/model/
point_cloud_transformer_model.py:13-80 with use_attn=False, model_coloring.py:37-65), driven by a state dict with the
reference's key names.  Every piece runs in the dtype it is given (float64 for the reference side of the tests, float32 for the
CPU yardsticks), except the inner PVCNN: that is oracle.ref_net.point_cloud_model_forward, whose native operators are float32.

    h = input_projection(x)
    per block:  h = h + PVCNN(norm0(h), t = 0);  h = h + fc2(gelu(fc1(norm2(h))))
    out = output_projection(h)            (`norm` is in the state dict and is NOT applied: reference quirk)

timm's Mlp is fc1 -> exact (erf) GELU -> fc2; LayerScale / DropPath are identities at the reachable defaults.

Also here: the elementwise error bound of the fused tail kernel (tail_bound), shared by the GPU test and its CPU mutants.
"""
import math

import torch

U = 2.0 ** -24   # unit roundoff of float32


def layer_norm(x, w, b, eps=1e-5, unbiased=False):
    """nn.LayerNorm over the last axis: biased variance, eps inside the root.  unbiased=True is the MUTANT (n - 1 divisor)."""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).sum(-1, keepdim=True) / (x.shape[-1] - (1 if unbiased else 0))
    return d / torch.sqrt(var + eps) * w.to(x.dtype) + b.to(x.dtype)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_tanh(x):
    """The MUTANT: the tanh approximation."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def linear(x, w, b):
    return x @ w.to(x.dtype).t() + b.to(x.dtype)


def mlp(sd, pre, x, gelu=gelu_erf):
    return linear(gelu(linear(x, sd[pre + "fc1.weight"], sd[pre + "fc1.bias"])), sd[pre + "fc2.weight"], sd[pre + "fc2.bias"])


def block_tail(sd, pre, h, p, gelu=gelu_erf, unbiased=False):
    """Second half of block `pre` ("blocks.0."): h, p (B, N, E) -> y (B, N, E)."""
    r = h + p
    return r + mlp(sd, pre + "mlp.", layer_norm(r, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], unbiased=unbiased), gelu)


def pvcnn(sd, pre, ln, dtype):
    """The block's PVCNN on its norm0 output (B, N, E), t = 0: float32 inside (the oracle's native operators), `dtype` out."""
    from oracle import ref_net
    sd32 = {k: v.float() for k, v in sd.items() if k.startswith(pre + "point_cloud_model.model.")}
    t = torch.zeros(ln.shape[0], dtype=torch.long)
    return ref_net.point_cloud_model_forward(sd32, ln.float().contiguous(), t, prefix=pre + "point_cloud_model.model.").to(dtype)


def block(sd, pre, h, pvcnn_input=None):
    """One block on h (B, N, E).  pvcnn_input (teacher forcing): the norm0 output the PVCNN is to see instead of this side's own."""
    ln = layer_norm(h, sd[pre + "norm0.weight"], sd[pre + "norm0.bias"])
    p = pvcnn(sd, pre, ln if pvcnn_input is None else pvcnn_input, h.dtype)
    return block_tail(sd, pre, h, p), ln, p


def num_layers(sd, prefix=""):
    return 1 + max(int(k[len(prefix) + 7:].split(".")[0]) for k in sd if k.startswith(prefix + "blocks."))


def transformer(sd, x, prefix="", trace=None):
    """x (B, N, in_channels) -> (B, N, out_channels) in x's dtype.  trace: receives per block (h, norm0(h), p, y)."""
    h = linear(x, sd[prefix + "input_projection.weight"], sd[prefix + "input_projection.bias"])
    for i in range(num_layers(sd, prefix)):
        y, ln, p = block(sd, f"{prefix}blocks.{i}.", h)
        if trace is not None:
            trace.append((h, ln, p, y))
        h = y
    return linear(h, sd[prefix + "output_projection.weight"], sd[prefix + "output_projection.bias"])


def colors(sd, x, mean=0.5, std=0.5, prefix="", trace=None):
    """PointCloudProjectionModel.denormalize of the transformer output: clamp(out * std + mean, 0, 1)."""
    return torch.clamp(transformer(sd, x, prefix, trace) * std + mean, 0, 1)


def sa_indices(coords):
    """Furthest-point-sample and ball-query indices of the four set-abstraction levels of PVCNN2 for the coordinates (B, 3, N)
    float32 (oracle operators; every level's coordinates are a gather of the level above, so they depend on `coords` alone)."""
    from oracle import ops as O
    from oracle.ref_net import SA_BLOCKS
    out, c = [], coords.float().contiguous()
    for _, (m, radius, u, _) in SA_BLOCKS:
        idx = O.furthest_point_sampling(c, m)
        centers = O.gather_features_forward(c, idx)
        out.append((idx, O.ball_query(centers, c, radius, u)))
        c = centers
    return out


# ---- elementwise error bound of bdm_color_block_tail -----------------------------------------------------------------------------------
# First-order forward error analysis in float64 around the float64 reference, for ANY summation order of each dot product, built the way
# tests/test_hip_pointwise.py builds its linear bound: a K-term fp32 dot product with bias obeys
#     |got - ref| <= (K + 4) u 1.01 (|W| |x| + |bias|) + |W| e_x            (u = 2^-24, e_x the error already in x)
# and the other stages propagate as follows (E = 64 channels, eps the LayerNorm epsilon):
#   r = h + p                    e_r   = u |r|
#   mu = mean(r)                 e_mu  = mean(e_r) + (E + 1) u mean|r|                      (E - 1 additions, one scaling)
#   d = r - mu                   e_d   = e_r + e_mu + u |d|
#   var = mean(d^2)              e_var = mean((2 |d| + e_d) e_d) + (E + 2) u var
#   s = sqrt(var + eps)          e_s   = e_var / (2 sqrt(max(var - e_var, 0) + eps)) + 2 u s
#   1 / s                        rho   = e_s / (s - e_s) + 4 u                              (relative; division and root <= 2 ulp each)
#   nrm = d / s                  e_n   = (e_d / s) (1 + rho) + |nrm| (rho + 2 u)
#   z = nrm g + b                e_z   = |g| e_n + 2 u (|nrm g| + |b|)
#   a = W1 z + b1                dot-product rule, K = E
#   gl = gelu(a)                 e_gl  = 1.13 e_a + 20 u |a|
#        (|gelu'| <= 1.129 everywhere; evaluation: 0.5 a (1 + erf(a / sqrt 2)) with erf to 16 ulp -- the OpenCL full-profile limit the
#         device library documents -- is 32 u absolute in erf, + u for the argument's two roundings (max |x erf'(x)| = 0.48), + 2 u for
#         the addition: <= 36 u in (1 + erf), times 0.5 |a|, + 2 u |gl| for the two products: < 20 u |a|)
#   m = W2 gl + b2               dot-product rule, K = 4 E
#   y = r + m                    e_y   = e_r + e_m + u (|r| + |m|)
#   ln_next = LayerNorm(y)       the LayerNorm rules above with e_y in the place of e_r
#   c = Wo y + bo                dot-product rule, K = E;  v = c std + mean: e_v = |std| e_c + 2 u (|c std| + |mean|);  clamp is 1-Lipschitz
# The 1.01 covers the second-order terms of the linear stages.  Nothing here was measured on the kernel.
def _dot_bound(k, w, x_abs, bias, e_x):
    wa = w.double().abs()
    return (k + 4) * U * 1.01 * (x_abs @ wa.t() + bias.double().abs()) + e_x @ wa.t()


def _ln_bound(x, e_x, g, b, eps):
    E = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    s = torch.sqrt(var + eps)
    nrm = d / s
    e_mu = e_x.mean(-1, keepdim=True) + (E + 1) * U * x.abs().mean(-1, keepdim=True)
    e_d = e_x + e_mu + U * d.abs()
    e_var = ((2 * d.abs() + e_d) * e_d).mean(-1, keepdim=True) + (E + 2) * U * var
    e_s = e_var / (2 * torch.sqrt((var - e_var).clamp_min(0) + eps)) + 2 * U * s
    rho = e_s / (s - e_s) + 4 * U
    assert bool((e_s < 0.5 * s).all()), "the first-order LayerNorm bound needs a relative error of the deviation well below 1"
    e_n = e_d / s * (1 + rho) + nrm.abs() * (rho + 2 * U)
    g, b = g.double(), b.double()
    return nrm * g + b, g.abs() * e_n + 2 * U * ((nrm * g).abs() + b.abs())


def tail_bound(sd, pre, h, p, eps=1e-5, next_norm=None, head=None):
    """float64 reference and elementwise bound of bdm_color_block_tail for fp32 inputs h, p (B, N, E) (any float dtype; taken to float64).
    -> dict: y, e_y [, ln, e_ln with next_norm = (weight, bias, eps)] [, v (unclamped), e_v with head = (weight, bias, mean, std)];
    also a (the fc1 pre-activations)."""
    h, p = h.double(), p.double()
    w = {k[len(pre):]: v.double() for k, v in sd.items() if k.startswith(pre)}
    r = h + p
    e_r = U * r.abs()
    z, e_z = _ln_bound(r, e_r, w["norm2.weight"], w["norm2.bias"], eps)
    a = z @ w["mlp.fc1.weight"].t() + w["mlp.fc1.bias"]
    e_a = _dot_bound(z.shape[-1], w["mlp.fc1.weight"], z.abs(), w["mlp.fc1.bias"], e_z)
    gl = gelu_erf(a)
    e_gl = 1.13 * e_a + 20 * U * a.abs()
    m = gl @ w["mlp.fc2.weight"].t() + w["mlp.fc2.bias"]
    e_m = _dot_bound(gl.shape[-1], w["mlp.fc2.weight"], gl.abs(), w["mlp.fc2.bias"], e_gl)
    y = r + m
    e_y = e_r + e_m + U * (r.abs() + m.abs())
    out = {"y": y, "e_y": e_y, "a": a}
    if next_norm is not None:
        out["ln"], out["e_ln"] = _ln_bound(y, e_y, next_norm[0], next_norm[1], next_norm[2])
    if head is not None:
        wo, bo, mean, std = head
        c = y @ wo.double().t() + bo.double()
        e_c = _dot_bound(y.shape[-1], wo, y.abs(), bo, e_y)
        out["v"], out["e_v"] = c * std + mean, abs(std) * e_c + 2 * U * ((c * std).abs() + abs(mean))
    return out
