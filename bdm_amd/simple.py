"""The simple point denoiser and PVCNN++ of the reference on the HIP path (experiments/model/simple/simple_model.py:9-34,
simple/simple_model_utils.py:158-279, pvcnn/pvcnn_plus_plus.py:9-42): same class names, constructor arguments and state-dict
keys, so a checkpoint trained with `model.point_cloud_model=simple|pvcnnplusplus` loads unchanged.  Sampling only.

Forward of SimplePointModel (csrc/simple_point.hip): the time embedding (bdm_time_embedding) and its share of the input
projection (a per-shape bias), the input projection with the positional encoding generated in registers, then one fused kernel
per FeedForward layer (pooled max / std, LayerNorm, gated 384 -> 512 -> 128 MLP, residual) preceded by a tiny per-shape
prologue, then output_projection (bdm_pointwise_conv).  The hidden layer is never written to memory.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .pvcnn import PVCNN2_PC2, create_classifier, run_classifier

N_FREQS = 10
WIDTH = 128  # the model width the fused kernels are built for (BasePointModel's default dim)


class PositionalEncoding(nn.Module):
    """simple_model_utils.py:87-120: [v, sin(f0 v), cos(f0 v), ..., sin(f9 v), cos(f9 v)], f = the `freq_bands` buffer."""

    def __init__(self, i_dim, N_freqs=N_FREQS):
        super().__init__()
        self.i_dim, self.o_dim, self.N_freqs = i_dim, 3 + 2 * N_freqs * 3, N_freqs
        self.register_buffer("freq_bands", 2 ** torch.linspace(1, N_freqs - 1, N_freqs))


class FeedForward(nn.Module):
    """simple_model_utils.py:158-201 as SimplePointModel builds it: LayerNorm(d_in), silu(layer1) * linear_v, layer2; no biases."""

    def __init__(self, d_in, d_hidden, d_out, dropout=0.1):
        super().__init__()
        self.layer1 = nn.Linear(d_in, d_hidden, bias=False)
        self.layer2 = nn.Linear(d_hidden, d_out, bias=False)
        self.dropout = nn.Dropout(dropout)
        self.activation = nn.SiLU()
        self.is_gated = True
        self.linear_v = nn.Linear(d_in, d_hidden, bias=False)
        self.use_layernorm = True
        self.layernorm = nn.LayerNorm(d_in)


def _pack_key(params):
    return tuple((p.data_ptr(), p._version) for p in params)


_ROWS = torch.tensor([(r & 3) + 8 * (r >> 2) for r in range(16)])  # accumulator register -> row of a 32 x 32 MFMA tile (half 0)


@torch.no_grad()
def pack_layer(ff):
    """Operand records of one FeedForward for bdm_simple_layer (include/bdm_hip.h section 6), gamma folded into the weights."""
    W1, V, W2 = ff.layer1.weight.float(), ff.linear_v.weight.float(), ff.layer2.weight.float()
    g, b = ff.layernorm.weight.float(), ff.layernorm.bias.float()
    D = W2.shape[0]
    assert D == WIDTH and W1.shape == (4 * D, 3 * D), "the fused layer is built for dim = 128"

    def a_pack(W):  # [k][s][l] = W[32 k + (l & 31)][s + 64 (l >> 5)] * g[s + 64 (l >> 5)]
        return (W[:, :D] * g[:D]).reshape(16, 32, 2, 64).permute(0, 3, 2, 1).contiguous()

    dev = W2.device
    rows = _ROWS.to(dev)
    ck = torch.arange(16, device=dev).view(16, 1, 1, 1, 1)
    ob = torch.arange(4, device=dev).view(1, 4, 1, 1, 1)
    r = rows.view(1, 1, 16, 1, 1)
    h = torch.arange(2, device=dev).view(1, 1, 1, 2, 1)
    li = torch.arange(32, device=dev).view(1, 1, 1, 1, 32)
    a2 = W2[(32 * ob + li).expand(16, 4, 16, 2, 32), (32 * ck + r + 4 * h).expand(16, 4, 16, 2, 32)].reshape(16, 4, 16, 64)
    Wc = torch.cat([W1, V])
    wms = (Wc[:, D:] * g[D:]).contiguous()
    d = (Wc[:, D:].double() @ g[D:].double()).float()
    e = (Wc.double() @ b.double()).float()
    vec = torch.stack([d[:4 * D], e[:4 * D], d[4 * D:], e[4 * D:]]).contiguous()
    return a_pack(W1), a_pack(V), a2.contiguous(), wms, vec


class SimplePointModel(nn.Module):
    """simple_model.py:9-34 on BasePointModel (simple_model_utils.py:204-279).  inputs (B, 3 + S, N) channel-first on the GPU,
    t (B,) -> (B, num_classes, N)."""

    def __init__(self, *, num_classes, embed_dim, extra_feature_channels, dim: int = WIDTH, num_layers: int = 6):
        super().__init__()
        self.extra_feature_channels = extra_feature_channels
        self.timestep_embed_dim = embed_dim
        self.output_dim = num_classes
        self.dim = dim
        self.num_layers = num_layers
        self.timestep_projection = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.LeakyReLU(0.1, inplace=True),
                                                 nn.Linear(embed_dim, embed_dim))
        self.positional_encoding = PositionalEncoding(i_dim=3, N_freqs=N_FREQS)
        self.input_projection = nn.Linear(3 + self.positional_encoding.o_dim + extra_feature_channels + embed_dim, dim)
        self.layers = nn.ModuleList([FeedForward(3 * dim, 4 * dim, dim) for _ in range(num_layers)])
        self.output_projection = nn.Linear(dim, num_classes)
        self._packs = None

    def _weight_packs(self):
        """Operand records of the input projection and the layers, rebuilt whenever a parameter or the freq_bands buffer is
        rewritten or replaced (cf. ops._pw_s3_weights)."""
        params = list(self.parameters()) + [self.positional_encoding.freq_bands]
        key = _pack_key(params)
        if self._packs is not None and self._packs[0] == key:
            return self._packs[1]
        if self.dim != WIDTH:
            raise NotImplementedError(f"the fused simple-model kernels are built for dim = {WIDTH}, got {self.dim}")
        W = self.input_projection.weight.detach().float()
        kin = W.shape[1] - self.timestep_embed_dim
        kp = kin + (kin & 1)
        wx = torch.zeros(WIDTH, kp, dtype=torch.float32, device=W.device)
        wx[:, :kin] = W[:, :kin]
        w_in = wx.reshape(4, 32, kp // 2, 2).permute(2, 0, 3, 1).contiguous()  # [s][o][h][li]
        packs = {"w_in": w_in, "w_t": W[:, kin:].contiguous(), "freq": self.positional_encoding.freq_bands.float().contiguous(),
                 "layers": [pack_layer(ff) for ff in self.layers],
                 "w_out": self.output_projection.weight.detach().float().contiguous()}
        self._packs = (key, packs, params)  # holds the parameters: their addresses cannot be recycled while the packs live
        return packs

    @torch.no_grad()
    def forward(self, inputs, t, _trace=None):
        """_trace (tests): a list that receives (x before each layer, pooled [max, std] of it) and the final x."""
        x_in = inputs if inputs.is_contiguous() else inputs.contiguous()
        B, C, N = x_in.shape
        if C != 3 + self.extra_feature_channels:
            raise ValueError(f"expected {3 + self.extra_feature_channels} input channels, got {C}")
        if N < 2:
            raise ValueError("the pooled standard deviation needs at least two points per shape")
        pk = self._weight_packs()
        lib, dev = L.lib(), x_in.device
        tp = self.timestep_projection
        te = ops.time_embedding(t, tp[0].weight, tp[0].bias, tp[2].weight, tp[2].bias)            # (B, E)
        bb = ops.pointwise_conv(te[:, :, None], pk["w_t"], self.input_projection.bias)            # (B, 128, 1)
        part = ops.workspace(lib.bdm_simple_partials_bytes(B, N), dev, "simple_partials")
        state = torch.empty(lib.bdm_simple_state_elems(B), dtype=torch.float32, device=dev)
        x = torch.empty(B, WIDTH, N, dtype=torch.float32, device=dev)
        L.check(lib.bdm_simple_input_proj(B, N, C, L.ptr(x_in), L.ptr(pk["freq"]), L.ptr(pk["w_in"]), L.ptr(bb), L.ptr(x),
                                          L.ptr(part), L.stream()), "simple_input_proj")
        y = torch.empty_like(x)
        for a1, av, a2, wms, vec in pk["layers"]:
            L.check(lib.bdm_simple_layer_prep(B, N, L.ptr(part), L.ptr(wms), L.ptr(state), L.stream()), "simple_layer_prep")
            if _trace is not None:
                _trace.append((x.clone(), state.view(B, -1)[:, :2 * WIDTH].clone()))
            L.check(lib.bdm_simple_layer(B, N, L.ptr(x), L.ptr(state), L.ptr(a1), L.ptr(av), L.ptr(a2), L.ptr(vec), L.ptr(y),
                                         L.ptr(part), L.stream()), "simple_layer")
            x, y = y, x
        if _trace is not None:
            _trace.append(x.clone())
        return ops.pointwise_conv(x, pk["w_out"], self.output_projection.bias)


class PVCNN2PlusPlus(nn.Module):
    """pvcnn_plus_plus.py:9-42: SimplePointModel(num_layers=3) -> x + PVCNN2_PC2(x) -> SharedMLP(64 -> 128), Conv1d(128 -> out).
    The inner PVCNN's coordinates are channels 0-2 of the simple model's output; its embedf IS the simple model's
    timestep_projection (one module under two state-dict names)."""

    def __init__(self, *, embed_dim, num_classes, extra_feature_channels):
        super().__init__()
        self.simple_point_model = SimplePointModel(num_classes=embed_dim, embed_dim=embed_dim,
                                                   extra_feature_channels=extra_feature_channels, num_layers=3)
        self.pvcnn = PVCNN2_PC2(num_classes=embed_dim, embed_dim=embed_dim, extra_feature_channels=embed_dim - 3)
        self.pvcnn.embedf = self.simple_point_model.timestep_projection
        self.output_projection = create_classifier(embed_dim, self.pvcnn.dropout, num_classes,
                                                   self.pvcnn.width_multiplier)

    @torch.no_grad()
    def forward(self, inputs, t):
        x = self.simple_point_model(inputs, t)                      # (B, E, N)
        y = self.pvcnn(x, t).contiguous()
        assert y.shape == x.shape
        s = torch.empty_like(x)
        L.check(L.lib().bdm_simple_add(x.numel(), L.ptr(x), L.ptr(y), L.ptr(s), L.stream()), "simple_add")
        return run_classifier(self.output_projection, s)
