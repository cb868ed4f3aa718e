"""Point-cloud transformer of the PC^2 colouring model on the HIP path (experiments/model/point_cloud_transformer_model.py:13-80):
same class names, constructor arguments and state-dict keys (`input_projection`, `blocks.{i}.norm0`,
`blocks.{i}.point_cloud_model.model.*`, `blocks.{i}.norm2`, `blocks.{i}.mlp.fc1|fc2`, `norm`, `output_projection`), so a reference
checkpoint loads with strict=True.  Inference only, and only the use_attn=False form the colouring configuration can reach.

A block is  x = x + PVCNN(norm0(x), t = 0);  x = x + fc2(gelu(fc1(norm2(x)))).  Tokens stay channel-first (B, E, N) from the
conditioning gather to the colour head.  Per block: the PVCNN as it runs everywhere else in the project, then everything after it --
both residual additions, norm2, the MLP, and either the next block's norm0 or the output projection with the colour denormalisation
-- either from the existing launches or in ONE kernel that never stores the (B, 4E, N) hidden tensor (bdm_color_block_tail,
csrc/color_block.hip); see TAIL_IMPL for which is the default and why.

Two quirks of the reference are kept: `norm` is constructed (its keys are in the state dict) but never applied, and the inner
PVCNN takes the first three channels of the norm0 output as its "coordinates".
"""
import os

import torch
import torch.nn as nn

from . import _lib as L
from . import ops

# "composed": everything after the PVCNN from the existing launches (bdm_simple_add, bdm_layer_norm_channels, two bdm_pointwise_conv,
# output projection); "fused": bdm_color_block_tail, one kernel.  Measured at B = 16, N = 4096 (tools/coloring_bench.py, DESIGN.md
# section 11): the fused kernel moves a sixth of the bytes but is NOT faster (0.19 ms against 0.16 - 0.18 ms), so the composed route is the
# default; BDM_COLOR_TAIL=fused selects the kernel.  Both are tested against the same float64 restatement.
TAIL_IMPL = os.environ.get("BDM_COLOR_TAIL", "composed")


class Mlp(nn.Module):
    """timm.layers.Mlp at its defaults: fc1 -> exact (erf) GELU -> fc2; the dropouts are identities at drop = 0."""

    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)


def _layer_norm(x, ln):
    B, D, N = x.shape
    out = torch.empty_like(x)
    L.check(L.lib().bdm_layer_norm_channels(B, D, N, L.ptr(x), L.ptr(ln.weight), L.ptr(ln.bias), L.c_float(ln.eps), L.ptr(out),
                                            L.stream()), "layer_norm_channels")
    return out


class PointCloudModelBlock(nn.Module):
    """point_cloud_transformer_model.py:13-61.  LayerScale (init_values=None) and DropPath (drop_path=0) are identities at the
    values the configuration can reach; anything else is refused."""

    def __init__(self, *, dim: int, model_type: str = "pvcnn", dropout: float = 0.1, width_multiplier: int = 1,
                 voxel_resolution_multiplier: int = 1, num_heads=6, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0.,
                 init_values=None, drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, use_attn=False):
        super().__init__()
        from .model import PointCloudModel
        if use_attn:
            raise NotImplementedError("use_attn=True cannot be set through PointCloudColoringModel; the HIP path has the use_attn=False block")
        if init_values or drop_path > 0. or drop > 0. or act_layer is not nn.GELU or norm_layer is not nn.LayerNorm:
            raise NotImplementedError("LayerScale / DropPath / dropout / another activation or norm are not reachable from the configuration")
        self.dim = dim
        self.use_attn = False
        self.norm0 = nn.LayerNorm(dim)
        self.point_cloud_model = PointCloudModel(model_type=model_type, in_channels=dim, out_channels=dim, embed_dim=dim, dropout=dropout,
                                                 width_multiplier=width_multiplier, voxel_resolution_multiplier=voxel_resolution_multiplier)
        self.ls0, self.drop_path0 = nn.Identity(), nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio))
        self.ls2, self.drop_path2 = nn.Identity(), nn.Identity()
        self._pack = None

    def apply_point_cloud_model(self, x_cf, t=None):
        """(B, E, N) channel-first (the norm0 output) -> (B, E, N); t defaults to zeros (point_cloud_transformer_model.py:52-54)."""
        t = t if t is not None else torch.zeros(len(x_cf), device=x_cf.device, dtype=torch.long)
        return self.point_cloud_model.model(x_cf, t).contiguous()

    def packed_weights(self):
        """fc1 / fc2 in the kernel's operand order, rebuilt whenever either weight is rewritten or replaced."""
        w1, w2 = self.mlp.fc1.weight, self.mlp.fc2.weight
        key = (w1.data_ptr(), w1._version, w2.data_ptr(), w2._version)
        if self._pack is None or self._pack[0] != key:
            lib = L.lib()
            n = lib.bdm_color_block_packed_elems(self.dim)
            if n == 0 or tuple(w1.shape) != (4 * self.dim, self.dim):
                raise NotImplementedError(f"bdm_color_block_tail is built for dim = 64 and mlp_ratio = 4, got dim {self.dim}, fc1 {tuple(w1.shape)}")
            packed = torch.empty(n, dtype=torch.float32, device=w1.device)
            L.check(lib.bdm_color_block_pack_weights(self.dim, L.ptr(L.f32(w1.detach())), L.ptr(L.f32(w2.detach())), L.ptr(packed),
                                                     L.stream()), "color_block_pack_weights")
            self._pack = (key, packed, (w1, w2))  # holds the weights: their addresses cannot be recycled while the pack lives
        return self._pack[1]

    def tail(self, h, p, next_norm=None, head=None):
        """Everything after the PVCNN.  h, p (B, E, N) -> y, extra: extra = LayerNorm(y) with `next_norm` (a nn.LayerNorm), or the
        clamped colours (B, N, 3) with head = (output_projection, colors_mean, colors_std), or None."""
        assert next_norm is None or head is None
        if TAIL_IMPL not in ("composed", "fused"):
            raise ValueError(f"BDM_COLOR_TAIL / TAIL_IMPL must be 'composed' or 'fused', got {TAIL_IMPL!r}")
        if TAIL_IMPL == "composed" or (head is not None and head[0].out_features != 3):
            return self._tail_composed(h, p, next_norm, head)
        B, E, N = h.shape
        y = torch.empty_like(h)
        ln_next = torch.empty_like(h) if next_norm is not None else None
        colors = torch.empty(B, N, 3, dtype=torch.float32, device=h.device) if head is not None else None
        proj, mean, std = head if head is not None else (None, 0.0, 1.0)
        L.check(L.lib().bdm_color_block_tail(
            B, E, N, L.ptr(h), L.ptr(p), L.ptr(self.norm2.weight), L.ptr(self.norm2.bias), L.c_float(self.norm2.eps),
            L.ptr(self.packed_weights()), L.ptr(self.mlp.fc1.bias), L.ptr(self.mlp.fc2.bias), L.ptr(y),
            L.ptr(next_norm.weight) if next_norm is not None else None, L.ptr(next_norm.bias) if next_norm is not None else None,
            L.c_float(next_norm.eps if next_norm is not None else 0.0), L.ptr(ln_next),
            L.ptr(proj.weight) if proj is not None else None, L.ptr(proj.bias) if proj is not None else None,
            L.c_float(mean), L.c_float(std), L.ptr(colors), L.stream()), "color_block_tail")
        return y, (ln_next if next_norm is not None else colors)

    def _tail_composed(self, h, p, next_norm, head):
        r = torch.empty_like(h)
        L.check(L.lib().bdm_simple_add(h.numel(), L.ptr(h), L.ptr(p), L.ptr(r), L.stream()), "simple_add")
        hid = ops.pointwise_conv(_layer_norm(r, self.norm2), self.mlp.fc1.weight, self.mlp.fc1.bias, act=3)
        y = ops.pointwise_conv(hid, self.mlp.fc2.weight, self.mlp.fc2.bias, residual=r)
        if next_norm is not None:
            return y, _layer_norm(y, next_norm)
        if head is not None:
            proj, mean, std = head
            c = ops.pointwise_conv(y, proj.weight, proj.bias)
            return y, torch.clamp(c * std + mean, 0, 1).transpose(1, 2).contiguous()
        return y, None

    @torch.no_grad()
    def forward(self, x_cf):
        """(B, E, N) channel-first -> (B, E, N)."""
        x_cf = x_cf.contiguous()
        return self.tail(x_cf, self.apply_point_cloud_model(_layer_norm(x_cf, self.norm0)))[0]


class PointCloudTransformerModel(nn.Module):
    """point_cloud_transformer_model.py:64-80 (diffusers' ModelMixin / ConfigMixin add no parameters)."""

    def __init__(self, num_layers: int, in_channels: int = 3, out_channels: int = 3, embed_dim: int = 64, **kwargs):
        super().__init__()
        self.num_layers = num_layers
        self.input_projection = nn.Linear(in_channels, embed_dim)
        self.blocks = nn.Sequential(*[PointCloudModelBlock(dim=embed_dim, **kwargs) for _ in range(num_layers)])
        self.norm = nn.LayerNorm(embed_dim)  # in the state dict, never applied (reference quirk)
        self.output_projection = nn.Linear(embed_dim, out_channels)

    def _run(self, inputs, head=None, trace=None):
        """inputs (B, N, in_channels) -> (last y (B, E, N), colours or None).  trace (tests): receives per block (h, norm0(h), p, y)."""
        if self.num_layers < 1:
            raise ValueError("the transformer needs at least one block")
        cond = getattr(inputs, "_bdm_cond", None)
        if cond is not None:   # every input channel is read here: complete a lazily built conditioned input
            cond.ensure_features()
        x = ops.transpose12(inputs)
        h = ops.pointwise_conv(x if x.is_contiguous() else x.contiguous(), self.input_projection.weight, self.input_projection.bias)
        ln = _layer_norm(h, self.blocks[0].norm0)
        extra = None
        for i, blk in enumerate(self.blocks):
            last = i + 1 == self.num_layers
            p = blk.apply_point_cloud_model(ln)
            y, extra = blk.tail(h, p, next_norm=None if last else self.blocks[i + 1].norm0, head=head if last else None)
            if trace is not None:
                trace.append((h, ln, p, y))
            h, ln = y, extra
        return h, extra

    @torch.no_grad()
    def forward(self, inputs):
        """(B, N, in_channels) -> (B, N, out_channels), the raw output projection."""
        h, _ = self._run(inputs)
        return ops.transpose12(ops.pointwise_conv(h, self.output_projection.weight, self.output_projection.bias))

    @torch.no_grad()
    def forward_colors(self, inputs, colors_mean, colors_std, trace=None):
        """(B, N, in_channels) -> clamp(forward(inputs) * colors_std + colors_mean, 0, 1) as (B, N, 3), the head fused into the last
        block's tail kernel."""
        return self._run(inputs, head=(self.output_projection, float(colors_mean), float(colors_std)), trace=trace)[1]
