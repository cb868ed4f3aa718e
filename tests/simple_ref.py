"""Pure-torch restatement of the reference's SimplePointModel and PVCNN2PlusPlus (simple/simple_model.py:9-34,
simple/simple_model_utils.py:158-279, pvcnn/pvcnn_plus_plus.py:9-42) over a state dict, CPU, fp32 (or float64 with dtype).
Pinned to the reference by the goldens tests/golden/{simple,pvcnnpp}_full_n*.npz (tests/test_simple_model.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_net

S, E = 387, 64


def golden(name):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    return {k: z[k] for k in z.files}


def filled(model, seed):
    """fill_module_ as tools/gen_golden_simple.py applies it: procedural weights, then the constructed freq_bands."""
    from bdm_amd.utils.procedural import fill_module_
    fill_module_(model, seed=seed)
    for m in model.modules():
        if hasattr(m, "freq_bands"):
            m.freq_bands.copy_(2 ** torch.linspace(1, 9, 10))
    return model


def posenc(v, freq):
    """The argument f * v is formed in fp32, as the reference module forms it, whatever the dtype of v: its fp32 rounding (up to
    half an ulp of 512 |v| rad) belongs to the model.  sin / cos are then taken in v's dtype."""
    pe = [v]
    for f in freq:
        a = (f.float() * v.float()).to(v.dtype)
        pe += [torch.sin(a), torch.cos(a)]
    return torch.cat(pe, dim=-1)


def embedf(sd, pre, t, dim):
    """ref_net.embedf with the sinusoidal embedding (fp32, as the reference forms it) cast to the weights' dtype."""
    w0 = sd[pre + "0.weight"]
    h = F.linear(ref_net.timestep_embedding(t, dim).to(w0.dtype), w0, sd[pre + "0.bias"])
    return F.linear(F.leaky_relu(h, 0.1), sd[pre + "2.weight"], sd[pre + "2.bias"])


def feed_forward(sd, pre, x_in):
    h = F.layer_norm(x_in, (x_in.shape[-1],), sd[pre + "layernorm.weight"], sd[pre + "layernorm.bias"], 1e-5)
    g = F.silu(F.linear(h, sd[pre + "layer1.weight"])) * F.linear(h, sd[pre + "linear_v.weight"])
    return F.linear(g, sd[pre + "layer2.weight"])


def layer(sd, pre, x):
    """one SimplePointModel layer on x (B, N, D): x + FeedForward([x, max_N x, std_N x])."""
    N = x.shape[1]
    mx = x.max(dim=1, keepdim=True).values.repeat(1, N, 1)
    sd_ = x.std(dim=1, keepdim=True).repeat(1, N, 1)
    return x + feed_forward(sd, pre, torch.cat([x, mx, sd_], dim=-1))


def input_projection(sd, pre, inputs, t, embed_dim=E):
    temb = embedf(sd, pre + "timestep_projection.", t, embed_dim)[:, None, :].expand(-1, inputs.shape[-1], -1)
    x = inputs.transpose(-2, -1)
    x = torch.cat([x, posenc(x[:, :, :3], sd[pre + "positional_encoding.freq_bands"]), temb], dim=2)
    return F.linear(x, sd[pre + "input_projection.weight"], sd[pre + "input_projection.bias"])


def simple_forward(sd, inputs, t, pre="", num_layers=6, states=None):
    """(B, 3 + S, N), (B,) -> (B, num_classes, N).  states: receives x before every layer and after the last."""
    x = input_projection(sd, pre, inputs, t)
    for i in range(num_layers):
        if states is not None:
            states.append(x)
        x = layer(sd, f"{pre}layers.{i}.", x)
    if states is not None:
        states.append(x)
    return F.linear(x, sd[pre + "output_projection.weight"], sd[pre + "output_projection.bias"]).transpose(-2, -1)


def pvcnnpp_forward(sd, inputs, t, pre="", sd64=None):
    """sd64 (the same weights in float64): the simple-model half in float64 on inputs.double(), rounded to fp32 before the
    PVCNN half, which runs on the fp32 oracle operators."""
    if sd64 is None:
        x = simple_forward(sd, inputs, t, pre + "simple_point_model.", num_layers=3)
    else:
        x = simple_forward(sd64, inputs.double(), t, pre + "simple_point_model.", num_layers=3).float()
    x = x + ref_net.pvcnn_forward(sd, x, t, prefix=pre + "pvcnn.")
    p = pre + "output_projection."
    h = ref_net.shared_mlp(sd, p + "0.", x)
    return F.conv1d(h, sd[p + "2.weight"], sd[p + "2.bias"])
