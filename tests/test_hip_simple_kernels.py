"""The simple-denoiser kernels (csrc/simple_point.hip) one at a time against float64, on the shape paths the whole-forward goldens
miss: the input projection alone (odd and even contraction length K, positional-encoding arguments up to 512 * 8 rad), every layer
at slice and wave edges (a workgroup owns a 128-point slice, each of its four waves 32 points), degenerate clouds, the grid-stride
tail of bdm_simple_add, and the weight-pack cache of SimplePointModel."""
import pytest
import torch

from helpers import check_rel_l2, parity
from simple_ref import E, filled, input_projection, layer, pvcnnpp_forward, simple_forward

pytestmark = pytest.mark.gpu

SLICE, WAVE = 128, 32


def _simple(c_in=3 + 387, seed=7):
    from bdm_amd.simple import SimplePointModel
    m = SimplePointModel(num_classes=3, embed_dim=E, extra_feature_channels=c_in - 3)
    return filled(m.eval(), seed).cuda()


def _inputs(B, C, N, seed, xyz_scale=0.5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, N, generator=g)
    x[:, :3] *= xyz_scale
    return x


def _t(B):
    return torch.arange(B) * 97 % 1000 + 3


def _sd64(net):
    return {k: v.double().cpu() for k, v in net.state_dict().items()}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _check_pooled(x, pooled, what):
    """pooled [max, std] of x (B, 128, N) as a layer kernel leaves it: max bit-equal to torch.amax, std within 1e-6 relative of
    float64 torch.std.  Where the float64 std is exactly 0 (all points equal), the error is taken relative to the channel's
    magnitude instead: the one-pass double merge (s2 - s mean) / (n - 1) leaves ~1e-8 |v| there, as s2 = n v^2 needs more than
    53 bits."""
    xn = x.transpose(1, 2)
    assert torch.equal(pooled[:, :128], xn.amax(dim=1)), f"{what}: max"
    std64 = xn.double().std(dim=1)
    scale = torch.where(std64 == 0, xn.double().abs().amax(dim=1), std64)
    err = (pooled[:, 128:].double() - std64).abs() / scale.clamp_min(1e-30)
    e = float(err.max())
    assert torch.isfinite(pooled).all(), f"{what}: pooled not finite"
    assert e <= 1e-6, f"{what}: std {e:.2e}"
    return e


def _check_layers(net, x, t, shapes, tag, skip_channels=()):
    """Every layer kernel of one forward against `layer` in float64 on the kernel's own input, for the shapes listed; pooled
    statistics of every shape.  Returns the worst layer figure."""
    trace = []
    net(x.cuda(), t.cuda(), _trace=trace)
    sd = _sd64(net)
    keep = [c for c in range(128) if c not in skip_channels]
    worst_std = worst = 0.0
    for i, (xi, pooled) in enumerate(trace[:-1]):
        worst_std = max(worst_std, _check_pooled(xi, pooled, f"{tag} layer {i}"))
        nxt = trace[i + 1]
        nxt = nxt[0] if isinstance(nxt, tuple) else nxt
        assert torch.isfinite(nxt).all(), f"{tag} layer {i}: not finite"
        xs = xi[shapes].transpose(1, 2).double().cpu()
        ref = layer(sd, f"layers.{i}.", xs)[:, :, keep]
        err = _rel(nxt[shapes].transpose(1, 2)[:, :, keep], ref)
        worst = max(worst, err)
        assert err <= 5e-6, f"{tag} layer {i}: {err:.2e}"
    parity(f"simple_kernels {tag} layer rel L2", worst, 5e-6)
    parity(f"simple_kernels {tag} pooled std", worst_std, 1e-6)
    return worst


# ---- 1. input projection alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["xyz_half_normal", "xyz_normal", "xyz_far_8"])
@pytest.mark.parametrize("c_in", [390, 3, 4], ids=["K453_odd", "K66_even", "K67_odd"])
def test_input_projection_vs_float64(hip, c_in, scale):
    """trace[0] (input_proj_kernel) against simple_ref.input_projection in float64.  Convention: each positional-encoding
    argument f * v is rounded to fp32 first, as the reference module (fp32) forms it, and only then is sin / cos taken in float64:
    the fp32 rounding of a 4096-rad argument is a property of the model, not a kernel error.  K = c_in + 63; the A operand is
    packed two k-rows per step, so odd K has a zero-padded last step.  The projection also leaves the pooled partials of the first
    layer: max bit-equal to torch.amax, std against float64."""
    B, N = 2, 1100                                                    # 9 slices, last one 76 points: a partial and an empty wave
    net = _simple(c_in, seed=11 + c_in)
    x = _inputs(B, c_in, N, seed=c_in, xyz_scale=1.0 if scale != "xyz_half_normal" else 0.5)
    far = []
    if scale == "xyz_far_8":
        far = [0, 1, 127, 128, 600, N - 1]
        sign = torch.tensor([1.0, -1.0, 1.0])
        for j, p in enumerate(far):
            x[:, :3, p] = 8.0 * sign.roll(j)
    t = _t(B)
    trace = []
    net(x.cuda(), t.cuda(), _trace=trace)
    x0, pooled = trace[0]
    ref = input_projection(_sd64(net), "", x.double(), t).transpose(1, 2)   # (B, 128, N)
    check_rel_l2(x0.double().cpu(), ref, 2e-6, "x0")
    if far:
        check_rel_l2(x0[:, :, far].double().cpu(), ref[:, :, far], 2e-6, "|x| = 8 points")
    e = _check_pooled(x0, pooled, "input projection")
    parity(f"simple_kernels input projection c_in={c_in} {scale} pooled std", e, 1e-6)


# ---- 2. layers at slice and wave edges ---------------------------------------------------------------------------------------
def _edge_id(n):
    full, r = divmod(n, SLICE)
    if r == 0:
        return f"N{n}-{full}slices-full"
    waves = -(-r // WAVE)
    tail = "partial" if r % WAVE else "full"
    return f"N{n}-{full + 1}slices-last{waves}waves-{tail}" + (f"-{4 - waves}empty" if waves < 4 else "")


EDGE_N = [2, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4096]


@pytest.mark.parametrize("B", [1, 5, 16])
@pytest.mark.parametrize("N", EDGE_N, ids=[_edge_id(n) for n in EDGE_N])
def test_layers_at_slice_and_wave_edges(hip, N, B):
    """Every layer kernel against float64 with the current bounds (max bit-equal, std 1e-6 relative, layer 5e-6 relative L2).
    N = 2 is the smallest allowed cloud, N < 128 one slice, N % 32 != 0 a partial last wave, N % 128 in (0, 96] empty waves.
    At B = 16 the layers are compared in float64 on the first and last shape (a layer is per shape given its pooled
    statistics); the pooled statistics of all 16."""
    net = _simple(seed=21)
    x = _inputs(B, 390, N, seed=1000 + N + B, xyz_scale=1.0)
    shapes = [0, B - 1] if B > 5 else list(range(B))
    _check_layers(net, x, _t(B), shapes, f"B={B} {_edge_id(N)}")


# ---- 3. degenerate clouds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 257])
def test_identical_points(hip, N):
    """Every point of a shape equal (shape 1), next to an ordinary shape (shape 0): pooled std 0, the std half of the LayerNorm
    input constant; the output is finite and every layer matches float64 (std with the absolute floor)."""
    net = _simple(seed=31)
    x = _inputs(2, 390, N, seed=N, xyz_scale=1.0)
    x[1] = x[1, :, N - 1:]
    trace = []
    net(x.cuda(), _t(2).cuda(), _trace=trace)
    assert torch.equal(trace[0][0][1], trace[0][0][1, :, :1].expand(-1, N)), "input projection: points of shape 1 differ"
    _check_layers(net, x, _t(2), [0, 1], f"identical points N={N}")
    y = net(x.cuda(), _t(2).cuda())
    assert torch.isfinite(y).all()
    ref = simple_forward(_sd64(net), x.double(), _t(2))
    check_rel_l2(y.double().cpu(), ref, 1e-5, f"N={N} forward")


@pytest.mark.parametrize("N", [1100, 4096])
def test_channel_offset_far_above_its_spread(hip, N):
    """One channel of the model state offset by 1e4 x its spread: the pooled std comes from the double sums merged as
    (s2 - s mean) / (n - 1) in layer_prep_kernel, where this offset cancels 8 of the 16 digits.  The layers are compared on the
    other 127 channels (the offset channel's own residual is fp32 storage at 1e4)."""
    net = _simple(seed=41)
    x = _inputs(1, 390, N, seed=N + 3, xyz_scale=1.0)
    t = _t(1)
    trace = []
    net(x.cuda(), t.cuda(), _trace=trace)
    c = 17
    spread = float(trace[0][0][0, c].double().std())
    with torch.no_grad():
        net.input_projection.bias[c] += 1e4 * spread
    trace = []
    net(x.cuda(), t.cuda(), _trace=trace)
    st = trace[0][0][0, c].double()
    assert float(st.mean().abs()) > 5e3 * float(st.std())
    _check_layers(net, x, t, [0], f"offset 1e4 N={N}", skip_channels=(c,))


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 129, 257])
def test_simple_forward_vs_float64(hip, N):
    B = 3
    net = _simple(seed=51)
    x = _inputs(B, 390, N, seed=N + 7, xyz_scale=1.0)
    y = net(x.cuda(), _t(B).cuda())
    ref = simple_forward(_sd64(net), x.double(), _t(B))
    check_rel_l2(y.double().cpu(), ref, 1e-5, f"N={N}")


def test_pvcnnpp_forward_vs_float64_simple_half(hip):
    """PVCNN++ at B = 2, N = 1100: the simple-model half against float64 (the fp32 oracle operators of the PVCNN half take fp32,
    so the float64 half is rounded to fp32 there), complementing the fp32 goldens."""
    from bdm_amd.model import PointCloudModel
    B, N = 2, 1100
    net = filled(PointCloudModel(model_type="pvcnnplusplus", in_channels=390, embed_dim=E).model.eval(), 61).cuda()
    x, t = _inputs(B, 390, N, seed=62), _t(B)
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    sd64 = _sd64(net)
    inner = net.simple_point_model(x.cuda(), t.cuda())
    ref_inner = simple_forward(sd64, x.double(), t, "simple_point_model.", num_layers=3)
    check_rel_l2(inner.double().cpu(), ref_inner, 1e-5, "simple half")
    y = net(x.cuda(), t.cuda())
    check_rel_l2(y.double().cpu(), pvcnnpp_forward(sd, x, t, sd64=sd64).double(), 1e-4, "whole")


# ---- 5. bdm_simple_add past its grid cap ----------------------------------------------------------------------------------------
def test_simple_add_grid_stride(hip):
    """add_kernel caps its grid at 65536 x 256 threads = 2^24 elements; 2^24 + 1000 takes the grid-stride path.  Bit-equal to
    a + b, and the 64 floats past the end of `out` untouched."""
    from bdm_amd import _lib as L
    n = (1 << 24) + 1000
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(n, generator=g, device="cuda")
    b = torch.randn(n, generator=g, device="cuda")
    out = torch.full((n + 64,), float("nan"), device="cuda")
    L.check(L.lib().bdm_simple_add(n, L.ptr(a), L.ptr(b), L.ptr(out), L.stream()), "simple_add")
    assert torch.equal(out[:n], a + b)
    assert torch.isnan(out[n:]).all()


# ---- 6. weight-pack cache ----------------------------------------------------------------------------------------------------
def _forward_follows_weights(net, x, t, before, what):
    y = net(x.cuda(), t.cuda())
    assert not torch.equal(y, before), f"{what}: output unchanged"
    check_rel_l2(y.double().cpu(), simple_forward(_sd64(net), x.double(), t), 1e-5, what)
    return y


@pytest.mark.parametrize("name", ["layers.2.layer1.weight", "layers.5.layernorm.weight", "layers.0.layer2.weight",
                                  "input_projection.weight"])
def test_pack_cache_in_place_edit(hip, name):
    net = _simple(3, seed=71)
    x, t = _inputs(2, 3, 300, seed=72), _t(2)
    y0 = net(x.cuda(), t.cuda())
    with torch.no_grad():
        net.get_parameter(name).mul_(1.25)
    _forward_follows_weights(net, x, t, y0, f"in-place {name}")


def test_pack_cache_replaced_parameter_state_dict_and_freq_bands(hip):
    net = _simple(3, seed=81)
    x, t = _inputs(2, 3, 300, seed=82, xyz_scale=1.0), _t(2)
    y = net(x.cuda(), t.cuda())
    ff = net.layers[4].linear_v
    ff.weight = torch.nn.Parameter(ff.weight.detach() * -0.75)
    y = _forward_follows_weights(net, x, t, y, "replaced Parameter")
    other = _simple(3, seed=83)
    net.load_state_dict(other.state_dict())
    y = _forward_follows_weights(net, x, t, y, "load_state_dict")
    net.positional_encoding.freq_bands.copy_(2 ** torch.linspace(0, 8, 10))
    _forward_follows_weights(net, x, t, y, "freq_bands.copy_")


def test_rejects_bad_shapes(hip):
    net = _simple(3, seed=91)
    with pytest.raises(ValueError):
        net(torch.randn(2, 3, 1).cuda(), _t(2).cuda())
    with pytest.raises(ValueError):
        net(torch.randn(2, 4, 64).cuda(), _t(2).cuda())
