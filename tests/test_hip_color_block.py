"""bdm_color_block_tail (bdm_amd/csrc/color_block.hip) against float64 on the same fp32 inputs, ELEMENTWISE.

The kernel is the second half of one block of the colouring model's transformer: r = h + p, y = r + fc2(gelu(fc1(LayerNorm(r)))),
then LayerNorm(y) (next block's norm0) or the clamped colour head.  A workgroup owns 128 consecutive points, a wave 32 of them:
the point counts below put the last point of a shape at the first / last lane of a wave and of a tile and one past them.

Bound (derived in tests/color_ref.py next to `tail_bound`, nothing measured on the kernel): the construction of
tests/test_hip_pointwise.py -- (K + 4) 2^-24 1.01 (|W| |x| + |bias|) per fp32 dot product in any summation order -- carried
through the stages: the rounding of h + p, the two-pass LayerNorm (mean, deviations, variance, root, reciprocal), fc1, the exact
GELU (Lipschitz constant 1.13; evaluation error 20 2^-24 |a| from a 16-ulp erf), fc2, the residual, and then the second
LayerNorm or the colour head and its affine map.  The CPU half runs the float32 restatement against the same bound, and two
mutants -- tanh-GELU, and the unbiased variance in the LayerNorm -- must break it.

Inputs that make errors visible: h + p at offset 100 with spread 1e-3 (a one-pass variance E[x^2] - E[x]^2 loses every digit
there: 2^-24 1e4 >> 1e-6); fc1 scaled so that the pre-activations span [-6, 6] (both GELU tails); a colour head scaled so that
rows land below 0 and above 1, which must come out as exactly 0.0 and 1.0.

Two weight sets.  "dense": procedural matrices, the shape sweep.  "selector": fc1 = [I; -I; 0; 0], fc2 = [I, -I / 2, 0, 0], no
biases, so that m = gelu(z) - gelu(-z) / 2 per channel.  The bound carries an error through a matrix as |W| e, which for a dense
matrix is sqrt(K) above what a random-sign error does; behind a dense MLP a wrong LayerNorm or GELU would drown in that slack.
With one or two non-zeros per row nothing is lost, so the offset case and the mutants run on the selector set, where the bound
on y is the bound on the LayerNorm output itself.  (The offset case is checked in the modes `y` and `colors`: a second LayerNorm
behind it has a worst-case input error of the size of its own spread, for which no first-order bound exists.)
"""
import itertools

import pytest
import torch

import color_ref as R
from helpers import current_test, parity

E = 64
PRE = "blocks.0."
NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1100)   # wave = 32 points, tile = 128 points
MODES = ("y", "ln_next", "colors")
MEAN, STD = 0.5, 0.5


def weights(fc1_scale=1.0, head_scale=1.0, kind="dense"):
    from bdm_amd.utils.procedural import procedural_tensor as T
    shapes = {"norm2.weight": (E,), "norm2.bias": (E,), "mlp.fc1.weight": (4 * E, E), "mlp.fc1.bias": (4 * E,),
              "mlp.fc2.weight": (E, 4 * E), "mlp.fc2.bias": (E,)}
    sd = {PRE + k: T(PRE + k, s, seed=3) for k, s in shapes.items()}
    sd[PRE + "mlp.fc1.weight"] = sd[PRE + "mlp.fc1.weight"] * fc1_scale
    if kind == "selector":
        eye, zero = torch.eye(E), torch.zeros(E, E)
        sd[PRE + "mlp.fc1.weight"] = torch.cat([eye, -eye, zero, zero])
        sd[PRE + "mlp.fc2.weight"] = torch.cat([eye, -0.5 * eye, zero, zero], dim=1)
        sd[PRE + "mlp.fc1.bias"], sd[PRE + "mlp.fc2.bias"] = torch.zeros(4 * E), torch.zeros(E)
    nxt = (T("blocks.1.norm0.weight", (E,), seed=3), T("blocks.1.norm0.bias", (E,), seed=3), 1e-5)
    head = (T("output_projection.weight", (3, E), seed=3) * head_scale, T("output_projection.bias", (3,), seed=3), MEAN, STD)
    return sd, nxt, head


def inputs(kind, b, n, seed=0):
    """h, p (b, n, E) float32, point-major (the kernel gets their channel-first transposes)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * n + b)
    if kind == "offset":   # h + p = 100 + 1e-3 N(0, 1)
        return 100.0 + 0.7e-3 * torch.randn(b, n, E, generator=g), 0.7e-3 * torch.randn(b, n, E, generator=g)
    return torch.randn(b, n, E, generator=g) * (0.5 + torch.rand(1, 1, E, generator=g)), torch.randn(b, n, E, generator=g)


def reference(sd, nxt, head, h, p, mode):
    return R.tail_bound(sd, PRE, h, p, next_norm=nxt if mode == "ln_next" else None, head=head if mode == "colors" else None)


def fractions(out, ref, mode):
    """Worst |got - ref| / bound per output (got: dict of CPU tensors, point-major)."""
    fr = {"y": float(((out["y"].double() - ref["y"]).abs() / ref["e_y"]).max())}
    if mode == "ln_next":
        fr["ln_next"] = float(((out["ln_next"].double() - ref["ln"]).abs() / ref["e_ln"]).max())
    if mode == "colors":
        fr["colors"] = float(((out["colors"].double() - ref["v"].clamp(0, 1)).abs() / ref["e_v"]).max())
    return fr


def restatement32(sd, nxt, head, h, p, mode, gelu=R.gelu_erf, unbiased=False):
    """The tail in plain float32 torch on the CPU (the yardstick the mutants are applied to)."""
    y = R.block_tail(sd, PRE, h.float(), p.float(), gelu=gelu, unbiased=unbiased)
    out = {"y": y}
    if mode == "ln_next":
        out["ln_next"] = R.layer_norm(y, nxt[0], nxt[1], nxt[2], unbiased=unbiased)
    if mode == "colors":
        out["colors"] = torch.clamp(R.linear(y, head[0], head[1]) * head[3] + head[2], 0, 1)
    return out


# ---- CPU half: the bound holds for a float32 restatement and catches the two mutants ---------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_float32_restatement_is_inside_the_bound(mode):
    for kind, wk in (("generic", "dense"), ("generic", "selector"), ("offset", "selector")):
        if kind == "offset" and mode == "ln_next":
            continue
        sd, nxt, head = weights(kind=wk)
        h, p = inputs(kind, 2, 300)
        fr = fractions(restatement32(sd, nxt, head, h, p, mode), reference(sd, nxt, head, h, p, mode), mode)
        for k, v in fr.items():
            parity(current_test() + f" {kind} {wk} {k}", v, 1.0)
            assert v <= 1.0, f"{kind}, {wk}, {k}: float32 PyTorch is {v:.3g} x the bound"


@pytest.mark.parametrize("mutant", ["tanh_gelu", "unbiased_variance"])
def test_mutants_break_the_bound(mutant):
    sd, nxt, head = weights(kind="selector")
    h, p = inputs("generic", 2, 300)
    kw = {"gelu": R.gelu_tanh} if mutant == "tanh_gelu" else {"unbiased": True}
    for mode in MODES:
        fr = fractions(restatement32(sd, nxt, head, h, p, mode, **kw), reference(sd, nxt, head, h, p, mode), mode)
        assert all(v > 1.0 for v in fr.values()), f"{mutant} passes the bound in mode {mode}: {fr}"


def test_offset_case_defeats_a_one_pass_variance():
    """The point of the offset inputs: E[x^2] - E[x]^2 in float32 is far outside the bound there, the two-pass form inside."""
    sd, nxt, head = weights(kind="selector")
    h, p = inputs("offset", 2, 1100)
    ref = reference(sd, nxt, head, h, p, "y")
    r = h + p
    var1 = (r * r).mean(-1, keepdim=True) - r.mean(-1, keepdim=True) ** 2
    z = (r - r.mean(-1, keepdim=True)) / torch.sqrt(var1.clamp_min(0) + 1e-5) * sd[PRE + "norm2.weight"] + sd[PRE + "norm2.bias"]
    y = r + R.mlp(sd, PRE + "mlp.", z)
    assert float(((y.double() - ref["y"]).abs() / ref["e_y"]).max()) > 1.0


def test_tail_inputs_reach_both_gelu_tails_and_both_clamps():
    sd, nxt, head = weights(fc1_scale=3.0, head_scale=4.0)
    h, p = inputs("generic", 1, 1100)
    ref = reference(sd, nxt, head, h, p, "colors")
    assert float(ref["a"].min()) < -6 and float(ref["a"].max()) > 6
    assert bool((ref["v"] < -ref["e_v"]).any()) and bool((ref["v"] > 1 + ref["e_v"]).any())


# ---- GPU half ------------------------------------------------------------------------------------------------------------------------
def run_tail(sd, nxt, head, h, p, mode, e=E):
    """The kernel on h, p (b, n, e) point-major CPU tensors -> (status, dict of CPU tensors, point-major)."""
    from bdm_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda")
    b, n = h.shape[:2]
    hc, pc = h.transpose(1, 2).contiguous().to(dev), p.transpose(1, 2).contiguous().to(dev)
    w = {k[len(PRE):]: v.to(dev).contiguous() for k, v in sd.items()}
    packed = torch.zeros(max(lib.bdm_color_block_packed_elems(e), 1), device=dev)
    if e == E:
        L.check(lib.bdm_color_block_pack_weights(e, L.ptr(w["mlp.fc1.weight"]), L.ptr(w["mlp.fc2.weight"]), L.ptr(packed), L.stream()), "pack")
    y = torch.full((b, e, n), 777.0, device=dev)
    ln = torch.full((b, e, n), 777.0, device=dev) if mode == "ln_next" else None
    col = torch.full((b, n, 3), 777.0, device=dev) if mode == "colors" else None
    nw, nb = (nxt[0].to(dev), nxt[1].to(dev)) if mode == "ln_next" else (None, None)
    ow, ob = (head[0].to(dev).contiguous(), head[1].to(dev)) if mode == "colors" else (None, None)
    rc = lib.bdm_color_block_tail(b, e, n, L.ptr(hc), L.ptr(pc), L.ptr(w["norm2.weight"]), L.ptr(w["norm2.bias"]), 1e-5, L.ptr(packed),
                                  L.ptr(w["mlp.fc1.bias"]), L.ptr(w["mlp.fc2.bias"]), L.ptr(y), L.ptr(nw), L.ptr(nb), nxt[2], L.ptr(ln),
                                  L.ptr(ow), L.ptr(ob), head[2], head[3], L.ptr(col), L.stream())
    torch.cuda.synchronize()
    out = {"y": y.transpose(1, 2).cpu()}
    if ln is not None:
        out["ln_next"] = ln.transpose(1, 2).cpu()
    if col is not None:
        out["colors"] = col.cpu()
    return rc, out


def check(sd, nxt, head, h, p, mode, what):
    rc, out = run_tail(sd, nxt, head, h, p, mode)
    assert rc == 0
    ref = reference(sd, nxt, head, h, p, mode)
    for k, v in fractions(out, ref, mode).items():
        print(f"{what} {k}: worst element {v:.4f} of its bound")
        parity(current_test() + f" {k}", v, 1.0, note=what)
        assert v <= 1.0, f"{what}, {k}: an element is {v:.3g} x its bound"
    return out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,mode", list(itertools.product((1, 2), NS, MODES)), ids=lambda v: str(v))
def test_tail_against_float64(hip, b, n, mode):
    sd, nxt, head = weights()
    h, p = inputs("generic", b, n)
    check(sd, nxt, head, h, p, mode, f"b {b} n {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("y", "colors"))
def test_offset_100_spread_1e_3(hip, mode):
    sd, nxt, head = weights(kind="selector")
    h, p = inputs("offset", 2, 1100)
    check(sd, nxt, head, h, p, mode, "offset 100, spread 1e-3")


@pytest.mark.gpu
def test_gelu_tails_and_exact_clamp(hip):
    sd, nxt, head = weights(fc1_scale=3.0, head_scale=4.0)
    h, p = inputs("generic", 1, 1100)
    out, ref = check(sd, nxt, head, h, p, "colors", "pre-activations over [-6, 6], colour head x 4")
    assert float(ref["a"].min()) < -6 and float(ref["a"].max()) > 6
    below, above = ref["v"] < -ref["e_v"], ref["v"] > 1 + ref["e_v"]
    assert bool(below.any()) and bool(above.any())
    assert bool((out["colors"][below] == 0.0).all()) and bool((out["colors"][above] == 1.0).all())
    assert float(out["colors"].min()) >= 0.0 and float(out["colors"].max()) <= 1.0
    check(sd, nxt, head, h, p, "ln_next", "pre-activations over [-6, 6]")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_selector_weights(hip, mode):
    """The weight set on which the bound on y is the bound on the LayerNorm / GELU output itself (what the mutants are caught on)."""
    sd, nxt, head = weights(kind="selector")
    h, p = inputs("generic", 2, 1100)
    check(sd, nxt, head, h, p, mode, "selector weights")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_point_does_not_see_its_tile(hip, mode):
    """Column j of an n = 1100 call carries the bits of the n = 1 call on that column."""
    sd, nxt, head = weights()
    h, p = inputs("generic", 2, 1100)
    _, whole = run_tail(sd, nxt, head, h, p, mode)
    for j in (0, 31, 32, 127, 128, 1023, 1099):
        _, one = run_tail(sd, nxt, head, h[:, j:j + 1].contiguous(), p[:, j:j + 1].contiguous(), mode)
        for k in one:
            assert torch.equal(one[k][:, 0], whole[k][:, j]), f"{k}: point {j} depends on the call it is part of"


@pytest.mark.gpu
def test_unsupported_width_writes_nothing(hip):
    from bdm_amd import _lib as L
    sd, nxt, head = weights()
    sd32 = {k: v[..., :32].contiguous() if v.dim() == 1 else v[:128, :32].contiguous() for k, v in sd.items()}
    h, p = torch.randn(1, 70, 32), torch.randn(1, 70, 32)
    for mode in MODES:
        rc, out = run_tail(sd32, (nxt[0][:32], nxt[1][:32], nxt[2]), (head[0][:, :32], head[1], MEAN, STD), h, p, mode, e=32)
        assert rc == 3, "BDM_ERR_UNSUPPORTED"
        assert all(bool((v == 777.0).all()) for v in out.values())
    lib = L.lib()
    assert lib.bdm_color_block_packed_elems(32) == 0 and lib.bdm_color_block_packed_elems(64) == 32768
    buf = torch.full((64,), 777.0, device="cuda")
    assert lib.bdm_color_block_pack_weights(32, L.ptr(buf), L.ptr(buf), L.ptr(buf), L.stream()) == 3
    torch.cuda.synchronize()
    assert bool((buf == 777.0).all())
