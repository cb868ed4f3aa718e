"""The simple and PVCNN++ denoisers on the host side: state-dict keys, the tied time embedding, the restatement against the
reference's goldens, configuration and the BDM-Merging restriction.  No GPU."""
import numpy as np
import pytest
import torch

from simple_ref import E, S, filled, golden, pvcnnpp_forward, simple_forward

CASES = [("simple", 1024), ("simple", 1100), ("pvcnnpp", 1024), ("pvcnnpp", 1100)]


def _module(kind):
    from bdm_amd.model import PointCloudModel
    return PointCloudModel(model_type="simple" if kind == "simple" else "pvcnnplusplus", in_channels=3 + S, embed_dim=E).model


@pytest.mark.parametrize("kind", ["simple", "pvcnnpp"])
def test_state_dict_keys_match_reference(kind):
    g = golden(f"{kind}_full_n1024.npz")
    sd = _module(kind).state_dict()
    assert list(sd.keys()) == list(g["keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g["shapes"])


def test_pvcnnpp_time_embedding_is_tied():
    m = _module("pvcnnpp")
    assert m.pvcnn.embedf is m.simple_point_model.timestep_projection
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["simple_point_model.timestep_projection.0.weight"] = torch.full_like(sd["simple_point_model.timestep_projection.0.weight"], 3.0)
    sd["pvcnn.embedf.0.weight"] = sd["simple_point_model.timestep_projection.0.weight"]
    m.load_state_dict(sd)
    assert m.pvcnn.embedf is m.simple_point_model.timestep_projection
    assert bool((m.pvcnn.embedf[0].weight == 3.0).all())


def test_positional_encoding_frequencies():
    m = _module("simple")
    f = m.positional_encoding.freq_bands
    assert "positional_encoding.freq_bands" in m.state_dict()
    assert torch.equal(f, 2 ** torch.linspace(1, 9, 10)) and abs(float(f[1]) - 3.7) < 0.01 and float(f[-1]) == 512.0


def test_output_head_initialisation():
    from bdm_amd.model import PointCloudModel
    torch.manual_seed(0)
    for t, last in (("simple", lambda m: m.output_projection), ("pvcnnplusplus", lambda m: m.output_projection[-1])):
        w = last(PointCloudModel(model_type=t, in_channels=3 + S).model).weight.detach()
        assert float(w.abs().max()) < 1e-5


@pytest.mark.parametrize("kind,N", CASES)
def test_restatement_matches_reference_golden(kind, N):
    g = golden(f"{kind}_full_n{N}.npz")
    from oracle.gen_golden import point_cloud_inputs
    m = filled(_module(kind).eval(), int(g["weight_seed"]))
    x = point_cloud_inputs(int(g["B"]), 3 + int(g["S"]), N, seed=int(g["input_seed"]))
    t = torch.from_numpy(g["t"])
    sd = m.state_dict()
    y = simple_forward(sd, x, t) if kind == "simple" else pvcnnpp_forward(sd, x, t)
    ref = torch.from_numpy(g["out"])
    err = float((y - ref).norm() / ref.norm())
    assert err <= 1e-6, err


@pytest.mark.parametrize("value", ["simple", "pvcnnplusplus"])
def test_config_accepts_model_type(value):
    from bdm_amd.config import parse_overrides
    cfg = parse_overrides([f"model.point_cloud_model={value}"])
    assert cfg.model.point_cloud_model == value
    from bdm_amd.model import get_model
    cfg.dataset.max_points = 64
    m = get_model(cfg)
    assert m.point_cloud_model.model_type == value


def test_early_sampler_off_for_simple_networks():
    from bdm_amd import pvcnn
    x = torch.zeros(1, 16, 3)
    for kind in ("simple", "pvcnnpp"):
        assert not hasattr(_module(kind), "sa_layers")
        assert pvcnn.early_first_sampler(_module(kind), x) is None


def test_merging_needs_pvcnn_recon_model():
    from bdm_amd.config import ProjectConfig
    from bdm_amd.model import get_fusion_model, get_model
    cfg = ProjectConfig()
    cfg.model.point_cloud_model = "simple"
    recon = get_model(cfg)
    with pytest.raises(ValueError, match="point_cloud_model"):
        get_fusion_model(cfg, None, recon)
