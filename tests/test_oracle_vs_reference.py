"""Pin the oracle against the reference's own outputs on seeded random models and inputs (tests/golden/reference_cases.pt, recorded from
the reference by oracle/make_golden_reference_cases.py: inputs, outputs and gradients of every case below; the weights are rebuilt here
from the seeded draw list the case carries)."""
import os

import pytest
import torch

from oracle import aria_oracle as O

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cases.pt")


def seeded_weights(spec, seed):
    """spec: [(name, shape, mean, std)] in draw order -> {name: fp32 tensor}, every tensor drawn from ONE CPU generator seeded with
    ``seed`` (oracle/make_golden_reference_cases.py loads exactly these values into the reference before it records a case)."""
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(shape, generator=g) * std + mean for n, shape, mean, std in spec}


@pytest.fixture(scope="module")
def cases():
    out = torch.load(CASES, map_location="cpu", weights_only=False)
    for group in out.values():
        for c in group if isinstance(group, list) else []:
            c["weights"] = seeded_weights(c["weight_spec"], c["weight_seed"])
    return out


def _lm_config(text):
    return O.LMConfig(**{k: v for k, v in text.items() if k in O.LMConfig.__dataclass_fields__})


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_moe_layer_and_lm_match_live_reference(cases, seed):
    c = cases["moe_and_lm"][seed]
    w, ocfg = c["weights"], _lm_config(c["text"])
    with torch.no_grad():
        got = O.lm_forward(w["model.embed_tokens.weight"][c["ids"]], w, ocfg)
    assert torch.allclose(got, c["logits"], atol=2e-5, rtol=1e-4)
    wl = {k[len("model.layers.0.mlp."):]: v for k, v in w.items() if k.startswith("model.layers.0.mlp.")}
    out, im = O.moe_layer(c["x"], wl, "", ocfg, return_intermediates=True)
    assert torch.equal(im["indices"], c["indices"]) and torch.equal(im["tokens_per_expert"], c["tokens_per_expert"])
    assert torch.allclose(out, c["out"], atol=2e-5)


def test_lora_restatement_matches_the_reference_grouped_gemm_modules(cases):
    """aria/lora/layers.py's forward line (:129-139) is three calls of the reference's own GroupedGEMM module: ``want`` is that composition,
    ``merged_out`` the reference's GroupedGEMM on base + the oracle's delta weight, both recorded from the reference."""
    c = cases["lora_grouped"]
    with torch.no_grad():
        got = O.lora_grouped_gemm(c["x"], c["base"], c["a"], c["b"], c["tpe"], c["scaling"])
        assert torch.allclose(got, c["want"], atol=1e-5, rtol=1e-5)
        assert torch.equal(c["base"] + O.lora_delta_weight(c["a"], c["b"], c["scaling"]), c["merged_weight"])
        assert torch.allclose(c["merged_out"], c["want"], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("case", range(6))
def test_lm_matches_live_reference_over_random_shapes(cases, case):
    """heads x head_dim, experts / top-k / shared experts, depth, vocabulary, eps, RoPE base, batch and length drawn per case (a 60-case sweep
    of the same generator was run once offline: no mismatch)."""
    c = cases["lm_random"][case]
    w = c["weights"]
    with torch.no_grad():
        assert torch.allclose(O.lm_forward(w["model.embed_tokens.weight"][c["ids"]], w, _lm_config(c["text"])), c["logits"], atol=5e-5, rtol=2e-4)


@pytest.mark.parametrize("case", range(4))
def test_vit_and_projector_match_live_reference_over_random_shapes(cases, case):
    """tower width / heads / depth, image side (2..5 patches), query count and a random valid pixel rectangle per image (down to a single
    pixel) drawn per case; the key-padding mask must be equal, features of valid patches and the projector output within 5e-5
    (a 40-case sweep of the same generator was run once offline: no mismatch)."""
    c = cases["vit_random"][case]
    w, vatts = c["weights"], c["image_atts"]
    vc = O.VisionConfig(**{n: v for n, v in c["vision"].items() if n in O.VisionConfig.__dataclass_fields__})
    feat, atts = O.vit_forward(c["pixel_values"], c["pixel_mask"], w, "vision_tower.", vc)
    got = O.projector_forward(feat, atts, w, "multi_modal_projector.", O.AriaOracleConfig(vision=vc, patch_to_query=c["p2q"], projector_heads=c["heads"]))
    assert torch.equal(atts, vatts)
    assert torch.allclose(feat[~vatts], c["features"][~vatts], atol=5e-5, rtol=2e-4)
    assert torch.allclose(got, c["projected"], atol=5e-5, rtol=2e-4)


@pytest.mark.parametrize("case", range(4))
def test_moe_training_path_matches_live_reference_over_random_shapes(cases, case):
    """MoELayer in train mode (z-loss and load-balancing gradients injected through MoEAuxLossAutoScaler with a random scale): output, dx and
    every parameter gradient of the oracle against the reference module (a 30-case sweep was run once offline: no mismatch)."""
    c = cases["moe_train_random"][case]
    O._AuxLossScaler.scale = c["scale"]
    try:
        w = {n: v.detach().clone().requires_grad_(True) for n, v in c["weights"].items()}
        xo = c["x"].clone().requires_grad_(True)
        yo = O.moe_layer(xo, w, "", _lm_config(c["text"]), training=True)
        yo.backward(c["gy"])
    finally:
        O._AuxLossScaler.scale = 1.0
    assert torch.allclose(yo, c["y"], atol=2e-5, rtol=1e-4) and torch.allclose(xo.grad, c["dx"], atol=5e-5, rtol=2e-4)
    for n, g in c["grads"].items():
        assert torch.allclose(w[n].grad, g, atol=5e-5, rtol=2e-4), n
