"""The drop-in seams of SURVEY section 8(b), kernels executed by the SIMT emulator build of the same sources:

* B1 (``experts_gemm``): every call the reference's own MoELayer makes in one bf16 forward / backward, replayed from
  tests/golden/seam_b1_calls.pt (arguments, the gradient that reached each output and the reference's results on its sequential_gemm
  fallback; oracle/make_golden_reference_cases.py) through the seam.
* B2 (attention): inside transformers' own Llama model, attention and mask code -- the classes the reference's AriaMoELMForCausalLM
  derives from (moe_lm.py:580-639 replace only the MLP) -- against the same model on eager attention, same bf16 weights and inputs."""
import os

import pytest
import torch

from tests.model_cases import rel_close

bf16 = torch.bfloat16

TEXT = dict(hidden_size=64, num_attention_heads=1, num_key_value_heads=1, num_hidden_layers=2, vocab_size=128, intermediate_size=64,
            rms_norm_eps=1e-6, rope_theta=5_000_000.0, max_position_embeddings=512, pad_token_id=0)


@pytest.fixture(scope="module", autouse=True)
def emu():
    from tests.emu import emu_lib

    emu_lib.install()
    yield
    emu_lib.uninstall()


def _init(module, std=0.08, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("norm.weight") or "layernorm" in n:
                p.fill_(1.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.dtype))


def test_b1_experts_gemm_inside_the_reference_moe_layer():
    from aria_amd import ops, seams

    recorded = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seam_b1_calls.pt"), map_location="cpu",
                          weights_only=False)
    assert len(recorded) == 2  # fc1 + fc2
    ns = type("moe_lm", (), {})()
    seams.install_experts_gemm(ns)
    calls, inner = [], ops.grouped_gemm
    ops.grouped_gemm = lambda *a, **k: (calls.append(k.get("w_is_kn", True)), inner(*a, **k))[1]
    try:
        for i, c in enumerate(recorded):
            x = c["input"].clone().requires_grad_(True)
            w = c["weight"].clone().requires_grad_(True)
            y = ns.experts_gemm(x, w, c["tokens_per_expert"])
            y.backward(c["grad_output"])
            for a, b, what in ((y.detach(), c["output"], "output"), (x.grad, c["grad_input"], "d input"), (w.grad, c["grad_weight"], "d weight")):
                rel_close(a, b, 2e-2, f"reference MoELayer's experts_gemm call {i} through seam B1: {what}")
    finally:
        ops.grouped_gemm = inner
    assert calls.count(True) == 2 and calls.count(False) == 2  # fc1 + fc2: forward ([E,K,N] form) and dgrad each, in the library


def _lm(attn):
    from transformers import LlamaConfig, LlamaForCausalLM

    lm = LlamaForCausalLM(LlamaConfig(**TEXT, attn_implementation=attn)).to(bf16)
    _init(lm, std=0.05)
    return lm.train()


@pytest.mark.parametrize("padded", [False, True])
def test_b2_attention_function_inside_the_reference_lm(padded):
    """transformers >= 4.48 route: ``attn_implementation="aria_hip"`` on the Llama causal LM the reference's AriaMoELMForCausalLM derives from selects
    aria_amd.seams.attention_interface; logits and gradients against the same model on eager attention."""
    from aria_amd import seams

    name = seams.register_attention("aria_hip")
    eager, ours = _lm("eager"), _lm(name)
    ours.load_state_dict(eager.state_dict())
    assert ours.config._attn_implementation == name
    ids = torch.randint(1, 128, (2, 40), generator=torch.Generator().manual_seed(3))
    mask = torch.ones(2, 40, dtype=torch.long)
    if padded:
        mask[1, 29:] = 0
    labels = ids.clone()
    labels[mask == 0] = -100

    def run(m):
        m.zero_grad()
        out = m(input_ids=ids, attention_mask=mask if padded else None, labels=labels)
        out.loss.backward()
        return out.logits.detach(), out.loss.detach(), m.model.layers[0].self_attn.q_proj.weight.grad.clone(), \
            m.model.embed_tokens.weight.grad.clone()

    lw, losw, gqw, gew = run(eager)
    lg, losg, gqg, geg = run(ours)
    # both runs are bf16 end to end: every valid position within 3e-2 of the logit scale, except at most 5 % of them within 2e-1
    keep = mask.bool()
    err = (lg.float() - lw.float()).abs().amax(-1)[keep]
    scale = lw.float().abs().max()
    assert (err <= 3e-2 * scale).float().mean() >= 0.95 and err.max() <= 2e-1 * scale, (err.topk(4).values, scale)
    assert abs(float(losg) - float(losw)) <= 2e-2 * abs(float(losw))
    rel_close(gqg, gqw, 6e-2, "d q_proj")
    rel_close(geg, gew, 6e-2, "d embed_tokens")


def test_b2_attention_class_with_the_4_46_signature():
    """transformers 4.46 route (the reference's pin): the class registered in LLAMA_ATTENTION_CLASSES is called by LlamaDecoderLayer with
    keywords and returns a 3-tuple; checked against the stock LlamaAttention (eager) on the same weights, 4-D additive mask, right padding."""
    import transformers.models.llama.modeling_llama as ml

    from aria_amd import seams

    cfg = ml.LlamaConfig(**TEXT, attn_implementation="eager")   # the base class of the reference's AriaMoELMConfig
    ref = ml.LlamaAttention(cfg, layer_idx=0).to(bf16)
    _init(ref, std=0.1)
    mine = seams.hf_attention_class()(cfg, layer_idx=0)
    mine.load_state_dict(ref.state_dict())
    B, S, D, hd = 2, 40, 64, 64
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, S, D, generator=g).to(bf16)
    gy = torch.randn(B, S, D, generator=g).to(bf16)
    rot = ml.LlamaRotaryEmbedding(cfg)
    pos = torch.arange(S)[None, :].expand(B, S)
    cos, sin = rot(x0, pos)
    n_valid = torch.tensor([S, 27])
    allowed = (torch.arange(S)[None, None, :] <= torch.arange(S)[None, :, None]) & (torch.arange(S)[None, None, :] < n_valid[:, None, None])
    add_mask = torch.zeros(B, 1, S, S).masked_fill(~allowed[:, None], torch.finfo(torch.float32).min).to(bf16)

    def run(attn, **kw):
        attn.zero_grad()
        x = x0.clone().requires_grad_(True)
        out = attn(hidden_states=x, attention_mask=add_mask, position_embeddings=(cos, sin), **kw)
        valid = (torch.arange(S)[None, :] < n_valid[:, None])[..., None]
        (out[0] * valid).backward(gy)
        return out, (out[0] * valid).detach(), x.grad.clone(), attn.q_proj.weight.grad.clone(), attn.o_proj.weight.grad.clone()

    ow, yw, dxw, gqw, gow = run(ref)
    og, yg, dxg, gqg, gog = run(mine, position_ids=pos, past_key_value=None, output_attentions=False, use_cache=False,
                                cache_position=torch.arange(S))
    assert len(og) == 3 and og[1] is None and og[2] is None
    rel_close(yg, yw, 3e-2, "attention output")
    rel_close(dxg, dxw, 6e-2, "dx")
    rel_close(gqg, gqw, 6e-2, "d q_proj")
    rel_close(gog, gow, 6e-2, "d o_proj")
    with pytest.raises(NotImplementedError):
        left = add_mask.flip(-1)
        mine(hidden_states=x0, attention_mask=left, position_embeddings=(cos, sin))


def test_b2_hf_generate_with_a_kv_cache_through_the_seam():
    """HF ``generate()`` as the reference drives it (README.md:45-88 quick-start path, ``aria/inference.py:102-130``; its LM's ``generate`` is
    LlamaForCausalLM's) with ``attn_implementation="aria_hip"``:
    prefill (causal, Sq == Skv) and single-query steps against the growing DynamicCache (Sq == 1 < Skv) both go through
    aria_amd.seams.attention_interface; greedy scores match eager attention step by step for as long as both picked the same tokens."""
    from aria_amd import seams

    name = seams.register_attention("aria_hip")
    eager, ours = _lm("eager").eval(), _lm(name).eval()
    ours.load_state_dict(eager.state_dict())
    ids = torch.randint(1, 128, (1, 12), generator=torch.Generator().manual_seed(3))
    kw = dict(max_new_tokens=6, do_sample=False, output_scores=True, return_dict_in_generate=True)
    with torch.no_grad():
        a, b = eager.generate(ids, **kw), ours.generate(ids, **kw)
    assert len(a.scores) == len(b.scores) == 6
    for step, (x, y) in enumerate(zip(a.scores, b.scores)):
        rel_close(y, x, 3e-2, f"greedy scores at step {step}")
        if int(a.sequences[0, 12 + step]) != int(b.sequences[0, 12 + step]):
            top2 = torch.topk(x.float().flatten(), 2).values
            assert float(top2[0] - top2[1]) <= 3e-2 * float(x.float().abs().max()), "a clear winner must be the same token"
            break


def test_image_rows_scatter_equals_masked_scatter_forward_and_backward():
    """modeling_aria.py:272-283 merges the projector's rows into the token embeddings with ``masked_scatter`` over a mask expanded along D;
    ``scatter_image_rows`` does it on the rows (no 42 M-element prefix sum / partition in the step): same values, same gradients."""
    import torch

    from aria_amd.modeling_aria import scatter_image_rows

    torch.manual_seed(0)
    B, S, D = 3, 17, 8
    is_img = torch.zeros(B, S, dtype=torch.bool)
    is_img[0, 2:6] = True
    is_img[1, 0] = True
    is_img[1, 13:16] = True          # sample 2: no image tokens at all
    n = int(is_img.sum())
    for feats_shape in ((2, n // 2, D), (n, D)):
        emb = torch.randn(B, S, D, requires_grad=True)
        emb2 = emb.detach().clone().requires_grad_(True)
        feats = torch.randn(*feats_shape, requires_grad=True)
        feats2 = feats.detach().clone().requires_grad_(True)
        got = scatter_image_rows(emb, is_img, feats)
        want = emb2.masked_scatter(is_img.unsqueeze(-1).expand_as(emb2), feats2)
        assert torch.equal(got, want)
        g = torch.randn_like(got)
        got.backward(g)
        want.backward(g)
        assert torch.equal(emb.grad, emb2.grad) and torch.equal(feats.grad, feats2.grad)
