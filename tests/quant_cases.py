"""Int8 weight-only quantization (aria_amd/quantize.py, the *_w8 kernels of csrc/decode.hip): cases shared by the emulator
(test_emu_quant.py) and the MI355X (test_gpu_quant.py)."""
import os
import subprocess
import sys

import torch

from tests.model_cases import rel_close

bf16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def toy_args(head_dim=64, n_layer=2):
    from aria_amd import gptfast as G

    H = 2
    return G.ModelArgs(block_size=64, vocab_size=136, n_layer=n_layer, n_head=H, dim=H * head_dim, intermediate_size=40, n_local_heads=H,
                       head_dim=head_dim, rope_base=10000.0, norm_eps=1e-5, num_experts=8, router_topk=3, num_shared_experts=2)


def toy_model(args, seed=12):
    from aria_amd import gptfast as G

    torch.manual_seed(seed)
    m = G.Transformer(args)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.ones(p.shape) + 0.1 * torch.randn(p.shape)).to(bf16) if "norm" in n else (torch.randn(p.shape) * 0.08).to(bf16))
    return m


# ------------------------------------------------------------------------------------------------ 1. quantizer (CPU, no library)
def case_quantizer():
    from aria_amd.quantize import quantize_rows

    g = torch.Generator().manual_seed(0)
    w = (torch.randn(37, 200, generator=g) * torch.rand(37, 1, generator=g) * 3).to(bf16)
    w[5] = 0
    q, s = quantize_rows(w)
    assert q.dtype == torch.int8 and s.dtype == bf16 and s.shape == (37,)
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    assert torch.isfinite(s.float()).all() and (q[5] == 0).all()
    sf = s.float().unsqueeze(-1)
    err = (w.float() - q.float() * sf).abs()
    assert (err <= 0.5 * sf * (1 + 2 ** -8)).all(), float((err / sf).max())
    q2, s2 = quantize_rows(w.clone())
    assert torch.equal(q, q2) and torch.equal(s, s2)


def case_state_dict_layout():
    """key set and dtypes of quantize_int8_ (gpt-fast's int8 naming) and of quantize_state_dict; save -> load_model_pth round trip is bit-exact;
    a mismatched shape raises"""
    from aria_amd import gptfast as G
    from aria_amd.quantize import quantize_int8_, quantize_state_dict

    args = toy_args()
    m = toy_model(args)
    sd_bf16 = {k: v.clone() for k, v in m.state_dict().items()}
    quantize_int8_(m)
    sd = m.state_dict()
    E, I, D, Is = args.num_experts, args.intermediate_size, args.dim, args.intermediate_size * args.num_shared_experts
    p = "layers.0."
    want = {p + "attention.wqkv.weight": (torch.int8, (3 * D, D)), p + "attention.wqkv.scales": (bf16, (3 * D,)),
            p + "attention.wo.weight": (torch.int8, (D, D)), p + "attention.wo.scales": (bf16, (D,)),
            p + "feed_forward.gate.weight": (bf16, (E, D)),
            p + "feed_forward.cond_ffn.w1": (torch.int8, (E, I, D)), p + "feed_forward.cond_ffn.scales1": (bf16, (E, I)),
            p + "feed_forward.cond_ffn.w2": (torch.int8, (E, D, I)), p + "feed_forward.cond_ffn.scales2": (bf16, (E, D)),
            p + "feed_forward.cond_ffn.w3": (torch.int8, (E, I, D)), p + "feed_forward.cond_ffn.scales3": (bf16, (E, I)),
            p + "feed_forward.shared_ffn.w1.weight": (torch.int8, (Is, D)), p + "feed_forward.shared_ffn.w1.scales": (bf16, (Is,)),
            p + "feed_forward.shared_ffn.w2.weight": (torch.int8, (D, Is)), p + "feed_forward.shared_ffn.w2.scales": (bf16, (D,)),
            p + "attention_norm.weight": (bf16, (D,)), "tok_embeddings.weight": (bf16, (args.vocab_size, D)),
            "output.weight": (torch.int8, (args.vocab_size, D)), "output.scales": (bf16, (args.vocab_size,)), "norm.weight": (bf16, (D,))}
    for k, (dt, shape) in want.items():
        assert sd[k].dtype == dt and tuple(sd[k].shape) == shape, (k, sd[k].dtype, tuple(sd[k].shape))
    sd2 = quantize_state_dict(sd_bf16)   # the offline form (python -m aria_amd.quantize) gives the same tensors
    assert sorted(sd2) == sorted(sd)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    # round trip through torch.save / load_model_pth into a fresh bf16 model
    import io

    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    m2 = G.Transformer(args)
    G.load_model_pth(m2, torch.load(buf, weights_only=True), strict=True)
    assert m2._w8
    for (k, a), (k2, b) in zip(sorted(m.state_dict().items()), sorted(m2.state_dict().items())):
        assert k == k2 and a.dtype == b.dtype and torch.equal(a, b), k
    bad = dict(sd)
    bad["layers.0.attention.wo.weight"] = bad["layers.0.attention.wo.weight"][:, :-8].contiguous()
    try:
        G.load_model_pth(G.Transformer(args), bad)
    except ValueError:
        pass
    else:
        raise AssertionError("a mismatched int8 shape must raise")
    bad = dict(sd)
    bad["layers.0.attention.wo.scales"] = bad["layers.0.attention.wo.scales"].float()
    try:
        G.load_model_pth(G.Transformer(args), bad)
    except ValueError:
        pass
    else:
        raise AssertionError("a mismatched scale dtype must raise (nothing is cast)")


def case_quantized_is_inference_only():
    from aria_amd import gptfast as G
    from aria_amd.expert_parallel import shard_expert_weights
    from aria_amd.lora import apply_lora_to_experts
    from aria_amd.quantize import quantize_int8_

    m = quantize_int8_(toy_model(toy_args()))
    for call in (lambda: apply_lora_to_experts(m), lambda: shard_expert_weights(m.layers[0].feed_forward.cond_ffn.w1,
                                                                                    m.layers[0].feed_forward.cond_ffn.w2, 0, 2)):
        try:
            call()
        except NotImplementedError:
            pass
        else:
            raise AssertionError("LoRA / EP on an int8 model must raise")
    assert isinstance(m, G.Transformer)


def case_aria_width_bytes():
    """At Aria's real widths (28 layers, V 100 352) the quantized LM's parameter + buffer bytes are <= 0.52 x the bf16 LM's (meta device)."""
    from aria_amd import gptfast as G
    from aria_amd.quantize import convert_structure_

    def nbytes(mod):
        return sum(t.numel() * t.element_size() for t in list(mod.parameters()) + list(mod.buffers()))

    with torch.device("meta"):
        m = G.Transformer(G.ModelArgs())
    b = nbytes(m)
    convert_structure_(m)
    r = nbytes(m) / b
    assert r <= 0.52, r
    return r


# ------------------------------------------------------------------------------------------------ 2. dequant kernel
def case_dequant(dev, shapes=((3, 8), (5, 13), (7, 1000), (64, 136), (2, 2560))):
    from aria_amd import ops

    g = torch.Generator().manual_seed(1)
    for shape in shapes:
        q = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
        q.view(-1)[:3] = torch.tensor([-128, 127, 0], dtype=torch.int8)
        s = (torch.rand(shape[:-1], generator=g) * 0.05 + 1e-4).to(bf16)
        got = ops.dequant_w8(q.to(dev), s.to(dev)).cpu()
        want = (q.float() * s.float().unsqueeze(-1)).to(bf16)
        assert torch.equal(got, want), shape


def case_dequant_expert_tensor(dev):
    """Aria's expert tensor [64 * 1664, 2560] (GPU only: 272 M codes)"""
    from aria_amd import ops

    q = torch.randint(-128, 128, (64 * 1664, 2560), dtype=torch.int8, device=dev)
    s = (torch.rand(64 * 1664, device=dev) * 0.05 + 1e-4).to(bf16)
    got = ops.dequant_w8(q, s)
    for r0 in (0, 50_000, 64 * 1664 - 64):   # slices: the reference in fp32 on the device
        want = (q[r0:r0 + 64].float() * s[r0:r0 + 64].float().unsqueeze(-1)).to(bf16)
        assert torch.equal(got[r0:r0 + 64], want), r0
    assert torch.equal(got, (q.float() * s.float().unsqueeze(-1)).to(bf16))


# ------------------------------------------------------------------------------------------------ 3. stand-alone int8 GEMV
def case_gemv(dev, Ks=(2560, 1664, 3328, 136, 1000), Ns=(37, 2560, 4100)):
    from aria_amd import ops
    from aria_amd.quantize import quantize_rows

    g = torch.Generator().manual_seed(2)
    for K in Ks:
        for N in Ns:
            for norm, res in ((False, False), (True, True), (True, False), (False, True)):
                w = (torch.randn(N, K, generator=g) * 0.05).to(bf16)
                q, s = quantize_rows(w)
                x = torch.randn(K, generator=g).to(bf16)
                nw = (1 + 0.1 * torch.randn(K, generator=g)).to(bf16) if norm else None
                r = torch.randn(N, generator=g).to(bf16) if res else None
                got = ops.gemv_w8(q.to(dev), s.to(dev), x.to(dev), None if nw is None else nw.to(dev), 1e-5,
                                  None if r is None else r.to(dev)).cpu()
                xd = x.double()
                if norm:
                    xd = (xd * torch.rsqrt(xd.pow(2).mean() + 1e-5)).to(bf16).double() * nw.double()
                y = xd @ (q.double() * s.double().unsqueeze(-1)).t()
                want = y.to(bf16) if r is None else (r.double() + y.to(bf16).double()).to(bf16)
                e = (got.double() - want.double()).norm() / want.double().norm()
                assert e <= 1e-2, (K, N, norm, res, float(e))


# ------------------------------------------------------------------------------------------------ 4. engine vs dequantizing tile path
def case_engine_vs_tile(dev, head_dim=64, max_seq=24):
    from aria_amd.quantize import quantize_int8_

    args = toy_args(head_dim)
    outs = {}
    for use_engine in (False, True):
        m = quantize_int8_(toy_model(args)).to(dev).eval()
        m.use_decode_engine = use_engine
        m.setup_caches(1, max_seq)
        ids = torch.tensor([[5, 9, 77, 3, 100]], device=dev)
        logs = []
        with torch.no_grad():
            lg = m(ids, torch.arange(5, device=dev))
            logs.append(lg[:, -1].float().cpu())
            for step, t in enumerate((17, 33, 2, 90)):
                lg = m(torch.tensor([[t]], device=dev), torch.tensor([5 + step], device=dev, dtype=torch.int32))
                logs.append(lg[:, -1].float().cpu().clone())
        kc = m.layers[1].attention.kv_cache
        outs[use_engine] = (logs, kc.k.float().cpu().clone(), kc.v.float().cpu().clone(), m._engine is not None and m._engine.w8)
    assert outs[True][3] and not outs[False][3], "the int8 engine must serve the engine run, and only it"
    for a, b in zip(outs[True][0], outs[False][0]):
        rel_close(a, b, 3e-2, "int8 engine logits vs dequantizing tile path")
        top2 = torch.topk(b.flatten(), 2).values
        if float(top2[0] - top2[1]) > 0.05 * float(b.abs().max()):
            assert int(a.argmax()) == int(b.argmax())
    rel_close(outs[True][1], outs[False][1], 3e-2, "k cache")
    rel_close(outs[True][2], outs[False][2], 3e-2, "v cache")


# ------------------------------------------------------------------------------------------------ 5. Aria width, one layer, vs the fp32 oracle
def _dequantized_hf(llm, od, layers=None):
    """the int8 model's weights as fp32 q.float() * s.float() (bf16 tensors as they are), mapped to the oracle's HF keys through
    checkpoint.gptfast_to_hf, one layer at a time (keys without the ``language_model.`` prefix, on ``od``)"""
    from aria_amd.checkpoint import gptfast_to_hf

    c = llm.config
    sd = llm.state_dict()

    def val(k):
        v = sd[k]
        if v.dtype != torch.int8:
            return v.float()
        sk = k[: -len("weight")] + "scales" if k.endswith(".weight") else k[:-2] + "scales" + k[-1]
        return v.float() * sd[sk].float().unsqueeze(-1)

    wf = {}
    groups = [[k for k in sd if not k.startswith("layers.")]]
    groups += [[k for k in sd if k.startswith(f"layers.{i}.")] for i in range(layers if layers is not None else c.n_layer)]
    for keys in groups:
        part = {"llm." + k: val(k) for k in keys if "scales" not in k}
        for k, v in gptfast_to_hf(part, c.n_head, c.head_dim).items():
            wf[k[len("language_model."):]] = v.to(od)
        del part
    return wf


def case_engine_aria_width(dev, n_tokens=2):
    """The int8 engine at Aria's real layer widths (the production instantiations: 5 / 4 / 7 chunks per lane, R = 4 routed up-projection,
    the (4, 7) down-projection) on ONE layer with a small vocabulary: tokens fed one at a time from an empty cache (every step an engine step),
    the last logits against the fp32 oracle over the whole sequence on the dequantized weights q.float() * s.float()."""
    from oracle import aria_oracle as O
    from tests.model_cases import _aria_width_gptfast, lmcfg

    from aria_amd.quantize import quantize_int8_

    m, _, d = _aria_width_gptfast(dev)
    quantize_int8_(m)
    m.use_decode_engine = True
    m.setup_caches(1, 16)
    ids = torch.tensor([5, 77, 300, 12, 401, 9][:n_tokens])
    with torch.no_grad():
        for t in range(n_tokens):
            lg = m(ids[t].view(1, 1).to(dev), torch.tensor([t], dtype=torch.int32, device=dev))
    assert m._engine is not None and m._engine.w8
    wf = _dequantized_hf(m, "cpu")
    with torch.no_grad():
        want = O.lm_forward(wf["model.embed_tokens.weight"][ids][None], wf, lmcfg(d))[0, -1]
    rel_close(lg.view(-1).float().cpu(), want, 3e-2, "Aria-width int8 engine vs oracle")


# ------------------------------------------------------------------------------------------------ 6. full depth (GPU)
def case_engine_full_depth(dev, case="int8_config2_28layers_prefill280_decode16", *, layers=28, vocab=100352, prompt=280, new_tokens=16,
                           seed=65, block_tol=1.7e-2):
    """Config #2's path on an int8 model at Aria's widths: prefill ``prompt`` positions (the dequantizing tile path), then ``new_tokens``
    greedy steps of aria_decode_token_w8.  After every step the engine's logits are compared with the fp32 oracle over the whole sequence on
    the dequantized weights (on the device), routing forced to what the device chose (prefill: ops.moe_route; steps: the engine's routing
    record).  Tolerances and per-layer router checks are case_decode_full_depth's (tests/fullwidth_cases.py), whose helpers this reuses."""
    from oracle import aria_oracle as O
    from tests import fullwidth_cases as F

    from aria_amd import gptfast as G
    from aria_amd.quantize import quantize_int8_

    hidden, heads, experts, topk, inter = 2560, 20, 64, 6, 1664
    F.oracle_device_pin(dev, hidden=hidden, heads=heads, experts=experts, topk=topk, inter=inter)
    ocfg = O.LMConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=heads, vocab_size=vocab,
                      moe_intermediate_size=inter, moe_num_experts=experts, moe_topk=topk)
    args = G.ModelArgs(block_size=prompt + new_tokens + 8, vocab_size=vocab, n_layer=layers, n_head=heads, dim=hidden, intermediate_size=inter,
                       rope_base=ocfg.rope_theta, norm_eps=ocfg.rms_norm_eps, num_experts=experts, router_topk=topk, num_shared_experts=2)
    with torch.device(dev):
        tf = G.Transformer(args)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for n, p in tf.named_parameters():
            if "norm" in n:
                p.copy_((torch.randn(p.shape, generator=g, device=dev) * 0.1 + 1.0).to(bf16))
            else:
                p.copy_((torch.randn(p.shape, generator=g, device=dev) * 0.02).to(bf16))
    quantize_int8_(tf)
    tf = tf.eval()
    tf.use_decode_engine = True
    tf.setup_caches(1, prompt + new_tokens + 8)
    ids = torch.randint(0, vocab, (1, prompt), generator=torch.Generator().manual_seed(seed + 1))
    with F._Recorder() as rec, torch.no_grad():
        lg = tf(ids.to(dev), torch.arange(prompt, device=dev), last_only=True).float().reshape(-1)
    assert len(rec.idx) == layers
    step_logits, step_idx, toks = [lg], [], []
    with torch.no_grad():
        for t in range(new_tokens):
            tok = int(step_logits[-1].argmax())
            toks.append(tok)
            lg = tf(torch.tensor([[tok]], device=dev), torch.tensor([prompt + t], dtype=torch.int32, device=dev)).float().reshape(-1)
            assert tf._engine is not None and tf._engine.w8, "the single-token step did not take the int8 engine"
            step_idx.append(tf._engine.routing_trace()[1].long().cpu())
            step_logits.append(lg.clone())
    wf = _dequantized_hf(tf, dev)
    del tf
    torch.cuda.empty_cache()
    seq = torch.cat([ids[0], torch.tensor(toks)]).to(dev)
    forced = [torch.cat([rec.idx[l]] + [step_idx[s][l][None] for s in range(new_tokens)]) for l in range(layers)]
    with O.forced_routing(forced), torch.no_grad():
        h = O.lm_forward(wf["model.embed_tokens.weight"][seq[None]], wf, ocfg, return_hidden=True)
        want_all = torch.nn.functional.linear(h[0, prompt - 1:], wf["lm_head.weight"])
    tol = F._depth_tol(block_tol, layers - 1, layers)
    rep = F.REPORT.setdefault(case, {})
    rep.update(layers=layers, prompt=prompt, new_tokens=new_tokens, tokens=toks)
    margins_ok = 0
    for t in range(new_tokens + 1):
        want = want_all[t]
        m = F.metrics(step_logits[t], want)
        rep[f"step{t:02d} logits"] = {k: round(v, 6) for k, v in m.items()}
        assert m["rel_l2"] <= tol and m["max_rel"] <= 2 * tol and m["cos"] >= 1 - 2 * tol * tol, (case, t, m, tol)
        top2 = want.topk(2).values
        if t < new_tokens and float(top2[0] - top2[1]) > 2 * float((step_logits[t] - want).abs().max()):
            margins_ok += 1
            assert int(want.argmax()) == toks[t], f"{case}: step {t}: the oracle's arg-max differs from the engine's token on a resolvable margin"
    rep["tokens_checked_on_resolvable_margin"] = margins_ok
    return rep


# ------------------------------------------------------------------------------------------------ 7. prefill equivalence
def case_prefill_equivalence(dev, head_dim=64, S=7):
    """A quantized model's prefill (full logits, KV caches) equals BIT FOR BIT a bf16 model holding bf16(q * s): the dequantizing path feeds the
    same tile kernels the same bf16 weights."""
    from aria_amd import gptfast as G
    from aria_amd.quantize import quantize_int8_

    args = toy_args(head_dim)
    mq = quantize_int8_(toy_model(args))
    mb = G.Transformer(args)
    sd = {}
    for k, v in mq.state_dict().items():
        if k.endswith("scales") or k[-7:-1] == "scales":
            continue
        if v.dtype == torch.int8:
            sk = k[: -len("weight")] + "scales" if k.endswith(".weight") else k[:-2] + "scales" + k[-1]
            v = (v.float() * mq.state_dict()[sk].float().unsqueeze(-1)).to(bf16)
        sd[k] = v
    mb.load_state_dict(sd, strict=True)
    res = []
    for m in (mq, mb):
        m = m.to(dev).eval()
        m.setup_caches(1, 16)
        ids = torch.tensor([[5, 9, 77, 3, 100, 4, 8][:S]], device=dev)
        with torch.no_grad():
            lg = m(ids, torch.arange(S, device=dev), last_only=False).cpu()
        c = m.layers[-1].attention.kv_cache
        res.append((lg, c.k.cpu().clone(), c.v.cpu().clone()))
    for a, b, what in zip(res[0], res[1], ("logits", "k cache", "v cache")):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ 8. surface
def case_generate(dev):
    from aria_amd import gptfast as G
    from aria_amd.quantize import quantize_int8_

    torch.manual_seed(3)
    args = toy_args(64)
    a = G.Aria(args, vision_config=_tiny_vision())
    with torch.no_grad():
        for n, p in a.llm.named_parameters():
            p.copy_((torch.ones(p.shape) + 0.1 * torch.randn(p.shape)).to(bf16) if "norm" in n else (torch.randn(p.shape) * 0.08).to(bf16))
    quantize_int8_(a)
    a = a.to(dev).eval()
    out, _ = G.generate(a, torch.tensor([[5, 9, 77, 3]], device=dev), 5, top_k=1, temperature=1.0)
    assert out.shape == (4 + 5,) and int(out.max()) < args.vocab_size
    return out


def _tiny_vision():
    from aria_amd.vision import AriaVisionConfig

    return AriaVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)


class _Tok:
    def encode(self, s):
        return [1]

    def decode(self, ids):
        return " ".join(str(i) for i in ids)


class _Proc:
    tokenizer = _Tok()

    def apply_chat_template(self, messages, add_generation_prompt=True):
        return messages[0]["content"]

    def __call__(self, text, images=None, return_tensors="pt"):
        return {"input_ids": torch.tensor([[5, 9, 77, 3]])}


def case_generator_from_int8_checkpoint(dev, tmp_path):
    """python -m aria_amd.quantize writes model_int8.pth; Generator's own loader (load_model_and_processor, shapes from ModelConfig) builds
    the int8 structure from it and generates -- the same greedy tokens as the bf16 model quantized in memory"""
    from aria_amd import gptfast as G
    from aria_amd import gptfast_generate as GG
    from aria_amd.quantize import quantize_int8_

    args = toy_args(64)
    torch.manual_seed(4)
    a = G.Aria(args, vision_config=_tiny_vision())
    with torch.no_grad():
        for n, p in a.named_parameters():
            p.copy_((torch.ones(p.shape) + 0.1 * torch.randn(p.shape)).to(bf16) if "norm" in n else (torch.randn(p.shape) * 0.08).to(bf16))
    torch.save(a.state_dict(), str(tmp_path / "model.pth"))
    r = subprocess.run([sys.executable, "-m", "aria_amd.quantize", "--checkpoint_path", str(tmp_path / "model.pth")], cwd=ROOT,
                       capture_output=True, text=True, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "model_int8.pth").exists()
    mc = GG.ModelConfig(tmp_path / "model_int8.pth", device=dev, model_args=args, vision_config=_tiny_vision())
    gen = GG.Generator(mc, GG.GenerationConfig(max_new_tokens=4, top_k=1, temperature=1.0, stop_strings=[]), processor=_Proc())
    assert gen.model.llm._w8 and gen.model.llm.output.weight.dtype == torch.int8
    # (same seed for both: top_k = 1 keeps every logit tied for the maximum, and the toy model has exact ties -- the sampler's draws pick)
    torch.manual_seed(0)
    out = gen.generate([{"role": "user", "content": "hi"}], detokenize=False)
    torch.manual_seed(0)
    want, _ = G.generate(quantize_int8_(a).to(dev).eval(), torch.tensor([[5, 9, 77, 3]], device=dev), 4, top_k=1, temperature=1.0)
    assert torch.equal(out.cpu(), want[4:].cpu()), (out, want)
    return out


def case_bf16_load_unchanged(dev):
    """The bf16 path is untouched by the int8 one: a bf16 model.pth state dict loaded through load_model_pth (its bf16 branch) decodes bit for
    bit like the model it was saved from, and both decode the same bits before and after an int8 model has run in the process (shared
    library state, the engine, the dequant scratch)."""
    from aria_amd import gptfast as G
    from aria_amd.quantize import quantize_int8_

    args = toy_args(64)

    def run(m):
        m = m.to(dev).eval()
        m.setup_caches(1, 16)
        with torch.no_grad():
            lg0 = m(torch.tensor([[5, 9, 77]], device=dev), torch.arange(3, device=dev)).cpu()
            lg1 = m(torch.tensor([[17]], device=dev), torch.tensor([3], device=dev, dtype=torch.int32)).cpu().clone()
        return lg0, lg1, m._engine is not None and not m._engine.w8

    direct = toy_model(args)
    before = run(direct)
    qm = quantize_int8_(toy_model(args)).to(dev).eval()
    qm.setup_caches(1, 16)
    with torch.no_grad():
        qm(torch.tensor([[5, 9, 77]], device=dev), torch.arange(3, device=dev))
        qm(torch.tensor([[17]], device=dev), torch.tensor([3], device=dev, dtype=torch.int32))
    loaded = G.Transformer(args)
    G.load_model_pth(loaded, {k: v.cpu() for k, v in toy_model(args).state_dict().items()}, strict=True)
    assert not loaded._w8
    for after in (run(direct), run(loaded)):
        assert before[2] and after[2]
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def case_head_wide(dev):
    """The dequantizing path's last_only head on a width aria_gemv_w8 does not take (K > 4096): the dequant + GEMM branch, not an error"""
    from types import SimpleNamespace

    from aria_amd import ops
    from aria_amd.quantize import head_logits, quantize_rows

    K, V = 4104, 24
    g = torch.Generator().manual_seed(5)
    q, s = quantize_rows((torch.randn(V, K, generator=g) * 0.05).to(bf16))
    out = SimpleNamespace(weight=q.to(dev), scales=s.to(dev))
    llm = SimpleNamespace(config=SimpleNamespace(dim=K, num_experts=1, intermediate_size=8, num_shared_experts=1, vocab_size=V), output=out)
    h = torch.randn(2, K, generator=g).to(bf16).to(dev)
    got = head_logits(llm, h, True)
    want = ops.gemm(h, (q.float() * s.float().unsqueeze(-1)).to(bf16).to(dev))
    assert torch.equal(got.cpu(), want.cpu())
