"""Prefill at a cache offset (aria_attn_fwd_offset, Transformer.forward with input_pos = p0 + arange(S), generate's prefill_chunk /
cached_prefix, Generator's reuse_prefix): cases shared by the emulator (test_emu_prefill_offset.py) and the MI355X
(test_gpu_prefill_offset.py)."""
import contextlib
import types

import pytest
import torch

from oracle import aria_oracle as O
from tests.kernel_cases import close
from tests.model_cases import rel_close
from tests.quant_cases import _Tok, _tiny_vision, toy_args, toy_model

bf16 = torch.bfloat16
JUNK = 100.0   # what cache rows nobody has written yet hold in these tests: finite, and one wrongly visible key wrecks the row


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _offset_inputs(B, H, Sq, q_off, Skv, hd):
    D = H * hd
    g = torch.Generator().manual_seed(1000 * B + 100 * H + Sq + 7 * q_off + Skv + hd)
    q = torch.randn(B * Sq, D, generator=g).to(bf16)
    kv = torch.randn(B, Skv, 2 * D, generator=g).to(bf16)
    kv[:, q_off + Sq:] = JUNK
    return q, kv.reshape(B * Skv, 2 * D)


def case_kernel(dev, B, H, Sq, q_off, Skv, hd, kv_len=None):
    """O and LSE of the offset launch against the fp32 oracle on the live rows: O.attention_eager is bottom-right aligned for sq != sk
    (query i sees keys <= sk - sq + i = q_off + i).  K / V have Skv rows per batch entry; the rows behind q_off + Sq hold JUNK."""
    from aria_amd import hip, ops

    D, live, scale = H * hd, q_off + Sq, hd ** -0.5
    q, kv = _offset_inputs(B, H, Sq, q_off, Skv, hd)
    kl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32)
    kvd = kv.to(dev)
    o, lse = ops.attention_fwd(q.to(dev), kvd[:, :D], kvd[:, D:], B, Sq, H, hd, scale, True, kv_len=None if kl is None else kl.to(dev),
                               Skv=Skv, q_offset=q_off)
    assert hip.get_lib().cdll.aria_last_attn_fwd_variant() == (3 if hd == 128 else 2)
    qh = q.float().view(B, Sq, H, hd).transpose(1, 2)
    kh, vh = (kv[:, i * D:(i + 1) * D].float().view(B, Skv, H, hd).transpose(1, 2)[:, :, :live] for i in range(2))
    pad = None if kl is None else torch.arange(live)[None, :] >= kl[:, None].long()
    want = torch.cat([O.attention_eager(qh[b:b + 1], kh[b:b + 1], vh[b:b + 1], scale, True, key_padding=None if pad is None else pad[b:b + 1])
                      for b in range(B)])
    close(o, want.transpose(1, 2).reshape(B * Sq, D), 2e-2, 2e-2)
    s = (qh @ kh.transpose(2, 3)) * scale
    dead = torch.arange(live)[None, :] > (q_off + torch.arange(Sq))[:, None]
    s = s.masked_fill(dead[None, None], float("-inf"))
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    close(lse, torch.logsumexp(s, dim=-1), 1e-3, 1e-3)


def case_zero_offset_is_plain_causal(dev, hd, B=2, H=2, S=330):
    """q_off = 0 with Sq == Skv walks the same tiles with a zero added to every position: O and LSE equal aria_attn_fwd(causal = 1) bit
    for bit.  Both exports are called directly."""
    from aria_amd import hip

    D = H * hd
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(B * S, 3 * D, generator=g).to(bf16).to(dev)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    lib = hip.get_lib()
    res = []
    for offset in (False, True):
        o = torch.empty(B * S, D, dtype=bf16, device=dev)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), None, None, B, S, S)
        tail = (H, hd, 3 * D, 3 * D, 3 * D, D, hd ** -0.5)
        if offset:
            lib.call("aria_attn_fwd_offset", *head, 0, *tail, None)
        else:
            lib.call("aria_attn_fwd", *head, *tail, 1, None)
        res.append((o.cpu(), lse.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def case_validation(dev):
    """Positions the launch cannot serve are refused before anything is enqueued."""
    from aria_amd import hip, ops

    H, hd = 2, 64
    q = torch.zeros(8, H * hd, dtype=bf16, device=dev)
    kv = torch.zeros(16, H * hd, dtype=bf16, device=dev)
    with pytest.raises(hip.AriaHipError, match="aria_attn_fwd_offset"):
        ops.attention_fwd(q, kv, kv, 1, 8, H, hd, 1.0, True, Skv=16, q_offset=9)      # q_off + Sq > Skv
    with pytest.raises(hip.AriaHipError, match="aria_attn_fwd_offset"):
        ops.attention_fwd(q, kv, kv, 1, 8, H, hd, 1.0, True, Skv=16, q_offset=-1)
    q72, kv72 = torch.zeros(8, 72, dtype=bf16, device=dev), torch.zeros(16, 72, dtype=bf16, device=dev)
    with pytest.raises(hip.AriaHipError, match="aria_attn_fwd_offset"):
        ops.attention_fwd(q72, kv72, kv72, 1, 8, 1, 72, 1.0, True, Skv=16, q_offset=4)  # hd 72 (the ViT) is never causal
    with pytest.raises(ValueError):
        ops.attention_fwd(q, kv, kv, 1, 8, H, hd, 1.0, False, Skv=16, q_offset=4)


# ------------------------------------------------------------------------------------------------ 2. the model, toy widths
def _ids43():
    return torch.randint(0, 136, (1, 43), generator=torch.Generator().manual_seed(43))


def _junk_caches(m):
    for layer in m.layers:
        layer.attention.kv_cache.k.fill_(JUNK)
        layer.attention.kv_cache.v.fill_(JUNK)


def case_model_continuation(dev, head_dim, int8=False):
    """43 tokens: prefill [:17] at 0, [17:40] at input_pos = 17 + arange(23), then three single-token steps -- against the cache-free
    forward (bf16) or the model's own one-shot prefill (int8), with the bounds case_gptfast_golden holds the one-shot prefill (2e-2) and
    the decode steps (3e-2) to; the cache rows 0..39 of the last layer against a one-shot 40-token prefill's."""
    m = toy_model(toy_args(head_dim))
    if int8:
        from aria_amd.quantize import quantize_int8_

        m = quantize_int8_(m)
    m = m.to(dev).eval()
    ids = _ids43().to(dev)
    with torch.no_grad():
        if int8:
            m.setup_caches(1, 48)
            full = m(ids, torch.arange(43, device=dev)).float().cpu()
        else:
            m.setup_caches(1, 43, training=True)
            full = m(ids).float().cpu()
            m.max_seq_length = -1
            m.setup_caches(1, 48)
        m(ids[:, :40], torch.arange(40, device=dev))
        c = m.layers[-1].attention.kv_cache
        k_ref, v_ref = c.k[:, :40].float().cpu().clone(), c.v[:, :40].float().cpu().clone()
        _junk_caches(m)
        m(ids[:, :17], torch.arange(17, device=dev))
        cont = m(ids[:, 17:40], 17 + torch.arange(23, device=dev))
        rel_close(cont, full[:, 17:40], 2e-2, "continuation at 17 vs the whole sequence")
        for t in range(40, 43):
            step = m(ids[:, t:t + 1], torch.tensor([t], device=dev, dtype=torch.int32))
            rel_close(step[:, 0], full[:, t], 3e-2, f"decode step {t} behind a continuation")
        if not int8:
            assert m._engine is not None   # the steps went through the decode engine
        c = m.layers[-1].attention.kv_cache
        rel_close(c.k[:, :40], k_ref, 2e-2, "k cache rows 0..39")
        rel_close(c.v[:, :40], v_ref, 2e-2, "v cache rows 0..39")
        last = m(ids[:, 17:40], 17 + torch.arange(23, device=dev), last_only=True)
        rel_close(last[:, 0], full[:, 39], 2e-2, "last_only continuation")


def case_model_batch2(dev, head_dim=64):
    """B = 2: the cache's batch stride (S_max rows) is larger than the live length, which rides in kv_len."""
    m = toy_model(toy_args(head_dim)).to(dev).eval()
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 136, (2, 30), generator=g).to(dev)
    with torch.no_grad():
        m.setup_caches(2, 30, training=True)
        full = m(ids).float().cpu()
        m.max_seq_length = -1
        m.setup_caches(2, 40)
        _junk_caches(m)
        m(ids[:, :11], torch.arange(11, device=dev))
        cont = m(ids[:, 11:], 11 + torch.arange(19, device=dev))
    rel_close(cont, full[:, 11:], 2e-2, "B = 2 continuation")


def case_model_errors(dev):
    m = toy_model(toy_args(64)).to(dev).eval()
    ids = _ids43().to(dev)
    m.setup_caches(1, 24)
    with torch.no_grad():
        with pytest.raises(ValueError):
            m(ids[:, :3], torch.tensor([3, 5, 6], device=dev))
        with pytest.raises(ValueError):
            m(ids[:, :10], 20 + torch.arange(10, device=dev))     # 20 + 10 > 24
        m.setup_caches(1, 24, training=True)                       # no caches: nothing to continue
        with pytest.raises(ValueError):
            m(ids[:, :4], 2 + torch.arange(4, device=dev))


# ------------------------------------------------------------------------------------------------ 3. the model, Aria's widths (GPU)
def case_aria_width_chunks(dev):
    """One layer at Aria's widths (20 heads x 128): 600 tokens one-shot, then as 256 + 256 + 88.  Every piece takes the fused projection +
    RoPE + cache-write launch (the two behind the first with explicit positions)."""
    from aria_amd import ops
    from tests.model_cases import _aria_width_gptfast

    m, _, _ = _aria_width_gptfast(dev)
    ids = torch.randint(0, 512, (1, 600), generator=torch.Generator().manual_seed(600)).to(dev)
    m.setup_caches(1, 600)
    calls = []
    orig = ops.gemm_qkv_rope_cache

    def counted(x, wqkv, freqs_cis, pos32, *a, **k):
        calls.append(pos32 is not None)
        return orig(x, wqkv, freqs_cis, pos32, *a, **k)

    ops.gemm_qkv_rope_cache = counted
    try:
        with torch.no_grad():
            want = m(ids, torch.arange(600, device=dev), last_only=True).float().cpu()
            c = m.layers[0].attention.kv_cache
            k_ref, v_ref = c.k.float().cpu().clone(), c.v.float().cpu().clone()
            _junk_caches(m)
            del calls[:]
            for s, e in ((0, 256), (256, 512), (512, 600)):
                got = m(ids[:, s:e], torch.arange(s, e, device=dev), last_only=True)
    finally:
        ops.gemm_qkv_rope_cache = orig
    assert calls == [False, True, True], calls
    rel_close(got, want, 2e-2, "last-position logits, 256 + 256 + 88 vs one-shot")
    rel_close(c.k, k_ref, 2e-2, "k cache")
    rel_close(c.v, v_ref, 2e-2, "v cache")


# ------------------------------------------------------------------------------------------------ 4. generate / Generator
def _toy_aria(dev):
    from aria_amd import gptfast as G

    torch.manual_seed(3)
    args = toy_args(64)
    a = G.Aria(args, vision_config=_tiny_vision())
    with torch.no_grad():
        for n, p in a.llm.named_parameters():
            p.copy_((torch.ones(p.shape) + 0.1 * torch.randn(p.shape)).to(bf16) if "norm" in n else (torch.randn(p.shape) * 0.08).to(bf16))
    return a.to(dev).eval()


@contextlib.contextmanager
def _greedy_sampler(captured):
    """gptfast.sample serves the prefill's logits only (the decode steps sample in their own launch): record them, return the argmax."""
    from aria_amd import gptfast as G

    orig = G.sample

    def sample(logits, temperature=1.0, top_k=None):
        captured.append(logits[0, -1].float().cpu().clone())
        return logits[0, -1].float().argmax().view(1).to(torch.int), None

    G.sample = sample
    try:
        yield
    finally:
        G.sample = orig


PROMPT11 = [5, 12, 77, 3, 100, 4, 8, 41, 27, 90, 6]   # (no 9: that is the image placeholder)


def case_generate_chunked(dev):
    """prefill_chunk = 4 on an 11-token prompt (4 + 4 + 3) gives the default call's prefill logits; a chunk of 5 ends on a one-token piece."""
    from aria_amd import gptfast as G

    a = _toy_aria(dev)
    ids = torch.tensor([PROMPT11], device=dev)
    logs = []
    with _greedy_sampler(logs):
        for chunk in (None, 4, 5, 64):
            torch.manual_seed(0)
            out, _ = G.generate(a, ids, 3, top_k=1, temperature=1.0, cache_size=32, prefill_chunk=chunk)
            assert out.shape == (14,)
    rel_close(logs[1], logs[0], 2e-2, "prefill logits, prefill_chunk=4")
    rel_close(logs[2], logs[0], 3e-2, "prefill logits, prefill_chunk=5")   # (the one-token piece is a decode-engine step: its bound)
    assert torch.equal(logs[3], logs[0])                                    # a chunk that holds the whole prompt is today's call
    with pytest.raises(ValueError):
        G.generate(a, ids, 3, prefill_chunk=0)


def case_generate_cached_prefix(dev):
    """A second prompt that extends what the first call left in the cache: cached_prefix = P prefills T - P tokens and gives the prefill
    logits of a fresh full prefill (3e-2: some resident rows were written by engine steps)."""
    from aria_amd import gptfast as G

    a = _toy_aria(dev)
    seen = []
    orig_prep = a.prepare_embeddings
    a.prepare_embeddings = lambda idx, *r, **k: (seen.append(idx.shape[1]), orig_prep(idx, *r, **k))[1]
    logs = []
    with _greedy_sampler(logs):
        torch.manual_seed(0)
        out1, dec = G.generate(a, torch.tensor([PROMPT11], device=dev), 5, top_k=1, temperature=1.0, cache_size=40)
        resident = out1[:-1]                      # the last sampled token was never fed
        ids2 = torch.cat([resident, torch.tensor([7, 20, 3, 55], device=dev)]).view(1, -1)
        P, T = resident.numel(), resident.numel() + 4
        torch.manual_seed(0)
        G.generate(a, ids2, 3, top_k=1, temperature=1.0, cache_size=40, decoder=dec, cached_prefix=P)
        G.generate(a, ids2, 3, top_k=1, temperature=1.0, cache_size=40, decoder=dec, cached_prefix=P, prefill_chunk=3)
        torch.manual_seed(0)
        G.generate(a, ids2, 3, top_k=1, temperature=1.0, cache_size=40, decoder=dec)
        with pytest.raises(ValueError):
            G.generate(a, ids2, 3, cached_prefix=T)                        # at least the last token is prefilled
        with pytest.raises(ValueError):
            G.generate(a, ids2, 3, cache_size=400, cached_prefix=P)        # growing the cache would drop the prefix
    assert seen == [11, T - P, T - P, T], seen
    rel_close(logs[1], logs[3], 3e-2, "prefill logits with cached_prefix vs a full prefill")
    rel_close(logs[2], logs[3], 3e-2, "prefill logits with cached_prefix in pieces vs a full prefill")


class _ListProc:
    """a processor whose 'text' is the token list itself"""
    tokenizer = _Tok()

    def apply_chat_template(self, messages, add_generation_prompt=True):
        return messages[0]["content"]

    def __call__(self, text, images=None, return_tensors="pt"):
        return {"input_ids": torch.tensor([list(text)])}


def case_generator_reuse(dev):
    """Two chat turns: with reuse_prefix the second prefills T2 - P tokens, P = reusable_prefix(resident ids, new ids), and its prefill
    logits are those of a generator without reuse (which prefills all T2 and behaves as before)."""
    from aria_amd import gptfast_generate as GG

    a = _toy_aria(dev)
    mc = GG.ModelConfig("unused", device=dev)

    def generator(reuse):
        gc = GG.GenerationConfig(max_new_tokens=4, top_k=1, temperature=1.0, stop_strings=[], cache_size=48, reuse_prefix=reuse)
        return GG.Generator(mc, gc, model=a, processor=_ListProc())

    logs = []
    with _greedy_sampler(logs):
        gen = generator(True)
        torch.manual_seed(0)
        new1 = gen.generate([{"role": "user", "content": PROMPT11}], detokenize=False).tolist()
        assert gen.last_prefill_tokens == 11 and len(new1) == 4
        turn2 = PROMPT11 + new1 + [33, 2, 64, 19, 50]       # the conversation so far (with the whole reply) and the next user message
        resident = PROMPT11 + new1[:-1]
        P = GG.reusable_prefix(resident, turn2, a.config.image_token_index, True)
        assert P == len(resident)
        torch.manual_seed(0)
        gen.generate([{"role": "user", "content": turn2}], detokenize=False)
        assert gen.last_prefill_tokens == len(turn2) - P
        plain = generator(False)
        torch.manual_seed(0)
        plain.generate([{"role": "user", "content": turn2}], detokenize=False)
        assert plain.last_prefill_tokens == len(turn2) and plain._resident is None
        plain.generate([{"role": "user", "content": turn2}], detokenize=False)
        assert plain.last_prefill_tokens == len(turn2)
    rel_close(logs[1], logs[2], 3e-2, "second-turn prefill logits, reuse_prefix vs a full prefill")


# ------------------------------------------------------------------------------------------------ 5. host logic (no library)
def case_reusable_prefix():
    from aria_amd.gptfast_generate import reusable_prefix as rp

    IMG = 9
    old = [1, 2, IMG, IMG, IMG, 4, 5, 60, 61]                      # prompt [1 2 <img x3> 4 5] + two fed reply tokens
    assert rp(old, old + [62, 7, 8], IMG, True) == len(old)        # identical prefix, every image inside: all of it
    assert rp(old, [1, 2, IMG, IMG, 7, 8], IMG, True) == 2         # the common prefix ends inside the image run: cut in front of it
    assert rp(old, old + [62, 7, 8], IMG, False) == 2              # the pixels differ: the placeholders' rows are stale
    assert rp(old, list(old), IMG, True) == len(old) - 1           # the same ids again: the last token still runs
    assert rp(old, [3, 2, IMG], IMG, True) == 0                    # nothing in common
    assert rp([1, 2, 3], [1, 2, 3, 4, IMG, IMG, 5], IMG, True) == 3   # no old image: text prefix kept, the new image is in the suffix
    assert rp(old, [1, 2], IMG, True) == 1
    assert rp([], [1, 2], IMG, True) == 0


def case_generator_image_bookkeeping():
    """Generator._cached_prefix on a stand-in model: which images the ViT may skip, and the re-allocation rule."""
    from aria_amd import gptfast_generate as GG

    IMG = 9
    model = types.SimpleNamespace(llm=types.SimpleNamespace(max_seq_length=64), config=types.SimpleNamespace(image_token_index=IMG))
    gen = GG.Generator(GG.ModelConfig("unused", device="cpu"), GG.GenerationConfig(max_new_tokens=4, reuse_prefix=True), model=model, processor=None)
    pv1, pm1 = torch.arange(12.0).view(1, 3, 2, 2), torch.ones(1, 2, 2, dtype=torch.bool)
    pv2 = torch.cat([pv1, pv1 + 1])
    pm2 = torch.cat([pm1, pm1])
    old = [1, IMG, IMG, 4, 5, 60]
    new = old + [61, 7, IMG, IMG, 8]
    ids = torch.tensor([new])
    assert gen._cached_prefix((old, pv1, pm1), ids, pv2, pm2) == (6, 1)          # first image cached, the second goes through the ViT
    assert gen._cached_prefix((old, pv1, pm1), ids, pv2 + 1, pm2) == (1, 0)      # other pixels: cut in front of the placeholders
    assert gen._cached_prefix((old, pv1, pm1), ids, None, None) == (1, 0)
    assert gen._cached_prefix(([1, 4, 5], None, None), torch.tensor([[1, 4, 5, 7, IMG, IMG]]), pv1, pm1) == (3, 0)
    model.llm.max_seq_length = 8                                                  # the call would re-allocate the cache
    assert gen._cached_prefix((old, pv1, pm1), ids, pv2, pm2) == (0, 0)
