"""gptfast-compatible inference surface (seam B4) on the HIP kernels: mirror of ``gptfast/model.py`` (ModelArgs :38-60,
KVCache :67-93, Transformer :96-234, MOEFeedForward / ConditionalFeedForward :300-366, Attention :389-447, RMSNorm :461-472,
precompute_freqs_cis / apply_rotary_emb :500-531, Aria :534-609) and of the sampling loop in ``gptfast/generate.py:35-177``.

The ``model.pth`` wire format of ``gptfast/scripts/convert_hf_checkpoint.py:90-162`` loads unchanged:
``wqkv.weight [3D, D]`` (q/k rows permuted for interleaved RoPE), ``cond_ffn.w1 / w3 [E, I, D]``, ``cond_ffn.w2 [E, D, I]``
-- those expert layouts are *reduction-contiguous*, i.e. exactly the fast (rc, rc) form of the grouped MFMA GEMM, so no weight
is converted or transposed.  One MoE path serves prefill and decode (the reference switches to a gather+einsum path below 50
tokens, ``model.py:318-325``; the results are the same function).  The decode step allocates nothing data-dependent and reads
the cursor from device memory, so it can be captured in a HIP graph (``torch.cuda.CUDAGraph``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import functional as Fn
from . import hip, ops, quantize
from .vision import AriaProjector, AriaVisionConfig, AriaVisionModel

bf16 = torch.bfloat16


@dataclass
class ModelArgs:
    block_size: int = 16384
    vocab_size: int = 100352
    n_layer: int = 28
    n_head: int = 20
    dim: int = 2560
    intermediate_size: int = 1664
    n_local_heads: int = -1
    head_dim: int = 64
    rope_base: float = 5000000
    norm_eps: float = 1e-5
    num_experts: int = 64
    router_topk: int = 6
    num_shared_experts: int = 2
    image_token_index: int = 9

    def __post_init__(self):
        if self.n_local_heads == -1:
            self.n_local_heads = self.n_head
        self.head_dim = self.dim // self.n_head
        if self.n_local_heads != self.n_head:
            raise NotImplementedError("Aria is MHA (gptfast/model.py:56-58)")


def precompute_freqs_cis(seq_len: int, n_elem: int, base: float = 10000, dtype=bf16) -> torch.Tensor:
    """gptfast/model.py:500-516 (built on the host, bf16 cache [S, n_elem/2, 2])."""
    freqs = 1.0 / (base ** (torch.arange(0, n_elem, 2)[: (n_elem // 2)].float() / n_elem))
    freqs = torch.outer(torch.arange(seq_len), freqs)
    fc = torch.polar(torch.ones_like(freqs), freqs)
    return torch.stack([fc.real, fc.imag], dim=-1).to(dtype)


def _p(*shape):
    return nn.Parameter(torch.empty(*shape, dtype=bf16), requires_grad=False)


class _W(nn.Module):
    """holder with a `.weight` so state-dict keys read `<name>.weight`"""

    def __init__(self, *shape):
        super().__init__()
        self.weight = _p(*shape)


def adjacent_pair(p1: nn.Parameter, p2: nn.Parameter) -> bool:
    """Re-home two equal-shaped parameters in ONE allocation, ``p2`` directly behind ``p1`` (both stay contiguous tensors under their own
    state-dict keys: the model.pth wire format is untouched).  The fused gate / up + SwiGLU launch reads w1 and w3 as ONE operand whose up
    rows lie a fixed number of rows behind the gate rows (``ops.glu_split_fusable``).  ``module.to(device)`` gives every parameter its own
    storage again; the feed-forward modules call this lazily (a 2 x tensor-size transient, once)."""
    if p1.shape != p2.shape or p1.device != p2.device or p1.dtype != p2.dtype:
        return False
    buf = torch.empty((2,) + tuple(p1.shape), dtype=p1.dtype, device=p1.device)
    buf[0].copy_(p1.data)
    buf[1].copy_(p2.data)
    p1.data, p2.data = buf[0], buf[1]
    return True


def _glu_pair_ready(w_gate: nn.Parameter, w_up: nn.Parameter) -> bool:
    """True when the fused gate / up launch can take the pair (re-homing it once if only the layout is in the way)."""
    I, K = w_gate.shape[-2], w_gate.shape[-1]
    if I % 128 or K % 64 or K < 64 or not ops.swiglu_fusion_enabled() or getattr(w_gate, "_glu_pair_rejected", False):
        return False
    if ops.glu_split_fusable(w_gate, w_up):
        return True
    # re-home the pair only when the adjacent layout WOULD be taken (the kernel's size limits first: a rejected pair must not cost a 2 x
    # tensor-size copy on every forward -- ADVICE r3) and remember a rejection on the parameter
    if (w_gate.shape == w_up.shape and ops.glu_split_offset_ok(2 * w_gate.numel(), I, K, w_gate.numel()) and adjacent_pair(w_gate, w_up)
            and ops.glu_split_fusable(w_gate, w_up)):
        return True
    w_gate._glu_pair_rejected = True
    return False


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim, dtype=bf16), requires_grad=False)

    def forward(self, x2d):
        return ops.rmsnorm(x2d, self.weight, self.eps, want_rstd=False)[0]


class KVCache:
    """Static cache [B, S_max, H*hd] per layer (token-major so the attention kernel reads it in place)."""

    def __init__(self, max_batch_size, max_seq_length, n_heads, head_dim, device):
        self.k = torch.zeros((max_batch_size, max_seq_length, n_heads * head_dim), dtype=bf16, device=device)
        self.v = torch.zeros_like(self.k)


class Attention(nn.Module):
    def __init__(self, config: ModelArgs):
        super().__init__()
        self.config = config
        self.wqkv = _W(3 * config.dim, config.dim)
        self.wo = _W(config.dim, config.dim)
        self.kv_cache: Optional[KVCache] = None
        self.hdp = Fn._pad_hd(config.head_dim, need_bwd=False)  # kernels are native for 64 / 72 / 128

    def forward(self, x2d, B, S, freqs_cis, pos32, kv_len, prefill: bool, pos_is_arange: bool = False, q_offset: Optional[int] = None):
        c = self.config
        D, H, hd, hdp = c.dim, c.n_head, c.head_dim, self.hdp
        if q_offset is not None:
            return self._forward_continuation(x2d, B, S, freqs_cis, pos32, q_offset)
        if (prefill and self.kv_cache is not None and B == 1 and hdp == hd and x2d.shape[0] == S and S <= self.kv_cache.k.shape[1]
                and pos_is_arange and ops.qkv_rope_cache_fusable(D, x2d.shape[1], hd)):
            # K7: projection + interleaved RoPE + KVCache.update (model.py:423-435, 67-93) as ONE launch -- q to its own buffer, rotated k and v
            # straight into the static cache, which the attention kernel then reads in place: no [T, 3D] product, no rotation pass, no
            # cache copies.  Taken only when Transformer.forward KNOWS the positions are arange(S) (it built them itself, or the caller's
            # tensor was checked once per shape): the kernel then derives the position from the row index (pos = None), so neither the
            # rotation nor the cache row depends on a device tensor nobody validated.  A prompt longer than the cache takes the
            # path below, whose copy raises.
            cache = self.kv_cache
            q = ops.gemm_qkv_rope_cache(x2d, self.wqkv.weight, freqs_cis, None, cache.k, cache.v, S, hd)
            o, _ = ops.attention_fwd(q, cache.k[0, :S], cache.v[0, :S], 1, S, H, hd, hd ** -0.5, True)
            return ops.gemm(o, self.wo.weight)
        qkv = ops.gemm(x2d, self.wqkv.weight)
        ops.rope_interleaved_(qkv[:, :2 * D], freqs_cis, 2 * H, hd, pos32)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        if hdp != hd:  # toy head dims only (tests)
            q, k, v = (Fn._pad_heads(t, H, hd, hdp) for t in (q, k, v))
        Dp = H * hdp
        cache = self.kv_cache
        if cache is None or prefill:
            if cache is not None:  # k/v rows go into the cache (positions 0..S-1)
                cache.k[:B, :S].copy_(k.reshape(B, S, Dp))
                cache.v[:B, :S].copy_(v.reshape(B, S, Dp))
            o, _ = ops.attention_fwd(q, k, v, B, S, H, hdp, hd ** -0.5, True)
        else:  # decode: one token per sequence, cursor on the device (graph-capturable)
            Smax = cache.k.shape[1]
            rows = torch.arange(B, device=x2d.device) * Smax + pos32.long()
            cache.k.view(-1, Dp).index_copy_(0, rows, k)
            cache.v.view(-1, Dp).index_copy_(0, rows, v)
            o, _ = ops.attention_fwd(q, cache.k.view(-1, Dp), cache.v.view(-1, Dp), B, 1, H, hdp, hd ** -0.5, False,
                                     kv_len=kv_len, Skv=Smax)
        if hdp != hd:
            o = Fn._unpad_heads(o, H, hd, hdp).contiguous()
        return ops.gemm(o, self.wo.weight)

    def _forward_continuation(self, x2d, B, S, freqs_cis, pos32, p0: int):
        """Prefill at a cache offset (chunked prefill, chat prefix reuse): the S tokens sit at positions p0 .. p0+S-1 (Transformer.forward
        checked that on the host), cache rows 0 .. p0-1 hold the prefix.  What the reference does with KVCache.update indexed by input_pos
        and the mask rows causal_mask[input_pos] over the whole cache (gptfast/model.py:76-91, 199-231): the new k / v rows go to cache rows
        p0.., and the attention kernel reads the cache in place with the queries' causal position shifted by p0 (aria_attn_fwd_offset)."""
        c = self.config
        D, H, hd, hdp = c.dim, c.n_head, c.head_dim, self.hdp
        cache = self.kv_cache
        Smax = cache.k.shape[1]
        if B == 1 and hdp == hd and x2d.shape[0] == S and ops.qkv_rope_cache_fusable(D, x2d.shape[1], hd):
            # K7 with explicit positions: rotation and cache row both come from pos32 (= p0 + arange(S), host-checked)
            q = ops.gemm_qkv_rope_cache(x2d, self.wqkv.weight, freqs_cis, pos32, cache.k, cache.v, S, hd)
        else:
            qkv = ops.gemm(x2d, self.wqkv.weight)
            ops.rope_interleaved_(qkv[:, :2 * D], freqs_cis, 2 * H, hd, pos32)
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            if hdp != hd:  # toy head dims only (tests)
                q, k, v = (Fn._pad_heads(t, H, hd, hdp) for t in (q, k, v))
            cache.k[:B, p0:p0 + S].copy_(k.reshape(B, S, H * hdp))
            cache.v[:B, p0:p0 + S].copy_(v.reshape(B, S, H * hdp))
        Dp = H * hdp
        if B == 1:
            o, _ = ops.attention_fwd(q, cache.k[0, :p0 + S], cache.v[0, :p0 + S], 1, S, H, hdp, hd ** -0.5, True, Skv=p0 + S, q_offset=p0)
        else:  # every batch entry's rows lie Smax apart: the whole cache is the operand, the live length rides in kv_len
            kv_len = torch.full((B,), p0 + S, dtype=torch.int32, device=x2d.device)
            o, _ = ops.attention_fwd(q, cache.k.view(-1, Dp), cache.v.view(-1, Dp), B, S, H, hdp, hd ** -0.5, True, kv_len=kv_len, Skv=Smax,
                                     q_offset=p0)
        if hdp != hd:
            o = Fn._unpad_heads(o, H, hd, hdp).contiguous()
        return ops.gemm(o, self.wo.weight)


class ConditionalFeedForward(nn.Module):
    def __init__(self, config: ModelArgs):
        super().__init__()
        E, I, D = config.num_experts, config.intermediate_size, config.dim
        self.w1, self.w2, self.w3 = _p(E, I, D), _p(E, D, I), _p(E, I, D)


class FeedForward(nn.Module):
    def __init__(self, dim, inter):
        super().__init__()
        self.w1, self.w3, self.w2 = _W(inter, dim), _W(inter, dim), _W(dim, inter)


class MOEFeedForward(nn.Module):
    def __init__(self, config: ModelArgs):
        super().__init__()
        self.config = config
        self.gate = _W(config.num_experts, config.dim)
        self.cond_ffn = ConditionalFeedForward(config)
        self.shared_ffn = FeedForward(config.dim, config.intermediate_size * config.num_shared_experts)

    def forward(self, x2d):
        k = self.config.router_topk
        if ops.router_fusable(x2d.shape[1], self.gate.weight.shape[0], k):   # K1: gate GEMM + topk + softmax (model.py:355-363) as one launch
            logits, scores, idx, counts = ops.moe_router_fused(x2d, self.gate.weight, k)
        else:
            logits = ops.gemm(x2d, self.gate.weight)
            scores, idx, counts = ops.moe_route(logits, k)             # topk + softmax (model.py:359-363)
        offsets, sorted_src, inv = ops.moe_sort(idx, counts)           # token_permutation (:243-254)
        cf = self.cond_ffn
        if _glu_pair_ready(cf.w1, cf.w3) and ops.gather_fusable(x2d.shape[1]):
            # K2 + K3: the dispatcher's row gather (model.py:243-254) in the A loader of the fused w1 / w3 / SwiGLU launch -- no permuted copy
            # of the tokens ([6T, D]: 1.6 GB written and read per layer of a 53 K-token prefill), no h1 / h3 round trip
            act = ops.grouped_gemm_swiglu_split_gather(x2d, ops.permuted_token_rows(sorted_src, k), cf.w1, cf.w3, offsets)[1]
        elif _glu_pair_ready(cf.w1, cf.w3):   # w1 / w3 GEMMs + SwiGLU in ONE launch (no h1 / h3 round trip: 2 x [6T, I] written and read)
            act = ops.grouped_gemm_swiglu_split(ops.moe_permute(x2d, sorted_src, k), cf.w1, cf.w3, offsets)[1]
        else:
            perm = ops.moe_permute(x2d, sorted_src, k)
            h1 = ops.grouped_gemm(perm, cf.w1, offsets, w_is_kn=False)     # sequential_gemm(w1) (:278-297): w1[e] is [I, D] = rc form
            h3 = ops.grouped_gemm(perm, cf.w3, offsets, w_is_kn=False)
            act = ops.swiglu(h1, h3)
        eo = ops.grouped_gemm(act, cf.w2, offsets, w_is_kn=False)
        sf = self.shared_ffn
        if _glu_pair_ready(sf.w1.weight, sf.w3.weight):
            sact = ops.gemm_swiglu_split(x2d, sf.w1.weight, sf.w3.weight)[1]
        else:
            sact = ops.swiglu(ops.gemm(x2d, sf.w1.weight), ops.gemm(x2d, sf.w3.weight))
        sh = ops.gemm(sact, sf.w2.weight)
        return ops.moe_unpermute(eo, inv, scores, k, add=sh)


class TransformerBlock(nn.Module):
    def __init__(self, config: ModelArgs):
        super().__init__()
        self.attention = Attention(config)
        self.feed_forward = MOEFeedForward(config)
        self.ffn_norm = RMSNorm(config.dim, config.norm_eps)
        self.attention_norm = RMSNorm(config.dim, config.norm_eps)

    def forward(self, res, delta, B, S, freqs_cis, pos32, kv_len, prefill, pos_is_arange=False, q_offset=None):
        """gptfast/model.py:236-260 with the two residual adds folded into the norm that follows each (``rmsnorm`` with a residual: the
        sum is rounded to bf16 and written once, then normalised -- the same bits as ``add`` followed by ``rmsnorm``, two launches and two
        passes over [T, D] less per layer).  The block's input is ``res + delta`` (``delta`` None for the first block); it returns
        (h, ffn_out), the two halves of its output, for the next block's attention_norm -- or the model's final norm -- to sum."""
        if delta is None:
            x, xn = res, self.attention_norm(res)
        else:
            xn, x, _ = ops.rmsnorm(delta, self.attention_norm.weight, self.attention_norm.eps, residual=res, want_rstd=False)
        a = self.attention(xn, B, S, freqs_cis, pos32, kv_len, prefill, pos_is_arange, q_offset)
        hn, h, _ = ops.rmsnorm(a, self.ffn_norm.weight, self.ffn_norm.eps, residual=x, want_rstd=False)
        return h, self.feed_forward(hn)


class Transformer(nn.Module):
    def __init__(self, config: ModelArgs):
        super().__init__()
        self.config = config
        self.tok_embeddings = nn.Embedding(config.vocab_size, config.dim, dtype=bf16)
        self.layers = nn.ModuleList(TransformerBlock(config) for _ in range(config.n_layer))
        self.norm = RMSNorm(config.dim, config.norm_eps)
        self.output = _W(config.vocab_size, config.dim)
        self.freqs_cis: Optional[torch.Tensor] = None
        self.max_batch_size = self.max_seq_length = -1
        self.use_decode_engine = True     # batch-1 single-token steps go through aria_decode_token (csrc/decode.hip)
        self.decode_graph = False         # ... optionally replayed from a natively captured HIP graph (measured SLOWER than the plain
        #                                   enqueue on ROCm 7.2: 6.2 vs 4.8 ms/token -- graph kernel nodes cost more than stream launches)
        self._engine: Optional["DecodeEngine"] = None
        self._w8 = False                  # int8 weight-only codes + row scales (aria_amd/quantize.py): inference only
        # bumped by whatever may re-home a weight (module.to / .cuda / casts; load_state_dict, also through a parent module, also assign=True):
        # the decode engine re-checks its whole pointer table only then
        self._weights_version = 0
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._bump_weights_version())

    def _bump_weights_version(self):
        self._weights_version += 1

    def _apply(self, fn, *a, **k):
        self._weights_version = getattr(self, "_weights_version", 0) + 1
        return super()._apply(fn, *a, **k)

    def _engine_capable(self) -> bool:
        """The one-call-per-token engine serves this model's shape (native head dims of the decode attention kernel)."""
        if self._w8 and not quantize.engine_serves(self.config):
            return False
        return self.layers[0].attention.hdp == self.config.head_dim and self.config.head_dim in (64, 128)

    def _engine_ok(self) -> bool:
        att = self.layers[0].attention
        if att.kv_cache is None or not self._engine_capable():
            return False
        if self._engine is None or not self._engine.valid_for(self):
            self._engine = DecodeEngine(self)
        return True

    def setup_caches(self, max_batch_size, max_seq_length, training: bool = False, **_):
        """gptfast/model.py:113-166 (no S x S mask is ever built: the attention kernel masks in-register)."""
        dev = self.output.weight.device
        rounded = (max_seq_length + 7) // 8 * 8
        c0 = self.layers[0].attention.kv_cache
        if (not training and c0 is not None and (self.max_batch_size, self.max_seq_length) == (max_batch_size, rounded)
                and c0.k.device == dev and self.freqs_cis is not None and self.freqs_cis.device == dev):
            return   # same geometry: the buffers are re-used as they are (positions beyond the cursor are never read; gptfast/model.py:67-93
            #          overwrites rows in place as well) and the decode engine's pointer table stays valid
        self.max_batch_size, self.max_seq_length = max_batch_size, rounded
        self._engine = None   # it holds raw addresses of the tensors replaced below
        for b in self.layers:
            b.attention.kv_cache = None if training else KVCache(max_batch_size, self.max_seq_length, self.config.n_head,
                                                                 b.attention.hdp, dev)
        self.freqs_cis = precompute_freqs_cis(max(self.config.block_size, self.max_seq_length), self.config.head_dim,
                                              self.config.rope_base).to(dev).contiguous()
        for b in self.layers:  # gate / up pairs into one allocation each NOW (the decode engine records parameter addresses later)
            if self._w8:   # (int8 codes: the dequantizing forward lays its bf16 pairs out adjacently itself)
                break
            ff = b.feed_forward
            _glu_pair_ready(ff.cond_ffn.w1, ff.cond_ffn.w3)
            _glu_pair_ready(ff.shared_ffn.w1.weight, ff.shared_ffn.w3.weight)

    def forward(self, idx: Optional[torch.Tensor], input_pos: Optional[torch.Tensor] = None,
                input_embeds: Optional[torch.Tensor] = None, last_only: bool = False) -> torch.Tensor:
        """idx [B,S]; input_pos [S] (prefill: arange(S), or p0 + arange(S) to continue behind p0 cached positions) or [1] / [B] device
        tensor (decode cursor).  -> logits [B,S,V]."""
        x = self.tok_embeddings(idx) if input_embeds is None else input_embeds
        B, S, D = x.shape
        x2d = x.reshape(B * S, D).contiguous()
        prefill = S > 1 or input_pos is None
        if not prefill and B == 1 and self.use_decode_engine and self._engine_ok():
            return self._engine.step(x, input_pos)
        pos_is_arange = input_pos is None
        q_offset = None   # p0 of a prefill that continues behind p0 cached positions
        if input_pos is None:
            input_pos = torch.arange(S, device=x.device)
        elif prefill and input_pos.numel() == S:
            # the prefill contract is input_pos = arange(S) (gptfast/generate.py:147-150; KVCache.update writes rows 0..S-1): checked here, once
            # per prefill call (a host read of S integers), so that the fused projection + RoPE + cache-write launch may take the position
            # from the row index instead of trusting a device tensor
            # p0 + arange(S), p0 > 0: prefill at a cache offset (the prefix's rows are resident).  Any other position list is refused: no
            # launch here serves scattered prefill positions, and writing rows 0..S-1 regardless was silently wrong.
            host_pos = input_pos.reshape(-1).long().cpu()
            p0 = int(host_pos[0])
            if not torch.equal(host_pos, p0 + torch.arange(S)) or p0 < 0:
                raise ValueError(f"Transformer.forward: a prefill's input_pos must be p0 + arange({S}); got {host_pos.tolist()[:8]}...")
            pos_is_arange = p0 == 0
            if p0 > 0:
                q_offset = p0
                if self.layers[0].attention.kv_cache is None:
                    raise ValueError("Transformer.forward: a prefill at position p0 > 0 needs setup_caches() and the prefix in the cache")
                if B > self.max_batch_size or p0 + S > self.max_seq_length:
                    raise ValueError(f"Transformer.forward: positions {p0}..{p0 + S - 1} of {B} sequences do not fit the caches "
                                     f"({self.max_batch_size} x {self.max_seq_length}): setup_caches() first")
        if prefill:
            pos32 = input_pos.to(torch.int32).reshape(1, S).expand(B, S).reshape(-1).contiguous()
            kv_len = None
        else:
            pos32 = input_pos.to(torch.int32).reshape(-1).expand(B).contiguous()
            kv_len = pos32 + 1
        res, delta = x2d, None
        if self._w8:
            return self._forward_w8(res, B, S, pos32, kv_len, prefill, pos_is_arange, last_only, q_offset)
        for layer in self.layers:
            res, delta = layer(res, delta, B, S, self.freqs_cis, pos32, kv_len, prefill, pos_is_arange, q_offset)
        h = ops.rmsnorm(delta, self.norm.weight, self.norm.eps, residual=res, want_rstd=False)[0] if delta is not None else self.norm(res)
        if last_only:
            h = h.view(B, S, D)[:, -1].contiguous()
            return ops.gemm(h, self.output.weight).view(B, 1, -1)
        return ops.gemm(h, self.output.weight).view(B, S, -1)

    def _forward_w8(self, res, B, S, pos32, kv_len, prefill, pos_is_arange, last_only, q_offset=None):
        """Every forward of an int8 model that the int8 engine does not take (prefill, B > 1, ``use_decode_engine = False``, shapes the
        engine declines): before a layer runs, its codes are expanded into ONE bf16 scratch sized for a layer (quantize.dequantized_layer)
        and the bf16 tile kernels run on views of it.  A correctness path, not a fast one: a B > 1 decode step pays a full dequant of every
        layer (~2.6 GB of traffic per layer at Aria's widths).  The ``last_only`` head is an int8 GEMV per row."""
        D = self.config.dim
        delta = None
        for layer in self.layers:
            with quantize.dequantized_layer(self, layer):
                res, delta = layer(res, delta, B, S, self.freqs_cis, pos32, kv_len, prefill, pos_is_arange, q_offset)
        h = ops.rmsnorm(delta, self.norm.weight, self.norm.eps, residual=res, want_rstd=False)[0]
        if last_only:
            return quantize.head_logits(self, h.view(B, S, D)[:, -1].contiguous(), True).view(B, 1, -1)
        return quantize.head_logits(self, h, False).view(B, S, -1)


class DecodeEngine:
    """One-call-per-token decode (aria_decode_token, csrc/decode.hip) for batch 1: builds the pointer / dims tables the C entry point
    wants from the module's own tensors (the model.pth layout, unchanged) and owns the small scratch buffers."""

    def __init__(self, model: "Transformer"):
        import ctypes

        import numpy as np

        c = model.config
        att0 = model.layers[0].attention
        if att0.kv_cache is None:
            raise RuntimeError("DecodeEngine needs setup_caches() first")
        if att0.hdp != c.head_dim or c.head_dim not in (64, 128):
            raise RuntimeError("DecodeEngine: head_dim must be 64 or 128 (native attention head dims)")
        dev = model.output.weight.device
        self.w8 = model._w8   # int8 weights: aria_decode_token_w8 on its own pointer table (no graph form)
        Is = c.intermediate_size * c.num_shared_experts
        self.dims = np.array([c.n_layer, c.dim, c.n_head, c.head_dim, c.num_experts, c.router_topk, c.intermediate_size, Is, c.vocab_size,
                              model.max_seq_length], dtype=np.int64)
        lib = hip.get_lib()
        self._lib = lib
        self._dims_p = self.dims.ctypes.data_as(ctypes.c_void_p)
        nbytes = int(lib.cdll.aria_decode_scratch_bytes(self._dims_p))
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.x_in = torch.zeros(c.dim, dtype=bf16, device=dev)
        self.logits = torch.zeros(c.vocab_size, dtype=bf16, device=dev)
        self.eps = float(c.norm_eps)
        tensors = self._table(model)
        for t in tensors:
            assert t.is_contiguous() and t.device == dev
        self._keep = tensors  # the table holds raw addresses: keep the tensors alive and detect re-allocation
        self._addr = [t.data_ptr() for t in tensors]
        self._version = model._weights_version
        self._cheap = self._cheap_key(model)
        self.ptrs = (ctypes.c_void_p * len(tensors))(*self._addr)
        # one graph launch per token instead of ~13 launches per layer (None: capture failed or disabled -> plain enqueue)
        self.graph = lib.cdll.aria_decode_graph_create(self.ptrs, self._dims_p, self.eps) if model.decode_graph and not self.w8 else None

    def __del__(self):
        try:
            if getattr(self, "graph", None):
                self._lib.cdll.aria_decode_graph_destroy(self.graph)
        except Exception:
            pass

    def _table(self, model: "Transformer"):
        """The pointer table of aria_decode_token, read from the MODEL's current tensors (weights, freqs_cis, KV cache) + the engine's own."""
        if self.w8:
            return self._table_w8(model)
        tensors = [model.freqs_cis, model.norm.weight, model.output.weight, self.scratch, self.pos, self.x_in, self.logits, self.pos]
        for blk in model.layers:
            a, f = blk.attention, blk.feed_forward
            tensors += [blk.attention_norm.weight, a.wqkv.weight, a.wo.weight, blk.ffn_norm.weight, f.gate.weight, f.cond_ffn.w1,
                        f.cond_ffn.w3, f.cond_ffn.w2, f.shared_ffn.w1.weight, f.shared_ffn.w3.weight, f.shared_ffn.w2.weight,
                        a.kv_cache.k, a.kv_cache.v]
        return tensors

    def _table_w8(self, model: "Transformer"):
        """aria_decode_token_w8's table (include/aria_hip.h: ARIA_DECODE_W8_*_PTRS)"""
        tensors = [model.freqs_cis, model.norm.weight, model.output.weight, self.scratch, self.pos, self.x_in, self.logits, self.pos,
                   model.output.scales]
        for blk in model.layers:
            a, f = blk.attention, blk.feed_forward
            cf, sf = f.cond_ffn, f.shared_ffn
            tensors += [blk.attention_norm.weight, a.wqkv.weight, a.wqkv.scales, a.wo.weight, a.wo.scales, blk.ffn_norm.weight, f.gate.weight,
                        cf.w1, cf.scales1, cf.w3, cf.scales3, cf.w2, cf.scales2, sf.w1.weight, sf.w1.scales, sf.w3.weight, sf.w3.scales,
                        sf.w2.weight, sf.w2.scales, a.kv_cache.k, a.kv_cache.v]
        return tensors

    def valid_for(self, model: "Transformer") -> bool:
        """The recorded addresses against what the model holds NOW: ``setup_caches`` allocates new K/V tensors and a fresh ``freqs_cis``,
        ``module.to`` / ``load_state_dict(assign=True)`` re-home weights -- the engine's own references stay alive and would never differ from themselves
        (a second cached generate() kept attending over the previous call's cache)."""
        if int(self.dims[9]) != model.max_seq_length or model.layers[0].attention.kv_cache is None:
            return False
        if model._weights_version == self._version:
            # per token (the full table was 8 + 13 L module lookups and data_ptr() calls per decoded token): what can be re-homed
            # WITHOUT bumping the model's weight version -- the caches and freqs_cis, replaced by setup_caches
            return self._cheap_key(model) == self._cheap
        ok = [t.data_ptr() for t in self._table(model)] == self._addr   # weights touched (_apply / load_state_dict): the full comparison, once
        if ok:
            self._version = model._weights_version
        return ok

    @staticmethod
    def _cheap_key(model: "Transformer"):
        key = [model.freqs_cis.data_ptr()]
        for blk in model.layers:
            c = blk.attention.kv_cache
            key += [c.k.data_ptr(), c.v.data_ptr()]
        return key

    def routing_trace(self):
        """Every layer's routing record of the LAST step (a host sync): (router logits [L, E] bf16, expert ids [L, k] int32, scores [L, k] bf16) --
        what TopKRouter (gptfast/model.py:355-366) saw and chose inside the engine; read by the full-depth parity case."""
        import ctypes

        import numpy as np

        lay = np.zeros(6, dtype=np.int64)
        self._lib.call("aria_decode_trace_layout", self._dims_p, lay.ctypes.data_as(ctypes.c_void_p))
        L, E, k = int(self.dims[0]), int(self.dims[4]), int(self.dims[5])

        def rows(off, stride, dtype, width):
            n = torch.empty(0, dtype=dtype).element_size()
            raw = self.scratch[off:off + L * stride].view(L, stride)[:, :width * n].contiguous()
            return raw.view(dtype).view(L, width).clone()

        return rows(int(lay[0]), int(lay[1]), bf16, E), rows(int(lay[2]), int(lay[3]), torch.int32, k), rows(int(lay[4]), int(lay[5]), bf16, k)

    def step(self, x_embed: torch.Tensor, input_pos: torch.Tensor) -> torch.Tensor:
        """x_embed [1,1,D] (embedding of the new token), input_pos: device tensor with the cursor -> logits [1,1,V] (a view of the
        engine's buffer: consume it before the next step)."""
        self.x_in.copy_(x_embed.reshape(-1))
        self.pos.copy_(input_pos.reshape(-1)[:1])
        stream = torch.cuda.current_stream(self.x_in.device).cuda_stream if self.x_in.is_cuda else None
        if self.graph:
            self._lib.call("aria_decode_graph_launch", self.graph, stream)
        else:
            self._lib.call("aria_decode_token_w8" if self.w8 else "aria_decode_token", self.ptrs, self._dims_p, self.eps, stream)
        return self.logits.view(1, 1, -1)


class Aria(nn.Module):
    """gptfast/model.py:534-609: vision_tower + multi_modal_projector (HF key names) + llm (gptfast key names)."""

    def __init__(self, config: ModelArgs, vision_config: Optional[AriaVisionConfig] = None, patch_to_query=None):
        super().__init__()
        self.config = config
        vc = vision_config or AriaVisionConfig()
        self.vision_tower = AriaVisionModel(vc)
        self.multi_modal_projector = AriaProjector(patch_to_query or {1225: 128, 4900: 256}, vc.hidden_size, vc.num_attention_heads,
                                                   vc.hidden_size, config.dim, config.dim)
        self.llm = Transformer(config)

    def setup_caches(self, *a, **k):
        self.llm.setup_caches(*a, **k)

    @torch.no_grad()
    def prepare_embeddings(self, idx, pixel_values=None, pixel_mask=None):
        emb = self.llm.tok_embeddings(idx)
        if pixel_values is not None:
            feat, atts = self.vision_tower(pixel_values, pixel_mask)
            img = self.multi_modal_projector(feat, attn_mask=atts)
            mask = (idx == self.config.image_token_index).unsqueeze(-1).expand_as(emb)
            emb = emb.masked_scatter(mask, img.to(emb.dtype))
        return emb

    def forward(self, idx, input_pos=None, input_embeds=None, last_only=False):
        return self.llm(idx, input_pos, input_embeds, last_only=last_only)


# ------------------------------------------------------------------------------------------------- generate.py
def multinomial_sample_one_no_sync(probs_sort):
    q = torch.empty_like(probs_sort).exponential_(1)
    return torch.argmax(probs_sort / q, dim=-1, keepdim=True).to(dtype=torch.int)


def logits_to_probs(logits, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                    min_p: Optional[float] = None):
    """``top_p`` / ``min_p`` (both ``None``: the reference's function, unchanged) follow aria_sample's definitions (include/aria_hip.h): over the
    top-k survivors a distinct logit value stays iff the probability mass strictly above it is < top_p (equal logits stay or go together);
    a logit stays iff its probability is >= min_p times the largest one."""
    logits = logits.float() / max(temperature, 1e-5)
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits = torch.where(logits < v.select(-1, -1).unsqueeze(-1), -float("Inf"), logits)
    if top_p is not None and top_p < 1.0:
        srt, order = torch.sort(logits, dim=-1, descending=True)
        ps = torch.softmax(srt, dim=-1)
        excl = ps.cumsum(-1) - ps
        new = torch.ones_like(srt, dtype=torch.bool)
        new[..., 1:] = srt[..., 1:] != srt[..., :-1]
        pos = torch.arange(srt.size(-1), device=srt.device).expand_as(srt)
        first = torch.where(new, pos, torch.zeros_like(pos)).cummax(-1).values     # where this value's group of equal logits begins
        drop = torch.zeros_like(new).scatter(-1, order, excl.gather(-1, first) >= top_p)
        logits = logits.masked_fill(drop, -float("Inf"))
    if min_p is not None and min_p > 0.0:
        mx = logits.max(dim=-1, keepdim=True).values
        logits = logits.masked_fill(logits - mx < math.log(min_p), -float("Inf"))
    return torch.softmax(logits, dim=-1)


def sample(logits, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None):
    probs = logits_to_probs(logits[0, -1], temperature, top_k, top_p, min_p)
    return multinomial_sample_one_no_sync(probs), probs


def sampling_options(top_p=None, min_p=None, repetition_penalty=None, logprobs=False):
    """-> (top_p, min_p, repetition_penalty, logprobs) with ``None`` replaced by the neutral value, validated"""
    top_p = 1.0 if top_p is None else min(float(top_p), 1.0)
    min_p = 0.0 if min_p is None else float(min_p)
    pen = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not top_p > 0.0 or not 0.0 <= min_p < 1.0 or not pen > 0.0:
        raise ValueError(f"sampling options: need 0 < top_p, 0 <= min_p < 1, repetition_penalty > 0; got {top_p}, {min_p}, {pen}")
    return top_p, min_p, pen, bool(logprobs)


NEUTRAL_OPTIONS = (1.0, 0.0, 1.0, False)


class DecodeGraph:
    """The decode model step captured once in a HIP graph (the reference uses torch.compile(mode="reduce-overhead"),
    gptfast/generate.py:232-238): static token / cursor / logits buffers, one replay per token.  Sampling (a handful of tiny
    torch kernels using the RNG) runs eagerly after the replay: capturing torch's RNG kernels in the same graph as the HIP
    launches faulted on the second replay on ROCm 7.2 / torch 2.10 (bisected in tools/bisect/debug_graph4.py)."""

    def __init__(self, model: Aria, temperature: float, top_k: Optional[int], use_graph: bool = True, top_p: Optional[float] = None,
                 min_p: Optional[float] = None, repetition_penalty: Optional[float] = None, logprobs: bool = False):
        """``top_p`` / ``min_p`` / ``repetition_penalty`` / ``logprobs`` all neutral (the default): sampling is ``ops.sample_topk``, as before.
        Otherwise every token goes through ``ops.sample`` (aria_sample): the decoder then owns ``seen`` (one bit per vocabulary entry, the tokens
        the penalty applies to: ``begin`` fills it from a prompt, every sampled token adds its own bit) and a float32 buffer with the
        log-probability of every token sampled since ``begin`` (``logprobs``)."""
        self.model, self.temperature, self.top_k = model, temperature, top_k
        self.options = sampling_options(top_p, min_p, repetition_penalty, logprobs)
        self.top_p, self.min_p, self.repetition_penalty, _ = self.options
        self.full = self.options != NEUTRAL_OPTIONS
        dev = model.llm.output.weight.device
        self.tok = torch.zeros((1, 1), dtype=torch.long, device=dev)
        # warm-up / capture run at the LAST cache slot so they never clobber live K/V rows
        self.pos = torch.full((1,), model.llm.max_seq_length - 1, dtype=torch.int32, device=dev)
        self.logits = torch.zeros((1, 1, model.config.vocab_size), dtype=bf16, device=dev)
        # sampling as ONE launch (ops.sample_topk) on Exp(1) draws of torch's generator: same seeds -> same tokens as the tensor path
        self._q = torch.empty(model.config.vocab_size, dtype=torch.float32, device=dev)
        self._ring = torch.zeros(model.llm.max_seq_length + 8, dtype=torch.int32, device=dev)  # one slot per new token: callers keep views
        self._slot = 0
        self.seen = self._lp = None
        self._n = 0
        if self.full:
            self.seen = torch.zeros((model.config.vocab_size + 31) // 32, dtype=torch.int32, device=dev)
            self._lp = torch.zeros(model.llm.max_seq_length + 8, dtype=torch.float32, device=dev)
        self.graph = None
        if use_graph and dev.type == "cuda":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._step()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._step()

    def _step(self):
        self.logits.copy_(self.model(self.tok, self.pos, last_only=True))

    @property
    def logprobs(self) -> Optional[torch.Tensor]:
        """float32 [n]: the log-probability (under the filtered distribution it was drawn from) of every token sampled since ``begin``"""
        return None if self._lp is None else self._lp[:min(self._n, self._lp.numel())]

    def begin(self, input_ids: torch.Tensor):
        """A new sequence: ``seen`` holds exactly the tokens of ``input_ids``, the log-prob buffer starts over."""
        self._n = 0
        if self.full and self.repetition_penalty != 1.0:
            self.seen.zero_()
            ops.token_bitmap(input_ids, self.model.config.vocab_size, out=self.seen)

    def sample(self, lg: torch.Tensor) -> torch.Tensor:
        """one token from the logits [V] (bf16, contiguous) with this decoder's options -> int32 [1] (a slot of the ring)"""
        self._q.exponential_(1)
        out = self._ring[self._slot:self._slot + 1]
        self._slot = (self._slot + 1) % self._ring.numel()
        if not self.full:
            return ops.sample_topk(lg, self._q, self.temperature, self.top_k, out=out)
        i = self._n % self._lp.numel()
        self._n += 1
        pen = self.repetition_penalty != 1.0
        return ops.sample(lg, self._q, self.temperature, self.top_k, self.top_p, self.min_p, self.repetition_penalty,
                          seen=self.seen if pen else None, update_seen=pen, out=out, logprob=self._lp[i:i + 1])

    def __call__(self, token: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        self.tok.copy_(token.view(1, 1))
        self.pos.copy_(pos.view(1))
        if self.graph is not None:
            self.graph.replay()
            lg = self.logits
        else:  # the engine's own logits buffer (consumed here, before the next step overwrites it): no 200 KB copy
            lg = self.model(self.tok, self.pos, last_only=True)
        lg = lg.reshape(-1)
        if lg.dtype != bf16 or not lg.is_contiguous():
            if self.full:
                raise TypeError("DecodeGraph: top_p / min_p / repetition_penalty / logprobs need the model's bf16 logits (aria_sample)")
            return sample(lg.view(1, 1, -1), self.temperature, self.top_k)[0].view(-1)
        return self.sample(lg)


import os as _os

_DEBUG_GEN = bool(_os.environ.get("ARIA_DEBUG_GEN"))


def _dbg(msg):
    if _DEBUG_GEN:
        torch.cuda.synchronize()
        print("[gen]", msg, flush=True)


@torch.no_grad()
def generate(model: Aria, input_ids: torch.Tensor, max_new_tokens: int, *, pixel_values=None, pixel_mask=None,
             temperature: float = 0.8, top_k: Optional[int] = 200, decoder: Optional[DecodeGraph] = None,
             stop_token: Optional[int] = None, use_graph: bool = False, callback=None,
             cache_size: Optional[int] = None, prefill_chunk: Optional[int] = None,
             cached_prefix: int = 0, top_p: Optional[float] = None, min_p: Optional[float] = None,
             repetition_penalty: Optional[float] = None, logprobs: bool = False) -> Tuple[torch.Tensor, Optional[DecodeGraph]]:
    """gptfast/generate.py:112-177: prefill (ViT + projector + full prompt) then token-by-token decode.  ``callback(new_tokens)`` is the
    reference's early-stop hook (decode_n_tokens :80-105: called after every token with the list of new token tensors, ``True`` stops);
    ``stop_token`` is the cheap form of the same for single-token stop strings.  ``cache_size`` pre-sizes the static KV cache (:139-150).
    ``cached_prefix`` = P: rows 0..P-1 of the KV cache already hold ``input_ids[:, :P]`` (an earlier call on this model left them there), so
    only the suffix is embedded and prefilled -- ``pixel_values`` / ``pixel_mask`` are then the images whose placeholders lie in the suffix.
    ``prefill_chunk``: the tokens to prefill run in pieces of at most that many (peak activation memory follows the piece, not the prompt);
    every piece behind the first is a prefill at a cache offset (Transformer.forward with input_pos = p0 + arange).
    ``top_p`` / ``min_p`` / ``repetition_penalty`` (HF's meanings, aria_sample's definitions in include/aria_hip.h) and ``logprobs``: with any
    of them set every token, the first one included, is drawn by ``ops.sample``; the penalty covers all of ``input_ids`` (a cached prefix
    too) and what the call generates; ``decoder.logprobs`` then holds the log-probabilities of the call's new tokens (float32 [n_new]).  A
    ``decoder`` built for other values of these four is replaced.  All four neutral: the sampling of earlier releases, launch for launch."""
    opts = sampling_options(top_p, min_p, repetition_penalty, logprobs)
    if decoder is not None and decoder.options != opts:
        decoder = None
    T = input_ids.size(1)
    dev = input_ids.device
    P = int(cached_prefix)
    if not 0 <= P <= max(T - 1, 0):
        raise ValueError(f"cached_prefix must lie in 0..{T - 1} (at least the last prompt token is prefilled); got {P}")
    if prefill_chunk is not None and prefill_chunk < 1:
        raise ValueError("prefill_chunk must be a positive number of tokens")
    if cache_size is not None and cache_size < T + max_new_tokens:
        raise ValueError("need cache_size to be greater than max_new_tokens + size-of-prompt")
    if model.llm.max_seq_length < max(T + max_new_tokens, cache_size or 0):
        if P > 0:
            raise ValueError(f"cached_prefix={P}: the KV cache ({model.llm.max_seq_length} positions) would have to be re-allocated for "
                             f"{max(T + max_new_tokens, cache_size or 0)}, which drops the prefix -- size the cache before the first call")
        model.setup_caches(1, max(T + max_new_tokens, cache_size or 0))
        decoder = None
    _dbg("start")
    emb = model.prepare_embeddings(input_ids[:, P:] if P else input_ids, pixel_values, pixel_mask)
    _dbg("emb")
    chunk = T - P if prefill_chunk is None else min(prefill_chunk, T - P)
    if P == 0 and chunk == T:
        input_pos = torch.arange(0, T, device=dev)
        logits = model(None, input_pos, emb, last_only=True)
    else:
        for s in range(P, T, chunk):   # (a one-token piece is a decode step at its position; only the last piece's logits are used)
            e = min(T, s + chunk)
            logits = model(None, torch.arange(s, e, device=dev), emb[:, s - P:e - P], last_only=True)
    _dbg("prefill")
    if opts == NEUTRAL_OPTIONS:
        nxt, _ = sample(logits, temperature, top_k)
        _dbg("sample")
    if decoder is None:
        # KNOWN ISSUE (round 1): a HIP-graph-captured decode step replays correctly inside one generate() call but faults
        # when replayed after a second image prefill (ROCm 7.2 / torch 2.10; bisection scripts tools/bisect/debug_graph*.py).
        # Decode therefore runs eagerly unless use_graph is requested explicitly.
        decoder = DecodeGraph(model, temperature, top_k, use_graph=use_graph, top_p=opts[0], min_p=opts[1], repetition_penalty=opts[2],
                              logprobs=opts[3])
        _dbg("capture")
    if decoder.full:   # the first token through the same launch as the others: penalty and log-prob cover it too
        decoder.begin(input_ids)
        lg = logits[0, -1]
        if lg.dtype != bf16:
            raise TypeError("generate: top_p / min_p / repetition_penalty / logprobs need the model's bf16 logits (aria_sample)")
        nxt = decoder.sample(lg.contiguous())
        _dbg("sample")
    toks: List[torch.Tensor] = [nxt.view(1)]
    pos = torch.tensor([T], device=dev, dtype=torch.int32)
    for _ in range(max_new_tokens - 1):
        nxt = decoder(toks[-1], pos)
        if _DEBUG_GEN:  # (formatting the message reads two device scalars: never on the normal path, it would sync every token)
            _dbg(f"decode pos {int(pos)} tok {int(nxt)}")
        toks.append(nxt.view(1))
        pos += 1
        if stop_token is not None and int(nxt) == stop_token:
            break
        if callback is not None and callback(toks) is True:
            break
    return torch.cat([input_ids.view(-1), torch.cat(toks).long()]), decoder


def load_model_pth(model: Aria, state_dict: dict, strict: bool = False):
    """Load a gptfast ``model.pth`` state dict (convert_hf_checkpoint.py output: ``llm.*`` gptfast names, vision / projector HF
    names) -- tensors are copied as they are, no layout conversion.  An int8 weight-only state dict (``*.scales`` keys: aria_amd/quantize.py,
    ``model_int8.pth``) first turns the model into the quantized structure; its codes and scales are then copied verbatim, and any dtype or
    shape mismatch raises."""
    if quantize.is_int8_state_dict(state_dict):
        quantize.convert_structure_(model)
        own = model.state_dict()
        for k, v in own.items():
            if k in state_dict and (state_dict[k].dtype != v.dtype or state_dict[k].shape != v.shape):
                raise ValueError(f"{k}: checkpoint has {state_dict[k].dtype} {tuple(state_dict[k].shape)}, the model {v.dtype} {tuple(v.shape)}")
    elif quantize.is_quantized(model):
        raise ValueError("load_model_pth: a bf16 state dict cannot be loaded into an int8-quantized model")
    else:
        bad = [k for k, v in state_dict.items() if v.dtype == torch.int8]
        if bad:
            raise ValueError(f"load_model_pth: int8 tensors {bad[:3]} without their *.scales keys (an incomplete int8 checkpoint)")
    own = model.state_dict()
    missing = [k for k in own if k not in state_dict]
    if strict and missing:
        raise KeyError(f"missing keys {missing[:5]}")
    with torch.no_grad():
        for k, v in own.items():
            if k in state_dict:
                v.copy_(state_dict[k].to(v.dtype))
    return missing
