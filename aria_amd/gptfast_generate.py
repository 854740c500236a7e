"""Host classes of the gptfast surface above ``generate()`` (gptfast/generate.py:187-346, gptfast/chat.py:8-66, gptfast/benchmark.py:10-48):
``ModelConfig`` / ``GenerationConfig`` / ``Generator`` / ``AriaChat`` / ``run_benchmark`` with the reference's constructor arguments and
method names, on ``aria_amd.gptfast`` (tile kernels for the prefill, the one-call-per-token engine for decode).  The ``compile*`` switches
are accepted and ignored: there is no tracing compiler on this path -- the decode step is already one C call."""
from __future__ import annotations

import time
from pathlib import Path
from statistics import mean, stdev
from typing import List, Optional

import torch

from . import gptfast as G


class GenerationConfig:
    def __init__(self, max_new_tokens: int = 100, top_k: int = 200, temperature: float = 0.8, cache_size: Optional[int] = None,
                 linear_causal_mask: bool = False, stop_strings: Optional[List[str]] = None, prefill_chunk: Optional[int] = None,
                 reuse_prefix: bool = False, top_p: Optional[float] = None, min_p: Optional[float] = None,
                 repetition_penalty: Optional[float] = None, logprobs: bool = False):
        """``top_p`` / ``min_p`` / ``repetition_penalty``: HF's meanings (``None`` = off; ``aria_amd.gptfast.generate``); ``logprobs``: keep the
        log-probabilities of the generated tokens (``Generator.last_logprobs``; they are also kept whenever one of the three is set).
        ``prefill_chunk``: prefill the prompt in pieces of at most that many tokens.  ``reuse_prefix``: a ``Generator`` keeps what its last
        call left in the KV cache and prefills only what the next prompt adds behind the common prefix (multi-turn chat)."""
        self.max_new_tokens, self.top_k, self.temperature = max_new_tokens, top_k, temperature
        self.cache_size, self.linear_causal_mask, self.stop_strings = cache_size, linear_causal_mask, stop_strings
        self.prefill_chunk, self.reuse_prefix = prefill_chunk, reuse_prefix
        self.top_p, self.min_p, self.repetition_penalty, self.logprobs = top_p, min_p, repetition_penalty, logprobs


class ModelConfig:
    def __init__(self, checkpoint_path, device: str = "cuda", precision: torch.dtype = torch.bfloat16, compile: bool = False,
                 compile_prefill: bool = False, apply_regional_compilation: bool = False, model_args: Optional[G.ModelArgs] = None,
                 vision_config=None):
        """``checkpoint_path``: a ``model.pth`` or an int8 ``model_int8.pth`` (aria_amd.quantize); ``precision`` is the compute dtype (bf16
        for both).  ``model_args`` / ``vision_config``: the LM's / the vision tower's shape when it is not Aria's."""
        self.checkpoint_path, self.device, self.precision = Path(checkpoint_path), device, precision
        self.model_args, self.vision_config = model_args, vision_config
        self.compile, self.compile_prefill, self.apply_regional_compilation = compile, compile_prefill, apply_regional_compilation


def load_model_and_processor(checkpoint_path: Path, device, precision=torch.bfloat16, model_args: Optional[G.ModelArgs] = None, processor=None,
                             vision_config=None):
    """``model.pth`` (convert_hf_checkpoint.py / aria_amd.checkpoint.convert_hf_checkpoint) -> ``Aria`` on ``device``; the processor comes
    from the tokenizer files next to it (generate.py:218-220) unless one is handed in."""
    if precision != torch.bfloat16:
        raise ValueError("the MI355X path computes in bf16")
    prev = torch.get_default_device() if hasattr(torch, "get_default_device") else None
    torch.set_default_device(device)
    try:
        model = G.Aria(model_args or G.ModelArgs(), vision_config=vision_config)
    finally:
        torch.set_default_device(prev if prev is not None else "cpu")
    G.load_model_pth(model, torch.load(str(checkpoint_path), map_location="cpu", mmap=True, weights_only=True), strict=True)
    if processor is None:
        from transformers import AutoTokenizer

        from .processing import AriaProcessor, AriaVisionProcessor

        processor = AriaProcessor(tokenizer=AutoTokenizer.from_pretrained(str(Path(checkpoint_path).parent), use_fast=False),
                                  image_processor=AriaVisionProcessor())
    return model.eval(), processor


def reusable_prefix(old_ids: List[int], new_ids: List[int], image_token_index: int, old_images_match: bool) -> int:
    """How many leading tokens of ``new_ids`` need no prefill when the KV cache holds ``old_ids`` (rows 0..len(old_ids)-1).
    L = the longest common prefix, capped at len(new_ids) - 1 (the last prompt token is always run: its logits are the first sample).
    If that prefix covers EVERY image placeholder of ``old_ids`` and ``old_images_match`` (the old call's pixel values and masks equal
    the leading ones of the new call), all of it is kept, and only the new call's further images go through the ViT.  Otherwise the cut
    falls in front of the first image placeholder: a run of placeholders is filled from the projector's output in order, so a suffix
    must hold whole images, and with different pixels the cached rows of the placeholders are stale."""
    L, cap = 0, min(len(old_ids), len(new_ids) - 1)
    while L < cap and old_ids[L] == new_ids[L]:
        L += 1
    n_img_old = sum(1 for t in old_ids if t == image_token_index)
    if old_images_match and sum(1 for t in new_ids[:L] if t == image_token_index) == n_img_old:
        return L
    first_img = next((i for i, t in enumerate(new_ids) if t == image_token_index), len(new_ids))
    return min(L, first_img)


class Generator:
    """generate.py:281-346.  ``Generator(model_config, generation_config).generate(messages, image, detokenize=True)``.
    With ``generation_config.reuse_prefix`` it remembers the token ids resident in the KV cache after a call (the prompt and every generated
    token that was fed back, i.e. all but the last sampled one) and that call's pixel values / masks; the next call prefills only the
    tokens behind ``reusable_prefix``.  ``last_prefill_tokens``: how many prompt tokens the last call prefilled.  ``last_logprobs``: the
    log-probabilities of the last call's new tokens (float32 [n_new]) when the configuration sets ``top_p`` / ``min_p`` /
    ``repetition_penalty`` / ``logprobs``, else ``None``."""

    def __init__(self, model_config: ModelConfig, generation_config: GenerationConfig, model: Optional[G.Aria] = None, processor=None):
        self.model_config, self.generation_config = model_config, generation_config
        self.model, self.processor = model, processor
        self._decoder = None
        self._resident = None            # (ids, pixel_values, pixel_mask) of what the KV cache holds (reuse_prefix)
        self.last_prefill_tokens = 0
        self.last_logprobs = None
        if self.model is None:
            self.model, self.processor = load_model_and_processor(model_config.checkpoint_path, model_config.device, model_config.precision,
                                                                  getattr(model_config, "model_args", None), processor=processor,
                                                                  vision_config=getattr(model_config, "vision_config", None))

    def _stops(self):
        """single-token stop strings become a device-side comparison; anything longer keeps the reference's decode-and-compare callback"""
        tok, single, multi = self.processor.tokenizer, [], []
        for s in self.generation_config.stop_strings or []:
            ids = tok.encode(s)
            (single if len(ids) == 1 else multi).append(ids[0] if len(ids) == 1 else s)
        return single, multi

    def _cached_prefix(self, resident, ids, pv, pm):
        """-> (P, n_old): the reusable prefix of this call against what the cache holds, and how many leading images the ViT may skip."""
        gc = self.generation_config
        old_ids, old_pv, old_pm = resident
        T = ids.shape[1]
        if self.model.llm.max_seq_length < max(T + gc.max_new_tokens, gc.cache_size or 0):
            return 0, 0   # generate() will re-allocate the cache: nothing survives
        n_old = 0 if old_pv is None else old_pv.shape[0]
        match = n_old == 0 or (pv is not None and pv.shape[0] >= n_old and pv.shape[1:] == old_pv.shape[1:] and torch.equal(pv[:n_old], old_pv)
                               and ((pm is None and old_pm is None) or (pm is not None and old_pm is not None and pm.shape[1:] == old_pm.shape[1:]
                                                                        and torch.equal(pm[:n_old], old_pm))))
        new_ids, img = ids.view(-1).tolist(), self.model.config.image_token_index
        P = reusable_prefix(old_ids, new_ids, img, match)
        kept_all = match and sum(1 for t in new_ids[:P] if t == img) == sum(1 for t in old_ids if t == img)
        return P, (n_old if (P > 0 and kept_all) else 0)

    def generate(self, messages: List[dict], image=None, detokenize: bool = True):
        gc, dev = self.generation_config, self.model_config.device
        text = self.processor.apply_chat_template(messages, add_generation_prompt=True)
        inputs = self.processor(text=text, images=image, return_tensors="pt")
        ids = inputs["input_ids"].to(dev)
        pv = inputs["pixel_values"].to(dev).to(torch.bfloat16) if inputs.get("pixel_values") is not None else None
        pm = inputs["pixel_mask"].to(dev) if inputs.get("pixel_mask") is not None else None
        single, multi = self._stops()
        tok = self.processor.tokenizer

        def early_stop(tokens):
            last = int(tokens[-1])
            if last in single[1:]:
                return True
            if multi:
                decoded = tok.decode(torch.cat(tokens).tolist())
                return any(decoded.endswith(s) for s in multi)
            return False

        P, resident = 0, self._resident
        self._resident = None   # (a call that raises leaves the cache in an unknown state)
        reuse = getattr(gc, "reuse_prefix", False)
        run_pv, run_pm = pv, pm
        if reuse and resident is not None:
            P, n_old = self._cached_prefix(resident, ids, pv, pm)
            if P > 0 and n_old > 0:   # the old images' placeholders all lie in the prefix: the ViT sees the further images only
                run_pv = pv[n_old:] if pv.shape[0] > n_old else None
                run_pm = pm[n_old:] if (pm is not None and run_pv is not None) else None
        self.last_prefill_tokens = ids.shape[1] - P
        out, self._decoder = G.generate(self.model, ids, gc.max_new_tokens, pixel_values=run_pv, pixel_mask=run_pm, temperature=gc.temperature,
                                        top_k=gc.top_k, decoder=self._decoder, stop_token=single[0] if single else None,
                                        callback=early_stop if (multi or len(single) > 1) else None, cache_size=gc.cache_size,
                                        prefill_chunk=getattr(gc, "prefill_chunk", None), cached_prefix=P, top_p=getattr(gc, "top_p", None),
                                        min_p=getattr(gc, "min_p", None), repetition_penalty=getattr(gc, "repetition_penalty", None),
                                        logprobs=getattr(gc, "logprobs", False))
        self.last_logprobs = self._decoder.logprobs.clone() if self._decoder.full else None
        if reuse:
            self._resident = (out[:-1].tolist(), pv, pm)
        new = out[ids.shape[1]:]  # the reference returns the generated part only (generate.py:174)
        return tok.decode(new.tolist()) if detokenize else new


class ChatMessage:
    def __init__(self, role: str, content: str, image_path: Optional[str] = None):
        self.role, self.content, self.image_path = role, content, image_path


class AriaChat:
    """chat.py:15-66: running history; every turn hands the whole conversation (images included) to the generator.  With
    ``GenerationConfig(reuse_prefix=True)`` the generator prefills only what the turn adds behind the cached common prefix, and images
    whose placeholders lie in that prefix skip the ViT; without it every turn re-computes everything, as the reference does."""

    def __init__(self, model_config: ModelConfig, generation_config: GenerationConfig, generator: Optional[Generator] = None):
        self.generator = generator or Generator(model_config, generation_config)
        self.history: List[ChatMessage] = []

    def add_message(self, role: str, content: str, image_path: Optional[str] = None):
        self.history.append(ChatMessage(role, content, image_path))

    def format_prompt(self):
        from PIL import Image

        messages, images = [], []
        for m in self.history:
            parts = []
            if m.image_path:
                parts.append({"text": None, "type": "image"})
                img = m.image_path
                if isinstance(img, str):
                    if img.startswith(("http://", "https://")):
                        raise RuntimeError("no network on this box: pass a local image path")
                    img = Image.open(img)
                images.append(img.convert("RGB"))
            parts.append({"text": m.content, "type": "text"})
            messages.append({"role": m.role, "content": parts})
        return messages, images

    def chat(self, message: str, image_path: Optional[str] = None) -> str:
        self.add_message("user", message, image_path)
        messages, images = self.format_prompt()
        reply = self.generator.generate(messages, images or None).split("<|assistant|>")[-1].strip()
        for s in self.generator.generation_config.stop_strings or []:
            reply = reply.replace(s, "").strip()
        self.add_message("assistant", reply)
        return reply

    def reset(self):
        self.history = []


def run_benchmark(generator: Generator, messages: List[dict], image, num_runs: int = 5, warmup: int = 2) -> dict:
    """benchmark.py:10-48 (the protocol behind the reference's published tokens/s): warm-up generations, then whole-generate latencies."""
    for _ in range(warmup):
        generator.generate(messages, image)
    lat, count = [], []
    dev = generator.model_config.device
    for _ in range(num_runs):
        t0 = time.perf_counter()
        out = generator.generate(messages, image, detokenize=False)
        if str(dev).startswith("cuda"):
            torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
        count.append(len(out))
    return {"mean_latency": mean(lat), "std_latency": stdev(lat) if len(lat) > 1 else 0, "mean_tokens": mean(count),
            "std_tokens": stdev(count) if len(count) > 1 else 0, "tokens_per_second": mean(count) / mean(lat)}
