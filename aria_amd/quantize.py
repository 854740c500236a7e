"""Int8 weight-only quantization of the gptfast LM (``gptfast.Aria`` / ``gptfast.Transformer``).

Format (gpt-fast's int8 naming, what ``Transformer.setup_caches`` of gptfast/model.py probes for): symmetric, one scale per output row,
``s = bf16(max(max|w_row|, 1e-8) / 127)`` computed in fp32, ``q = clamp(round_half_even(w / float(s)), -127, 127)`` as int8, ``w ~ q * s``.
  * Linear-like weights ``X.weight`` (``attention.wqkv`` -- its q/k row permutation kept: a per-row scale commutes with it --,
    ``attention.wo``, ``shared_ffn.w1 / w2 / w3``, ``output``) become int8 of the same shape, plus ``X.scales`` bf16 ``[rows]``;
  * the routed experts keep ``cond_ffn.w1 / w2 / w3`` as int8 ``[E, I, D] / [E, D, I] / [E, I, D]``, plus ``cond_ffn.scales1 [E, I]``,
    ``scales2 [E, D]``, ``scales3 [E, I]``.
The router ``gate``, the norms, ``tok_embeddings``, the vision tower and the projector stay bf16.  A quantized model is inference-only.

``python -m aria_amd.quantize --checkpoint_path <dir>/model.pth`` writes ``<dir>/model_int8.pth``.
"""
from __future__ import annotations

import argparse
import os
import re
from contextlib import contextmanager
from pathlib import Path
from typing import Dict, Tuple

import torch
import torch.nn as nn

bf16 = torch.bfloat16
LINEARS = ("attention.wqkv", "attention.wo", "feed_forward.shared_ffn.w1", "feed_forward.shared_ffn.w2", "feed_forward.shared_ffn.w3")
_LAYER_KEY = re.compile(r"^(.*layers\.\d+\.)(attention\.wqkv|attention\.wo|feed_forward\.shared_ffn\.w[123])\.weight$")
_EXPERT_KEY = re.compile(r"^(.*layers\.\d+\.feed_forward\.cond_ffn\.)w([123])$")
_HEAD_KEY = re.compile(r"^((?:llm\.)?)output\.weight$")


def quantize_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [..., K] -> (q int8 [..., K], s bf16 [...]): one symmetric scale per row (the module docstring's formulas)."""
    wf = w.float()
    s = (wf.abs().amax(dim=-1).clamp_min(1e-8) / 127).to(bf16)
    q = torch.round(wf / s.float().unsqueeze(-1)).clamp_(-127, 127).to(torch.int8)
    return q, s


def _quantize_big(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """quantize_rows one leading slice at a time (an expert tensor in fp32 would be 4 x its bf16 size)"""
    if w.dim() < 3:
        return quantize_rows(w)
    q = torch.empty(w.shape, dtype=torch.int8, device=w.device)
    s = torch.empty(w.shape[:-1], dtype=bf16, device=w.device)
    for e in range(w.shape[0]):
        q[e], s[e] = quantize_rows(w[e])
    return q, s


def _llm(model: nn.Module) -> nn.Module:
    return model.llm if hasattr(model, "llm") else model


def is_quantized(model: nn.Module) -> bool:
    return bool(getattr(_llm(model), "_w8", False))


def reject_quantized(model: nn.Module, what: str) -> None:
    """Training, LoRA and expert parallelism work on bf16 weights only."""
    if any(getattr(m, "_w8", False) for m in model.modules()):
        raise NotImplementedError(f"{what}: the model holds int8 weight-only quantized weights (inference only); load the bf16 checkpoint")


def _holders(llm: nn.Module):
    """(module, weight attribute, scales attribute) of every quantized tensor, layer by layer, then the head"""
    for blk in llm.layers:
        for name in LINEARS:
            yield blk.get_submodule(name), "weight", "scales"
        cf = blk.feed_forward.cond_ffn
        for i in (1, 2, 3):
            yield cf, f"w{i}", f"scales{i}"
    yield llm.output, "weight", "scales"


def _set(mod: nn.Module, wname: str, sname: str, q: torch.Tensor, s: torch.Tensor) -> None:
    mod._parameters[wname] = nn.Parameter(q, requires_grad=False)
    if sname in mod._buffers:
        mod._buffers[sname] = s
    else:
        mod.register_buffer(sname, s)


def _mark(llm: nn.Module) -> None:
    llm._w8 = True
    llm._w8_scratch = None
    llm._engine = None
    llm._bump_weights_version()


@torch.no_grad()
def quantize_int8_(model: nn.Module) -> nn.Module:
    """Convert a ``gptfast.Aria`` / ``gptfast.Transformer`` in place, tensor by tensor: each bf16 weight is released as soon as its codes
    exist, so the peak stays near the bf16 model's size.  Drops the decode engine (it holds raw addresses)."""
    llm = _llm(model)
    if getattr(llm, "_w8", False):
        return model
    for mod, wname, sname in _holders(llm):
        w = mod._parameters[wname]
        q, s = _quantize_big(w.data)
        mod._parameters[wname] = None
        del w
        _set(mod, wname, sname, q, s)
    _mark(llm)
    return model


def convert_structure_(model: nn.Module) -> nn.Module:
    """The quantized module structure with uninitialised codes and scales (what ``gptfast.load_model_pth`` copies an int8 checkpoint into)."""
    llm = _llm(model)
    if getattr(llm, "_w8", False):
        return model
    for mod, wname, sname in _holders(llm):
        w = mod._parameters[wname]
        q = torch.empty(w.shape, dtype=torch.int8, device=w.device)
        s = torch.empty(w.shape[:-1], dtype=bf16, device=w.device)
        mod._parameters[wname] = None
        del w
        _set(mod, wname, sname, q, s)
    _mark(llm)
    return model


def is_int8_state_dict(sd: Dict[str, torch.Tensor]) -> bool:
    return any(k.endswith(".scales") or re.search(r"\.cond_ffn\.scales[123]$", k) for k in sd)


@torch.no_grad()
def quantize_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A bf16 gptfast state dict (``model.pth``) -> the int8 one; the tensors that stay bf16 are passed through."""
    out = {}
    for k, v in sd.items():
        m1, m2, m3 = _LAYER_KEY.match(k), _EXPERT_KEY.match(k), _HEAD_KEY.match(k)
        if m1 or m3:
            out[k], out[k[: -len("weight")] + "scales"] = quantize_rows(v)
        elif m2:
            out[k], out[m2.group(1) + "scales" + m2.group(2)] = _quantize_big(v)
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------- the dequantizing forward
def _align(n: int) -> int:
    return (n + 127) // 128 * 128   # bf16 elements: 256 bytes


def _layer_layout(c):
    """element offsets of one layer's dequantized weights in the scratch (every view 256-byte aligned; w1 | w3 and the shared pair adjacent,
    so the fused gate / up launches take them as they take the bf16 model's re-homed pairs)"""
    D, E, I, Is = c.dim, c.num_experts, c.intermediate_size, c.intermediate_size * c.num_shared_experts
    shapes = [("wqkv", (3 * D, D)), ("wo", (D, D)), ("w13", (2, E, I, D)), ("w2", (E, D, I)), ("s13", (2, Is, D)), ("s2", (D, Is))]
    off, lay = 0, {}
    for name, shape in shapes:
        lay[name] = (off, shape)
        n = 1
        for d in shape:
            n *= d
        off += _align(n)
    return lay, off


def _scratch(llm) -> torch.Tensor:
    c = llm.config
    dev = llm.output.weight.device
    _, n = _layer_layout(c)
    n = max(n, _align(c.vocab_size * c.dim))
    sc = getattr(llm, "_w8_scratch", None)
    if sc is None or sc.device != dev or sc.numel() < n:
        llm._w8_scratch = sc = torch.empty(n, dtype=bf16, device=dev)
    return sc


def _view(sc, lay, name):
    off, shape = lay[name]
    n = 1
    for d in shape:
        n *= d
    return sc[off:off + n].view(shape)


@contextmanager
def dequantized_layer(llm, blk):
    """Run ``blk`` on bf16 weights: its codes are expanded into the model's one-layer scratch and its modules see views of it for the duration
    (the tile kernels of the bf16 model then run unchanged)."""
    from . import ops

    sc = _scratch(llm)
    lay, _ = _layer_layout(llm.config)
    a, f = blk.attention, blk.feed_forward
    cf, sf = f.cond_ffn, f.shared_ffn
    w13, s13 = _view(sc, lay, "w13"), _view(sc, lay, "s13")
    plan = [(a.wqkv, "weight", "scales", _view(sc, lay, "wqkv")), (a.wo, "weight", "scales", _view(sc, lay, "wo")),
            (cf, "w1", "scales1", w13[0]), (cf, "w3", "scales3", w13[1]), (cf, "w2", "scales2", _view(sc, lay, "w2")),
            (sf.w1, "weight", "scales", s13[0]), (sf.w3, "weight", "scales", s13[1]), (sf.w2, "weight", "scales", _view(sc, lay, "s2"))]
    saved = []
    try:
        for mod, wname, sname, view in plan:
            q = mod._parameters[wname]
            ops.dequant_w8(q.data, mod._buffers[sname], out=view)
            saved.append((mod, wname, q))
            mod._parameters[wname] = nn.Parameter(view, requires_grad=False)
        yield
    finally:
        for mod, wname, q in saved:
            mod._parameters[wname] = q


def gemv_w8_serves(K: int) -> bool:
    """aria_gemv_w8's reduction limits (8-element chunks, at most 8 per lane)"""
    return K % 8 == 0 and 0 < K <= 4096


def head_logits(llm, h: torch.Tensor, last_only: bool) -> torch.Tensor:
    """The output head of a quantized model on h [rows, D]: one int8 GEMV per row for ``last_only`` (no 257 MB dequant), else the head
    dequantized into the scratch and the tile GEMM (also for ``last_only`` when the GEMV does not take the width)."""
    from . import ops

    q, s = llm.output.weight, llm.output.scales
    if last_only and gemv_w8_serves(q.shape[1]):
        return torch.stack([ops.gemv_w8(q, s, h[r]) for r in range(h.shape[0])])
    sc = _scratch(llm)
    w = sc[: q.numel()].view(q.shape)
    ops.dequant_w8(q.data, s, out=w)
    return ops.gemm(h, w)


def _atoi(s: str) -> int:
    """C atoi: optional leading whitespace and sign, then the leading digits; 0 when there are none"""
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def engine_serves(c) -> bool:
    """aria_decode_token_w8's shape limits (csrc/decode.hip): the six-launch schedule with a fused down-projection form"""
    e = os.environ.get("ARIA_DECODE_FUSE")
    if e is not None and _atoi(e) == 0:   # parsed as the library parses it (decode.hip decode_fuse_enabled: atoi)
        return False
    Is = c.intermediate_size * c.num_shared_experts

    def nc(k):
        return (k // 8 + 63) // 64

    ncI, ncS = nc(c.intermediate_size), nc(Is)
    forms = (ncI == 4 and ncS == 7) or (ncI == 1 and ncS == 1) or (ncI <= 2 and ncS <= 4)
    return (1 <= c.router_topk <= 6 and c.router_topk <= c.num_experts and c.num_experts <= 256 and Is % c.intermediate_size == 0 and forms
            and c.dim % 8 == 0 and c.intermediate_size % 8 == 0 and max(c.dim, c.intermediate_size, Is) <= 4096)


def main(argv=None):
    ap = argparse.ArgumentParser(description="int8 weight-only quantization of a gptfast model.pth -> model_int8.pth next to it")
    ap.add_argument("--checkpoint_path", type=Path, required=True)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args(argv)
    sd = torch.load(str(a.checkpoint_path), map_location="cpu", mmap=True, weights_only=True)
    if is_int8_state_dict(sd):
        raise SystemExit(f"{a.checkpoint_path} is already int8-quantized")
    out = a.out or a.checkpoint_path.with_name("model_int8.pth")
    torch.save(quantize_state_dict(sd), str(out))
    print(f"wrote {out}")
    return out


if __name__ == "__main__":
    main()
