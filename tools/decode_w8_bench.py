"""bf16 vs int8 weight-only decode of the gptfast LM at Aria's widths, interleaved in ONE process on the same device.

Two LMs from the same random weights (28 layers, D 2560, 64 experts top-6, I 1664, shared 3328, V 100 352): one bf16, one converted by
aria_amd.quantize.quantize_int8_.  Per round and model: a prefill of --prompt tokens (the int8 one includes its per-layer dequant), then
--steps batch-1 engine steps (one aria_decode_token / aria_decode_token_w8 call each, timed with a device synchronise); the models
alternate round by round.  Reported: prefill ms, engine ms per token (median / min over every timed step), tok/s, the weight bytes a
token streams (counted from the shapes: every layer's attention, router, top-k routed experts, shared expert, and the head) and their
rate against 8 TB/s.  One JSON line on stdout, and the same under --out.
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from aria_amd import gptfast as G  # noqa: E402
from aria_amd.quantize import quantize_int8_  # noqa: E402

bf16 = torch.bfloat16


def token_bytes(c, w8: bool) -> int:
    D, E, k, I, Is, V = c.dim, c.num_experts, c.router_topk, c.intermediate_size, c.intermediate_size * c.num_shared_experts, c.vocab_size
    wb = 1 if w8 else 2
    sb = 2 if w8 else 0   # one bf16 scale per streamed row
    rows = {"qkv": (3 * D, D), "wo": (D, D), "up": (2 * k * I + 2 * Is, D), "down": ((k + 1) * D, None)}
    layer = 0
    for name, (n, K) in rows.items():
        if name == "down":
            layer += wb * (k * D * I + D * Is) + sb * n
        else:
            layer += wb * n * K + sb * n
    layer += 2 * E * D + 2 * 2 * D   # router gate (bf16 in both) + the two norm weights
    return c.n_layer * layer + wb * V * D + sb * V + 2 * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt", type=int, default=280)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    c = G.ModelArgs(n_layer=a.layers)
    models = {}
    for name in ("bf16", "int8"):
        torch.manual_seed(0)
        with torch.device(dev):
            m = G.Transformer(c)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "norm" in n:
                    p.fill_(1.0)
                else:
                    p.normal_(0, 0.02)
        if name == "int8":
            quantize_int8_(m)
        m.eval().setup_caches(1, a.prompt + a.steps + 8)
        models[name] = m
    torch.cuda.synchronize()
    ids = torch.randint(0, c.vocab_size, (1, a.prompt), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res = {n: {"prefill_ms": [], "step_ms": []} for n in models}
    for rnd in range(a.rounds + 1):   # round 0: warm-up (code objects, engine tables, the int8 scratch)
        for name, m in models.items():
            with torch.no_grad():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lg = m(ids, torch.arange(a.prompt, device=dev), last_only=True)
                torch.cuda.synchronize()
                pre = (time.perf_counter() - t0) * 1e3
                tok = lg.reshape(-1).argmax().view(1, 1)
                steps = []
                for s in range(a.steps):
                    pos = torch.tensor([a.prompt + s], device=dev, dtype=torch.int32)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lg = m(tok, pos)
                    torch.cuda.synchronize()
                    steps.append((time.perf_counter() - t0) * 1e3)
                    tok = lg.reshape(-1).argmax().view(1, 1)
                assert m._engine is not None and m._engine.w8 == (name == "int8")
            if rnd:
                res[name]["prefill_ms"].append(pre)
                res[name]["step_ms"] += steps
    out = {"what": "gptfast LM decode, bf16 vs int8 weight-only, interleaved in one process", "layers": a.layers, "prompt": a.prompt,
           "steps_per_round": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name, r in res.items():
        med = statistics.median(r["step_ms"])
        nb = token_bytes(c, name == "int8")
        out[name] = {"engine_ms_per_token_median": round(med, 4), "engine_ms_per_token_min": round(min(r["step_ms"]), 4),
                     "tok_per_s": round(1e3 / med, 1), "prefill_ms_median": round(statistics.median(r["prefill_ms"]), 2),
                     "weight_bytes_per_token": nb, "weight_TBps": round(nb / (med * 1e-3) / 1e12, 3),
                     "fraction_of_8TBps": round(nb / (med * 1e-3) / 8e12, 3)}
    out["int8_over_bf16_ms"] = round(out["int8"]["engine_ms_per_token_median"] / out["bf16"]["engine_ms_per_token_median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
