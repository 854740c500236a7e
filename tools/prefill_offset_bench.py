"""Prefill at a cache offset on the gptfast surface at Aria's widths: what chunked prefill and chat prefix reuse cost and save, one process,
arms interleaved round by round on the same device (random weights, synthetic image; nothing is compared with a threshold).

  prefill  one-shot vs chunked (--chunk, default 4096) prefill of --tokens (16 384) tokens through Transformer.forward, 28 layers: ms per
           prefill (host clock around a device synchronise) and the peak of torch's allocator above what was resident before the call.
  chat     time to the first token of a second chat turn (--turn2 new tokens, default 30) behind a first turn of --turn1 (2048) tokens with
           one 980-pixel image (256 placeholders): gptfast.generate(max_new_tokens=1) on the whole conversation with the image, against
           generate(cached_prefix=P) on the same ids with the first turn (prompt, image, reply) resident in the KV cache.
  kernel   aria_attn_fwd_offset alone (device events, H 20, hd 128) at Sq 4096 / q_off 12 288 and Sq 32 / q_off 2048, next to the one-shot
           causal aria_attn_fwd at S 16 384 for scale.

One JSON line on stdout, and the same under --out.  An arm that raises is reported with its error; the others still run.
"""
import argparse
import json
import statistics
import sys
import time
import traceback

import torch

sys.path.insert(0, ".")
from aria_amd import gptfast as G  # noqa: E402
from aria_amd import ops  # noqa: E402

bf16 = torch.bfloat16


def init_(module, gen):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("norm.weight") or "layer_norm" in n and n.endswith("weight") or "ln_" in n and n.endswith("weight"):
                p.fill_(1.0)
            elif n.endswith("bias"):
                p.zero_()
            else:
                flat = p.view(-1)
                for o in range(0, flat.numel(), 1 << 28):
                    flat[o:o + (1 << 28)].normal_(0.0, 0.02, generator=gen)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def timed(dev, fn):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return (time.perf_counter() - t0) * 1e3, out


def med(xs):
    return round(statistics.median(xs), 3)


def arm_prefill(llm, dev, a, gen):
    T, chunk = a.tokens, a.chunk
    llm.setup_caches(1, T + 8)
    ids = torch.randint(10, llm.config.vocab_size, (1, T), generator=gen, device=dev)

    def one_shot():
        return llm(ids, torch.arange(T, device=dev), last_only=True)

    def chunked():
        for s in range(0, T, chunk):
            e = min(T, s + chunk)
            lg = llm(ids[:, s:e], torch.arange(s, e, device=dev), last_only=True)
        return lg

    res = {"one_shot": {"ms": [], "peak": []}, "chunked": {"ms": [], "peak": []}}
    last = {}
    for rnd in range(a.rounds + 1):   # round 0 warms up both arms' shapes
        for name, fn in (("one_shot", one_shot), ("chunked", chunked)):
            with torch.no_grad():
                base = 0
                if dev.type == "cuda":
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                ms, lg = timed(dev, fn)
                peak = torch.cuda.max_memory_allocated() - base if dev.type == "cuda" else 0
            last[name] = lg.float().cpu()
            if rnd:
                res[name]["ms"].append(ms)
                res[name]["peak"].append(peak)
    scale = float(last["one_shot"].abs().max())
    return {"tokens": T, "chunk": chunk,
            "one_shot": {"ms_median": med(res["one_shot"]["ms"]), "ms_all": [round(x, 2) for x in res["one_shot"]["ms"]],
                         "peak_bytes_above_resident": max(res["one_shot"]["peak"])},
            "chunked": {"ms_median": med(res["chunked"]["ms"]), "ms_all": [round(x, 2) for x in res["chunked"]["ms"]],
                        "peak_bytes_above_resident": max(res["chunked"]["peak"])},
            "last_logits_max_abs_diff_over_max_abs": round(float((last["one_shot"] - last["chunked"]).abs().max()) / max(scale, 1e-30), 5)}


def arm_chat(model, dev, a, gen):
    T1, n_reply, n_turn2 = a.turn1, 20, a.turn2
    vocab = model.config.vocab_size
    cache = T1 + n_reply + n_turn2 + 16
    model.llm.max_seq_length = -1
    model.setup_caches(1, cache)
    ids1 = torch.randint(10, vocab, (1, T1), generator=gen, device=dev)
    ids1[:, 8:264] = model.config.image_token_index
    pv = torch.randn((1, 3, 980, 980), generator=gen, device=dev).clamp_(-1, 1).to(bf16)
    pm = torch.ones((1, 980, 980), dtype=torch.bool, device=dev)
    user2 = torch.randint(10, vocab, (n_turn2,), generator=gen, device=dev)
    res = {"reuse": [], "full": []}
    decoder = None
    for rnd in range(a.rounds + 1):
        out1, decoder = G.generate(model, ids1, n_reply, pixel_values=pv, pixel_mask=pm, top_k=200, decoder=decoder, cache_size=cache)
        ids2 = torch.cat([out1, user2]).view(1, -1)
        P = out1.numel() - 1   # the reply's last token was sampled but never fed
        ms_reuse, _ = timed(dev, lambda: G.generate(model, ids2, 1, top_k=200, decoder=decoder, cache_size=cache, cached_prefix=P))
        ms_full, _ = timed(dev, lambda: G.generate(model, ids2, 1, pixel_values=pv, pixel_mask=pm, top_k=200, decoder=decoder,
                                                   cache_size=cache))
        if rnd:
            res["reuse"].append(ms_reuse)
            res["full"].append(ms_full)
    return {"first_turn_tokens": T1, "image_tokens": 256, "reply_tokens": n_reply, "second_turn_new_tokens": n_turn2,
            "second_turn_prompt_tokens": int(ids2.numel()), "cached_prefix": int(P),
            "ttft_ms_reuse_prefix": {"median": med(res["reuse"]), "all": [round(x, 2) for x in res["reuse"]]},
            "ttft_ms_full_prefill": {"median": med(res["full"]), "all": [round(x, 2) for x in res["full"]]}}


def arm_kernel(dev, a, gen):
    H, hd = 20, 128
    D, S = H * hd, 16384
    kv = torch.randn((S, 2 * D), generator=gen, device=dev).to(bf16)
    q = torch.randn((S, D), generator=gen, device=dev).to(bf16)
    k, v = kv[:, :D], kv[:, D:]
    o = torch.empty((S, D), dtype=bf16, device=dev)
    arms = {"offset_Sq4096_qoff12288": lambda: ops.attention_fwd(q[:4096], k, v, 1, 4096, H, hd, hd ** -0.5, True, out=o[:4096], Skv=S,
                                                                 q_offset=12288),
            "offset_Sq32_qoff2048": lambda: ops.attention_fwd(q[:32], k[:2080], v[:2080], 1, 32, H, hd, hd ** -0.5, True, out=o[:32], Skv=2080,
                                                              q_offset=2048),
            "one_shot_causal_S16384": lambda: ops.attention_fwd(q, k, v, 1, S, H, hd, hd ** -0.5, True, out=o)}
    times = {n: [] for n in arms}
    iters = 10
    for rnd in range(a.rounds + 1):
        for name, fn in arms.items():
            if dev.type == "cuda":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / iters
            else:
                ms = timed(dev, fn)[0]
            if rnd:
                times[name].append(ms)
    return {"H": H, "hd": hd, "launches_per_sample": iters,
            **{n: {"ms_median": round(statistics.median(t), 4), "ms_all": [round(x, 4) for x in t]} for n, t in times.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--vit-layers", type=int, default=27)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--turn1", type=int, default=2048)
    ap.add_argument("--turn2", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default="kernel,prefill,chat")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("prefill_offset_bench: no GPU -- nothing here can be measured without one")
    from aria_amd.vision import AriaVisionConfig

    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"what": "prefill at a cache offset: chunked prefill, chat prefix reuse, the offset attention kernel", "layers": a.layers,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0) if dev.type == "cuda" else str(dev)}
    arms = a.arms.split(",")
    model = None
    if "prefill" in arms or "chat" in arms:
        torch.set_default_device(dev)
        try:
            model = G.Aria(G.ModelArgs(n_layer=a.layers), AriaVisionConfig(num_hidden_layers=a.vit_layers))
        finally:
            torch.set_default_device("cpu")
        init_(model, gen)
        model.eval()
    for name in arms:
        try:
            with torch.no_grad():
                if name == "kernel":
                    out[name] = arm_kernel(dev, a, gen)
                elif name == "prefill":
                    out[name] = arm_prefill(model.llm, dev, a, gen)
                elif name == "chat":
                    out[name] = arm_chat(model, dev, a, gen)
                else:
                    raise SystemExit(f"unknown arm {name!r}")
        except Exception as e:  # noqa: BLE001 -- the other arms' numbers are still worth having
            out[name] = {"error": f"{type(e).__name__}: {e}", "traceback": traceback.format_exc()[-1500:]}
        print(f"[prefill_offset_bench] arm {name} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
