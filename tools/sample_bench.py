"""The one-launch samplers at Aria's vocabulary (V = 100 352), interleaved in ONE process on the same device.

Per round every variant runs --reps launches back to back between two device events (time per launch = elapsed / reps); the variants
alternate round by round and the medians over the rounds are reported:
  sample_topk          aria_sample_topk (temperature + top-k): the default path's launch, the yardstick
  sample_neutral       aria_sample with top_p = 1, min_p = 0, no penalty (the same passes plus the kept-set sum for the log-prob)
  sample_top_p         aria_sample with top-k and top-p (adds the mass histogram to pass B and, usually, pass C)
  sample_all           aria_sample with top-k, top-p, min-p, repetition penalty (bitmap of --seen tokens, update_seen) and log-prob
  torch_chain          the same options from torch ops: penalty (gather / where / scatter), temperature, top-k, sort-based top-p, min-p,
                       softmax, divide by the draws, arg-max
The draws are made once (the `exponential_` launch is common to all).  One JSON line on stdout, and the same under --out.
"""
import argparse
import json
import math
import statistics
import sys

import torch

sys.path.insert(0, ".")
from aria_amd import ops  # noqa: E402

bf16 = torch.bfloat16


def torch_chain(logits, q, ids, T, top_k, top_p, min_p, pen):
    x = logits.float()
    s = x.gather(0, ids)
    x = x.scatter(0, ids, torch.where(s < 0, s * pen, s / pen))
    x = x / T
    v, _ = torch.topk(x, top_k)
    x = torch.where(x < v[-1], -float("inf"), x)
    srt, order = torch.sort(x, descending=False)
    drop = srt.softmax(-1).cumsum(-1) <= 1 - top_p
    drop[-1] = False
    x = x.masked_fill(drop.scatter(0, order, drop), -float("inf"))
    x = x.masked_fill(x - x.max() < math.log(min_p), -float("inf"))
    return torch.argmax(torch.softmax(x, -1) / q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=100352)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seen", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    V, T, K, P, M, PEN = a.vocab, 0.8, 200, 0.9, 0.02, 1.05
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn(V, device=dev, generator=g) * 3.0).to(bf16)
    q = torch.empty(V, device=dev).exponential_(1, generator=g)
    ids = torch.randint(0, V, (a.seen,), device=dev, generator=g)
    seen = ops.token_bitmap(ids, V)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    lp = torch.zeros(1, dtype=torch.float32, device=dev)
    kept = torch.zeros(1, dtype=torch.int32, device=dev)
    variants = {
        "sample_topk": lambda: ops.sample_topk(logits, q, T, K, out=out),
        "sample_neutral": lambda: ops.sample(logits, q, T, K, out=out, logprob=lp),
        "sample_top_p": lambda: ops.sample(logits, q, T, K, P, out=out, logprob=lp),
        "sample_all": lambda: ops.sample(logits, q, T, K, P, M, PEN, seen=seen, update_seen=True, out=out, logprob=lp, kept=kept),
        "torch_chain": lambda: torch_chain(logits, q, ids, T, K, P, M, PEN),
    }
    us = {n: [] for n in variants}
    for rnd in range(a.rounds + 2):   # rounds 0, 1: warm-up (code objects, the caching allocator)
        for name, fn in variants.items():
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            beg.record()
            for _ in range(a.reps):
                fn()
            end.record()
            torch.cuda.synchronize()
            if rnd >= 2:
                us[name].append(beg.elapsed_time(end) * 1e3 / a.reps)
    variants["sample_all"]()
    torch.cuda.synchronize()
    res = {"what": "one token's sampling, time per launch (us), variants interleaved in one process", "vocab": V, "rounds": a.rounds,
           "reps_per_round": a.reps, "options": {"temperature": T, "top_k": K, "top_p": P, "min_p": M, "repetition_penalty": PEN, "seen": a.seen},
           "device": torch.cuda.get_device_name(0), "kept_with_all_options": int(kept)}
    for name, v in us.items():
        res[name] = {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2)}
    for name in ("sample_neutral", "sample_top_p", "sample_all", "torch_chain"):
        res[name]["over_sample_topk"] = round(res[name]["us_median"] / res["sample_topk"]["us_median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
