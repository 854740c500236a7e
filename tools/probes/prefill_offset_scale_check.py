"""Prefill at a cache offset against the one-shot prefill at 16 384 tokens (random weights, Aria widths), on the GPU:
  * aria_attn_fwd_offset at Sq 4096 / q_off 12 288 and Sq 32 / q_off 2048 against the same rows of the one-shot causal launch (both kernel
    families): expected bit-identical -- the same key tiles in the same order;
  * Transformer.forward in pieces of 8192 / 4096 against one call, at 1 / 2 / 4 / 28 layers: last-position logits and KV-cache rows, next to
    a yardstick for how far this random model amplifies a small change (ONE of the 16 384 prompt tokens replaced).
Written to profiles/r08_prefill_offset_scale_check.json (python tools/probes/prefill_offset_scale_check.py [out.json])."""
import json, os, sys
import torch
sys.path.insert(0, ".")
from aria_amd import gptfast as G, ops
bf16 = torch.bfloat16
dev = torch.device("cuda")
out = {}
g = torch.Generator(device=dev).manual_seed(0)
H, hd, S = 20, 128, 16384
D = H * hd
q = torch.randn((S, D), generator=g, device=dev).to(bf16)
kv = torch.randn((S, 2 * D), generator=g, device=dev).to(bf16)
k, v = kv[:, :D], kv[:, D:]
for ver in ("3", "2"):
    os.environ["ARIA_ATTN_FWD"] = ver
    o1, l1 = ops.attention_fwd(q, k, v, 1, S, H, hd, hd ** -0.5, True)
    o2, l2 = ops.attention_fwd(q[12288:], k, v, 1, 4096, H, hd, hd ** -0.5, True, Skv=S, q_offset=12288)
    o3, l3 = ops.attention_fwd(q[2048:2080], k[:2080], v[:2080], 1, 32, H, hd, hd ** -0.5, True, Skv=2080, q_offset=2048)
    torch.cuda.synchronize()
    out[f"attn_v{ver}_offset12288_equals_one_shot_rows"] = bool(torch.equal(o1[12288:], o2) and torch.equal(l1[:, :, 12288:], l2))
    out[f"attn_v{ver}_offset2048_equals_one_shot_rows"] = bool(torch.equal(o1[2048:2080], o3) and torch.equal(l1[:, :, 2048:2080], l3))
os.environ.pop("ARIA_ATTN_FWD")
print(json.dumps(out), flush=True)
T = 16384
for nl in (1, 2, 4, 28):
    with torch.device(dev):
        m = G.Transformer(G.ModelArgs(n_layer=nl))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.fill_(1.0)
            else:
                p.normal_(0, 0.02, generator=g)
    m.eval().setup_caches(1, T + 8)
    ids = torch.randint(10, 100000, (1, T), generator=g, device=dev)
    r = {}
    with torch.no_grad():
        a = m(ids, torch.arange(T, device=dev), last_only=True).float()
        a2 = m(ids, torch.arange(T, device=dev), last_only=True).float()
        c = m.layers[0].attention.kv_cache
        k0, v0 = c.k.clone(), c.v.clone()
        cl = m.layers[-1].attention.kv_cache
        kl = cl.k.float().clone()
        for chunk in (8192, 4096):
            for s in range(0, T, chunk):
                b = m(ids[:, s:s + chunk], torch.arange(s, s + chunk, device=dev), last_only=True).float()
            r[f"chunk{chunk}_logits_maxdiff_over_max"] = float((a - b).abs().max() / a.abs().max())
            r[f"chunk{chunk}_layer0_kcache_equal"] = bool(torch.equal(c.k, k0)) and bool(torch.equal(c.v, v0))
            r[f"chunk{chunk}_lastlayer_kcache_maxdiff_over_max"] = float((cl.k.float() - kl).abs().max() / kl.abs().max())
            r[f"chunk{chunk}_lastlayer_kcache_rel_l2"] = float((cl.k.float() - kl).norm() / kl.norm())
        # noise yardstick: the one-shot prefill of the same prompt with ONE early token changed, logits of the last position
        ids2 = ids.clone(); ids2[0, 5] = (ids2[0, 5] + 1) % 100000
        p = m(ids2, torch.arange(T, device=dev), last_only=True).float()
        r["one_token_of_16384_changed_logits_maxdiff_over_max"] = float((a - p).abs().max() / a.abs().max())
    r["one_shot_repeat_equal"] = bool(torch.equal(a, a2))
    out[f"layers{nl}"] = r
    print(json.dumps({f"layers{nl}": r}), flush=True)
    del m, c, cl, k0, v0, kl
    torch.cuda.empty_cache()
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else "profiles/r08_prefill_offset_scale_check.json", "w"), indent=1)
