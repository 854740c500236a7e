"""The full sampler (aria_sample / aria_token_bitmap, ops.sample / ops.token_bitmap, the top_p / min_p / repetition_penalty / logprobs
options of gptfast.generate, Generator and AriaForConditionalGeneration.generate): cases shared by the emulator (test_emu_sample.py) and
the MI355X (test_gpu_sample.py).

The oracle is a float64 restatement of the semantics stated next to aria_sample's prototype (include/aria_hip.h).

Boundary margin -- a condition on the inputs, not a tolerance: the device's masses differ from float64 by about 1e-6 of the total at most
(fp32 exp, V * 2^-40 of fixed-point rounding), so no case puts top_p closer than 2e-5 to a cumulative mass: a case names a NOMINAL top_p,
the real one is the midpoint between the cumulative masses of the two distinct-value groups around it, and the half-gap is asserted.  In the
same way min_p is placed so that no (l_i - max) / T lies within 1e-3 of ln(min_p)."""
import math

import pytest
import torch

bf16 = torch.bfloat16
LOGPROB_TOL = 1e-4      # |got - want| <= LOGPROB_TOL * max(1, |want|); the fp32 arithmetic bounds it near 1e-5 * max(1, |want|)
TOP_P_MARGIN = 2e-5
MIN_P_MARGIN = 1e-3
OBSERVED = {"logprob_err": 0.0}   # the largest |got - want| / max(1, |want|) seen by this process (printed by the test modules)


# ------------------------------------------------------------------------------------------------ the oracle
def penalised(logits, seen_ids, pen):
    """bf16 logits [V] -> float32 [V] holding the bf16 values the later steps see: l < 0 ? l * pen : l / pen in fp32, rounded to bf16, on the
    tokens of seen_ids (ids outside [0, V) ignored, duplicates fine)"""
    l = logits.float().clone()
    ids = sorted({int(i) for i in seen_ids if 0 <= int(i) < l.numel()})
    if pen != 1.0 and ids:
        idx = torch.tensor(ids)
        x = l[idx]
        l[idx] = torch.where(x < 0, x * torch.tensor(pen, dtype=torch.float32), x / torch.tensor(pen, dtype=torch.float32)).to(bf16).float()
    return l


def _z_and_topk(l, T, top_k):
    x = l.double()
    z = (x - x.max()) / max(T, 1e-5)
    keep = torch.ones(l.numel(), dtype=torch.bool)
    if top_k is not None and 0 < top_k < l.numel():
        keep = x >= torch.sort(x, descending=True).values[top_k - 1]
    return x, z, keep


def _mass_above(x, e):
    """per element: the mass of the elements with a strictly greater logit"""
    vals, inv = torch.unique(x, return_inverse=True)          # ascending
    gm = torch.zeros(vals.numel(), dtype=torch.float64).scatter_add_(0, inv, e)
    above = gm.flip(0).cumsum(0).flip(0) - gm
    return above[inv]


def oracle(l, q, T, top_k=None, top_p=1.0, min_p=0.0):
    """l: float32 [V] (penalised, bf16 values) -> (kept count, token for these Exp(1) draws, its log-prob, keep mask, p / q, the log-prob of
    every token), in float64"""
    x, z, keep = _z_and_topk(l, T, top_k)
    e = torch.exp(z) * keep
    if top_p < 1.0:
        keep = keep & (_mass_above(x, e) < top_p * e.sum())
    if min_p > 0.0:
        keep = keep & (z >= math.log(min_p))
    e = torch.exp(z) * keep
    score = e / q.double()
    tok = int(torch.argmax(score))
    lps = z - torch.log(e.sum())
    return int(keep.sum()), tok, float(lps[tok]), keep, score, lps


def real_top_p(l, T, top_k, nominal):
    """the midpoint between the cumulative masses (of the logits strictly above each distinct surviving value, then 1) around ``nominal``"""
    x, z, keep = _z_and_topk(l, T, top_k)
    e = torch.exp(z) * keep
    c = torch.unique((_mass_above(x, e) / e.sum())[keep]).tolist() + [1.0]
    j = max(i for i, v in enumerate(c[:-1]) if v < nominal)
    lo, hi = c[j], c[j + 1]
    assert (hi - lo) / 2 >= TOP_P_MARGIN, ("top_p boundary margin", nominal, lo, hi)
    return (lo + hi) / 2


def real_min_p(l, T, nominal):
    """min_p with ln(min_p) midway between the two distinct values of (l - max) / T around ln(nominal)"""
    z = torch.unique(_z_and_topk(l, T, None)[1])
    t = math.log(nominal)
    below, above = z[z < t], z[z >= t]
    assert below.numel() and above.numel(), ("min_p: nothing to cut", nominal)
    lo, hi = float(below.max()), float(above.min())
    assert (hi - lo) / 2 >= MIN_P_MARGIN, ("min_p boundary margin", nominal, lo, hi)
    return math.exp((lo + hi) / 2)


def assert_margins(l, T, top_k, top_p, min_p):
    """the same two conditions for options that a case cannot place itself (the surface cases: the model makes the logits)"""
    x, z, keep = _z_and_topk(l, T, top_k)
    if top_p < 1.0:
        e = torch.exp(z) * keep
        c = torch.unique((_mass_above(x, e) / e.sum())[keep])
        assert float((c - top_p).abs().min()) >= TOP_P_MARGIN, "top_p boundary margin"
    if min_p > 0.0:
        assert float((z - math.log(min_p)).abs().min()) >= MIN_P_MARGIN, "min_p boundary margin"


def check_outputs(got_tok, got_lp, got_kept, want, tag):
    kept, tok, lp, keep, score, lps = want
    assert got_kept is None or got_kept == kept, (tag, "kept", got_kept, kept)
    if got_tok != tok:   # only an exact or last-ulp fp tie of p / q may pick the other index (the rule of kernel_cases.case_sample_topk)
        assert 0 <= got_tok < keep.numel() and bool(keep[got_tok]), (tag, "token outside the kept set", got_tok, tok)
        assert abs(float(score[tok] - score[got_tok])) <= 1e-6 * float(score[tok]), (tag, "token", got_tok, tok)
        lp = float(lps[got_tok])
    if got_lp is not None:
        err = abs(got_lp - lp) / max(1.0, abs(lp))
        OBSERVED["logprob_err"] = max(OBSERVED["logprob_err"], err)
        print(f"{tag}: logprob {got_lp:.7f} want {lp:.7f} rel err {err:.2e} kept {kept}")
        assert err <= LOGPROB_TOL, (tag, "logprob", got_lp, lp)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def run(dev, logits, q, T, top_k, top_p=1.0, min_p=0.0, pen=1.0, seen=None, update_seen=False):
    """one aria_sample launch -> (token, logprob, kept) as Python numbers"""
    from aria_amd import ops

    lp = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    kept = torch.full((1,), -1, dtype=torch.int32, device=dev)
    tok = ops.sample(logits.to(dev), q.to(dev), T, top_k, top_p, min_p, pen, seen=seen, update_seen=update_seen, logprob=lp, kept=kept)
    return int(tok.cpu()), float(lp.cpu()), int(kept.cpu())


def randn_logits(V, sigma, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * sigma).to(bf16), g


def case_sample(dev, logits, g, T, top_k=None, top_p=None, min_p=None, pen=1.0, seen_ids=(), trials=2, tag=""):
    """kept count, token and log-prob against the oracle on ``trials`` sets of draws; top_p / min_p are NOMINAL values (see the module
    docstring); the bitmap comes from aria_token_bitmap"""
    from aria_amd import ops

    V = logits.numel()
    l = penalised(logits, seen_ids, pen)
    p = 1.0 if top_p is None else real_top_p(l, T, top_k, top_p)
    m = 0.0 if min_p is None else real_min_p(l, T, min_p)
    seen = ops.token_bitmap(torch.tensor(list(seen_ids), dtype=torch.int64).to(dev), V) if pen != 1.0 else None
    kept = None
    for trial in range(trials):
        q = torch.empty(V).exponential_(1, generator=g)
        want = oracle(l, q, T, top_k, p, m)
        tok, lp, kept = run(dev, logits, q, T, top_k, p, m, pen, seen)
        check_outputs(tok, lp, kept, want, f"{tag} V={V} T={T} k={top_k} p={top_p} m={min_p} pen={pen} #{trial}")
    return kept


def seen_for(logits, g, n=40):
    """ids for the penalty: random ones (duplicates likely), the arg-max token, two outside the vocabulary"""
    V = logits.numel()
    ids = torch.randint(0, V, (min(n, V),), generator=g).tolist()
    return ids + [int(logits.float().argmax()), ids[0], -3, V, V + 77]


def case_vocab(dev, V, sigma):
    """One vocabulary size through both shapes of the launch: top-p alone (no top-k pass, the boundary found in pass C), and every option at
    once (top-k, top-p, min-p, penalty).  V = 1, 7 (tail only), 8, 1000 (not a multiple of 8, fewer chunks than threads), 8200 (a second
    chunk for some threads), 100352."""
    logits, g = randn_logits(V, sigma)
    case_sample(dev, logits, g, 0.9, None, 0.9, tag="top-p")
    if V >= 1000:
        case_sample(dev, logits, g, 2.0, 200, 0.9, 0.05 if sigma == 1 else 1e-3, 1.3, seen_for(logits, g), tag="all")
    else:
        case_sample(dev, logits, g, 2.0, 5, 0.9, None, 1.3, seen_for(logits, g), tag="all")


def case_peaked(dev):
    """one logit holds more than 0.97 of the mass: top_p = 0.9 keeps it alone"""
    logits, g = randn_logits(1000, 1.0)
    logits[417] = 14.0
    assert float(torch.softmax(logits.double(), -1)[417]) > 0.97
    assert case_sample(dev, logits, g, 1.0, None, 0.9, tag="peaked") == 1


def case_all_equal(dev, V=100352):
    """every logit equal (counts above 16 bits in one bin): the group stays whole, kept == V, log-prob == -ln V"""
    logits = torch.full((V,), 0.75).to(bf16)
    g = torch.Generator().manual_seed(3)
    assert case_sample(dev, logits, g, 0.8, None, 0.5, trials=1, tag="equal") == V
    assert case_sample(dev, logits, g, 0.8, 50, 0.5, trials=1, tag="equal, top-k") == V


def case_two_values(dev, V=1000):
    """two distinct values: 10 high ones hold ~0.35 of the mass, so top_p = 0.6 falls inside the lower group, which is kept whole"""
    logits = torch.zeros(V)
    hi = torch.randperm(V, generator=torch.Generator().manual_seed(4))[:10]
    logits[hi] = math.log(0.35 / 0.65 * (V - 10) / 10)
    logits = logits.to(bf16)
    g = torch.Generator().manual_seed(5)
    assert case_sample(dev, logits, g, 1.0, None, 0.6, tag="two values") == V
    assert case_sample(dev, logits, g, 1.0, None, 0.2, tag="two values, high group only") == 10


def case_interplay(dev):
    """which filter binds: top-k (top-p would keep more), top-p (top-k would keep more), min-p alone, min-p under top-p and top-p under min-p"""
    logits, g = randn_logits(8200, 1.0, seed=2)
    l = logits.float()
    n_p = oracle(l, torch.ones(8200), 0.9, None, real_top_p(l, 0.9, None, 0.9))[0]
    assert n_p > 300
    assert case_sample(dev, logits, g, 0.9, 50, 0.9, tag="top-k binds") < 50 + 5          # top-p acts inside the 50 survivors only
    k_big = case_sample(dev, logits, g, 0.9, 5000, 0.5, tag="top-p binds")
    assert k_big < 2500
    n_m = case_sample(dev, logits, g, 0.9, None, None, 0.05, tag="min-p alone")
    assert 1 < n_m < 8200
    assert case_sample(dev, logits, g, 0.9, None, 0.995, 0.05, tag="min-p binds under top-p") == n_m
    assert case_sample(dev, logits, g, 0.9, None, 0.3, 0.002, tag="top-p binds under min-p") < n_m
    assert case_sample(dev, logits, g, 0.9, 3000, 0.95, 0.01, tag="all three") > 1


def case_penalty(dev):
    """the arg-max token is in `seen` and stops being the maximum; penalised negative logits (pushed further down); pen < 1 (the other way);
    the bitmap built from ids with duplicates and out-of-range entries equals the host's"""
    from aria_amd import ops

    V = 1000
    logits, g = randn_logits(V, 1.0, seed=6)
    top = int(logits.float().argmax())
    neg = [int(i) for i in torch.nonzero(logits.float() < -1.0).view(-1)[:20]]
    ids = [top, top, neg[0]] + neg + [-1, V, 2 ** 31 - 1, V + 31]
    l = penalised(logits, ids, 2.0)
    assert int(l.argmax()) != top and bool((l[neg] < logits.float()[neg]).all())
    seen = ops.token_bitmap(torch.tensor(ids, dtype=torch.int64).to(dev), V).cpu()
    want = torch.zeros((V + 31) // 32, dtype=torch.int64)
    for i in set(ids):
        if 0 <= i < V:
            want[i >> 5] |= 1 << (i & 31)
    assert torch.equal(seen.long() & 0xffffffff, want)
    for pen in (2.0, 1.3, 0.7):
        case_sample(dev, logits, g, 0.7, None, 0.9, None, pen, ids, tag="penalty")
        case_sample(dev, logits, g, 0.7, 100, None, None, pen, ids, tag="penalty, top-k")
    lp2 = penalised(logits, ids, 2.0)   # top_k = 1 and equal draws: the returned token is the penalised maximum, not the raw one
    tok, _, kept = run(dev, logits, torch.ones(V), 0.05, 1, 1.0, 0.0, 2.0, ops.token_bitmap(torch.tensor(ids).to(dev), V))
    assert tok == int(lp2.argmax()) != top and kept == 1
    # seen == None or pen == 1: no penalty, whatever the bitmap says
    full = torch.full(((V + 31) // 32,), -1, dtype=torch.int32, device=dev)
    assert run(dev, logits, torch.ones(V), 0.05, 1, pen=1.0, seen=full)[0] == top
    assert run(dev, logits, torch.ones(V), 0.05, 1, pen=2.0, seen=None)[0] == top


def case_update_seen(dev):
    """update_seen sets exactly the returned token's bit (also with pen == 1), and nothing without it"""
    from aria_amd import ops

    for V in (1000, 37):
        logits, g = randn_logits(V, 1.0, seed=7)
        ids = torch.randint(0, V, (12,), generator=g)
        for pen in (1.5, 1.0):
            seen = ops.token_bitmap(ids.to(dev), V)
            before = seen.cpu().clone()
            q = torch.empty(V).exponential_(1, generator=g)
            tok, _, _ = run(dev, logits, q, 1.0, None, 1.0, 0.0, pen, seen, update_seen=False)
            assert torch.equal(seen.cpu(), before)
            tok, _, _ = run(dev, logits, q, 1.0, None, 1.0, 0.0, pen, seen, update_seen=True)
            after = before.long() & 0xffffffff
            after[tok >> 5] |= 1 << (tok & 31)
            assert torch.equal(seen.cpu().long() & 0xffffffff, after), (V, pen, tok)


NEUTRAL_GRID = [(k, T) for k in (None, 200) for T in (0.5, 0.9, 2.0)]


def case_neutral(dev, V, sigma=1.0):
    """top_p = 1, min_p = 0, pen = 1: the token of ops.sample_topk on the same draws, kept = the top-k set with its ties, for every
    (top_k, temperature) of the grid"""
    from aria_amd import ops

    logits, g = randn_logits(V, sigma)
    ld = logits.to(dev)
    for top_k, T in NEUTRAL_GRID:
        q = torch.empty(V).exponential_(1, generator=g)
        want = int(ops.sample_topk(ld, q.to(dev), T, top_k).cpu())
        tok, lp, kept = run(dev, logits, q, T, top_k)
        assert tok == want, (V, top_k, T, tok, want)
        check_outputs(tok, lp, kept, oracle(logits.float(), q, T, top_k), f"neutral V={V} k={top_k} T={T}")


def case_determinism(dev, V=8200):
    """the same call twice: the three outputs bit for bit"""
    from aria_amd import ops

    logits, g = randn_logits(V, 1.0, seed=8)
    ids = seen_for(logits, g)
    l = penalised(logits, ids, 1.2)
    p = real_top_p(l, 0.9, 3000, 0.9)
    q = torch.empty(V).exponential_(1, generator=g)
    outs = []
    for _ in range(2):
        seen = ops.token_bitmap(torch.tensor(ids).to(dev), V)
        lp = torch.zeros(1, dtype=torch.float32, device=dev)
        kept = torch.zeros(1, dtype=torch.int32, device=dev)
        tok = ops.sample(logits.to(dev), q.to(dev), 0.9, 3000, p, 0.001, 1.2, seen=seen, update_seen=True, logprob=lp, kept=kept)
        outs.append((tok.cpu(), lp.cpu().view(torch.int32), kept.cpu(), seen.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def case_validation(dev):
    from aria_amd import hip, ops

    logits = torch.zeros(64, dtype=bf16, device=dev)
    q = torch.ones(64, dtype=torch.float32, device=dev)
    nan = float("nan")
    for kw in (dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=nan), dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=nan),
               dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=nan), dict(temperature=nan),
               dict(update_seen=True)):   # (update_seen without a bitmap)
        args = dict(temperature=1.0, top_k=None)
        args.update(kw)
        with pytest.raises(hip.AriaHipError, match="ARIA_ERR_INVALID"):
            ops.sample(logits, q, **args)
    lib = hip.get_lib()
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(hip.AriaHipError, match="ARIA_ERR_UNSUPPORTED"):   # beyond the documented limit (nothing is read: refused first)
        lib.call("aria_sample", logits.data_ptr(), q.data_ptr(), (1 << 20) + 1, 0, 1.0, 1.0, 0.0, 1.0, None, 0, out.data_ptr(), None, None, None)
    with pytest.raises(hip.AriaHipError, match="ARIA_ERR_INVALID"):
        lib.call("aria_token_bitmap", None, 3, 64, out.data_ptr(), None)
    assert int(ops.sample(logits, q, 1.0, None, top_p=1.5)) == 0          # top_p >= 1 keeps all; all tied: the lowest index
    ops.token_bitmap(torch.zeros(0, dtype=torch.int64, device=dev), 64)   # no ids: a zero bitmap, no launch


# ------------------------------------------------------------------------------------------------ 2. the oracle against transformers
def distinct_logits(V, scale, seed):
    """V distinct bf16 values of magnitude 2^-6 * scale .. 8 * scale in random order: no two tokens tie"""
    pool = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(bf16).float()
    pool = pool[torch.isfinite(pool) & (pool.abs() >= scale / 64) & (pool.abs() <= 8 * scale)]
    g = torch.Generator().manual_seed(seed)
    assert pool.numel() >= V
    return pool[torch.randperm(pool.numel(), generator=g)[:V]].to(bf16), g


def case_oracle_vs_transformers():
    """The oracle's kept set == the finite entries HF's processors leave, chained in HF's order, and its log-prob == HF's log-softmax.
    Penalised logits are rounded to bf16 before the warpers see them (the documented deviation), and no tie sits at a boundary: the logits
    are distinct, and the lowest kept value is asserted to be a single token."""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (MinPLogitsWarper, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)

    for V, scale, T, top_k, top_p, min_p, pen in ((1000, 1.0, 0.9, None, 0.9, None, 1.3), (2000, 2.0, 2.0, 200, 0.9, 1e-3, 1.2),
                                                  (2000, 1.0, 0.5, 200, 0.6, None, 1.0), (1000, 0.5, 2.0, None, None, 0.05, 0.8),
                                                  (2000, 0.5, 0.9, 800, 0.95, 0.01, 1.0)):
        logits, g = distinct_logits(V, scale, seed=11)
        ids = [i for i in seen_for(logits, g) if 0 <= i < V]
        scores = logits.float()[None]
        if pen != 1.0:
            scores = RepetitionPenaltyLogitsProcessor(pen)(torch.tensor([ids]), scores)
            scores = scores.to(bf16).float()
        l = penalised(logits, ids, pen)
        assert torch.equal(scores[0], l)
        p = 1.0 if top_p is None else real_top_p(l, T, top_k, top_p)
        m = 0.0 if min_p is None else real_min_p(l, T, min_p)
        scores = TemperatureLogitsWarper(T)(None, scores.double())
        if top_k is not None:
            scores = TopKLogitsWarper(top_k)(None, scores)
        if top_p is not None:
            scores = TopPLogitsWarper(p)(None, scores)
        if min_p is not None:
            scores = MinPLogitsWarper(m)(None, scores)
        kept, tok, lp, keep, _, _ = oracle(l, torch.ones(V), T, top_k, p, m)
        assert int((l == l[keep].min()).sum()) == 1                  # no tie at the boundary
        assert 1 < kept < (top_k or V)
        assert torch.equal(torch.isfinite(scores[0]), keep), (V, T, top_k, top_p, min_p, int(torch.isfinite(scores[0]).sum()), kept)
        want_lp = torch.log_softmax(scores[0], -1)[tok]
        assert abs(float(want_lp) - lp) < 1e-9


def case_tensor_path(dev="cpu"):
    """gptfast.logits_to_probs(top_p=, min_p=) -- the tensor form of the same definitions -- keeps the oracle's set; both None: today's function"""
    from aria_amd import gptfast as G

    logits, g = randn_logits(8200, 1.0, seed=12)
    logits[torch.randperm(8200, generator=g)[:40]] = logits[7].clone()           # a group of equal logits
    l = logits.float()
    for T, top_k, top_p, min_p in ((0.9, None, 0.9, None), (0.5, 200, 0.9, 0.01), (2.0, None, None, 0.05), (1.0, 3000, 0.3, None)):
        p = None if top_p is None else real_top_p(l, T, top_k, top_p)
        m = None if min_p is None else real_min_p(l, T, min_p)
        probs = G.logits_to_probs(logits, T, top_k, p, m)
        keep = oracle(l, torch.ones(8200), T, top_k, 1.0 if p is None else p, 0.0 if m is None else m)[3]
        assert torch.equal(probs > 0, keep) and abs(float(probs.sum()) - 1) < 1e-5
    assert torch.equal(G.logits_to_probs(logits, 0.8, 50, None, None), G.logits_to_probs(logits, 0.8, 50))


# ------------------------------------------------------------------------------------------------ 3. the surface (toy gptfast model)
PROMPT = [5, 12, 77, 3, 100, 4, 8, 41, 27, 90, 6, 12, 12]
# the toy model's logits spread over about +-2: top-p binds inside the 60 survivors of the first set, min-p (a cut in the sparse upper tail,
# where the margin condition is easy to meet) in the second
OPTION_SETS = [dict(temperature=0.9, top_k=60, top_p=0.8, min_p=None, repetition_penalty=1.3),
               dict(temperature=0.7, top_k=None, top_p=0.95, min_p=0.3, repetition_penalty=1.15)]


def _toy(dev):
    from tests.prefill_offset_cases import _toy_aria

    return _toy_aria(dev)


def case_generate_vs_oracle(dev, opts, n_new=4):
    """generate(top_p, min_p, repetition_penalty) == a loop here that runs the same model steps, draws from the same generator and applies
    the oracle to every step's logits (the first token included; `seen` = the prompt and everything generated so far); decoder.logprobs
    within the log-prob bound"""
    from aria_amd import gptfast as G

    a = _toy(dev)
    V = a.config.vocab_size
    ids = torch.tensor([PROMPT], device=dev)
    T = ids.shape[1]
    torch.manual_seed(21)
    out, dec = G.generate(a, ids, n_new, cache_size=32, **opts)
    T_, k_, p_, m_ = opts["temperature"], opts["top_k"], opts["top_p"] or 1.0, opts["min_p"] or 0.0
    new = out[T:].tolist()
    lps = dec.logprobs.cpu().tolist()
    assert len(new) == n_new == len(lps)
    torch.manual_seed(21)
    with torch.no_grad():
        logits = a(None, torch.arange(T, device=dev), a.prepare_embeddings(ids), last_only=True)
        seen = list(PROMPT)
        for step in range(n_new):
            q = torch.empty(V, dtype=torch.float32, device=dev).exponential_(1).cpu()
            l = penalised(logits.reshape(-1).cpu(), seen, opts["repetition_penalty"])
            assert_margins(l, T_, k_, p_, m_)
            want = oracle(l, q, T_, k_, p_, m_)
            assert 1 < want[0] < (k_ or V)               # a filter behind top-k binds, and leaves a choice
            check_outputs(new[step], lps[step], None, want, f"generate step {step}")
            seen.append(new[step])
            logits = a(torch.tensor([[new[step]]], device=dev), torch.tensor([T + step], device=dev, dtype=torch.int32), last_only=True)
    bits = dec.seen.cpu()
    for i in range(V):   # the decoder's bitmap: the prompt and every sampled token, nothing else
        assert bool((int(bits[i >> 5]) >> (i & 31)) & 1) == (i in seen), i


def case_generate_options(dev, n_new=3):
    """a low top_p changes the stream of a fixed seed; neutral arguments reproduce the default call exactly (and take its launch); logprobs
    alone goes through aria_sample and still returns the default call's tokens; a decoder built for other options is replaced"""
    from aria_amd import gptfast as G
    from aria_amd import ops

    a = _toy(dev)
    ids = torch.tensor([PROMPT], device=dev)

    def gen(**kw):
        torch.manual_seed(22)
        return G.generate(a, ids, n_new, temperature=1.0, top_k=100, cache_size=32, **kw)

    base, dec0 = gen()
    assert not dec0.full and dec0.logprobs is None
    low, dec1 = gen(top_p=0.05)
    assert not torch.equal(low, base) and dec1.full
    calls = []
    orig = ops.sample
    ops.sample = lambda *x, **k: (calls.append(1), orig(*x, **k))[1]
    try:
        same, dec2 = gen(top_p=1.0, min_p=0.0, repetition_penalty=1.0, decoder=dec0)
        assert torch.equal(same, base) and dec2 is dec0 and not calls
        withlp, dec3 = gen(logprobs=True, decoder=dec0)
        assert dec3 is not dec0 and len(calls) == n_new and dec3.logprobs.shape == (n_new,)
        assert torch.equal(withlp, base)
        again, dec4 = gen(logprobs=True, decoder=dec3)
        assert dec4 is dec3 and torch.equal(again, base) and dec4.logprobs.shape == (n_new,)
    finally:
        ops.sample = orig
    lp = dec4.logprobs.cpu()
    assert bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    with pytest.raises(ValueError):
        gen(top_p=0.0)


def case_generator_turns(dev):
    """a reused Generator: the second turn's `seen` holds its own ids and new tokens only -- not the first turn's -- and last_logprobs
    has one entry per new token"""
    from aria_amd import gptfast_generate as GG
    from tests.prefill_offset_cases import _ListProc

    a = _toy(dev)
    V = a.config.vocab_size
    gc = GG.GenerationConfig(max_new_tokens=3, top_k=50, temperature=1.0, stop_strings=[], cache_size=48, top_p=0.9, repetition_penalty=1.2)
    gen = GG.Generator(GG.ModelConfig("unused", device=dev), gc, model=a, processor=_ListProc())
    torch.manual_seed(0)
    new1 = gen.generate([{"role": "user", "content": PROMPT}], detokenize=False).tolist()
    assert gen.last_logprobs.shape == (3,)
    dec = gen._decoder
    turn2 = [33, 2, 64, 19, 50]
    new2 = gen.generate([{"role": "user", "content": turn2}], detokenize=False).tolist()
    assert gen._decoder is dec and gen.last_logprobs.shape == (3,)
    bits = dec.seen.cpu()
    for i in range(V):
        assert bool((int(bits[i >> 5]) >> (i & 31)) & 1) == (i in turn2 + new2), (i, new1, new2)
    plain = GG.Generator(GG.ModelConfig("unused", device=dev), GG.GenerationConfig(max_new_tokens=1, top_k=50, stop_strings=[], cache_size=48),
                         model=a, processor=_ListProc())
    plain.generate([{"role": "user", "content": turn2}], detokenize=False)
    assert plain.last_logprobs is None and not plain._decoder.full


def case_hf_generate(dev, golden):
    """AriaForConditionalGeneration.generate(top_p=...) changes the output relative to omitting it (it used to be swallowed by **unused);
    the options join the cached decoder's key; do_sample=False stays greedy and still honours the penalty"""
    from aria_amd.modeling_aria import AriaConfig, AriaForConditionalGeneration
    from tests.model_cases import _load

    g = golden("aria")
    cfg = AriaConfig(vision_config=dict(g["vision_cfg"]), text_config=dict(g["text_cfg"]), projector_patch_to_query_dict=g["p2q"],
                     image_token_index=g["image_token_index"])
    model = AriaForConditionalGeneration(cfg)
    for part in ("vision_tower", "multi_modal_projector", "language_model"):
        _load(getattr(model, part), g["weights"], part + ".")
    model = model.to(dev).eval()
    text = [int(t) for t in g["input_ids"].view(-1).tolist() if t != g["image_token_index"]][:9]
    ids = torch.tensor([text], device=dev)

    def gen(**kw):
        torch.manual_seed(23)
        return model.generate(input_ids=ids, max_new_tokens=4, do_sample=True, temperature=1.0, top_k=None, **kw)[0, ids.shape[1]:].cpu()

    gen()                                            # (the first call builds the gptfast twin, which draws from the generator)
    base = gen()
    dec0 = model._gptfast_decoder
    assert not dec0.full
    low = gen(top_p=0.02)
    assert not torch.equal(low, base) and model._gptfast_decoder is not dec0 and model._gptfast_decoder.full
    assert torch.equal(gen(top_p=1.0, min_p=0.0, repetition_penalty=1.0), base) and not model._gptfast_decoder.full
    pen = model.generate(input_ids=ids, max_new_tokens=4, do_sample=False, top_p=0.02, repetition_penalty=50.0)[0, ids.shape[1]:].tolist()
    assert model._gptfast_decoder.full and model._gptfast_decoder.options[:2] == (1.0, 0.0)   # greedy: top_p / min_p play no part
    assert len(set(pen)) == 4 and not set(pen) & set(text), (text, pen)   # a huge penalty: greedy never returns a seen token


def case_inference_flags():
    from aria_amd.inference import parse_arguments

    base = ["--base_model_path", "m", "--tokenizer_path", "t", "--image_path", "i", "--prompt", "p"]
    a = parse_arguments(base)
    assert a.top_p is None and a.min_p is None and a.repetition_penalty is None
    a = parse_arguments(base + ["--top_p", "0.9", "--min_p", "0.05", "--repetition_penalty", "1.05"])
    assert (a.top_p, a.min_p, a.repetition_penalty) == (0.9, 0.05, 1.05)
