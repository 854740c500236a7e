// The full sampler of the decode path as ONE launch of one workgroup: repetition penalty, temperature, top-k, top-p, min-p (the order of
// HF's processor chain), the arg-max of p / q on the caller's Exp(1) draws, the log-probability of the returned token and the size of the
// kept set.  aria_sample_topk (decode.hip) stays the default path's launch; this kernel has its structure -- an exact radix select on
// the 16-bit order key of a bf16, per-wave 256-bin histograms in LDS -- and adds to it:
//   * the penalty: a token whose bit is set in the `seen` bitmap (global memory, one bit per vocabulary entry) has its logit replaced by
//     bf16_rne(l < 0 ? l * pen : l / pen), recomputed in every pass (one byte of the bitmap per 16-byte chunk of logits).  Rounded to
//     bf16, a penalised logit still has a 16-bit key, so the select stays exact;
//   * top-p, decided on INTEGER masses: m_i = trunc(exp((l_i - max) / T) * 2^40) (<= 2^40; V <= 2^20 keeps every sum below 2^60).  A sum
//     of integers does not depend on the order of the LDS atomics that form it, so the boundary is a pure function of the inputs.  Pass B
//     adds m_i into per-wave 256-bin mass histograms over the high byte (next to the low-byte counts of the top-k boundary bin); a scan
//     from the top finds the bin in which the mass above reaches top_p * total; pass C counts the low bytes inside that bin, where a bin
//     holds ONE value and its mass is count * m(value).  A distinct value is kept iff the mass strictly above it is < top_p * total, so
//     equal logits stay together and the maximum is always kept;
//   * min-p as a predicate of the last pass: (l_i - max) / T >= ln(min_p);
//   * the last pass sums the masses of the kept set (integers again) for the log-probability and counts it.
// Passes over the logits: A (maximum, high-byte counts), B (top-k and / or top-p active), C (top-p boundary outside the top-k bin), D.
#include "aria_device.h"
#include "aria_hip.h"
#include <cmath>

namespace {
using namespace ad;

typedef unsigned long long u64;
constexpr int SAMPLE_THREADS = 1024;
constexpr int NWV = SAMPLE_THREADS / 64;
constexpr float MASS_SCALE = 1099511627776.0f;  // 2^40
constexpr int64_t SAMPLE_MAX_V = 1ll << 20;

__device__ __forceinline__ uint32_t order_key(bf16_t b) { return (b & 0x8000u) ? (~uint32_t(b) & 0xffffu) : (uint32_t(b) | 0x8000u); }
__device__ __forceinline__ bf16_t key_value(uint32_t key) { return bf16_t((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu)); }
__device__ __forceinline__ bf16_t penalise(bf16_t b, float pen) {
    const float x = bf2f(b);
    return f2bf(x < 0.f ? x * pen : x / pen);
}
// the ONE definition of a logit's integer mass (pass B's histogram, the per-value masses of a boundary bin, pass D's sum)
__device__ __forceinline__ u64 mass_fx(bf16_t b, float mx, float inv_temp) { return u64(expf((bf2f(b) - mx) * inv_temp) * MASS_SCALE); }
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int d) {
    const uint32_t lo = shfl_xor(uint32_t(v), d), hi = shfl_xor(uint32_t(v >> 32), d);
    return (u64(hi) << 32) | lo;
}

// seen_rd: the bitmap the penalty reads (NULL: no penalty); seen_wr: where the returned token's bit is set (NULL: nowhere)
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(const bf16_t* logits, const float* q, int V, int k, float inv_temp, float top_p,
                                                                float ln_min_p, float pen, const uint32_t* seen_rd, uint32_t* seen_wr,
                                                                int32_t* out_token, float* out_logprob, int32_t* out_kept) {
    ARIA_SMEM_STATIC int hist[NWV][256];   // counts, one histogram per wave, folded into hist[0]
    ARIA_SMEM_STATIC u64 mass[NWV][256];   // integer masses over the high byte, folded into mass[0]; mass[1] = per-value masses of a boundary bin
    ARIA_SMEM_STATIC int sel[4];           // [0] top-k boundary high byte (-1: top-k keeps all)  [1] rank wanted inside it  [2] threshold key
                                           // [3] top-p boundary high byte still to be resolved (-1: none)
    ARIA_SMEM_STATIC u64 selm[2];          // [0] mass above the bin sel[3]  [1] total mass of the top-k survivors
    ARIA_SMEM_STATIC float red_v[NWV];
    ARIA_SMEM_STATIC int red_i[NWV];
    ARIA_SMEM_STATIC int red_c[NWV];
    ARIA_SMEM_STATIC u64 red_m[NWV];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const bool all = k >= V, do_p = top_p < 1.0f;
    const int nch = V >> 3;  // 16-byte chunks (8 logits); the tail (V % 8) goes element-wise
    const uint8_t* seen_b = reinterpret_cast<const uint8_t*>(seen_rd);  // byte c of the bitmap = the bits of chunk c (little endian)
    auto scan = [&](auto&& f) {  // f(penalised logit, index) over this thread's share of the vocabulary
        for (int c = t; c < nch; c += SAMPLE_THREADS) {
            const u32x4 v = ld16(logits + (long long)c * 8);
            const uint32_t sb = seen_b ? uint32_t(seen_b[c]) : 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bf16_t b = bf16_t(e & 1 ? v[e >> 1] >> 16 : v[e >> 1] & 0xffffu);
                if ((sb >> e) & 1u) b = penalise(b, pen);
                f(b, c * 8 + e);
            }
        }
        for (int i = nch * 8 + t; i < V; i += SAMPLE_THREADS) {
            bf16_t b = logits[i];
            if (seen_rd && ((seen_rd[i >> 5] >> (i & 31)) & 1u)) b = penalise(b, pen);
            f(b, i);
        }
    };
    auto clear = [&](bool masses) {
        for (int i = t; i < NWV * 256; i += SAMPLE_THREADS) {
            (&hist[0][0])[i] = 0;
            if (masses) (&mass[0][0])[i] = 0;
        }
        sync();
    };
    auto fold = [&](bool masses) {  // row 0 = sum over the waves
        sync();
        if (t < 256) {
            int c = 0;
            for (int ww = 0; ww < NWV; ++ww) c += hist[ww][t];
            hist[0][t] = c;
            if (masses) {
                u64 m = 0;
                for (int ww = 0; ww < NWV; ++ww) m += mass[ww][t];
                mass[0][t] = m;
            }
        }
        sync();
    };
    // pass A: the maximum and the histogram of the high byte
    float mx = -INFINITY;
    clear(false);
    scan([&](bf16_t b, int) {
        mx = fmaxf(mx, bf2f(b));
        if (!all) atomic_add(&hist[w][order_key(b) >> 8], 1);
    });
    mx = wave_max(mx);
    if (l == 0) red_v[w] = mx;
    fold(false);
    if (t == 0) {
        float m = red_v[0];
        for (int i = 1; i < NWV; ++i) m = fmaxf(m, red_v[i]);
        red_v[0] = m;
        int above = 0, b1 = -1;
        if (!all) {
            for (b1 = 255; b1 > 0; --b1) {
                if (above + hist[0][b1] >= k) break;
                above += hist[0][b1];
            }
        }
        sel[0] = b1;
        sel[1] = k - above;
        sel[2] = 0;
        sel[3] = -1;
    }
    sync();
    mx = red_v[0];
    const int b1 = sel[0], want = sel[1];
    sync();
    // the per-value masses of a boundary bin whose low-byte counts are in hist[0]: mass[1][lo] = count * m(value); then thread 0 walks down
    // from the top value while the mass strictly above stays below the target, and returns the lowest key it kept
    auto bin_masses = [&](int bin) {
        if (t < 256) mass[1][t] = hist[0][t] ? u64(hist[0][t]) * mass_fx(key_value(uint32_t(bin << 8 | t)), mx, inv_temp) : 0;
        sync();
    };
    auto walk_bin = [&](int bin, int lo_min, u64 cum, double target, int thr) {
        for (int lo = 255; lo >= lo_min; --lo) {
            if (!hist[0][lo]) continue;
            if (!(double(cum) < target)) break;
            thr = bin << 8 | lo;
            cum += mass[1][lo];
        }
        return thr;
    };
    // pass B: low-byte counts inside the top-k boundary bin (-> the exact top-k threshold) and the masses of everything above that bin
    if (!all || do_p) {
        clear(do_p);
        scan([&](bf16_t b, int) {
            const uint32_t key = order_key(b);
            const int hi = int(key >> 8);
            if (hi == b1) atomic_add(&hist[w][key & 255u], 1);
            if (do_p && hi > b1) atomic_add(&mass[w][hi], mass_fx(b, mx, inv_temp));
        });
        fold(do_p);
        if (do_p && !all) bin_masses(b1);
        if (t == 0) {
            int b2 = 0;
            if (!all) {
                int cum = 0;
                for (b2 = 255; b2 > 0; --b2) {
                    cum += hist[0][b2];
                    if (cum >= want) break;
                }
                sel[2] = b1 << 8 | b2;
            }
            if (do_p) {
                u64 total = 0;
                for (int h = 255; h > b1; --h) total += mass[0][h];
                if (!all)
                    for (int lo = 255; lo >= b2; --lo) total += mass[1][lo];
                const double target = double(top_p) * double(total);
                u64 cum = 0;
                int bp = -1;
                for (int h = 255; h > b1; --h) {
                    if (!mass[0][h]) continue;
                    if (!(double(cum + mass[0][h]) < target)) {
                        bp = h;
                        break;
                    }
                    cum += mass[0][h];
                }
                sel[3] = bp;
                selm[0] = cum;
                selm[1] = total;
                if (bp < 0 && !all) sel[2] = walk_bin(b1, b2, cum, target, sel[2]);  // the boundary lies in the top-k bin (or nowhere)
            }
        }
        sync();
    }
    // pass C: the top-p boundary inside a bin above the top-k bin
    const int bp = sel[3];
    if (bp >= 0) {
        sync();
        clear(false);
        scan([&](bf16_t b, int) {
            const uint32_t key = order_key(b);
            if (int(key >> 8) == bp) atomic_add(&hist[w][key & 255u], 1);
        });
        fold(false);
        bin_masses(bp);
        if (t == 0) sel[2] = walk_bin(bp, 0, selm[0], double(top_p) * double(selm[1]), sel[2]);
        sync();
    }
    const uint32_t thr = uint32_t(sel[2]);
    // pass D: arg-max of p_i / q_i over the kept logits (the lowest index wins ties), their count and their mass
    float best = -1.f;
    int besti = 0x7fffffff, cnt = 0;
    u64 msum = 0;
    scan([&](bf16_t b, int i) {
        const float z = (bf2f(b) - mx) * inv_temp;
        if (order_key(b) >= thr && z >= ln_min_p) {
            const float e = expf(z);
            const float s = e / q[i];
            ++cnt;
            msum += u64(e * MASS_SCALE);
            if (s > best || (s == best && i < besti)) {
                best = s;
                besti = i;
            }
        }
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = shfl_xor(best, d);
        const int oi = shfl_xor(besti, d);
        cnt += shfl_xor(cnt, d);
        msum += shfl_xor_u64(msum, d);
        if (ov > best || (ov == best && oi < besti)) {
            best = ov;
            besti = oi;
        }
    }
    if (l == 0) {
        red_v[w] = best;
        red_i[w] = besti;
        red_c[w] = cnt;
        red_m[w] = msum;
    }
    sync();
    if (t == 0) {
        for (int i = 1; i < NWV; ++i) {
            cnt += red_c[i];
            msum += red_m[i];
            if (red_v[i] > best || (red_v[i] == best && red_i[i] < besti)) {
                best = red_v[i];
                besti = red_i[i];
            }
        }
        if (besti >= V) besti = 0;  // (NaN logits: nothing compared greater -- stay in range)
        out_token[0] = besti;
        if (out_kept) out_kept[0] = cnt;
        if (out_logprob) {
            bf16_t b = logits[besti];
            if (seen_rd && ((seen_rd[besti >> 5] >> (besti & 31)) & 1u)) b = penalise(b, pen);
            out_logprob[0] = (bf2f(b) - mx) * inv_temp - logf(float(msum) * (1.0f / MASS_SCALE));
        }
        if (seen_wr) seen_wr[besti >> 5] |= 1u << (besti & 31);  // (the only writer: every read of the bitmap lies behind the barrier above)
    }
}

__global__ void token_bitmap_kernel(const int32_t* ids, long long n, int V, uint32_t* seen) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    if (id >= 0 && id < V) atomic_or(&seen[id >> 5], 1u << (id & 31));
}

}  // namespace

extern "C" int aria_sample(const void* logits, const float* q, int64_t V, int64_t top_k, float temperature, float top_p, float min_p,
                           float repetition_penalty, uint32_t* seen, int update_seen, int32_t* out_token, float* out_logprob, int32_t* out_kept,
                           void* stream) {
    if (!logits || !q || !out_token || V <= 0) return ARIA_ERR_INVALID;
    if (!(top_p > 0.f) || !(min_p >= 0.f) || min_p >= 1.f || !(repetition_penalty > 0.f) || temperature != temperature) return ARIA_ERR_INVALID;
    if (update_seen && !seen) return ARIA_ERR_INVALID;
    if (V > SAMPLE_MAX_V) return ARIA_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(logits) & 15) return ARIA_ERR_ALIGN;  // 16-byte loads
    const float t = temperature > 1e-5f ? temperature : 1e-5f;
    const int k = (top_k <= 0 || top_k >= V) ? int(V) : int(top_k);
    const uint32_t* seen_rd = repetition_penalty != 1.0f ? seen : nullptr;
    ARIA_LAUNCH(sample_kernel, dim3(1), dim3(SAMPLE_THREADS), 0, stream, static_cast<const bf16_t*>(logits), q, int(V), k, 1.0f / t, top_p,
                min_p > 0.f ? logf(min_p) : -INFINITY, repetition_penalty, seen_rd, update_seen ? seen : nullptr, out_token, out_logprob, out_kept);
    return aria_check_launch();
}

extern "C" int aria_token_bitmap(const int32_t* ids, int64_t n, int64_t V, uint32_t* seen, void* stream) {
    if (n < 0 || V <= 0 || !seen || (n > 0 && !ids)) return ARIA_ERR_INVALID;
    if (V > SAMPLE_MAX_V || n >= (1ll << 31) * 256) return ARIA_ERR_UNSUPPORTED;
    if (n == 0) return ARIA_OK;
    ARIA_LAUNCH(token_bitmap_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, ids, (long long)n, int(V), seen);
    return aria_check_launch();
}
