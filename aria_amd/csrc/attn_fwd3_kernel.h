// attn_fwd3_kernel / attn_fwd3_off_kernel: included by attn.hip (inside its anonymous namespace) once per value of ATTN_FWD_OFFSET, with
// the meaning attn_fwd2_kernel.h gives it: row index q0 / q_wmin / q_abs for Q, O and LSE, causal position p0 / p_wmin / p_abs = row + q_off
// for every visibility decision.  q_off, p0 and p_wmin are wave-uniform (scalar registers); p_abs is read by the mask of edge and
// diagonal tiles only.
#if ATTN_FWD_OFFSET
#define ATTN_FWD3_NAME attn_fwd3_off_kernel
#define ATTN_FWD_QOFF_PARAM , int q_off
#else
#define ATTN_FWD3_NAME attn_fwd3_kernel
#define ATTN_FWD_QOFF_PARAM
#endif
template <int HD, int NW, bool PIPE>
__global__ __launch_bounds__(NW * 64) void ATTN_FWD3_NAME(const bf16_t* Q, const bf16_t* K, const bf16_t* V, bf16_t* O, float* LSE,
                                                        const int32_t* kv_len, const uint8_t* key_mask, int Sq, int S, int H,
                                                        long long ldq, long long ldk, long long ldv, long long ldo, float scale,
                                                        int causal, int nbatch ATTN_FWD_QOFF_PARAM) {
    using F = FwdFmt<HD>;
    using L = Fwd3Smem<HD>;
    constexpr int KS = F::KS, DT = F::DT;
    ARIA_DYN_SMEM(smem);
    char* sK = smem + L::K0;
    char* sV = smem + L::V0;
    uint8_t* sM = reinterpret_cast<uint8_t*>(smem + L::M0);   // [3][64]: the key-mask bytes of tiles t, t + 1, t + 2
    int* sFlag = reinterpret_cast<int*>(smem + L::FLAG0);     // [3]: bit 0 every key of the tile valid, bit 1 none
    const int t = threadIdx.x, l = t & 63, w = first_lane(t >> 6), h2 = l >> 5;
    int qblk, head, b;
    constexpr int QB = NW * 32, KA = PIPE ? 1 : 0;  // queries per workgroup; how many tiles K runs ahead of V in LDS
    static_assert(HD != 128 || NW == 8, "tile_dma3 deals a tile's 16 pieces to 8 waves");
    if (!attn_block_coords((Sq + QB - 1) / QB, H, nbatch, causal, true, qblk, head, b)) return;
    const int q0 = qblk * QB;
    const long long tok0 = (long long)b * S, tokq0 = (long long)b * Sq;
    const bf16_t* Qb = Q + tokq0 * ldq + head * HD;
    const bf16_t* Kb = K + tok0 * ldk + head * HD;
    const bf16_t* Vb = V + tok0 * ldv + head * HD;
    const uint8_t* kmb = key_mask ? key_mask + tok0 : nullptr;
    const int q_wmin = q0 + 32 * w, q_abs = q_wmin + (l & 31);
#if ATTN_FWD_OFFSET
    const int p0 = q0 + q_off, p_wmin = q_wmin + q_off, p_abs = q_abs + q_off;
    const int slen = min(S, q_off + Sq);
#else
    const int p0 = q0, p_wmin = q_wmin, p_abs = q_abs, slen = S;
#endif
    const int klen = kv_len ? min(slen, kv_len[b]) : slen;
    const float scale2 = scale * 1.4426950408889634f;
    F fmt;
    fmt.init(w, l, NW);

    s16x8 qf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        u32x4 v = zero16();
        const int col = kk * 16 + h2 * 8;
        if (q_abs < Sq && col < HD) v = ld16(Qb + (long long)q_abs * ldq + col);
        qf[kk] = __builtin_bit_cast(s16x8, v);
    }
    f32x16 o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = zero_acc();
    float m = -INFINITY, lsum = 0.f;
    int kv_end = klen;
    if (causal) kv_end = min(kv_end, p0 + QB);
    const int ntiles = (kv_end + 63) / 64;

    // key-mask bytes of one tile -> ring slot tile % 3 (threads 0..63: wave 0)
    auto mask_fetch = [&](int tile) __attribute__((always_inline)) -> uint8_t { return (tile * 64 + t < S) ? kmb[tile * 64 + t] : uint8_t(0); };
    auto mask_park = [&](int tile, uint8_t mv) __attribute__((always_inline)) {
        sM[(tile % 3) * 64 + t] = mv;
        const unsigned long long all = ballot(mv != 0);
        if (t == 0) sFlag[tile % 3] = int(all == ~0ull) | (int(all == 0ull) << 1);
    };
    if (ntiles > 0) {
        if (HD == 72) {  // what the pad-column reads behind the last rows touch must hold finite values (0 x NaN = NaN)
            if (t < 2) st16(sK + t * F::KTILE + F::KTILE - 16, zero16());
            if (t >= 64 && t < 68) st16(sV + ((t - 64) >> 1) * F::VTILE + F::VTILE - 32 + 16 * (t & 1), zero16());
        }
        fmt.dma_k(Kb, ldk, 0, S - 1, sK, w, l);
        fmt.dma_v(Vb, ldv, 0, S - 1, sV, w, l);
        if (PIPE && ntiles > 1) fmt.dma_k(Kb, ldk, 64, S - 1, sK + F::KTILE, w, l);
        if (kmb && t < 64) {
            mask_park(0, mask_fetch(0));
            if (ntiles > 1) mask_park(1, mask_fetch(1));
        }
    }
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) settle(qf[kk]);
    // tiles this wave works on: the causal diagonal ends its run early (the workgroup's later tiles hold no key it may see); a tile
    // WITHOUT a valid key (padded image rows) is worked on like any other -- every probability is exp2(-inf) = 0 and the running maximum
    // does not move, so it contributes exactly nothing (v2 skipped it; same bits)
    const int nmine = causal ? min(ntiles, (p_wmin + 31) / 64 + 1) : ntiles;
    auto tile_masked = [&](int tile) __attribute__((always_inline)) -> bool {
        return (tile * 64 + 64 > klen) || (causal && tile * 64 + 63 > p_wmin) || (kmb && !(sFlag[tile % 3] & 1));
    };
    // the part of an iteration every wave owes the workgroup: the tile barrier, its DMA pieces of K(it + 2) / V(it + 1), the mask bytes
    uint8_t mv = 0;
    auto duties = [&](int it) __attribute__((always_inline)) {
        wait_vm<0>();  // this wave's pieces of K(it + KA) and V(it) have landed
        sync();        // ... everybody's; every wave is done with K(it + KA - 1) and V(it - 1)
        if (it + KA + 1 < ntiles) fmt.dma_k(Kb, ldk, (it + KA + 1) * 64, S - 1, sK + ((it + KA + 1) & 1) * F::KTILE, w, l);
        if (it + 1 < ntiles) fmt.dma_v(Vb, ldv, (it + 1) * 64, S - 1, sV + ((it + 1) & 1) * F::VTILE, w, l);
        if (kmb && t < 64 && it + 2 < ntiles) mv = mask_fetch(it + 2);
    };
    auto park = [&](int it) __attribute__((always_inline)) {
        if (kmb && t < 64 && it + 2 < ntiles) mask_park(it + 2, mv);
    };
    f32x16 sa[2], sb[2];
    if (PIPE && ntiles > 0) {
        wait_vm<0>();
        sync();
        if (nmine > 0) fwd3_qk<HD>(sa, sK, qf, l);
    }
    // one iteration: tile `it` (PIPE: its scores are in `cur`) -> softmax + P V; PIPE: tile it + 1 -> scores into `nxt`
    auto iterate = [&](int it, f32x16 (&cur)[2], f32x16 (&nxt)[2]) __attribute__((always_inline)) {
        duties(it);
        if (!PIPE) fwd3_qk<HD>(cur, sK + (it & 1) * F::KTILE, qf, l);
        if (tile_masked(it)) fwd3_mask(cur, sM + (it % 3) * 64, kmb != nullptr, it * 64, klen, causal, p_abs, l);
        fwd3_step<HD, PIPE>(cur, nxt, o, m, lsum, qf, sV + (it & 1) * F::VTILE, sK + ((it + 1) & 1) * F::KTILE, scale2, l);
        park(it);
    };
    int it = 0;
    if (PIPE) {
        for (; it + 1 < nmine; it += 2) {
            iterate(it, sa, sb);
            iterate(it + 1, sb, sa);
        }
        if (it < nmine) {
            iterate(it, sa, sb);
            ++it;
        }
    } else {
        for (; it < nmine; ++it) iterate(it, sa, sb);
    }
    for (; it < ntiles; ++it) {  // the workgroup's remaining tiles (other waves' diagonals): barriers and staging only
        duties(it);
        park(it);
    }
    // ROWSUM_IN_MFMA: feature row HD = 32 (DT-1) + 8 sits in accumulator register 4 of the lanes with h2 == 0
    const float ltot = F::ROWSUM_IN_MFMA ? shfl(o[DT - 1][4], l & 31) : lsum + shfl_xor(lsum, 32);
    const float inv = ltot > 0.f ? 1.f / ltot : 0.f;
    if (q_abs < Sq) {
        if (h2 == 0 && LSE)
            LSE[((long long)b * H + head) * Sq + q_abs] = (ltot > 0.f) ? (m + log2f(ltot)) * 0.6931471805599453f : -INFINITY;
        bf16_t* orow = O + (tokq0 + q_abs) * ldo + head * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d0 = 32 * dt + 8 * rg + 4 * h2;
                if (d0 < HD) {
                    u32x2 v;
                    v[0] = pack2bf(o[dt][4 * rg] * inv, o[dt][4 * rg + 1] * inv);
                    v[1] = pack2bf(o[dt][4 * rg + 2] * inv, o[dt][4 * rg + 3] * inv);
                    *reinterpret_cast<u32x2*>(orow + d0) = v;
                }
            }
    }
}
#undef ATTN_FWD3_NAME
#undef ATTN_FWD_QOFF_PARAM
