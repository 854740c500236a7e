// attn_fwd2_kernel / attn_fwd2_off_kernel: included by attn.hip (inside its anonymous namespace) once per value of ATTN_FWD_OFFSET.
//  0: attn_fwd2_kernel -- query row i is at causal position i (Sq == S when causal).
//  1: attn_fwd2_off_kernel -- causal forward of Sq new queries against a cache of S rows per batch entry, read in place: row i sits at
//     position q_off + i and sees key j iff j <= q_off + i and j < klen = min(S, q_off + Sq[, kv_len[b]]); the rows behind klen hold
//     finite junk and get probability exactly 0.  (aria_attn_fwd_offset; the reference's KVCache.update + causal_mask[input_pos],
//     gptfast/model.py:199-231, 76-91.)
// Two roles are kept apart: the ROW INDEX (q0, q_wmin, q_abs) addresses Q, O and LSE and is tested against Sq; the CAUSAL POSITION
// (p0, p_wmin, p_abs = row + q_off) decides which tiles are worked on, which need the mask, and which keys are dead.
#if ATTN_FWD_OFFSET
#define ATTN_FWD2_NAME attn_fwd2_off_kernel
#define ATTN_FWD_QOFF_PARAM , int q_off
#else
#define ATTN_FWD2_NAME attn_fwd2_kernel
#define ATTN_FWD_QOFF_PARAM
#endif
template <int HD, int NW>
__global__ __launch_bounds__(NW * 64) void ATTN_FWD2_NAME(const bf16_t* Q, const bf16_t* K, const bf16_t* V, bf16_t* O, float* LSE,
                                                        const int32_t* kv_len, const uint8_t* key_mask, int Sq, int S, int H,
                                                        long long ldq, long long ldk, long long ldv, long long ldo, float scale,
                                                        int causal, int nbatch ATTN_FWD_QOFF_PARAM) {
    using C = Cfg2<HD, NW>;
    ARIA_DYN_SMEM(smem);
    bf16_t* sK = reinterpret_cast<bf16_t*>(smem);          // [2][64][KP]
    bf16_t* sV = sK + 2 * 64 * C::KP;                      // [2][64][VP]
    uint8_t* sM = reinterpret_cast<uint8_t*>(sV + 2 * 64 * C::VP);  // [2][64]
    int* sFlag = reinterpret_cast<int*>(sM + 128);         // [2]
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h2 = l >> 5;
    int qblk, head, b;
    if (!attn_block_coords((Sq + C::QB - 1) / C::QB, H, nbatch, causal, true, qblk, head, b)) return;
    const int q0 = qblk * C::QB;
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

    s16x8 qf[C::KS];
#pragma unroll
    for (int kk = 0; kk < C::KS; ++kk) {
        u32x4 v = zero16();
        const int col = kk * 16 + h2 * 8;
        if (q_abs < Sq && col < HD) v = ld16(Qb + (long long)q_abs * ldq + col);
        qf[kk] = __builtin_bit_cast(s16x8, v);
    }
#pragma unroll
    for (int kk = 0; kk < C::KS; ++kk) settle(qf[kk]);  // (see settle(): keeps the wait for Q out of the key-tile loop)
    f32x16 o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = zero_acc();
    float m = -INFINITY, lsum = 0.f;

    int kv_end = klen;
    if (causal) kv_end = min(kv_end, p0 + C::QB);
    const int ntiles = (kv_end + 63) / 64;

    // pad columns: K's reduction pad must be zero (Q's is), V's pad only feeds discarded output rows but must not be NaN-free
    // garbage either way -> zero both once (tile stores never touch them)
    if (C::HDK != HD || C::VP > HD) {
        for (int i = t; i < 2 * 64; i += C::NT2) {
            if (C::HDK != HD) st16(sK + i * C::KP + HD, zero16());
            for (int c = HD; c < C::VP; c += 8) st16(sV + i * C::VP + c, zero16());
            if (C::ROWSUM_IN_MFMA) sV[i * C::VP + HD] = 0x3F80;  // bf16 1.0: the "ones" column
        }
    }
    u32x4 rk[C::NCH], rv[C::NCH];
    if (ntiles > 0) {
        tile2_load<HD, NW>(rk, Kb, ldk, 0, S, t);
        tile2_load<HD, NW>(rv, Vb, ldv, 0, S, t);
        tile2_store<HD, NW, C::KP>(rk, sK, t);
        tile2_store<HD, NW, C::VP>(rv, sV, t);
        if (kmb && t < 64) {
            const uint8_t mv = t < S ? kmb[t] : 0;
            sM[t] = mv;
            const unsigned long long all = ballot(mv != 0);
            if (t == 0) sFlag[0] = int(all == ~0ull) | (int(all == 0ull) << 1);  // bit 0: every key of the tile valid, bit 1: none
        }
    }
    for (int it = 0; it < ntiles; ++it) {
        if (!(ARIA_ATTN_ABL & 64)) sync();  // tile `it` complete in buffer it&1; every wave is done reading the other buffer
        const int cur = it & 1, kv0 = it * 64;
        const bool more = it + 1 < ntiles && !(ARIA_ATTN_ABL & 32);
        if (more) {
            tile2_load<HD, NW>(rk, Kb, ldk, kv0 + 64, S, t);
            tile2_load<HD, NW>(rv, Vb, ldv, kv0 + 64, S, t);
        }
        const bf16_t* cK = sK + cur * 64 * C::KP;
        const bf16_t* cV = sV + cur * 64 * C::VP;
        // (a tile without a single valid key -- the padded bottom rows of an image are one contiguous patch range -- contributes exactly
        // nothing: every probability is exp2(-inf) = 0 and the running maximum does not move)
        if (!(causal && kv0 > p_wmin + 31) && !(kmb && (sFlag[cur] & 2))) {  // wave-uniform: this wave has at least one visible key in the tile
            f32x16 st[2];
            st[0] = zero_acc();
            st[1] = zero_acc();
            if (ARIA_ATTN_ABL & 1) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[i][r] = float((it * 7 + r * 3 + i + l) & 31) * 0.03125f;
            } else {
                // r04: the K fragments of k-step kk + 1 are requested before the two MFMAs of k-step kk are issued -- left to itself the
                // scheduler sank every read to just in front of its MFMA (read, lgkmcnt(0), multiply: ten exposed LDS round trips per tile)
                auto kf = [&](int i, int kk) __attribute__((always_inline)) -> s16x8 {
                    return (ARIA_ATTN_ABL & 16) ? qf[(kk + i) % C::KS]
                                                : *reinterpret_cast<const s16x8*>(cK + (i * 32 + (l & 31)) * C::KP + kk * 16 + h2 * 8);
                };
                s16x8 fr[2][2];
                fr[0][0] = kf(0, 0);
                fr[0][1] = kf(1, 0);
#pragma unroll
                for (int kk = 0; kk < C::KS; ++kk) {
                    if (kk + 1 < C::KS) {
                        fr[(kk + 1) & 1][0] = kf(0, kk + 1);
                        fr[(kk + 1) & 1][1] = kf(1, kk + 1);
                    }
                    sched_fence();
#pragma unroll
                    for (int i = 0; i < 2; ++i) st[i] = mfma32(fr[kk & 1][i], qf[kk], st[i]);
                    sched_fence();
                }
            }
            const bool need_mask = (kv0 + 64 > klen) || (causal && kv0 + 63 > p_wmin) || (kmb && !(sFlag[cur] & 1));
            if (need_mask) {
                const uint8_t* cM = sM + cur * 64;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kvl = i * 32 + acc_row(r, l);
                        const int kv = kv0 + kvl;
                        bool dead = kv >= klen || (causal && kv > p_abs);
                        if (kmb) dead = dead || !cM[kvl];
                        if (dead) st[i][r] = -INFINITY;
                    }
            }
            float mx = st[0][0];
            if (!(ARIA_ATTN_ABL & 128)) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
                mx = fmaxf(mx, shfl_xor(mx, 32));
            } else {
                mx = 8.f;
            }
            const float m_new = fmaxf(m, mx * scale2);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;
            if (ballot(m_new > m) != 0ull) {  // wave-uniform lazy rescale: exact (alpha == 1 whenever it is skipped)
                const float alpha = exp2_fast(m - m_safe);
                if (!C::ROWSUM_IN_MFMA) lsum *= alpha;
#pragma unroll
                for (int i = 0; i < C::DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
                m = m_new;
            }
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2 x = fma2(st[i][r], st[i][r + 1], scale2, -m_safe);
#pragma unroll
                    for (int z = 0; z < 2; ++z) {
                        const float p = (ARIA_ATTN_ABL & 2) ? x[z] : exp2_fast(x[z]);
                        st[i][r + z] = p;
                        if (!C::ROWSUM_IN_MFMA) ps += p;
                    }
                }
            if (!C::ROWSUM_IN_MFMA) lsum += ps;
            // O^T += V^T P^T
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const s16x8 pf = pack_frag(st[i], u);
                    if (ARIA_ATTN_ABL & 4) {
                        abl_keep(pf);
                        continue;
                    }
                    const bf16_t* vrow = cV + (i * 32 + 16 * u + 4 * h2 + ((l & 15) >> 2)) * C::VP + 16 * ((l >> 4) & 1) + 4 * (l & 3);
#pragma unroll
                    for (int dt = 0; dt < C::DT; ++dt) {
                        s16x8 vf;
                        if (ARIA_ATTN_ABL & 8) {
                            vf = qf[dt];
                        } else {
                            const s16x4 a0 = ds_read_tr16(vrow + 32 * dt);
                            const s16x4 a1 = ds_read_tr16(vrow + 8 * C::VP + 32 * dt);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                vf[e] = a0[e];
                                vf[4 + e] = a1[e];
                            }
                        }
                        o[dt] = mfma32(vf, pf, o[dt]);
                    }
                }
        }
        if (more) {  // stage tile it+1 into the other buffer (nobody reads it before the next barrier)
            const int nb = cur ^ 1, kvn = kv0 + 64;
            tile2_store<HD, NW, C::KP>(rk, sK + nb * 64 * C::KP, t);
            tile2_store<HD, NW, C::VP>(rv, sV + nb * 64 * C::VP, t);
            if (kmb && t < 64) {
                const uint8_t mv = (kvn + t < S) ? kmb[kvn + t] : 0;
                sM[nb * 64 + t] = mv;
                const unsigned long long all = ballot(mv != 0);
                if (t == 0) sFlag[nb] = int(all == ~0ull) | (int(all == 0ull) << 1);
            }
        }
    }
    // ROWSUM_IN_MFMA: feature row HD = 32 (DT-1) + 8 sits in accumulator register 4 of the lanes with h2 == 0
    const float ltot = C::ROWSUM_IN_MFMA ? shfl(o[C::DT - 1][4], l & 31) : lsum + shfl_xor(lsum, 32);
    const float inv = ltot > 0.f ? 1.f / ltot : 0.f;
    if (q_abs < Sq) {
        if (h2 == 0 && LSE)
            LSE[((long long)b * H + head) * Sq + q_abs] = (ltot > 0.f) ? (m + log2f(ltot)) * 0.6931471805599453f : -INFINITY;
        bf16_t* orow = O + (tokq0 + q_abs) * ldo + head * HD;
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt)
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
#undef ATTN_FWD2_NAME
#undef ATTN_FWD_QOFF_PARAM
