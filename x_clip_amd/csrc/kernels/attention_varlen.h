// attention_varlen.h -- attention over samples of DIFFERENT lengths laid end to end (the packed text tower: only the kept rows of a padded
// batch exist, functional.py `_Pass.layout`).  Reference arithmetic: Attention.forward x_clip.py:213-245 with a key-padding mask, restricted
// to the rows the mask keeps -- a masked key has probability exactly 0 there and a masked QUERY row is read by nobody under the CLS head.
//
//   qkv  [R, 3, heads, HS]   packed q | k | v rows; sample s owns rows cu[s] .. cu[s+1] (1 <= its length <= max_len), cu int32 [batch + 1]
//   out  [R, heads * HS]
//   lse  [heads, R] fp32     natural log-sum-exp of the scaled scores of a row's own sample (head-major: a (sample, head) unit's values are
//                            one contiguous run, as [batch, heads, n] is in the dense kernels)
//   dqkv [R, 3, heads, HS]   fully overwritten
// Every key of a sample is visible to every query of that sample and to no other: no mask, no causal flag, no dropout.  A work-group (or
// wave) only ever stores rows of the unit it owns, so nothing is written outside [0, R); no atomics, a fixed summation order.
//
// Two forms:
//   * head-resident (bf16, HS = 64, max_len <= A3_MAX_N): attention3.h's kernels with the unit's row range read from cu instead of
//     computed from (sample, n) -- K / V (backward: then Q / dO) of the (sample, head) unit are DMA'd into LDS once and swept with MFMA,
//     built from the same device functions (a3_dma_image, a3_fwd_step, a3_bwd_dq_sweep, a3_bwd_dkv_sweep, the single-tail-row forms).
//     The launch is sized by max_len (waves, LDS); a unit shorter than that leaves its surplus waves at the barriers only.
//   * plain (fp32, HS = 128, max_len > A3_MAX_N): one wave per (row, head), attention_pool.h's wave-wide key loads and online softmax with
//     that row as the query; the backward's wave takes its row first as a query (dQ) and then as a key (dK, dV: the sample's queries
//     stream past it).  O(len) work per row, L2-resident re-reads: a correctness path, not a fast one.
#pragma once
#include "attention3.h"
#include "attention_pool.h"

namespace xc {

struct AttnVarlenParams {
    const void* qkv; const int* cu;
    void* out; float* lse;                       // forward results (backward: inputs)
    const void* dout; void* dqkv;                // backward
    int rows, batch, heads, max_len;
    float scale;
};

// ---- plain form ---------------------------------------------------------------------------------------------------------------------
// the sample that owns row r: the largest s with cu[s] <= r (cu ascending, cu[0] = 0, cu[batch] = rows > r)
XC_DEV int av_sample_of(const int* cu, int batch, int r) {
    int lo = 0, hi = batch;                                    // invariant: cu[lo] <= r < cu[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_varlen_plain_fwd_kernel(AttnVarlenParams p) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    static_assert(CH >= 1 && CH <= 64 && (CH & (CH - 1)) == 0, "chunks per key row must be a power of two");
    const int lane = lane_id();
    const long unit = (long)blockIdx.x * 4 + wave_id();
    if (unit >= (long)p.rows * p.heads) return;                // whole wave leaves; no barriers below
    const int r = (int)(unit / p.heads), h = (int)(unit % p.heads);
    const int s = av_sample_of(p.cu, p.batch, r);
    const int k0 = p.cu[s], k1 = p.cu[s + 1];
    const int inner = p.heads * HS;
    const long ldq = 3L * inner;
    const int g = lane / CH, c = lane % CH;                    // key within the wave-wide load, 16-byte chunk of its row
    const T* base = static_cast<const T*>(p.qkv) + (long)h * HS + c * VEC;
    float qv[VEC];
    load_vec<T>(base + (long)r * ldq, qv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) qv[e] *= p.scale;
    float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int j0 = k0; j0 < k1; j0 += KPL) {
        const int j = j0 + g;
        const bool live = j < k1;
        const int jr = live ? j : k1 - 1;                      // (past the sample's end: a valid address, the value is not used)
        float kf[VEC], vf[VEC];
        load_vec<T>(base + (long)jr * ldq + inner, kf);
        load_vec<T>(base + (long)jr * ldq + 2 * inner, vf);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) part += qv[e] * kf[e];
        const float sc = group_sum<CH>(part);
        if (live) {                                            // (uniform over the CH lanes of a key)
            const float mn = fmaxf(m, sc);
            const float fac = fast_exp(m - mn), pj = fast_exp(sc - mn);
            l = l * fac + pj;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * fac + pj * vf[e];
            m = mn;
        }
    }
    const float mt = cross_max<CH>(m);                         // merge the KPL groups: a group that saw no key has m = -inf, l = 0
    const float w = (m == -INFINITY) ? 0.f : fast_exp(m - mt);
    const float lt = cross_sum<CH>(l * w);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = cross_sum<CH>(acc[e] * w) * inv;
    if (g == 0) store_vec<T>(static_cast<T*>(p.out) + (long)r * inner + (long)h * HS + c * VEC, o);
    if (lane == 0) p.lse[(long)h * p.rows + r] = mt + logf(lt);
}

template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_varlen_plain_bwd_kernel(AttnVarlenParams p) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    const int lane = lane_id();
    const long unit = (long)blockIdx.x * 4 + wave_id();
    if (unit >= (long)p.rows * p.heads) return;
    const int r = (int)(unit / p.heads), h = (int)(unit % p.heads);
    const int s = av_sample_of(p.cu, p.batch, r);
    const int k0 = p.cu[s], k1 = p.cu[s + 1];
    const int inner = p.heads * HS;
    const long ldq = 3L * inner;
    const int g = lane / CH, c = lane % CH;
    const long hoff = (long)h * HS + c * VEC;
    const T* qkv = static_cast<const T*>(p.qkv) + hoff;
    const T* dO = static_cast<const T*>(p.dout) + hoff;
    const T* O = static_cast<const T*>(p.out) + hoff;
    const float* lse = p.lse + (long)h * p.rows;
    T* dqkv = static_cast<T*>(p.dqkv) + (long)r * ldq + hoff;
    // ---- row r as a QUERY: dQ = sum_j dS_j k_j ----
    float qv[VEC], dov[VEC], ov[VEC];
    load_vec<T>(qkv + (long)r * ldq, qv);
    load_vec<T>(dO + (long)r * inner, dov);
    load_vec<T>(O + (long)r * inner, ov);
    float dpart = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dpart += dov[e] * ov[e];
    const float delta = group_sum<CH>(dpart);                  // rowsum(dO o O) = rowsum(P dP)
    const float lse_r = lse[r];
    float dq[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dq[e] = 0.f;
    for (int j0 = k0; j0 < k1; j0 += KPL) {
        const int j = j0 + g;
        const bool live = j < k1;
        const int jr = live ? j : k1 - 1;
        float kf[VEC], vf[VEC];
        load_vec<T>(qkv + (long)jr * ldq + inner, kf);
        load_vec<T>(qkv + (long)jr * ldq + 2 * inner, vf);
        float sp = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sp += qv[e] * kf[e]; dp += dov[e] * vf[e]; }
        const float sc = group_sum<CH>(sp) * p.scale;
        const float dpj = group_sum<CH>(dp);
        const float pj = live ? fast_exp(sc - lse_r) : 0.f;
        const float ds = pj * (dpj - delta) * p.scale;
#pragma unroll
        for (int e = 0; e < VEC; ++e) dq[e] += ds * kf[e];
    }
    float t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = cross_sum<CH>(dq[e]);
    if (g == 0) store_vec<T>(dqkv, t);
    // ---- row r as a KEY: dK = sum_i dS_i q_i, dV = sum_i P_i dO_i over the queries i of its sample ----
    float kv_[VEC], vv[VEC], dk[VEC], dv[VEC];
    load_vec<T>(qkv + (long)r * ldq + inner, kv_);
    load_vec<T>(qkv + (long)r * ldq + 2 * inner, vv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
    for (int i0 = k0; i0 < k1; i0 += KPL) {
        const int i = i0 + g;
        const bool live = i < k1;
        const int ir = live ? i : k1 - 1;
        float qf[VEC], df[VEC], of[VEC];
        load_vec<T>(qkv + (long)ir * ldq, qf);
        load_vec<T>(dO + (long)ir * inner, df);
        load_vec<T>(O + (long)ir * inner, of);
        const float lse_i = lse[ir];
        float sp = 0.f, dp = 0.f, dl = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sp += qf[e] * kv_[e]; dp += df[e] * vv[e]; dl += df[e] * of[e]; }
        const float sc = group_sum<CH>(sp) * p.scale;
        const float dpi = group_sum<CH>(dp), delta_i = group_sum<CH>(dl);
        const float pi = live ? fast_exp(sc - lse_i) : 0.f;
        const float ds = pi * (dpi - delta_i) * p.scale;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { dk[e] += ds * qf[e]; dv[e] += pi * df[e]; }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = cross_sum<CH>(dk[e]);
    if (g == 0) store_vec<T>(dqkv + inner, t);
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = cross_sum<CH>(dv[e]);
    if (g == 0) store_vec<T>(dqkv + 2 * inner, t);
}

// ---- head-resident form: attention3.h's forward on the rows [cu[s], cu[s+1]) of one head --------------------------------------------
// blockDim = 64 a3_waves(max_len): every length up to max_len finds the waves attn3_fwd_kernel would have been launched with (a3_waves is
// monotonic up to its cooperative-tail dip, which max_len's own value covers); wave w >= a3_waves(n) owns no query block of this unit.
__global__ __launch_bounds__(576) XC_FOUR_WAVES_PER_SIMD void attn_varlen_fwd_kernel(AttnVarlenParams p) {
    XC_LDS_DYNAMIC(lds);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c31 = lane & 31;
    const int wave = uniform(tid >> 6), nwaves = blockDim.x >> 6;
    const int bh = xcd_remap(blockIdx.x, p.batch * p.heads);
    const int hh = bh % p.heads, bi = bh / p.heads;
    const int row0 = uniform(p.cu[bi]);
    const int n = uniform(p.cu[bi + 1]) - row0, npad = (n + 31) & ~31;
    if (n < 1 || n > p.max_len) return;                        // (uniform; a layout the launch was not sized for: nothing is read or written)
    unsigned char* Ks = lds;
    unsigned char* Vs = Ks + npad * 128;
    unsigned char* Ms = Vs + npad * 128;                       // [npad] key validity (rows past n)
    float* Ts = reinterpret_cast<float*>(Ms + npad);           // [nwaves][A3_TAIL_MAX][A3_TAIL_REC] tail partials
    const long ldq = 3L * p.heads * ATT_DH;
    const bf16_t* Qb = reinterpret_cast<const bf16_t*>(p.qkv) + (long)row0 * ldq + hh * ATT_DH;
    const bf16_t* Kb = Qb + (long)p.heads * ATT_DH;
    const bf16_t* Vb = Kb + (long)p.heads * ATT_DH;
    bf16_t* out = reinterpret_cast<bf16_t*>(p.out) + (long)row0 * p.heads * ATT_DH + hh * ATT_DH;
    float* lse_out = p.lse + (long)hh * p.rows + row0;
    const bool coop = a3_coop_tail(n);
    const bool own = wave < a3_waves(n);                       // (uniform) this wave has a 32-query block of its own
    const int tail0 = (n >> 5) << 5, ntail = n & 31;
    const int q0 = wave * 32;
    const int qrow = q0 + c31;
    const int qld = qrow < n ? qrow : n - 1;
    u32x4 qf[4];
    const int qfirst = coop ? (tail0 + c31 < n ? tail0 + c31 : n - 1) : qld;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) qf[kb] = ld16(Qb + (long)qfirst * ldq + kb * 16 + h * 8);
    a3_dma_image(Ks, Kb, ldq, n, npad, wave, nwaves, lane);
    a3_dma_image(Vs, Vb, ldq, n, npad, wave, nwaves, lane);
    a3_key_validity(Ms, nullptr, 0, n, npad);
    f32x16 o[2];
    wait_vmem();
    sync();
    const int nsub = npad >> 5;
    const float scale2 = p.scale * 1.4426950408889634f;
    if (coop) {                                                // tail queries x this wave's share of the key sub-tiles
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
        float m = ATT_NEG, l = 0.f;
        int tcoop = nsub;
        if (a3_single_tail(n)) {                               // (uniform) the tail query against the tail key: the last wave's partial starts from it
            tcoop = nsub - 1;
            if (wave == nwaves - 1) {
                m = a3_tail_dot(Ks, tcoop, 0, qf, lane) * scale2;
                l = 1.f;
                a3_tail_outer(Vs, tcoop, 0, 1.f, lane, o);
            }
        }
        for (int t = wave; t < tcoop; t += nwaves) a3_fwd_step_auto<false>(Ks, Vs, Ms, t, qf, scale2, lane, tail0, o, m, l);
        if (c31 < ntail) {
            float* rec = Ts + ((long)wave * A3_TAIL_MAX + c31) * A3_TAIL_REC;
            if (h == 0) { rec[0] = m; rec[1] = l; }
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) rec[2 + db * 32 + mfma_row(r, lane)] = o[db][r];
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) qf[kb] = ld16(Qb + (long)qld * ldq + kb * 16 + h * 8);
    }
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m = ATT_NEG, l = 0.f;
    if (own) {
        int tend = nsub;
        if (a3_single_tail(n)) {                               // (uniform) the tail key first: it initialises (m, l, O) -- see a3_tail_dot
            tend = nsub - 1;
            m = a3_tail_dot(Ks, tend, 0, qf, lane) * scale2;
            l = 1.f;
            a3_tail_outer(Vs, tend, 0, 1.f, lane, o);
        }
        for (int t = 0; t < tend; ++t) a3_fwd_step_auto<false>(Ks, Vs, Ms, t, qf, scale2, lane, q0, o, m, l);
    }
    sync();                                                    // every wave is done with the K / V images (and the tail partials are in)
    if (own) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        a2_store_rows(lds + wave * 32 * 144, o, inv, out, (long)p.heads * ATT_DH, q0, coop ? tail0 : n, lane);
        if (h == 0 && qrow < (coop ? tail0 : n)) lse_out[qrow] = m * 0.6931471805599453f + logf(l);    // m is in log2 units
    }
    if (coop && wave == 0) {                                   // merge the nwaves partials of every tail row; lane = feature d
        // (the staging blocks of a2_store_rows lie in [0, nwaves 32 144) of the LDS, the partials behind both images: no overlap)
        for (int q = 0; q < ntail; ++q) {
            float M = ATT_NEG;
            for (int w = 0; w < nwaves; ++w) M = fmaxf(M, Ts[((long)w * A3_TAIL_MAX + q) * A3_TAIL_REC]);
            float L = 0.f, acc = 0.f;
            for (int w = 0; w < nwaves; ++w) {
                const float* rec = Ts + ((long)w * A3_TAIL_MAX + q) * A3_TAIL_REC;
                const float f = fast_exp2(rec[0] - M);
                L += rec[1] * f;
                acc += rec[2 + lane] * f;
            }
            out[(long)(tail0 + q) * p.heads * ATT_DH + lane] = f2bf(L > 0.f ? acc / L : 0.f);
            if (lane == 0) lse_out[tail0 + q] = M * 0.6931471805599453f + logf(L);
        }
    }
}

// ---- head-resident backward: attention3.h's two-phase kernel on the rows of one unit (its block loops already stride by the wave count) ----
__global__ __launch_bounds__(256) void attn_varlen_bwd_kernel(AttnVarlenParams p) {
    XC_LDS_DYNAMIC(lds);
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c31 = lane & 31;
    const int wave = uniform(tid >> 6), nwaves = blockDim.x >> 6;
    const int bh = xcd_remap(blockIdx.x, p.batch * p.heads);
    const int hh = bh % p.heads, bi = bh / p.heads;
    const int row0 = uniform(p.cu[bi]);
    const int n = uniform(p.cu[bi + 1]) - row0, npad = (n + 31) & ~31;
    if (n < 1 || n > p.max_len) return;                        // (uniform)
    const int img = npad * 128;
    unsigned char* R0 = lds;                                   // K, then Q
    unsigned char* R1 = R0 + img;                              // V, then dO
    unsigned char* Ms = R1 + img;                              // [npad] key validity
    float* Ls = reinterpret_cast<float*>(Ms + npad);           // [npad] lse log2(e) per query
    float* Ds = Ls + npad;                                     // [npad] delta per query
    float* Tp = Ds + npad;                                     // [nwaves][A3_TAIL_MAX][128] tail partials: dQ (phase A), dK | dV (phase B)
    const long ldq = 3L * p.heads * ATT_DH, ldo = (long)p.heads * ATT_DH;
    const bf16_t* Qb = reinterpret_cast<const bf16_t*>(p.qkv) + (long)row0 * ldq + hh * ATT_DH;
    const bf16_t* Kb = Qb + (long)p.heads * ATT_DH;
    const bf16_t* Vb = Kb + (long)p.heads * ATT_DH;
    const bf16_t* dOb = reinterpret_cast<const bf16_t*>(p.dout) + (long)row0 * ldo + hh * ATT_DH;
    const bf16_t* Ob = reinterpret_cast<const bf16_t*>(p.out) + (long)row0 * ldo + hh * ATT_DH;
    const float* lse_in = p.lse + (long)hh * p.rows + row0;
    bf16_t* dQ = reinterpret_cast<bf16_t*>(p.dqkv) + (long)row0 * ldq + hh * ATT_DH;
    bf16_t* dK = dQ + (long)p.heads * ATT_DH;
    bf16_t* dV = dK + (long)p.heads * ATT_DH;
    a3_dma_image(R0, Kb, ldq, n, npad, wave, nwaves, lane);
    a3_dma_image(R1, Vb, ldq, n, npad, wave, nwaves, lane);
    a3_key_validity(Ms, nullptr, 0, n, npad);
    const bool coop = a3_coop_tail(n);
    const int tail0 = (n >> 5) << 5, ntail = n & 31;
    const int nblk = a3_waves(n);                              // 32-row blocks owned by single waves (without a cooperative tail)
    const int nsub = npad >> 5;
    const float scale2 = p.scale * 1.4426950408889634f;
    for (int blk = wave; blk < nsub; blk += nwaves) {          // delta_i = sum_d dO[i, d] O[i, d] and lse_i log2(e)
        const int row_ = blk * 32 + c31;
        const int rl = row_ < n ? row_ : n - 1;
        const float lse_r = lse_in[rl];
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float a[8], b[8];
            load_vec<bf16_t>(Ob + (long)rl * ldo + h * 32 + c * 8, a);
            load_vec<bf16_t>(dOb + (long)rl * ldo + h * 32 + c * 8, b);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += a[k] * b[k];
        }
        acc += shfl_xor(acc, 32);
        if (h == 0) {
            Ds[row_] = row_ < n ? acc : 0.f;
            Ls[row_] = row_ < n ? lse_r * 1.4426950408889634f : 0.f;
        }
    }
    wait_vmem();
    sync();
    uint32_t plain_bits = 0;                                   // bit t: every key of sub-tile t is valid (npad <= 288: 9 sub-tiles)
    for (int t = 0; t < nsub; ++t) plain_bits |= wave_all(Ms[t * 32 + c31] != 0) ? (1u << t) : 0u;

    // ---- phase A: dQ^T[d, query] for the wave's query blocks, streaming the key sub-tiles of the K / V images ----
    u32x4 f0[4], f1[4];                                        // the block's own rows: (Q, dO) in phase A, (K, V) in phase B
    f32x16 g0[2], g1[2];                                       // dQ in phase A; dK, dV in phase B
    if (coop) {                                                // tail queries first: this wave's share of the key sub-tiles
        const int trow = tail0 + c31 < n ? tail0 + c31 : n - 1;
        a3_row_frags(Qb, ldq, trow, lane, f0);
        a3_row_frags(dOb, ldo, trow, lane, f1);
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) g0[db][r] = 0.f;
        const float lq = Ls[tail0 + c31], dl = Ds[tail0 + c31];
        int tcoop = nsub;
        if (a3_single_tail(n)) {                               // (uniform) tail query x tail key: the last wave's partial starts from it
            tcoop = nsub - 1;
            const float st = a3_tail_dot(R0, tcoop, 0, f0, lane), dt_ = a3_tail_dot(R1, tcoop, 0, f1, lane);
            if (wave == nwaves - 1) a3_tail_outer(R0, tcoop, 0, fast_exp2(st * scale2 - lq) * (dt_ - dl), lane, g0);
        }
        a3_bwd_dq_sweep<false>(R0, R1, Ms, wave, tcoop, nwaves, plain_bits, f0, f1, lq, dl, scale2, lane, tail0 + c31, g0);
        if (c31 < ntail) a3_put_col(Tp + ((long)wave * A3_TAIL_MAX + c31) * 128, g0, lane);
    }
    for (int rb = wave; rb < nblk; rb += nwaves) {
        const int row = rb * 32 + c31;
        const int rl = row < n ? row : n - 1;
        a3_row_frags(Qb, ldq, rl, lane, f0);
        a3_row_frags(dOb, ldo, rl, lane, f1);
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) g0[db][r] = 0.f;
        const float lse_q = Ls[row], delta_q = Ds[row];
        int tend = nsub;
        if (a3_single_tail(n)) {                               // (uniform) the tail key: dQ starts at dS k_tail
            tend = nsub - 1;
            const float pt = fast_exp2(a3_tail_dot(R0, tend, 0, f0, lane) * scale2 - lse_q);
            const float ds = pt * (a3_tail_dot(R1, tend, 0, f1, lane) - delta_q);        // dS / scale
            a3_tail_outer(R0, tend, 0, ds, lane, g0);
        }
        a3_bwd_dq_sweep<false>(R0, R1, Ms, 0, tend, 1, plain_bits, f0, f1, lse_q, delta_q, scale2, lane, row, g0);
        a3_store_rows_direct(g0, dQ, ldq, rb * 32, coop ? tail0 : n, lane, p.scale);
    }
    sync();                                                    // every wave is done with the K / V images; the tail partials are complete
    a3_dma_image(R0, Qb, ldq, n, npad, wave, nwaves, lane);
    a3_dma_image(R1, dOb, ldo, n, npad, wave, nwaves, lane);
    if (coop && wave == 0) {                                   // tail dQ = sum of the waves' partials; lane = feature d
        for (int q = 0; q < ntail; ++q) {
            float acc = 0.f;
            for (int w = 0; w < nwaves; ++w) acc += Tp[((long)w * A3_TAIL_MAX + q) * 128 + lane];
            dQ[(long)(tail0 + q) * ldq + lane] = f2bf(acc * p.scale);
        }
    }
    wait_vmem();
    sync();                                                    // Q / dO images in place; Tp may be reused

    // ---- phase B: dK^T, dV^T for the wave's key blocks, streaming the query sub-tiles of the Q / dO images ----
    for (int rb = wave; rb < nblk; rb += nwaves) {
        const int row = rb * 32 + c31;
        const int rl = row < n ? row : n - 1;
        a3_row_frags(Kb, ldq, rl, lane, f0);
        a3_row_frags(Vb, ldq, rl, lane, f1);
        const bool kvalid = Ms[row] != 0;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) { g0[db][r] = 0.f; g1[db][r] = 0.f; }
        const bool keys_plain = wave_all(kvalid);              // (uniform: no padding among this block's keys)
        int qend = nsub;
        if (a3_single_tail(n)) {                               // (uniform) the tail query: dK / dV start at its contribution
            qend = nsub - 1;
            const float st = a3_tail_dot(R0, qend, 0, f0, lane);
            const float pt = kvalid ? fast_exp2(st * scale2 - Ls[tail0]) : 0.f;
            const float ds = pt * (a3_tail_dot(R1, qend, 0, f1, lane) - Ds[tail0]);              // dS / scale
            a3_tail_outer(R0, qend, 0, ds, lane, g0);
            a3_tail_outer(R1, qend, 0, pt, lane, g1);
        }
        a3_bwd_dkv_sweep<false>(R0, R1, Ls, Ds, 0, qend, 1, n, keys_plain, f0, f1, kvalid, scale2, lane, row, g0, g1);
        a3_store_rows_direct(g0, dK, ldq, rb * 32, coop ? tail0 : n, lane, p.scale);
        a3_store_rows_direct(g1, dV, ldq, rb * 32, coop ? tail0 : n, lane);
    }
    if (coop) {                                                // tail keys: this wave's share of the query sub-tiles
        const int trow = tail0 + c31 < n ? tail0 + c31 : n - 1;
        a3_row_frags(Kb, ldq, trow, lane, f0);
        a3_row_frags(Vb, ldq, trow, lane, f1);
        const bool tvalid = Ms[tail0 + c31] != 0;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) { g0[db][r] = 0.f; g1[db][r] = 0.f; }
        int tcoop = nsub;
        if (a3_single_tail(n)) {                               // (uniform) tail key x tail query: the last wave's partial starts from it
            tcoop = nsub - 1;
            const float st = a3_tail_dot(R0, tcoop, 0, f0, lane), dt_ = a3_tail_dot(R1, tcoop, 0, f1, lane);
            if (wave == nwaves - 1) {
                const float pt = tvalid ? fast_exp2(st * scale2 - Ls[tail0]) : 0.f;
                a3_tail_outer(R0, tcoop, 0, pt * (dt_ - Ds[tail0]), lane, g0);
                a3_tail_outer(R1, tcoop, 0, pt, lane, g1);
            }
        }
        a3_bwd_dkv_sweep<false>(R0, R1, Ls, Ds, wave, tcoop, nwaves, n, false, f0, f1, tvalid, scale2, lane, tail0 + c31, g0, g1);
        if (c31 < ntail) {
            float* rec = Tp + ((long)wave * A3_TAIL_MAX + c31) * 128;
            a3_put_col(rec, g0, lane);
            a3_put_col(rec + 64, g1, lane);
        }
        sync();
        if (wave == 0) {
            for (int q = 0; q < ntail; ++q) {
                float ak = 0.f, av = 0.f;
                for (int w = 0; w < nwaves; ++w) {
                    const float* rec = Tp + ((long)w * A3_TAIL_MAX + q) * 128;
                    ak += rec[lane];
                    av += rec[64 + lane];
                }
                dK[(long)(tail0 + q) * ldq + lane] = f2bf(ak * p.scale);
                dV[(long)(tail0 + q) * ldq + lane] = f2bf(av);
            }
        }
    }
}

// launch sizes for a batch whose longest sample has max_len rows: every shorter unit fits the same carve
inline int attn_varlen_fwd_waves(int max_len) { return a3_waves(max_len); }
inline int attn_varlen_bwd_waves(int max_len) { return a3_bwd_waves(max_len); }
inline int attn_varlen_fwd_lds_bytes(int max_len) {
    const int npad = (max_len + 31) & ~31, nw = attn_varlen_fwd_waves(max_len);
    const int a = 2 * npad * 128 + npad + nw * A3_TAIL_MAX * A3_TAIL_REC * 4, b = nw * 32 * 144;
    return (a > b ? a : b) + 64;
}
inline int attn_varlen_bwd_lds_bytes(int max_len) {
    const int npad = (max_len + 31) & ~31;
    return 2 * npad * 128 + npad + 2 * npad * 4 + attn_varlen_bwd_waves(max_len) * A3_TAIL_MAX * 128 * 4 + 64;
}

}  // namespace xc
