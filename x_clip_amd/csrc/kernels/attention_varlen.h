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
// EVERY row [0, R) is written: R may exceed cu[batch] (packing.text_layout(row_multiple=) rounds the row count up so that the GEMMs around
// the attention get an M their fast kernels take), and the FILLER rows [cu[batch], R), which no sample owns, get out = 0, lse = 0, dqkv = 0 in
// the same launch -- by the units of the last sample (head-resident, av_zero_filler) or by the row's own waves (plain, av_plain_filler).
// The *_causal_* kernels are the same over the same arrays with ONE more rule (the autoregressive text encoder, x_clip.py:231-234): key row j
// is visible to query row i of its sample iff j <= i, by PACKED row index -- kept rows keep their order, so that is the dense rule on the
// rows that exist.  A row's lse is then over keys [cu[s], row], and a row sees at least itself.
//
// Two forms:
//   * head-resident (bf16, HS = 64, max_len <= A3_MAX_N): wrappers around attention3.h's bodies a3_fwd_unit / a3_bwd_unit, which the dense
//     kernels run too -- only the unit's row range differs, read from cu here instead of computed from (sample, n).  K / V (backward: then
//     Q / dO) of the (sample, head) unit are DMA'd into LDS once and swept with MFMA.
//     The launch is sized by max_len (waves, LDS); a unit shorter than that leaves its surplus waves at the barriers only.
//   * plain (fp32, HS = 128, max_len > A3_MAX_N): one wave per (row, head), attention_pool.h's key sweep (ap_fwd_unit / ap_bwd_unit)
//     with that row as the query of its sample's keys (the pooled kernels run them too: for a sample's first row the two give
//     the same out, lse and dQ bits, tests/pooled_packed_cases.py case_plain_varlen_equals_pool_varlen_bits).  The forward is a wrapper
//     around ap_fwd_unit; the backward's wave takes its row first as a query (dQ: a copy of ap_bwd_unit's loop, see the kernel) and then as
//     a key (dK, dV: the sample's queries stream past it -- another loop, three loads per row).  O(len) work per row, L2-resident
//     re-reads: a correctness path, not a fast one.  Causal: the forward's visible range ends at the row itself (ApUnit::kvis = r + 1), the
//     backward's query half runs over keys [k0, r] and its key half over queries [r, k1).
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

// A wave whose row lies behind the last sample (r >= cu[batch]: a filler row of a layout whose row count was rounded up) owns no unit: it
// zeroes its head's slot of that row -- out and lse (forward) or the three slots of dqkv (BWD) -- with 16-byte stores and leaves before
// the sample search, whose invariant needs r < cu[batch].  -> true: the row was filler
template <typename T, int HS, bool BWD>
XC_DEV bool av_plain_filler(const AttnVarlenParams& p, int r, int h) {
    if (r < p.cu[p.batch]) return false;
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC;
    const int lane = lane_id(), inner = p.heads * HS;
    if (BWD) {
        T* d = static_cast<T*>(p.dqkv) + (long)r * 3 * inner + (long)h * HS;
        for (int i = lane; i < 3 * CH; i += 64) st16(d + (long)(i / CH) * inner + (i % CH) * VEC, zero16());
    } else {
        if (lane < CH) st16(static_cast<T*>(p.out) + (long)r * inner + (long)h * HS + lane * VEC, zero16());
        if (lane == 0) p.lse[(long)h * p.rows + r] = 0.f;
    }
    return true;
}

// the unit of wave blockIdx.x * 4 + wave_id(): row r of head h as the QUERY of its own sample's keys, all of them visible; false: the wave
// is past the last unit and leaves whole (no barriers anywhere).  attention_pool.h's ApUnit with K / V in the same array as the query
// (CAUSAL: the keys behind the row are hidden, kvis = r + 1)
template <typename T, int HS, bool CAUSAL = false>
XC_DEV bool av_plain_unit(const AttnVarlenParams& p, ApUnit<T>& u) {
    const long unit = (long)blockIdx.x * 4 + wave_id();
    if (unit >= (long)p.rows * p.heads) return false;
    const int r = (int)(unit / p.heads), h = (int)(unit % p.heads);
    if (av_plain_filler<T, HS, false>(p, r, h)) return false;
    const int s = av_sample_of(p.cu, p.batch, r);
    const int inner = p.heads * HS, k0 = p.cu[s], k1 = p.cu[s + 1];
    const long ldq = 3L * inner, at = (long)r * inner + (long)h * HS;
    const T* qkv = static_cast<const T*>(p.qkv) + (long)h * HS;
    T* dqkv = static_cast<T*>(p.dqkv) + (long)h * HS;
    u = {qkv + r * ldq, static_cast<const T*>(p.dout) + at, static_cast<T*>(p.out) + at, p.lse + (long)h * p.rows + r,
         qkv + inner, ldq, inner, nullptr, k0, k1, CAUSAL ? r + 1 : k1, dqkv + r * ldq, dqkv + inner};
    return true;
}

template <typename T, int HS, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attn_varlen_plain_fwd_kernel(AttnVarlenParams p) {
    ApUnit<T> u;
    if (av_plain_unit<T, HS, CAUSAL>(p, u)) ap_fwd_unit<T, HS>(u, p.scale);
}

// The query half below is ap_bwd_unit's loop without the dK / dV stores, kept as its own copy: called through the body, the bf16 HS = 128
// instantiation takes 82 registers instead of 80 and falls from 6 to 5 waves per SIMD (measured 5 % slower; profiles/r19_pool_one_loop_*).
// CAUSAL only moves the two loops' bounds (constants of the instantiation): keys [k0, r] for the row as a query, queries [r, k1) for it as a key.
template <typename T, int HS, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attn_varlen_plain_bwd_kernel(AttnVarlenParams p) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    const int lane = lane_id();
    const long unit = (long)blockIdx.x * 4 + wave_id();
    if (unit >= (long)p.rows * p.heads) return;
    const int r = (int)(unit / p.heads), h = (int)(unit % p.heads);
    if (av_plain_filler<T, HS, true>(p, r, h)) return;
    const int s = av_sample_of(p.cu, p.batch, r);
    const int k0 = p.cu[s], k1 = p.cu[s + 1];
    const int kend = CAUSAL ? r + 1 : k1;                      // the keys row r sees: [k0, kend)
    const int q0 = CAUSAL ? r : k0;                            // the queries that see row r: [q0, k1)
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
    for (int j0 = k0; j0 < kend; j0 += KPL) {
        const int j = j0 + g;
        const bool live = j < kend;
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
    for (int i0 = q0; i0 < k1; i0 += KPL) {
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

// ---- head-resident form: attention3.h's bodies (a3_fwd_unit, a3_bwd_unit) on the rows [cu[s], cu[s+1]) of one head ------------------
// the unit of work-group blockIdx.x; false (uniform) for a layout the launch was not sized for: nothing is read or written then
XC_DEV bool av_unit(const AttnVarlenParams& p, A3Unit& u) {
    const int bh = xcd_remap(blockIdx.x, p.batch * p.heads);
    const int hh = bh % p.heads, bi = bh / p.heads;
    const int row0 = uniform(p.cu[bi]);
    const int n = uniform(p.cu[bi + 1]) - row0;
    if (n < 1 || n > p.max_len) return false;
    u = a3_unit(reinterpret_cast<const bf16_t*>(p.qkv), reinterpret_cast<const bf16_t*>(p.out), reinterpret_cast<const bf16_t*>(p.dout),
                reinterpret_cast<bf16_t*>(p.out), reinterpret_cast<bf16_t*>(p.dqkv), p.lse + (long)hh * p.rows + row0, row0, n, p.heads, hh);
    return true;                                               // (no key mask, abl = the literal 0: a3_unit's defaults)
}
// Filler rows [cu[batch], rows): the units of the LAST sample zero their own head's slots there after the body's stores -- 16-byte stores
// spread over all the work-group's threads (every wave leaves the bodies: the surplus ones wait at their barriers only), the head's lse run with
// one float per thread.  BWD: the three slots of dqkv; otherwise out and lse.  No filler: zero iterations, nothing read but cu[batch].
template <bool BWD>
XC_DEV void av_zero_filler(const AttnVarlenParams& p) {
    const int bh = xcd_remap(blockIdx.x, p.batch * p.heads);
    if (bh / p.heads != p.batch - 1) return;                   // (uniform)
    const int hh = bh % p.heads;
    int r0 = uniform(p.cu[p.batch]);
    r0 = r0 > 0 ? r0 : 0;                                      // a cu that does not describe the array: never a row before the first
    const int nfill = p.rows - r0;
    const long ldo = (long)p.heads * ATT_DH;
    constexpr int CH = ATT_DH / 8, PER_ROW = (BWD ? 3 : 1) * CH;         // 16-byte chunks of a head slot, of a row's slots
    bf16_t* base = reinterpret_cast<bf16_t*>(BWD ? p.dqkv : p.out) + (long)hh * ATT_DH;
    for (long i = threadIdx.x; i < (long)nfill * PER_ROW; i += blockDim.x) {
        const int row = r0 + (int)(i / PER_ROW), rem = (int)(i % PER_ROW);
        st16(base + (long)row * (BWD ? 3 : 1) * ldo + (rem / CH) * ldo + (rem % CH) * 8, zero16());
    }
    if (!BWD)
        for (int i = threadIdx.x; i < nfill; i += blockDim.x) p.lse[(long)hh * p.rows + r0 + i] = 0.f;
}
// blockDim = 64 a3_waves(max_len): every length up to max_len finds the waves attn3_fwd_kernel would have been launched with (a3_waves is
// monotonic up to its cooperative-tail dip, which max_len's own value covers); wave w >= a3_waves(n) owns no query block of this unit
// (a3_fwd_unit's RAGGED).
__global__ __launch_bounds__(576) XC_FOUR_WAVES_PER_SIMD void attn_varlen_fwd_kernel(AttnVarlenParams p) {
    A3Unit u;
    if (av_unit(p, u)) { a3_fwd_unit<false, true>(u, p.scale); av_zero_filler<false>(p); }
}
__global__ __launch_bounds__(256) void attn_varlen_bwd_kernel(AttnVarlenParams p) {
    A3Unit u;
    if (av_unit(p, u)) { a3_bwd_unit<false>(u, p.scale); av_zero_filler<true>(p); }
}
// the causal twins: the same unit, launch sizing and bounds; the bodies' CAUSAL skips the sub-tiles above the diagonal
__global__ __launch_bounds__(576) XC_FOUR_WAVES_PER_SIMD void attn_varlen_causal_fwd_kernel(AttnVarlenParams p) {
    A3Unit u;
    if (av_unit(p, u)) { a3_fwd_unit<true, true, false>(u, p.scale); av_zero_filler<false>(p); }      // (no key mask in a packed unit)
}
__global__ __launch_bounds__(256) void attn_varlen_causal_bwd_kernel(AttnVarlenParams p) {
    A3Unit u;
    if (av_unit(p, u)) { a3_bwd_unit<true>(u, p.scale); av_zero_filler<true>(p); }
}

// launch sizes for a batch whose longest sample has max_len rows: every shorter unit fits the same carve.  The backward always carves the
// tail partials: a unit shorter than max_len may have a cooperative tail where max_len itself has none.
inline int attn_varlen_fwd_waves(int max_len) { return a3_waves(max_len); }
inline int attn_varlen_bwd_waves(int max_len) { return a3_bwd_waves(max_len); }
inline int attn_varlen_fwd_lds_bytes(int max_len) { return attn3_fwd_lds_bytes(max_len); }
inline int attn_varlen_bwd_lds_bytes(int max_len) { return a3_bwd_lds_bytes(max_len, true); }

}  // namespace xc
