// attention_pool_varlen.h -- attention_pool.h's one query row per (sample, head) over samples of DIFFERENT lengths laid end to end: the last
// layer of the packed text tower under the CLS head (functional.py `_layer_forward_pooled_packed`).  Reference arithmetic: Attention.forward
// x_clip.py:213-245 restricted to the CLS query, under the key-padding mask of x_clip.py:334, on the rows that mask keeps -- a masked key has
// probability exactly 0 in the dense form, so dropping it changes nothing.
//
//   q    [batch, heads * HS]        the samples' first rows' queries (to_qkv's first third applied to those rows only)
//   kv   [rows, 2 * heads * HS]     keys | values of EVERY kept row; sample s owns rows cu[s] .. cu[s+1], cu int32 [batch + 1]
//   out  [batch, heads * HS], lse [batch, heads] (natural log, of the scaled scores: attention_pool.h's convention)
//   backward: dq [batch, heads * HS], dkv [rows, 2 * heads * HS]: a key's dK = dS q, dV = P dO, written by the unit that owns the row
//
// The form of attention_pool.h: HBM-bound, one wave per (sample, head), four waves to a work-group (the heads of one sample side by side read
// neighbouring 128-byte pieces of the same kv rows), wave-wide loads of KPL = 64 / CH whole key rows, an online softmax per lane group, one
// merge at the end.  No MFMA, no LDS, no atomics, a fixed summation order.  Every key of a sample is visible: no mask, no causal flag, no
// dropout.  The last wave-wide load of a sample may reach past its end: those lanes re-read the sample's last row (never a neighbour's, never
// row `rows`) and store nothing.  A unit of length 0 writes out = 0, lse = 0, dq = 0 and no dkv row (the dense kernels' "no visible key").
#pragma once
#include "attention_pool.h"

namespace xc {

struct AttnPoolVarlenParams {
    const void* q; const void* kv; const int* cu;
    void* out; float* lse;                       // forward results (backward: inputs)
    const void* dout; void* dq; void* dkv;       // backward
    int batch, heads, rows;
    float scale;
};

// the row range of sample b, cut to [0, rows]: a cu that does not describe the array can make a unit short, never reach outside it
XC_DEV void apv_range(const AttnPoolVarlenParams& p, int b, int& k0, int& k1) {
    k1 = p.cu[b + 1];
    k1 = k1 < p.rows ? k1 : p.rows;
    k0 = p.cu[b];
    k0 = k0 > 0 ? k0 : 0;
    k1 = k1 > k0 ? k1 : k0;
}

template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_varlen_fwd_kernel(AttnPoolVarlenParams p) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    static_assert(CH >= 1 && CH <= 64 && (CH & (CH - 1)) == 0, "chunks per key row must be a power of two");
    const int lane = lane_id();
    const long bh = (long)blockIdx.x * 4 + wave_id();
    if (bh >= (long)p.batch * p.heads) return;                 // whole wave leaves; no barriers below
    const int b = (int)(bh / p.heads), h = (int)(bh % p.heads);
    int k0, k1;
    apv_range(p, b, k0, k1);
    const int inner = p.heads * HS;
    const int g = lane / CH, c = lane % CH;                    // key within the wave-wide load, 16-byte chunk of its row
    const long hoff = (long)h * HS + c * VEC;
    const T* kv = static_cast<const T*>(p.kv) + hoff;
    float qv[VEC];
    load_vec<T>(static_cast<const T*>(p.q) + (long)b * inner + hoff, qv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) qv[e] *= p.scale;
    float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int j0 = k0; j0 < k1; j0 += KPL) {
        const int j = j0 + g;
        const bool live = j < k1;
        const int jr = live ? j : k1 - 1;                      // (past the sample's end: its own last row, the value is not used)
        float kf[VEC], vf[VEC];
        load_vec<T>(kv + (long)jr * 2 * inner, kf);
        load_vec<T>(kv + (long)jr * 2 * inner + inner, vf);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) part += qv[e] * kf[e];
        const float s = group_sum<CH>(part);
        if (live) {                                            // (uniform over the CH lanes of a key)
            const float mn = fmaxf(m, s);
            const float fac = fast_exp(m - mn), pj = fast_exp(s - mn);      // m = -inf at a group's first key: fac = 0
            l = l * fac + pj;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = acc[e] * fac + pj * vf[e];
            m = mn;
        }
    }
    // merge the KPL groups: a group that saw no key has m = -inf, l = 0
    const float mt = cross_max<CH>(m);
    const float w = (m == -INFINITY) ? 0.f : fast_exp(m - mt);
    const float lt = cross_sum<CH>(l * w);
    const float inv = lt > 0.f ? 1.f / lt : 0.f;               // a unit of length 0: output 0
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = cross_sum<CH>(acc[e] * w) * inv;
    if (g == 0) store_vec<T>(static_cast<T*>(p.out) + (long)b * inner + hoff, o);
    if (lane == 0) p.lse[bh] = lt > 0.f ? mt + logf(lt) : 0.f;
}

template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_varlen_bwd_kernel(AttnPoolVarlenParams p) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    const int lane = lane_id();
    const long bh = (long)blockIdx.x * 4 + wave_id();
    if (bh >= (long)p.batch * p.heads) return;
    const int b = (int)(bh / p.heads), h = (int)(bh % p.heads);
    int k0, k1;
    apv_range(p, b, k0, k1);
    const int inner = p.heads * HS;
    const int g = lane / CH, c = lane % CH;
    const long hoff = (long)h * HS + c * VEC;
    const T* kv = static_cast<const T*>(p.kv) + hoff;
    T* dkv = static_cast<T*>(p.dkv) + hoff;
    float qv[VEC], dov[VEC], ov[VEC];
    load_vec<T>(static_cast<const T*>(p.q) + (long)b * inner + hoff, qv);
    load_vec<T>(static_cast<const T*>(p.dout) + (long)b * inner + hoff, dov);
    load_vec<T>(static_cast<const T*>(p.out) + (long)b * inner + hoff, ov);
    float dpart = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dpart += dov[e] * ov[e];
    const float delta = group_sum<CH>(dpart);                  // rowsum(dO o) = rowsum(P dP)
    const float lse = p.lse[bh];
    float dq[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dq[e] = 0.f;
    for (int j0 = k0; j0 < k1; j0 += KPL) {                    // every row of the unit is written once, by its own lane group
        const int j = j0 + g;
        const bool live = j < k1;
        const int jr = live ? j : k1 - 1;
        float kf[VEC], vf[VEC];
        load_vec<T>(kv + (long)jr * 2 * inner, kf);
        load_vec<T>(kv + (long)jr * 2 * inner + inner, vf);
        float sp = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sp += qv[e] * kf[e]; dp += dov[e] * vf[e]; }
        const float s = group_sum<CH>(sp) * p.scale;
        const float dpj = group_sum<CH>(dp);
        const float pj = live ? fast_exp(s - lse) : 0.f;
        const float ds = pj * (dpj - delta) * p.scale;         // d loss / d (q . k_j)
        float dk[VEC], dv[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            dq[e] += ds * kf[e];
            dk[e] = ds * qv[e];
            dv[e] = pj * dov[e];
        }
        if (live) {
            store_vec<T>(dkv + (long)j * 2 * inner, dk);
            store_vec<T>(dkv + (long)j * 2 * inner + inner, dv);
        }
    }
    float dqt[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dqt[e] = cross_sum<CH>(dq[e]);
    if (g == 0) store_vec<T>(static_cast<T*>(p.dq) + (long)b * inner + hoff, dqt);
}

}  // namespace xc
