// attention_pool.h -- attention for ONE query row against the keys of its sample, one wave per (query, head) unit: the last layer of a tower
// whose caller reads a single token row (the CLS head, x_clip.py:708 `enc_text[:, 0]`; functional.py stack_forward `pool_row`).  Reference
// arithmetic: Attention.forward x_clip.py:213-245 restricted to that query -- sim = scale q k^T over every key of the sample, key mask,
// softmax, out = attn v.
//
// HBM-bound by construction (every key / value row is read once, every dK / dV row written once; 4 n HS flops per head): four waves to a
// work-group (the heads of one sample side by side read neighbouring 128-byte pieces of the same rows), no MFMA, no LDS, no atomics, a fixed
// summation order.  A wave-wide load fetches KPL = 64 / CH whole key rows (CH = 16-byte chunks per row: 8 for 64 bf16 features); the CH
// lanes of a key reduce its dot product with CH-lane butterflies, and every lane group runs its OWN online softmax over the keys it sees (no
// cross-group traffic inside the loop); the KPL partial results are merged once at the end.
//
// The key sweep exists ONCE, as ap_fwd_unit / ap_bwd_unit over an ApUnit that says where the unit's rows live; the kernels only fill it:
//   * dense (attn_pool_*):           q [batch, heads * HS], kv [batch, n, 2 * heads * HS] keys | values of EVERY row; a unit owns the n rows of
//                                    its sample and sees [0, nvis) of them (n, or row + 1 under a causal mask) where the key mask keeps them;
//                                    dkv [batch, n, 2 * heads * HS] fully written (hidden keys: zeros)
//   * packed (attn_pool_varlen_*):   samples of DIFFERENT lengths laid end to end (functional.py `_layer_forward_pooled_packed`): kv
//                                    [rows, 2 * heads * HS], sample s owns rows cu[s] .. cu[s+1] (cu int32 [batch + 1]) and sees all of them --
//                                    a masked key has probability exactly 0 in the dense form, so dropping it changes nothing; dkv
//                                    [rows, 2 * heads * HS], a row written by the unit that owns it; a unit of length 0 writes out = 0, lse = 0,
//                                    dq = 0 and no dkv row; rows [cu[batch], rows), which no sample owns (filler), get zeros from the last
//                                    sample's units, so every row of dkv is written
//   * plain varlen (attention_varlen.h attn_varlen_plain_fwd_kernel): every row of a packed qkv as the query of its own sample
//   out [batch, heads * HS], lse [batch, heads] (natural log, of the scaled scores); backward: dq [batch, heads * HS], a key's dK = dS q,
//   dV = P dO (one query's outer products)
#pragma once
#include "common.h"

namespace xc {

struct AttnPoolParams {
    const void* q; const void* kv; const unsigned char* mask;
    void* out; float* lse;                       // forward results (backward: inputs)
    const void* dout; void* dq; void* dkv;       // backward
    int batch, n, heads;
    int nvis;                                    // keys [0, nvis) are visible to the pooled query (n, or row + 1 under a causal mask)
    float scale;
};

struct AttnPoolVarlenParams {
    const void* q; const void* kv; const int* cu;
    void* out; float* lse;                       // forward results (backward: inputs)
    const void* dout; void* dq; void* dkv;       // backward
    int batch, heads, rows;
    float scale;
};

// sum over the CH lanes of a key group (CH a power of two <= 64; groups are aligned lane ranges)
template <int CH>
XC_DEV float group_sum(float v) {
#pragma unroll
    for (int m = 1; m < CH; m <<= 1) v += shfl_xor(v, m);
    return v;
}
// sum / max over the KPL groups (lanes with equal chunk index)
template <int CH>
XC_DEV float cross_sum(float v) {
#pragma unroll
    for (int m = CH; m < 64; m <<= 1) v += shfl_xor(v, m);
    return v;
}
template <int CH>
XC_DEV float cross_max(float v) {
#pragma unroll
    for (int m = CH; m < 64; m <<= 1) v = fmaxf(v, shfl_xor(v, m));
    return v;
}

// One wave's unit: a query and the key rows of its sample.  Every pointer is at the unit's head (its HS columns); the lane's 16-byte chunk is
// added by the bodies.
template <typename T>
struct ApUnit {
    const T* q; const T* dout;                   // the query row; the gradient of its output row (backward; the forward reads none of dout, dq, dk, dv)
    T* out; float* lse;                          // its output row and log-sum-exp (forward: written; backward: read)
    const T* k; long ld; int v_at;               // key row j is at k + j ld, its value row v_at elements behind it
    const unsigned char* mask;                   // nullptr, or byte j != 0 keeps key j
    int k0, k1, kvis;                            // the unit owns rows [k0, k1) and sees [k0, kvis), kvis <= k1
    T* dq; T* dk;                                // backward: the query's gradient; row j's dK at dk + j ld, its dV v_at behind it
};

// Why one sweep serves every kernel bit for bit (the arithmetic below is what each of them had; only these four points differed):
//   * clamp: a lane group whose row j is past k1 re-reads row k1 - 1 -- the unit's own last row, never a neighbour's or one past the array --
//     and its value is discarded (not live, not stored).  The dense kernels clamped to n - 1, which IS k1 - 1 with k1 = n.
//   * range: the forward sweeps the visible rows [k0, kvis), the backward all owned rows [k0, k1) with p = 0 for a row that is not live, so
//     that every owned row's dK / dV is written (zeros where hidden).  Dense: k0 = 0, k1 = n, kvis = nvis; packed: kvis = k1.
//   * mask: its byte is read only for j < kvis <= k1, i.e. at an owned row; a lane past the end never indexes it.
//   * lse: `lt > 0 ? mt + logf(lt) : 0` -- a unit with no live key stores out = 0, lse = 0.  The plain varlen forward had no guard: its units
//     hold at least one key by the entry point's contract, so lt >= 1 there and the guard selects the same value.
template <typename T, int HS>
XC_DEV void ap_fwd_unit(const ApUnit<T>& u, float scale) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    static_assert(CH >= 1 && CH <= 64 && (CH & (CH - 1)) == 0, "chunks per key row must be a power of two");
    const int lane = lane_id();
    const int g = lane / CH, c = lane % CH;                    // key within the wave-wide load, 16-byte chunk of its row
    float qv[VEC];
    load_vec<T>(u.q + c * VEC, qv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) qv[e] *= scale;
    float m = -INFINITY, l = 0.f, acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int j0 = u.k0; j0 < u.kvis; j0 += KPL) {
        const int j = j0 + g;
        const bool live = j < u.kvis && (u.mask == nullptr || u.mask[j] != 0);
        const int jr = j < u.k1 ? j : u.k1 - 1;
        float kf[VEC], vf[VEC];
        const T* kr = u.k + jr * u.ld + c * VEC;
        load_vec<T>(kr, kf);
        load_vec<T>(kr + u.v_at, vf);
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
    const float inv = lt > 0.f ? 1.f / lt : 0.f;               // no live key at all: output 0 (as the dense kernels of attention.h)
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = cross_sum<CH>(acc[e] * w) * inv;
    if (g == 0) store_vec<T>(u.out + c * VEC, o);
    if (lane == 0) *u.lse = lt > 0.f ? mt + logf(lt) : 0.f;
}

template <typename T, int HS>
XC_DEV void ap_bwd_unit(const ApUnit<T>& u, float scale) {
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC, KPL = 64 / CH;
    const int lane = lane_id();
    const int g = lane / CH, c = lane % CH;
    float qv[VEC], dov[VEC], ov[VEC];
    load_vec<T>(u.q + c * VEC, qv);
    load_vec<T>(u.dout + c * VEC, dov);
    load_vec<T>(u.out + c * VEC, ov);
    float dpart = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dpart += dov[e] * ov[e];
    const float delta = group_sum<CH>(dpart);                  // rowsum(dO o) = rowsum(P dP)
    const float lse = *u.lse;
    float dq[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dq[e] = 0.f;
    for (int j0 = u.k0; j0 < u.k1; j0 += KPL) {                // every owned row is written once, by its own lane group
        const int j = j0 + g;
        const bool inb = j < u.k1;
        const bool live = j < u.kvis && (u.mask == nullptr || u.mask[j] != 0);
        const int jr = inb ? j : u.k1 - 1;
        float kf[VEC], vf[VEC];
        const T* kr = u.k + jr * u.ld + c * VEC;
        load_vec<T>(kr, kf);
        load_vec<T>(kr + u.v_at, vf);
        float sp = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sp += qv[e] * kf[e]; dp += dov[e] * vf[e]; }
        const float s = group_sum<CH>(sp) * scale;
        const float dpj = group_sum<CH>(dp);
        const float pj = live ? fast_exp(s - lse) : 0.f;
        const float ds = pj * (dpj - delta) * scale;           // d loss / d (q . k_j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) dq[e] += ds * kf[e];
        if (inb) {
            float dk[VEC], dv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { dk[e] = ds * qv[e]; dv[e] = pj * dov[e]; }
            T* dkr = u.dk + j * u.ld + c * VEC;
            store_vec<T>(dkr, dk);
            store_vec<T>(dkr + u.v_at, dv);
        }
    }
    float dqt[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) dqt[e] = cross_sum<CH>(dq[e]);
    if (g == 0) store_vec<T>(u.dq + c * VEC, dqt);
}

// ---- the wrappers: wave blockIdx.x * 4 + wave_id() is unit (b, h); a wave past the last unit leaves whole (no barriers anywhere) ----
// the fields the dense and the packed layouts share: q / out / dout / dq rows of sample b, lse [batch, heads], keys | values side by side
template <typename T, typename P>
XC_DEV ApUnit<T> ap_unit(const P& p, int b, int h, int HS, const unsigned char* mask, long row0, int k0, int k1, int kvis) {
    const int inner = p.heads * HS;
    const long at = (long)b * inner + (long)h * HS;
    const T* kv = static_cast<const T*>(p.kv) + row0 * 2 * inner + (long)h * HS;
    T* dkv = static_cast<T*>(p.dkv) + row0 * 2 * inner + (long)h * HS;
    return {static_cast<const T*>(p.q) + at, static_cast<const T*>(p.dout) + at, static_cast<T*>(p.out) + at, p.lse + (long)b * p.heads + h,
            kv, 2L * inner, inner, mask, k0, k1, kvis, static_cast<T*>(p.dq) + at, dkv};
}
template <typename T, int HS>
XC_DEV bool attn_pool_unit(const AttnPoolParams& p, ApUnit<T>& u) {
    const long bh = (long)blockIdx.x * 4 + wave_id();
    if (bh >= (long)p.batch * p.heads) return false;
    const int b = (int)(bh / p.heads);
    u = ap_unit<T>(p, b, (int)(bh % p.heads), HS, p.mask ? p.mask + (long)b * p.n : nullptr, (long)b * p.n, 0, p.n, p.nvis);
    return true;
}
template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_fwd_kernel(AttnPoolParams p) {
    ApUnit<T> u;
    if (attn_pool_unit<T, HS>(p, u)) ap_fwd_unit<T, HS>(u, p.scale);
}
template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_bwd_kernel(AttnPoolParams p) {
    ApUnit<T> u;
    if (attn_pool_unit<T, HS>(p, u)) ap_bwd_unit<T, HS>(u, p.scale);
}

// the row range of sample b, cut to [0, rows]: a cu that does not describe the array can make a unit short, never reach outside it
XC_DEV void apv_range(const AttnPoolVarlenParams& p, int b, int& k0, int& k1) {
    k1 = p.cu[b + 1];
    k1 = k1 < p.rows ? k1 : p.rows;
    k0 = p.cu[b];
    k0 = k0 > 0 ? k0 : 0;
    k1 = k1 > k0 ? k1 : k0;
}
template <typename T, int HS>
XC_DEV bool attn_pool_varlen_unit(const AttnPoolVarlenParams& p, ApUnit<T>& u) {
    const long bh = (long)blockIdx.x * 4 + wave_id();
    if (bh >= (long)p.batch * p.heads) return false;
    const int b = (int)(bh / p.heads);
    int k0, k1;
    apv_range(p, b, k0, k1);
    u = ap_unit<T>(p, b, (int)(bh % p.heads), HS, nullptr, 0, k0, k1, k1);
    return true;
}
template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_varlen_fwd_kernel(AttnPoolVarlenParams p) {
    ApUnit<T> u;
    if (attn_pool_varlen_unit<T, HS>(p, u)) ap_fwd_unit<T, HS>(u, p.scale);
}
// Filler rows [cu[batch], rows) of dkv (a layout whose row count was rounded up, packing.text_layout(row_multiple=)) belong to no unit: the
// wave of the LAST sample's head h zeroes that head's key and value slots there, behind its own stores, so that every row of dkv is written
template <typename T, int HS>
XC_DEV void apv_zero_filler(const AttnPoolVarlenParams& p) {
    const long bh = (long)blockIdx.x * 4 + wave_id();
    if ((int)(bh / p.heads) != p.batch - 1) return;
    constexpr int VEC = Elem<T>::VEC, CH = HS / VEC;
    const int h = (int)(bh % p.heads), inner = p.heads * HS;
    int r0 = p.cu[p.batch];
    r0 = r0 > 0 ? r0 : 0;
    T* d = static_cast<T*>(p.dkv) + (long)h * HS;
    for (long i = lane_id(); i < (long)(p.rows - r0) * 2 * CH; i += 64) {
        const int rem = (int)(i % (2 * CH));
        st16(d + (r0 + i / (2 * CH)) * 2 * inner + (long)(rem / CH) * inner + (rem % CH) * VEC, zero16());
    }
}
template <typename T, int HS>
__global__ __launch_bounds__(256) void attn_pool_varlen_bwd_kernel(AttnPoolVarlenParams p) {
    ApUnit<T> u;
    if (attn_pool_varlen_unit<T, HS>(p, u)) { ap_bwd_unit<T, HS>(u, p.scale); apv_zero_filler<T, HS>(p); }
}

}  // namespace xc
