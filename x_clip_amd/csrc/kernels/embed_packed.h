// embed_packed.h -- the text embedding for a PACKED batch: only the rows the key-padding mask keeps exist (x_clip_amd/packing.py), laid end
// to end, sample s in rows cu[s] .. cu[s+1].  Reference: TextTransformer.forward x_clip.py:320-331 restricted to those rows.
//   forward   out[r] = cls                                  where has_cls and pos[r] == 0 (the CLS row: always kept, first of its sample)
//             out[r] = E[tok[r]] + P[pos[r] - has_cls]      elsewhere (P == nullptr: no abs-pos table)
//   backward  dcls = column sum of dout over the CLS rows cu[0 .. batch) -- fp32, one atomic per column per wave, as text_embed_bwd_kernel.
//             dE and dP are segmented sums over the packed ids / positions: xclip_sort_ids + xclip_scatter_add_sorted (sort.h, rows.h), the
//             vision tower's gathered-position precedent; no [batch, n + 1, D] array exists on either side.
// An id outside [0, vocab) reads nothing out of bounds: its row is NaN and *bad_flag is set (tokens.h text_embed_fwd_kernel).
#pragma once
#include "common.h"

namespace xc {

template <typename T>
__global__ __launch_bounds__(256) void text_embed_packed_fwd_kernel(const long long* __restrict__ tok, const int* __restrict__ pos,
                                                                    const T* __restrict__ E, const T* __restrict__ P, const T* __restrict__ cls,
                                                                    T* __restrict__ out, long rows, int D, long long vocab, int npos,
                                                                    int* __restrict__ bad_flag) {
    constexpr int VEC = Elem<T>::VEC;
    const int lane = lane_id();
    const long row = (long)blockIdx.x * 4 + wave_id();
    if (row >= rows) return;
    const int has_cls = cls != nullptr ? 1 : 0;
    const int j = pos[row] - has_cls;                          // token position; -1 on the CLS row
    const int nch = D / VEC;
    long long id = (j < 0) ? 0 : tok[row];
    // (wave-uniform; a position past the table is a malformed layout -- where there is a table: without one npos is 0 and no position is read)
    const bool bad = id < 0 || id >= vocab || (P != nullptr && j >= npos);
    if (bad) {
        id = 0;
        if (lane == 0 && bad_flag != nullptr) *bad_flag = 1;
    }
    const T* src = (j < 0) ? cls : E + (long)id * D;
    for (int c = lane; c < nch; c += 64) {
        float v[VEC];
        load_vec<T>(src + c * VEC, v);
        if (bad) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = __builtin_nanf("");
        } else if (j >= 0 && P != nullptr) {
            float pv[VEC];
            load_vec<T>(P + (long)j * D + c * VEC, pv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] += pv[k];
        }
        store_vec<T>(out + row * (long)D + c * VEC, v);
    }
}

// dcls[d] += sum_s dout[cu[s], d]; grid = sample splits, 4 waves each striding over the samples
template <typename T, int MAXC>
__global__ __launch_bounds__(256) void text_embed_packed_dcls_kernel(const T* __restrict__ dout, const int* __restrict__ cu, float* __restrict__ dcls,
                                                                     int batch, int D) {
    constexpr int VEC = Elem<T>::VEC;
    const int lane = lane_id();
    const int nch = D / VEC;
    float acc[MAXC][VEC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[i][k] = 0.f;
    for (int s = blockIdx.x * 4 + wave_id(); s < batch; s += gridDim.x * 4) {
        const T* src = dout + (long)cu[s] * D;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                float v[VEC];
                load_vec<T>(src + c * VEC, v);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[i][k] += v[k];
            }
        }
    }
    // the four waves' sums meet in LDS in a fixed order; one atomic per column per work-group (a single work-group up to 32 samples: reproducible)
    XC_LDS_DYNAMIC(lds);
    float* red = reinterpret_cast<float*>(lds);                // [3][D]
    const int wave = wave_id();
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < nch)
#pragma unroll
                for (int k = 0; k < VEC; ++k) red[(wave - 1) * D + c * VEC + k] = acc[i][k];
        }
    }
    sync();
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = lane + 64 * i;
            if (c < nch)
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    atomic_add(dcls + c * VEC + k, acc[i][k] + red[c * VEC + k] + red[D + c * VEC + k] + red[2 * D + c * VEC + k]);
        }
    }
}

}  // namespace xc
