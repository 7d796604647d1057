// pack_rows.h -- the step between the packed text tower and a head that indexes by (sample, position): the rows of a packed [rows, D] array
// (x_clip_amd/packing.py: only the rows the key-padding mask keeps, laid end to end, sample s in rows cu[s] .. cu[s+1], row r at position
// pos[r] of its padded sample) put back where a dense [batch, n_out, D] array has them, and the transpose.  Reference: the row selection
// `enc_text[:, 1:]` of x_clip.py:704 (pos0 = 1 drops the CLS row) restricted to the rows that exist; a dropped position reads as +0.
//   unpack  dense[s, p - pos0, :] = packed[r, :]   for the row r of sample s with pos[r] == p, pos0 <= p < pos0 + n_out;  +0 elsewhere
//   pack    packed[r, :] = dense[s(r), pos[r] - pos0, :]   for r < cu[batch] with pos0 <= pos[r] < pos0 + n_out;           +0 elsewhere
//           (the CLS rows when pos0 = 1, and the filler rows [cu[batch], rows) of a layout whose row count was rounded up)
// The two are adjoints (a 0/1 selection and its transpose): each is the other's backward.
// One wave per OUTPUT row: every output row is written exactly once, whole, by the wave that owns it, in the same launch -- no fill kernel in
// front, no atomics, nothing outside the array.  All control flow is wave-uniform (the row, its sample and its source are the same for the 64
// lanes); the lanes differ only in the 16-byte chunk they move, so a row leaves as consecutive 16-byte stores.
//   unpack works by DENSE row and finds its source by a binary search of pos[cu[s] .. cu[s+1]) (strictly ascending inside a sample):
//     at most ceil(log2(n + 1)) L2-resident 4-byte reads in front of a row of D elements;
//   pack works by PACKED row and finds its sample with av_sample_of (attention_varlen.h): ceil(log2(batch)) reads of cu.
#pragma once
#include "attention_varlen.h"

namespace xc {

// the packed row of sample rows [k0, k1) at position p, or -1: pos is strictly ascending there.  Wave-uniform in, wave-uniform out
XC_DEV int pr_find_pos(const int* __restrict__ pos, int k0, int k1, int p) {
    int lo = k0, hi = k1;                                      // invariant: pos[k0 .. lo) < p <= pos[hi .. k1)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (uniform(pos[mid]) < p) lo = mid + 1; else hi = mid;
    }
    return (lo < k1 && uniform(pos[lo]) == p) ? lo : -1;
}

template <typename T>
XC_DEV void pr_move_row(T* __restrict__ dst, const T* __restrict__ src, int nch) {      // src == nullptr: the row is +0
    constexpr int VEC = Elem<T>::VEC;
    const int lane = lane_id();
    if (src != nullptr) {
        for (int c = lane; c < nch; c += 64) st16(dst + c * VEC, ld16(src + c * VEC));
    } else {
        for (int c = lane; c < nch; c += 64) st16(dst + c * VEC, zero16());
    }
}

// grid: ceil(batch n_out / 4) work-groups of 4 waves, wave w of work-group g owns dense row 4 g + w
template <typename T>
__global__ __launch_bounds__(256) void unpack_rows_kernel(const T* __restrict__ packed, const int* __restrict__ cu, const int* __restrict__ pos,
                                                          T* __restrict__ dense, int rows, int batch, int n_out, int pos0, int D) {
    const long d = (long)blockIdx.x * 4 + wave_id();
    if (d >= (long)batch * n_out) return;
    const int s = (int)(d / n_out), p = pos0 + (int)(d % n_out);
    int k0 = uniform(cu[s]), k1 = uniform(cu[s + 1]);
    if (k0 < 0 || k1 > rows || k0 > k1) k0 = k1 = 0;           // a malformed layout reads nothing outside pos / packed: the row is +0
    const int r = pr_find_pos(pos, k0, k1, p);
    pr_move_row<T>(dense + d * D, r < 0 ? nullptr : packed + (long)r * D, D / Elem<T>::VEC);
}

// grid: ceil(rows / 4) work-groups of 4 waves, wave w of work-group g owns packed row 4 g + w
template <typename T>
__global__ __launch_bounds__(256) void pack_rows_kernel(const T* __restrict__ dense, const int* __restrict__ cu, const int* __restrict__ pos,
                                                        T* __restrict__ packed, int rows, int batch, int n_out, int pos0, int D) {
    const long r = (long)blockIdx.x * 4 + wave_id();
    if (r >= rows) return;
    const T* src = nullptr;
    if (batch > 0 && r < uniform(cu[batch])) {                 // (behind the last sample: a filler row, no owner)
        const int s = av_sample_of(cu, batch, (int)r);
        const int j = uniform(pos[r]) - pos0;
        if (j >= 0 && j < n_out) src = dense + ((long)s * n_out + j) * D;
    }
    pr_move_row<T>(packed + r * D, src, D / Elem<T>::VEC);
}

}  // namespace xc
