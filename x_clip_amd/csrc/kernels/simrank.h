// simrank.h -- in-batch retrieval metrics of the contrastive head (reference x_clip.py:813-847: the same S = scale * Q K^T the loss
// reduces) WITHOUT the logits: per row the number of negatives that beat a threshold (the row's positive: its rank), the hardest
// negative and its column.  A third epilogue on the similarity tile loop beside Sim5LseEpilogue / Sim5FastGradEpilogue: where the
// forward spends an fma + v_exp + add per logit, this one spends a compare-and-count and a running max.
//   partial : per row and 64-column slot   cnt  = #{j != i + diag_off, j < nk : s_ij > thr[i]}          (strict)
//                                          hmax = max of s_ij over the same columns (SIM_NEG if there are none)
//                                          harg = col0 + j of that max, the lowest column among equal maxima
//             s_ij = acc * sim_scale(p), formed exactly as the forward forms `pos`: a threshold taken from the forward is bit-consistent
//   pos     : thr[i] = dot(q_i, k_{i + diag_off}) * sim_scale for the rows whose positive lies in this chunk
//   combine : folds a row's slots: rank = sum cnt, hard_val = max hmax, hard_idx = its column (lowest among equal maxima, whatever the
//             order the chunks were consumed in).  Integer sums and a max with a total tie rule: the result does not depend on any order.
// No atomics, no LDS beyond the tile loop's own.
#pragma once
#include "simloss5.h"

namespace xc {

struct SimRankParams {
    SimParams s;                           // Q, K, nq, nk, d, scale, log_scale, diag_off, tiles_m, tiles_n (the forward's fields)
    const float* thr;                      // [nq]
    uint32_t* cnt; float* hmax; int* harg; // [slots][nq] each, already offset to this chunk's first slot
    int col0;                              // the chunk's first global column
};

constexpr int SIMRANK_NONE = 0x7fffffff;   // harg of a slot (and the fold's start) that holds no negative

// the ring-loop form: a lane owns ONE logit row of a 32-row group and 32 of the wave's 64 columns (simloss3.h); the two half-waves meet
// in one shuffle per value
struct Sim5RankEpilogue {
    const SimRankParams& p;
    float scale;                 // sim_scale(p.s), read once per work-group
    // an interior tile leaves exactly 8 small stores behind: per row group one store that carries cnt (lower half-wave) AND hmax (upper
    // half-wave, into the second table), and one for harg -- the forward's budget (g5_run: LOOSE8)
    static constexpr bool LOOSE8 = true;
    XC_DEV void finish() {}
    XC_DEV bool packs_lines(int, int) const { return false; }
    XC_DEV void pack_lines(f32x16 (&)[4][2], unsigned char*, u32x4 (&)[4][4], int, int) const {}
    template <bool NT = false> XC_DEV void store_lines(const u32x4 (&)[4][4], int, int) const {}

    // PLAIN: an interior tile off the diagonal -- no range or diagonal tests
    template <bool PLAIN>
    XC_DEV void tile(f32x16 (&acc)[4][2], int m0, int c0, int wm, int lane) const {
        const SimParams& s = p.s;
        const int h = lane >> 5;
        const long slot = c0 >> 6;
        // the wave's 4 x 32 thresholds, once per tile and ahead of the arithmetic
        float thr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            thr[i] = p.thr[PLAIN ? gm : (gm < s.nq ? gm : s.nq - 1)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool valid = PLAIN || gm < s.nq;
            const int dl = gm + s.diag_off - (c0 + 4 * h);         // the positive, relative to the lane's first column
            const int nl = s.nk - (c0 + 4 * h);                    // the first column out of range, likewise
            const float t = thr[i];
            uint32_t cnt = 0;
            float mx = SIM_NEG;
            // count and max; the scaled logit replaces the accumulator for the index pass
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cl = j * 32 + (r & 3) + 8 * (r >> 2);
                    float v = acc[i][j][r] * scale;
                    const bool ok = PLAIN || (cl < nl && cl != dl);
                    if (!PLAIN) v = ok ? v : SIM_NEG;
                    acc[i][j][r] = v;
                    cnt += (ok && v > t) ? 1u : 0u;
                    mx = fmaxf(mx, v);
                }
            // one equality pass over the logits still in registers, from the highest column down: the lowest equal one is written last
            int arg = SIMRANK_NONE;
#pragma unroll
            for (int j = 1; j >= 0; --j)
#pragma unroll
                for (int r = 15; r >= 0; --r) {
                    const int cl = j * 32 + (r & 3) + 8 * (r >> 2);
                    arg = (acc[i][j][r] == mx) ? cl : arg;
                }
            // (general tile: a lane whose 32 columns hold no negative has mx = SIM_NEG and matched its masked entries; either tile: a
            //  lane whose logits are all NaN -- diverged latents -- matched nothing and must not turn the sentinel into a column)
            arg = (arg != SIMRANK_NONE && (PLAIN || mx > SIM_NEG)) ? arg + p.col0 + c0 + 4 * h : SIMRANK_NONE;
            const float m2 = shfl_xor(mx, 32);
            const int a2 = shfl_xor(arg, 32), c2 = shfl_xor((int)cnt, 32);
            const float mm = fmaxf(mx, m2);
            const int lo = arg < a2 ? arg : a2;
            const int aa = (mx > m2) ? arg : ((m2 > mx) ? a2 : lo);
            const uint32_t cc = cnt + (uint32_t)c2;
            if (valid) {
                uint32_t* const two = h ? reinterpret_cast<uint32_t*>(p.hmax) : p.cnt;
                two[slot * s.nq + gm] = h ? f2u(mm) : cc;
                if (h == 0) p.harg[slot * s.nq + gm] = aa;
            }
        }
    }
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char*) const {
        return sim5_slot_tile(*this, p.s, acc, m0, n0) ? 8 : 0;   // a plain tile's vector-memory instructions left behind
    }
};

__global__ __launch_bounds__(G2_THREADS, 2) void sim5_rank_kernel(SimRankParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g5_run<false, false, Sim5RankEpilogue>(g, lds, Sim5RankEpilogue{p, sim_scale(p.s)});
}

// the general form (fp32, bf16 with other d, fewer than 128 rows or columns): sim_lse_partial_kernel's tile loop, two threads per row,
// each walking one 64-column slot in column order
template <typename T>
__global__ __launch_bounds__(256) void sim_rank_partial_kernel(SimRankParams p) {
    constexpr int LDC = GemmCfg<T>::LDC;
    XC_LDS_DYNAMIC(lds);
    const SimParams& s = p.s;
    const float* Cs = reinterpret_cast<const float*>(lds);
    const int tid = threadIdx.x;
    int m0, n0, tn;
    sim_general_tile<T>(s, lds, m0, n0, tn);
    const float scale = sim_scale(s);
    const int row = tid >> 1, half = tid & 1;
    const int gm = m0 + row;
    if (gm >= s.nq || n0 + half * 64 >= s.nk) return;
    const int dcol = gm + s.diag_off;
    const float t = p.thr[gm];
    uint32_t cnt = 0;
    float mx = SIM_NEG;
    int arg = SIMRANK_NONE;
    for (int c4 = 0; c4 < 16; ++c4) {
        const int col = half * 64 + c4 * 4;
        float v[4];
        load_vec<float>(Cs + row * LDC + col, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gn = n0 + col + k;
            const float sv = v[k] * scale;
            if (gn < s.nk && gn != dcol) {
                cnt += (sv > t) ? 1u : 0u;
                if (sv > mx) {                                     // strict: the lowest column among equal maxima stays
                    mx = sv;
                    arg = p.col0 + gn;
                }
            }
        }
    }
    const long slot = (long)tn * 2 + half;
    p.cnt[slot * s.nq + gm] = cnt;
    p.hmax[slot * s.nq + gm] = mx;
    p.harg[slot * s.nq + gm] = arg;
}

// thr[i] = dot(q_i, k_{i + diag_off}) * scale for the rows whose positive lies in this chunk (the others are left alone): one wave
// per row, fp32 accumulation (rows.h rowdot_kernel)
template <typename T>
__global__ __launch_bounds__(256) void simrank_pos_kernel(const T* __restrict__ Q, const T* __restrict__ K, int nq, int nk, int d,
                                                          float scale, const float* __restrict__ log_scale, int diag_off,
                                                          float* __restrict__ thr) {
    constexpr int VEC = Elem<T>::VEC;
    const int lane = lane_id();
    const long row = (long)blockIdx.x * 4 + wave_id();
    if (row >= nq) return;
    const long col = row + diag_off;
    if (col < 0 || col >= nk) return;
    const T* q = Q + row * d;
    const T* k = K + col * d;
    float acc = 0.f;
    for (int c = lane; c < d / VEC; c += 64) {
        float u[VEC], w[VEC];
        load_vec<T>(q + c * VEC, u);
        load_vec<T>(k + c * VEC, w);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc += u[j] * w[j];
    }
    acc = wave_sum(acc);
    SimParams sp{};                                                // (the forward's own expression for the scale, bit for bit)
    sp.scale = scale;
    sp.log_scale = log_scale;
    if (lane == 0) thr[row] = acc * sim_scale(sp);
}

// Fold the per-slot partials.  Work-group = 64 rows x 16 waves as sim_lse_combine_kernel: lane = row, wave w folds slots w, w + 16, ...
// in slot order, the 16 per-wave results of a row meet in LDS and are folded in wave order.
__global__ __launch_bounds__(1024) void simrank_combine_kernel(const uint32_t* __restrict__ cnt, const float* __restrict__ hmax,
                                                               const int* __restrict__ harg, int* __restrict__ rank,
                                                               float* __restrict__ hard_val, int* __restrict__ hard_idx, int nq, int slots) {
    XC_LDS_DYNAMIC(lds);
    uint32_t* red_c = reinterpret_cast<uint32_t*>(lds);     // [16][64]
    float* red_m = reinterpret_cast<float*>(lds) + 16 * 64;
    int* red_a = reinterpret_cast<int*>(lds) + 2 * 16 * 64;
    const int lane = lane_id(), wave = wave_id();
    const int i = blockIdx.x * 64 + lane;
    uint32_t c = 0;
    float m = SIM_NEG;
    int a = SIMRANK_NONE;
    if (i < nq) {
        for (int t = wave; t < slots; t += 16) {
            const float pm = hmax[(long)t * nq + i];
            const int pa = harg[(long)t * nq + i];
            c += cnt[(long)t * nq + i];
            if (pm > m || (pm == m && pa < a)) {
                m = pm;
                a = pa;
            }
        }
    }
    red_c[wave * 64 + lane] = c;
    red_m[wave * 64 + lane] = m;
    red_a[wave * 64 + lane] = a;
    sync();
    if (wave == 0 && i < nq) {
        uint32_t cc = 0;
        float mm = SIM_NEG;
        int aa = SIMRANK_NONE;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const float pm = red_m[w * 64 + lane];
            const int pa = red_a[w * 64 + lane];
            cc += red_c[w * 64 + lane];
            if (pm > mm || (pm == mm && pa < aa)) {
                mm = pm;
                aa = pa;
            }
        }
        rank[i] = (int)cc;
        hard_val[i] = mm;
        hard_idx[i] = aa == SIMRANK_NONE ? -1 : aa;
    }
}

}  // namespace xc
