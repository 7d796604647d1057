// simtopk.h -- retrieval / zero-shot classification on the contrastive head's similarity (reference x_clip.py:813-847: the same
// S = scale * Q K^T the loss reduces) WITHOUT the logits: per query row the k best gallery columns (1 <= k <= 32) and their logits,
// ordered by (value descending, column ascending).  Threshold select, two sweeps of the similarity tile loop and no sort:
//   slot maxima : the rank partial (simrank.h) with thr = +inf and a diag_off no row reaches: hmax[slot][row], every full tile PLAIN
//   select      : tau_i = the k-th largest of row i's slot maxima (SIM_NEG when the row has fewer than k slots).  k slots hold a logit
//                 >= tau_i each, so at least min(k, ng) logits of the row are >= tau_i, and every top-k logit is
//   mask        : a FOURTH epilogue on the tile loop: per (row, 64-column slot) the 64-bit mask of the in-range columns with
//                 s_ij >= tau_i.  Same loop, tile shape, grid and chunk cuts as the first sweep: the same logit bits, which is what
//                 carries the select's invariant over to the masks
//   finish      : per chunk, one wave per row: every set bit's logit is recomputed as simrank_pos_kernel forms it (wave dot, fp32, the
//                 same sim_scale expression) and inserted into the row's k best under the TOTAL order above -- so the merge depends
//                 neither on how the gallery is cut nor on the order the chunks are consumed in.  Cost ~ the number of candidates:
//                 k to a few k per row on real latents, the whole row when all logits are equal (tests/topk_cases.py pins that case)
// Chunk independence of the RESULT: the candidates are chosen by the tile loop's logit against tau, and tau follows the slot boundaries,
// i.e. the cuts (a cut may also move a chunk between the ring and the general form); the ranking uses the re-scored logit.  Where both
// logits are the same bits (exactly representable dot products: the exact tests) the result is independent of cuts and order, bit for
// bit.  On real latents a column whose two logits straddle tau under one cut and not under another may enter or leave: only among
// near-ties inside the fp32 accumulation error, the band the realistic tests hold every row to.
// A row of NaN latents has hmax = SIM_NEG everywhere, tau = SIM_NEG, and no logit that compares >= : no candidate, the row keeps its
// padding (index -1, value SIM_NEG).  No atomics, no LDS beyond the tile loop's own; bit-reproducible from launch to launch.
#pragma once
#include "simrank.h"

namespace xc {

constexpr int SIMTOPK_MAX_K = 32;

struct SimTopkParams {
    SimParams s;                           // Q, K, nq, nk, d, scale, log_scale, tiles_m, tiles_n (the forward's fields; diag_off unused)
    const float* tau;                      // [nq]
    uint32_t* mlo; uint32_t* mhi;          // [slots][nq] each, already offset to this chunk's first slot: columns 0-31 / 32-63 of the slot
};

// the ring-loop form: a lane owns ONE logit row of a 32-row group and 32 of the wave's 64 columns (simrank.h's lane <-> column map);
// the two half-waves swap the word the other one stores in one shuffle
struct Sim5MaskEpilogue {
    const SimTopkParams& p;
    float scale;                 // sim_scale(p.s), read once per work-group
    // an interior tile leaves 4 store instructions behind (per row group ONE: the lower half-wave writes the low word, the upper one the
    // high word into the second table) -- fewer than the LOOSE8 budget.  g5_run's relaxed wait counts exactly 8, so this epilogue
    // reports 0 and the next tile's first K step takes the strict wait (as SigLossEpilogue)
    XC_DEV void finish() {}
    XC_DEV bool packs_lines(int, int) const { return false; }
    XC_DEV void pack_lines(f32x16 (&)[4][2], unsigned char*, u32x4 (&)[4][4], int, int) const {}
    template <bool NT = false> XC_DEV void store_lines(const u32x4 (&)[4][4], int, int) const {}

    // PLAIN: a full tile -- no range tests (nothing is excluded: there is no diagonal here)
    template <bool PLAIN>
    XC_DEV void tile(f32x16 (&acc)[4][2], int m0, int c0, int wm, int lane) const {
        const SimParams& s = p.s;
        const int h = lane >> 5;
        const long slot = c0 >> 6;
        // the wave's 4 x 32 thresholds, once per tile and ahead of the arithmetic
        float tau[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            tau[i] = p.tau[PLAIN ? gm : (gm < s.nq ? gm : s.nq - 1)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool valid = PLAIN || gm < s.nq;
            const int nl = s.nk - (c0 + 4 * h);                    // the first column out of range, relative to the lane's first column
            const float t = tau[i];
            uint32_t w[2] = {0u, 0u};                              // this lane's bits of the slot's two words, before the half-wave shift
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int b = (r & 3) + 8 * (r >> 2);          // cl = j * 32 + b
                    const float v = acc[i][j][r] * scale;
                    const bool ok = PLAIN || (j * 32 + b < nl);
                    w[j] |= (ok && v >= t) ? (1u << b) : 0u;       // (NaN compares false: a diverged row sets no bit)
                }
            w[0] <<= 4 * h;
            w[1] <<= 4 * h;
            const uint32_t other = (uint32_t)shfl_xor((int)(h ? w[0] : w[1]), 32);
            const uint32_t mine = (h ? w[1] : w[0]) | other;
            if (valid) {
                uint32_t* const two = h ? p.mhi : p.mlo;
                two[slot * s.nq + gm] = mine;
            }
        }
    }
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char*) const {
        sim5_slot_tile(*this, p.s, acc, m0, n0);
        return 0;
    }
};

__global__ __launch_bounds__(G2_THREADS, 2) void sim5_mask_kernel(SimTopkParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g5_run<false, false, Sim5MaskEpilogue>(g, lds, Sim5MaskEpilogue{p, sim_scale(p.s)});
}

// the general form (fp32, bf16 with other d, fewer than 128 rows or columns): sim_rank_partial_kernel's tile loop, two threads per row,
// each walking one 64-column slot in column order
template <typename T>
__global__ __launch_bounds__(256) void sim_mask_partial_kernel(SimTopkParams p) {
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
    const float t = p.tau[gm];
    uint32_t w[2] = {0u, 0u};
    for (int c4 = 0; c4 < 16; ++c4) {
        const int col = half * 64 + c4 * 4;
        float v[4];
        load_vec<float>(Cs + row * LDC + col, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gn = n0 + col + k;
            const float sv = v[k] * scale;
            if (gn < s.nk && sv >= t) w[c4 >> 3] |= 1u << ((c4 & 7) * 4 + k);
        }
    }
    const long slot = (long)tn * 2 + half;
    p.mlo[slot * s.nq + gm] = w[0];
    p.mhi[slot * s.nq + gm] = w[1];
}

// tau[i] = the k-th largest (with multiplicity) of hmax[0 .. slots)[i], SIM_NEG when slots < k.  One wave per row; a descent over the
// DISTINCT values from the top: per round the largest value below the last one and how often it occurs -- at most k rounds.  A lane
// keeps its first 8 slots in registers (512 slots = 32768 columns), the others are re-read (they stay in the L2).
__global__ __launch_bounds__(256) void simtopk_select_kernel(const float* __restrict__ hmax, float* __restrict__ tau, int nq, int slots,
                                                            int k) {
    constexpr int REG = 8;
    const float ABSENT = -__builtin_inff();                        // (a slot maximum is never below SIM_NEG)
    const int lane = lane_id();
    const long row = (long)blockIdx.x * 4 + wave_id();
    if (row >= nq) return;
    if (slots < k) {
        if (lane == 0) tau[row] = SIM_NEG;
        return;
    }
    float reg[REG];
#pragma unroll
    for (int t = 0; t < REG; ++t) {
        const int sl = lane + 64 * t;
        reg[t] = sl < slots ? hmax[(long)sl * nq + row] : ABSENT;
    }
    float cur = 0.f, result = SIM_NEG;
    bool first = true;
    int remaining = k;
    for (int round = 0; round < k; ++round) {                      // (everything below is wave-uniform)
        float m = ABSENT;
#pragma unroll
        for (int t = 0; t < REG; ++t) m = (first || reg[t] < cur) ? fmaxf(m, reg[t]) : m;
        for (int sl = lane + 64 * REG; sl < slots; sl += 64) {
            const float v = hmax[(long)sl * nq + row];
            m = (first || v < cur) ? fmaxf(m, v) : m;
        }
        m = wave_max(m);
        int c = 0;
#pragma unroll
        for (int t = 0; t < REG; ++t) c += (reg[t] == m) ? 1 : 0;
        for (int sl = lane + 64 * REG; sl < slots; sl += 64) c += (hmax[(long)sl * nq + row] == m) ? 1 : 0;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) c += shfl_xor(c, x);
        if (c >= remaining) {
            result = m;
            break;
        }
        remaining -= c;
        cur = m;
        first = false;
    }
    if (lane == 0) tau[row] = result;
}

// One chunk's candidates into the row's k best: values / indices [nq, k] hold what the chunks before left (index -1 = empty; the first
// call finds them all empty), lane r < k of the row's wave holds entry r, sorted.  Per set bit of the row's masks: the logit as
// simrank_pos_kernel forms it, then one shifted read of the list -- an entry stays, takes the candidate or takes its left neighbour.
template <typename T>
__global__ __launch_bounds__(256) void simtopk_finish_kernel(const T* __restrict__ Q, const T* __restrict__ K, int nq, int nk, int d,
                                                            float scale, const float* __restrict__ log_scale, int col0,
                                                            const uint32_t* __restrict__ mlo, const uint32_t* __restrict__ mhi, int k,
                                                            float* __restrict__ values, int* __restrict__ indices) {
    constexpr int VEC = Elem<T>::VEC;
    const int lane = lane_id();
    const long row = (long)blockIdx.x * 4 + wave_id();
    if (row >= nq) return;
    float bv = SIM_NEG;
    int bi = -1;
    if (lane < k) {
        bv = values[row * k + lane];
        bi = indices[row * k + lane];
    }
    SimParams sp{};                                                // (the forward's own expression for the scale, bit for bit)
    sp.scale = scale;
    sp.log_scale = log_scale;
    const float sc = sim_scale(sp);
    const T* q = Q + row * d;
    const int nslots = (nk + 63) / 64;
    for (int base = 0; base < nslots; base += 64) {
        const int sl = base + lane;
        uint32_t lo = 0u, hi = 0u;
        if (sl < nslots) {
            lo = mlo[(long)sl * nq + row];
            hi = mhi[(long)sl * nq + row];
        }
        uint64_t any = wave_ballot64((lo | hi) != 0u);
        while (any != 0) {                                         // slots in column order, then bits in column order (wave-uniform)
            const int src = __builtin_ctzll(any);
            any &= any - 1;
            const uint32_t wlo = (uint32_t)uniform(shfl((int)lo, src)), whi = (uint32_t)uniform(shfl((int)hi, src));
            uint64_t bits = (uint64_t)wlo | ((uint64_t)whi << 32);
            while (bits != 0) {
                const int b = __builtin_ctzll(bits);
                bits &= bits - 1;
                const long col = (long)(base + src) * 64 + b;
                if (col >= nk) continue;                           // (the mask sweep sets in-range bits only; a foreign mask must not steer a read)
                const T* kr = K + col * d;
                float acc = 0.f;
                for (int c = lane; c < d / VEC; c += 64) {
                    float u[VEC], w[VEC];
                    load_vec<T>(q + c * VEC, u);
                    load_vec<T>(kr + c * VEC, w);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc += u[j] * w[j];
                }
                const float s = wave_sum(acc) * sc;
                if (!(s == s)) continue;                           // (uniform)
                const int gcol = col0 + (int)col;
                const float pv = shfl(bv, lane - 1);
                const int pi = shfl(bi, lane - 1);
                // an entry precedes the candidate: it is not empty and it is larger, or equal with the lower column
                const bool stay = bi >= 0 && (bv > s || (bv == s && bi < gcol));
                const bool left_stays = lane == 0 || (pi >= 0 && (pv > s || (pv == s && pi < gcol)));
                if (!stay) {
                    bv = left_stays ? s : pv;
                    bi = left_stays ? gcol : pi;
                }
            }
        }
    }
    if (lane < k) {
        values[row * k + lane] = bv;
        indices[row * k + lane] = bi;
    }
}

}  // namespace xc
