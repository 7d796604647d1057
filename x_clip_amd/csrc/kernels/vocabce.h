// vocabce.h -- the MLM vocabulary head (reference mlm.py:100-107: logits = to_logits(x), F.cross_entropy over the masked rows) as two more
// epilogues on the similarity tile loop of the contrastive head: the logits z = x W^T + bias are formed tile by tile and never stored.
//   x [nm, D] the gathered masked rows, W [V, D] the vocabulary projection AS IT IS (ragged V is masked here, the way the head masks nk),
//   label[row] plays the role of the diagonal.
//   partial : per row and 64-column slot   max_j z_ij and sum_j exp(z_ij - max) over the slot's valid columns (part_m / part_l, as
//             simloss.h writes them); the lane that holds column label[row] stores z into zlab[row] -- one writer per row, no atomics
//   combine : lse_i = the row's slots folded in a fixed order (sim_lse_combine_kernel's order), rowloss_i = lse_i - zlab_i; then
//             *loss += sum_i rowloss_i by sigloss_total_kernel: one addition, in a fixed order -- two calls give the same bits
//   grad    : G_ij = s (exp(z_ij - lse_i) - [j == label_i]),  s = *gmul / nm, written once in the storage dtype; columns [V, ldg
//             rounded to the chunk) are +0.  dx = G W, dW = G^T x are ordinary GEMMs; db = the column sum of G as stored (tokens.h
//             colsum_wide_kernel), the quantity the unfused path sums.
// Arithmetic: z = acc + bias in fp32 and exp(z - reference) in the natural domain -- the differences are formed exactly where they
// matter (z near the reference) and nothing overflows for any finite z; columns >= V count as SIM_NEG (exp -> 0).
// The bias row arrives as an fp32 copy padded with zeros to whole 256-column tiles (vocab_bias_kernel, V elements per call): every
// epilogue load of it is an unconditional aligned 16-byte load.
// Ring form (bf16, D a whole number of K steps, at least 128 rows and columns): forward = g5_run with VocabLseEpilogue (every tile, the
// ragged ones through the same function's general branch); G = g5_run with VocabGradEpilogue for every FULL tile (whole-line stores,
// sim5_store_g_lines) + g3_run over the edge-tile list (Sim5EdgeTiles) with VocabGradEdgeEpilogue.  Everything else (fp32, small or odd
// shapes) runs on simloss.h's general loop.
#pragma once
#include "sigloss.h"

namespace xc {

struct VocabParams {
    SimParams s;                           // Q = x, K = W, nq = nm, nk = V, d = D, tiles_m, tiles_n; forward: part_m, part_l [slots][nm], pos = zlab [nm];
                                           // backward: lse_q = lse [nm], gmul (device scalar, required), G, ldg
    const float* bias;                     // fp32, zero-padded to a multiple of 256 columns
    const long long* label;                // [nm], each in [0, V)
};

template <typename T>
__global__ __launch_bounds__(256) void vocab_bias_kernel(const T* __restrict__ bias, float* __restrict__ out, int V, int padded) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < padded) out[c] = c < V ? to_f32(bias[c]) : 0.f;
}

// ---- forward on the ring loop: a lane owns ONE logit row of a 32-row group and 32 of the wave's 64 columns (simloss3.h); the two
// half-waves meet in one shuffle.  The row's label column belongs to exactly one lane of one wave of one tile.
struct VocabLseEpilogue {
    const VocabParams& p;
    // (a tile leaves 8 partial stores and up to 4 zlab stores behind: g5_run's relaxed wait counts exactly 8, so this epilogue reports 0
    //  and the next tile's first K step takes the strict wait, as SigLossEpilogue does)
    XC_DEV void finish() {}
    XC_DEV bool packs_lines(int, int) const { return false; }
    XC_DEV void pack_lines(f32x16 (&)[4][2], unsigned char*, u32x4 (&)[4][4], int, int) const {}
    template <bool NT = false> XC_DEV void store_lines(const u32x4 (&)[4][4], int, int) const {}
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char*) const {
        const SimParams& s = p.s;
        const int lane = threadIdx.x & 63, h = lane >> 5;
        const int wave = uniform(threadIdx.x >> 6), wm = wave >> 2, wn = wave & 3;
        const int c0 = n0 + wn * 64;                               // this wave's 64-column slot
        if (c0 >= s.nk) return 0;
        const long slot = c0 >> 6;
        const bool full = sim5_full_tile(s, m0, n0);               // (uniform) no range tests
        const float* const bcol = p.bias + c0 + 4 * h;
        const int nl = s.nk - (c0 + 4 * h);                        // the first column out of range, relative to the lane's first column
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool valid = full || gm < s.nq;
            const int dl = (int)p.label[valid ? gm : s.nq - 1] - (c0 + 4 * h);      // the label, likewise
            float mx = SIM_NEG;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const u32x4 t = ld16(bcol + j * 32 + 8 * q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float z = acc[i][j][4 * q + k] + u2f(t[k]);
                        if (!full) z = (j * 32 + 8 * q + k < nl) ? z : SIM_NEG;
                        acc[i][j][4 * q + k] = z;
                        mx = fmaxf(mx, z);
                    }
                }
            float l = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) l += fast_exp(acc[i][j][r] - mx);
            if (valid && (unsigned)dl < 64u) {                       // the label lies in this slot: in this lane's half of it?
                float zl = 0.f;
                bool hit = false;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool sel = dl == j * 32 + (r & 3) + 8 * (r >> 2);
                        zl = sel ? acc[i][j][r] : zl;
                        hit = hit || sel;
                    }
                if (hit) s.pos[gm] = zl;
            }
            const float m2 = shfl_xor(mx, 32), l2 = shfl_xor(l, 32);
            const float mm = fmaxf(mx, m2);
            const float ll = l * fast_exp(mx - mm) + l2 * fast_exp(m2 - mm);
            if (h == 0 && valid) {
                s.part_m[slot * s.nq + gm] = mm;
                s.part_l[slot * s.nq + gm] = ll;
            }
        }
        return 0;
    }
};

__global__ __launch_bounds__(G2_THREADS, 2) void vocab5_lse_kernel(VocabParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g5_run<false, false, VocabLseEpilogue>(g, lds, VocabLseEpilogue{p});
}

// the general form (fp32, bf16 with other D, fewer than 128 rows or columns): sim_lse_partial_kernel's tile loop, two threads per row,
// each walking one 64-column slot in column order
template <typename T>
__global__ __launch_bounds__(256) void vocab_lse_partial_kernel(VocabParams p) {
    constexpr int LDC = GemmCfg<T>::LDC;
    XC_LDS_DYNAMIC(lds);
    const SimParams& s = p.s;
    const float* Cs = reinterpret_cast<const float*>(lds);
    const int tid = threadIdx.x;
    int m0, n0, tn;
    sim_general_tile<T>(s, lds, m0, n0, tn);
    const int row = tid >> 1, half = tid & 1;
    const int gm = m0 + row;
    if (gm >= s.nq || n0 + half * 64 >= s.nk) return;
    const int lab = (int)p.label[gm];
    float m = SIM_NEG, l = 0.f;
    for (int c4 = 0; c4 < 16; ++c4) {
        const int col = half * 64 + c4 * 4;
        float v[4], b[4];
        load_vec<float>(Cs + row * LDC + col, v);
        load_vec<float>(p.bias + n0 + col, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gn = n0 + col + k;
            const float z = v[k] + b[k];
            if (gn < s.nk) {
                if (gn == lab) s.pos[gm] = z;
                if (z > m) {
                    l = l * fast_exp(m - z) + 1.0f;
                    m = z;
                } else {
                    l += fast_exp(z - m);
                }
            }
        }
    }
    const long slot = (long)tn * 2 + half;
    s.part_m[slot * s.nq + gm] = m;
    s.part_l[slot * s.nq + gm] = l;
}

// Fold the per-slot partials: lse_i and rowloss_i = lse_i - zlab_i.  Work-group = 64 rows x 16 waves as sim_lse_combine_kernel: lane =
// row, wave w folds slots w, w + 16, ... in slot order, the 16 per-wave pairs of a row meet in LDS and are folded in wave order.  Nothing
// is added anywhere: sigloss_total_kernel sums rowloss.
__global__ __launch_bounds__(1024) void vocab_combine_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                             const float* __restrict__ zlab, float* __restrict__ lse,
                                                             float* __restrict__ rowloss, int nq, int slots) {
    XC_LDS_DYNAMIC(lds);
    float* red_m = reinterpret_cast<float*>(lds);           // [16][64]
    float* red_l = red_m + 16 * 64;
    const int lane = lane_id(), wave = wave_id();
    const int i = blockIdx.x * 64 + lane;
    float m = SIM_NEG, l = 0.f;
    if (i < nq) {
        for (int t = wave; t < slots; t += 16) {
            const float pm = part_m[(long)t * nq + i], pl = part_l[(long)t * nq + i];
            const float mm = fmaxf(m, pm);
            l = l * fast_exp(m - mm) + pl * fast_exp(pm - mm);
            m = mm;
        }
    }
    red_m[wave * 64 + lane] = m;
    red_l[wave * 64 + lane] = l;
    sync();
    if (wave == 0 && i < nq) {
        float mm = SIM_NEG;
#pragma unroll
        for (int w = 0; w < 16; ++w) mm = fmaxf(mm, red_m[w * 64 + lane]);
        float ll = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) ll += red_l[w * 64 + lane] * fast_exp(red_m[w * 64 + lane] - mm);
        const float v = mm + logf(ll);                          // (ll >= 1: the row's maximum is one of its terms)
        lse[i] = v;
        rowloss[i] = v - zlab[i];
    }
}

// ---- backward: G on the ring loop, every FULL tile, as Sim5FastGradEpilogue handles them: the accumulators become G in place, column
// quad by column quad (the quad's four bias values live only that long), and leave through the plain GEMM's line exchange as whole-line
// stores.  The label's logit is corrected per quad behind ONE vote: a quad holds a label of one of the wave's 128 rows in 8 * 128 / V of
// the cases.
template <bool STREAM>
struct VocabGradEpilogue {
    const VocabParams& p;
    const Gemm2Params& gp;       // C = G, ldc = ldg, alpha = 1: what the line stores address
    float sc;                    // *gmul / nm, read once per work-group
    static constexpr bool DEFER_FRAGS = true;                 // (gemm4.h g5_defer_frags: the 24 registers of the next tile's first fragments)
    XC_DEV void finish() {}
    XC_DEV bool packs_lines(int, int) const { return false; }
    XC_DEV void pack_lines(f32x16 (&)[4][2], unsigned char*, u32x4 (&)[4][4], int, int) const {}
    template <bool NT = false> XC_DEV void store_lines(const u32x4 (&)[4][4], int, int) const {}
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char* scratch) {
        if (!sim5_full_tile(p.s, m0, n0)) return 0;                 // (uniform) the edge launch's tile
        to_g(acc, m0, n0);
        return sim5_store_g_lines<STREAM>(acc, gp, m0, n0, scratch);
    }
    XC_DEV void to_g(f32x16 (&acc)[4][2], int m0, int n0) {
        const int lane = threadIdx.x & 63, h = lane >> 5;
        const int wave = uniform(threadIdx.x >> 6), wm = wave >> 2, wn = wave & 3;
        const float* const bcol = p.bias + n0 + wn * 64 + 4 * h;
        const float s_ = sc;
        float lq[4];                                                 // the row's lse
        int dl[4];                                                   // the row's label, relative to the lane's first column
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            lq[i] = p.s.lse_q[gm];
            dl[i] = (int)p.label[gm] - (n0 + wn * 64 + 4 * h);
        }
        u32x4 t = ld16(bcol);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u32x4 tn = t;
                if (j * 4 + q < 7) tn = ld16(bcol + (j * 4 + q + 1 < 4 ? 0 : 32) + 8 * ((j * 4 + q + 1) & 3));   // the next quad's four bias values
                const int base = j * 32 + 8 * q;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float z = acc[i][j][4 * q + k] + u2f(t[k]);
                        acc[i][j][4 * q + k] = s_ * fast_exp(z - lq[i]);
                    }
                bool mine = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) mine = mine || (unsigned)(dl[i] - base) < 4u;
                if (wave_any(mine)) {                                // (uniform; rare)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float g = acc[i][j][4 * q + k];
                            acc[i][j][4 * q + k] = (dl[i] == base + k) ? g - s_ : g;
                        }
                }
                t = tn;
                sched_fence();
            }
    }
};

// the tiles VocabGradEpilogue skips (Sim5EdgeTiles), through the general form on simloss3.h's loop: per-element range and label tests,
// 16-byte row stores, rows of G padded to a whole chunk with zeros
struct VocabGradEdgeEpilogue {
    const VocabParams& p;
    XC_DEV void finish() {}
    XC_DEV int operator()(f32x16 (&acc)[4][2], int m0, int n0) {
        const SimParams& s = p.s;
        const int lane = threadIdx.x & 63, h = lane >> 5;
        const int wave = uniform(threadIdx.x >> 6), wm = wave >> 2, wn = wave & 3;
        const float sc = *s.gmul / (float)s.nq;
        const int nkp = (s.nk + 7) & ~7;                           // G rows are padded to a whole 16-byte chunk with zeros
        bf16_t* G = reinterpret_cast<bf16_t*>(s.G);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool row_ok = gm < s.nq;
            const float lq = s.lse_q[row_ok ? gm : s.nq - 1];
            const int lab = (int)p.label[row_ok ? gm : s.nq - 1];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nb = n0 + wn * 64 + j * 32;
                uint32_t pk[4][2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const u32x4 t = ld16(p.bias + nb + 4 * h + 8 * q);
                    float g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int gn = nb + 4 * h + 8 * q + k;
                        const float z = acc[i][j][4 * q + k] + u2f(t[k]);
                        float v = 0.f;
                        if (row_ok && gn < s.nk) {
                            v = sc * fast_exp(z - lq);
                            v = (gn == lab) ? v - sc : v;
                        }
                        g[k] = v;
                    }
                    pk[q][0] = (uint32_t)f2bf(g[0]) | ((uint32_t)f2bf(g[1]) << 16);
                    pk[q][1] = (uint32_t)f2bf(g[2]) | ((uint32_t)f2bf(g[3]) << 16);
                }
#pragma unroll
                for (int qq = 0; qq < 4; qq += 2) {
                    permlane32_swap(pk[qq][0], pk[qq + 1][0]);
                    permlane32_swap(pk[qq][1], pk[qq + 1][1]);
                    const int gn = nb + qq * 8 + 8 * h;
                    if (row_ok && gn < nkp) {
                        u32x4 o = {pk[qq][0], pk[qq][1], pk[qq + 1][0], pk[qq + 1][1]};
                        st16(G + (long)gm * s.ldg + gn, o);
                    }
                }
            }
        }
        return 0;
    }
};

template <bool STREAM>
__global__ __launch_bounds__(G2_THREADS, 2) void vocab5_grad_kernel(VocabParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim5_g_gemm_params(p.s, STREAM);
    g5_run<false, false, VocabGradEpilogue<STREAM>>(g, lds, VocabGradEpilogue<STREAM>{p, g, *p.s.gmul / (float)p.s.nq});
}
__global__ __launch_bounds__(G2_THREADS, 2) void vocab5_grad_edge_kernel(VocabParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g3_run<false, false, 0>(g, lds, VocabGradEdgeEpilogue{p}, Sim5EdgeTiles{p.s});
}

// the general form (fp32, bf16 with other D, fewer than 128 rows or columns) on sim_grad_kernel's loop
template <typename T>
__global__ __launch_bounds__(256) void vocab_grad_kernel(VocabParams p) {
    constexpr int VEC = Elem<T>::VEC, LDC = GemmCfg<T>::LDC;
    XC_LDS_DYNAMIC(lds);
    const SimParams& s = p.s;
    const float* Cs = reinterpret_cast<const float*>(lds);
    const int tid = threadIdx.x;
    int m0, n0, tn;
    sim_general_tile<T>(s, lds, m0, n0, tn);
    constexpr int CPR = 128 / VEC;
    T* G = reinterpret_cast<T*>(s.G);
    const float sc = *s.gmul / (float)s.nq;
    for (int id = tid; id < 128 * CPR; id += GEMM_THREADS) {
        const int row = id / CPR, col = (id % CPR) * VEC;
        const int gm = m0 + row, gn0 = n0 + col;
        if (gm < s.nq && gn0 < s.nk) {                      // G rows are padded to a whole chunk: columns >= V get 0
            const float lq = s.lse_q[gm];
            const int lab = (int)p.label[gm];
            float g[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int gn = gn0 + k;
                float v = 0.f;
                if (gn < s.nk) {
                    v = sc * fast_exp(Cs[row * LDC + col + k] + p.bias[gn] - lq);
                    v = (gn == lab) ? v - sc : v;
                }
                g[k] = v;
            }
            store_vec<T>(G + (long)gm * s.ldg + gn0, g);
        }
    }
}

}  // namespace xc
