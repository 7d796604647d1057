// sigloss.h -- the pairwise sigmoid loss (Zhai et al., "Sigmoid Loss for Language Image Pre-Training", 2023) as a fourth and fifth epilogue
// on the similarity tile loop of the contrastive head (S = scale * Q K^T as simloss.h forms it, reference x_clip.py:813-817; the reference
// has no sigmoid loss).  Every logit is an independent binary term: no log-sum-exp, nothing to gather between ranks, no reference point.
//   l_ij = s_ij + beta,  z_ij = +1 if j == i + diag_off else -1
//   partial : per row and 64-column slot   sum_j softplus(-z_ij l_ij) over the slot's valid columns          (nothing else is written)
//   combine : rowloss_i = the row's slots folded in a fixed order (wave w of 16 folds slots w, w + 16, ..., then the waves in order);  *loss += coef * sum_i rowloss_i, one addition, in a fixed order
//   grad    : G_ij = gmul coef (-z_ij) sigma(-z_ij l_ij)  (x scale with g_times_scale), written once;  dtau += sum G o s,  dbias += sum G
//             In the edge and general forms sum G o s is accumulated SPLIT: with w = (-z) sigma(-z l) = one + small, one in {-1, 0, 1} and |small| <= 1/2 (sig_dsplit),
//             sum one * acc and sum small * acc are carried apart and meet once per wave.  At beta = +10 every sigma is ~1 and
//             dtau = gc sum s cancels to 1/500 of its terms: summed as sum G * acc, the rounding of each G -- the same for equal logits --
//             left 1e-5 of dtau; the "one" part sums the accumulators themselves.
// Arithmetic (emulator and GPU alike).  One exponential per logit, in the base-2 domain: l2 = l log2(e) is ONE fma of the accumulator,
// e = exp2(-|l2|) <= 1 a bare v_exp_f32 -- nothing overflows for any finite l, and an underflow to 0 is the correct limit.
//   softplus(x) = max(x, 0) + log1p(e)           (summed as max(l2, 0) + log2(1 + e), times ln 2 once per row)
//   sigma(x)    = x >= 0 ? 1 / (1 + e) : e / (1 + e)
// log1p must be accurate RELATIVE TO e: at SigLIP's own initialisation (t = 10, beta = -10) the negatives sit at l in [-20, 0], tens of
// thousands of terms near 1e-8 per row carry the loss, and 1 + e rounds to 1 for all of them.  Below SIG_SERIES_BELOW = 0.0221 (2^-5.5)
// the three-term series e - e^2/2 + e^3/3 is used: its truncation error is below e^4/4, i.e. e^3/4 <= 2.7e-6 relative.  At or above the
// threshold log2(1 + e) is a bare v_log_f32: forming 1 + e rounds by at most 2^-24 absolute, i.e. 2^-24 / e <= 2.7e-6 relative to
// log1p(e) ~ e.  The threshold is where the two bounds meet.
#pragma once
#include "simloss5.h"

namespace xc {

struct SigParams {
    SimParams s;                           // Q, K, nq, nk, d, scale, log_scale, diag_off, tiles_m, tiles_n; backward: gmul, g_times_scale, G, ldg, dtau
    const float* bias;                     // device scalar beta
    float* part;                           // forward: [slots][nq], already offset to this chunk's first slot
    float coef;                            // backward: w / B_global
    float* dbias;                          // backward: scalar accumulator or null
};

constexpr float SIG_LOG2E = 1.4426950408889634f, SIG_LN2 = 0.6931471805599453f;
constexpr float SIG_SERIES_BELOW = 0.0221f;

XC_DEV float sig_log2(float u) {           // 1 <= u <= 2: no denormal pre-scaling needed around the bare instruction
#if defined(__HIP__)
    return __builtin_amdgcn_logf(u);
#else
    return log2f(u);
#endif
}
// log2(1 + e) for 0 <= e <= 1, accurate relative to e (the file comment has the bounds)
XC_DEV float sig_log2_1p(float e) {
    const float ser = e * (SIG_LOG2E + e * (-0.5f * SIG_LOG2E + e * (SIG_LOG2E / 3.0f)));
    const float lg = sig_log2(1.0f + e);
    return e < SIG_SERIES_BELOW ? ser : lg;
}
// softplus(-z l) / ln 2 for l2 = l log2(e); pos: z = +1
XC_DEV float sig_term2(float l2, bool pos) {
    const float e = fast_exp2(-fabsf(l2));
    return fmaxf(pos ? -l2 : l2, 0.f) + sig_log2_1p(e);
}
// (-z) sigma(-z l): sigma(l) for a negative, -sigma(-l) for the positive (formed directly: sigma(l) - 1 would cancel)
XC_DEV float sig_dterm(float l2, bool pos) {
    const float e = fast_exp2(-fabsf(l2));
    const float r = fast_rcp(1.0f + e);
    const bool ge = l2 >= 0.f;
    const float num = pos ? (ge ? -e : -1.0f) : (ge ? 1.0f : e);
    return num * r;
}

// the same weight split for the tau sum: w = one + small, one = [l >= 0] for a negative and [l >= 0] - 1 for the positive,
// small = -u for l >= 0 and +u otherwise, u = e / (1 + e) <= 1/2
XC_DEV void sig_dsplit(float l2, bool pos, float& one, float& small) {
    const float e = fast_exp2(-fabsf(l2));
    const float u = e * fast_rcp(1.0f + e);
    const bool ge = l2 >= 0.f;
    one = (ge ? 1.0f : 0.f) - (pos ? 1.0f : 0.f);
    small = ge ? -u : u;
}

// ---- forward on the ring loop: a lane owns ONE logit row of a 32-row group and 32 of the wave's 64 columns (simloss3.h); the two
// half-waves meet in one shuffle
struct SigLossEpilogue {
    const SigParams& p;
    float scale2, bias2;         // sim_scale(p.s) log2(e) and *p.bias log2(e), read once per work-group
    // an interior tile leaves 4 small stores behind (one partial per row group): fewer than the LOOSE8 budget of the other forward
    // epilogues.  g5_run's relaxed wait counts exactly 8, so this epilogue reports 0 and the next tile's first K step takes the strict wait
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
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool valid = PLAIN || gm < s.nq;
            const int dl = gm + s.diag_off - (c0 + 4 * h);         // the positive, relative to the lane's first column
            const int nl = s.nk - (c0 + 4 * h);                    // the first column out of range, likewise
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cl = j * 32 + (r & 3) + 8 * (r >> 2);
                    const float l2 = acc[i][j][r] * scale2 + bias2;
                    float v = sig_term2(l2, !PLAIN && cl == dl);
                    if (!PLAIN) v = cl < nl ? v : 0.f;
                    sum += v;
                }
            sum += shfl_xor(sum, 32);
            if (h == 0 && valid) p.part[slot * s.nq + gm] = sum * SIG_LN2;
        }
    }
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char*) const {
        sim5_slot_tile(*this, p.s, acc, m0, n0);
        return 0;
    }
};

__global__ __launch_bounds__(G2_THREADS, 2) void sig5_loss_kernel(SigParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g5_run<false, false, SigLossEpilogue>(g, lds, SigLossEpilogue{p, sim_scale(p.s) * SIG_LOG2E, *p.bias * SIG_LOG2E});
}

// the general form (fp32, bf16 with other d, fewer than 128 rows or columns): sim_lse_partial_kernel's tile loop, two threads per row,
// each walking one 64-column slot in column order
template <typename T>
__global__ __launch_bounds__(256) void sig_partial_kernel(SigParams p) {
    constexpr int LDC = GemmCfg<T>::LDC;
    XC_LDS_DYNAMIC(lds);
    const SimParams& s = p.s;
    const float* Cs = reinterpret_cast<const float*>(lds);
    const int tid = threadIdx.x;
    int m0, n0, tn;
    sim_general_tile<T>(s, lds, m0, n0, tn);
    const float scale2 = sim_scale(s) * SIG_LOG2E, bias2 = *p.bias * SIG_LOG2E;
    const int row = tid >> 1, half = tid & 1;
    const int gm = m0 + row;
    if (gm >= s.nq || n0 + half * 64 >= s.nk) return;
    const int dcol = gm + s.diag_off;
    float sum = 0.f;
    for (int c4 = 0; c4 < 16; ++c4) {
        const int col = half * 64 + c4 * 4;
        float v[4];
        load_vec<float>(Cs + row * LDC + col, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int gn = n0 + col + k;
            if (gn < s.nk) sum += sig_term2(v[k] * scale2 + bias2, gn == dcol);
        }
    }
    const long slot = (long)tn * 2 + half;
    p.part[slot * s.nq + gm] = sum * SIG_LN2;
}

// Fold the per-slot partials into rowloss.  Work-group = 64 rows x 16 waves as sim_lse_combine_kernel: lane = row, wave w folds slots
// w, w + 16, ... in slot order, the 16 per-wave sums of a row meet in LDS and are folded in wave order.
__global__ __launch_bounds__(1024) void sigloss_combine_kernel(const float* __restrict__ part, float* __restrict__ rowloss, int nq, int slots) {
    XC_LDS_DYNAMIC(lds);
    float* red = reinterpret_cast<float*>(lds);             // [16][64]
    const int lane = lane_id(), wave = wave_id();
    const int i = blockIdx.x * 64 + lane;
    float l = 0.f;
    if (i < nq)
        for (int t = wave; t < slots; t += 16) l += part[(long)t * nq + i];
    red[wave * 64 + lane] = l;
    sync();
    if (wave == 0 && i < nq) {
        float ll = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) ll += red[w * 64 + lane];
        rowloss[i] = ll;
    }
}
// *loss += coef * sum_i rowloss_i by ONE work-group: thread t sums rows t, t + 1024, ... in order, the wave's butterfly and the 16 waves'
// sums in wave order follow -- the same bits on every launch (one atomic per work-group, as the InfoNCE combine issues it, would leave
// the order of the nq / 64 additions to the scheduler)
__global__ __launch_bounds__(1024) void sigloss_total_kernel(const float* __restrict__ rowloss, float* __restrict__ loss, int nq, float coef) {
    XC_LDS_DYNAMIC(lds);
    float* red = reinterpret_cast<float*>(lds);             // [16]
    const int lane = lane_id(), wave = wave_id();
    float l = 0.f;
    for (int i = threadIdx.x; i < nq; i += 1024) l += rowloss[i];
    l = wave_sum(l);
    if (lane == 0) red[wave] = l;
    sync();
    if (threadIdx.x == 0) {
        float ll = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) ll += red[w];
        atomic_add(loss, coef * ll);
    }
}

// ---- backward: G on the ring loop, every FULL tile (on the diagonal or off it), as Sim5FastGradEpilogue handles them: the accumulators
// become G in place and leave through the plain GEMM's line exchange as whole-line stores.  No lse loads, no vote, no exact / fast split:
// sigma needs nothing but the logit.  Across the K loops the lane carries its shares of sum G o acc and sum G (two registers).
template <bool STREAM>
struct SigGradEpilogue {
    const SigParams& p;
    const Gemm2Params& gp;       // C = G, ldc = ldg, alpha = 1: what the line stores address
    float scale, bias2, gc;      // sim_scale(p.s), *p.bias log2(e), gmul coef (x scale with g_times_scale): read once per work-group
    float* red;                  // the work-group's LDS (free once the tile loop has ended): [2][waves] for finish()
    float dt_acc = 0.f, db_acc = 0.f;   // the lane's shares of sum G o acc and sum G (two registers across the K loops)
    // (the split tau sum of the edge and general forms -- sig_dsplit -- is NOT used here: with its extra select and sum per logit the
    //  kernel spilled 237 - 291 vector registers, with or without DEFER_FRAGS and scheduling fences; tests/test_sigloss_isa.py.  On
    //  full tiles dtau is therefore sum G * acc: where it cancels -- beta = +10, every sigma ~1 -- the rounding of G leaves up to 8e-6 of it, tests/sigloss_cases.py case_regime)
    // the waves' sums meet in LDS and are folded in wave order: ONE atomic pair per work-group.  (Per wave, as Sim5FastGradEpilogue
    // adds dtau, the 2048 additions in scheduler order made two launches differ by more than 1e-6 of the sum at 272 tiles.)
    XC_DEV void finish() {
        constexpr int NW = G2_THREADS / 64;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const float dt = wave_sum(dt_acc), db = wave_sum(db_acc);
        sync();                                                     // every wave is done with the operand stages
        if (lane == 0) {
            red[wave] = dt;
            red[NW + wave] = db;
        }
        sync();
        if (threadIdx.x == 0) {
            float t = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                t += red[w];
                b += red[NW + w];
            }
            const float gs = p.s.g_times_scale ? scale : 1.0f;
            if (p.s.dtau != nullptr) atomic_add(p.s.dtau, t * (scale / gs));
            if (p.dbias != nullptr) atomic_add(p.dbias, b / gs);
        }
    }
    XC_DEV bool packs_lines(int, int) const { return false; }
    XC_DEV void pack_lines(f32x16 (&)[4][2], unsigned char*, u32x4 (&)[4][4], int, int) const {}
    template <bool NT = false> XC_DEV void store_lines(const u32x4 (&)[4][4], int, int) const {}
    XC_DEV int with_scratch(f32x16 (&acc)[4][2], int m0, int n0, unsigned char* scratch) {
        if (!sim5_full_tile(p.s, m0, n0)) return 0;                 // (uniform) the edge launch's tile
        to_g(acc, m0, n0);
        return sim5_store_g_lines<STREAM>(acc, gp, m0, n0, scratch);
    }
    // Per logit: one fma (l2), a bare v_exp_f32, an add and a v_rcp_f32, a compare-and-select for the numerator, two multiplies, and
    // an fma and an add for the two sums.  A tile that holds a piece of the positive diagonal (uniform test; O(tiles_m) tiles) saves the
    // row's positive accumulator in front of the row group's arithmetic and replaces that one entry behind it (two small blocks, as
    // Sim5FastGradEpilogue places its diagonal correction: a per-logit select in the one loop would tax every tile).
    XC_DEV void to_g(f32x16 (&acc)[4][2], int m0, int n0) {
        const int lane = threadIdx.x & 63, h = lane >> 5;
        const int wave = uniform(threadIdx.x >> 6), wm = wave >> 2, wn = wave & 3;
        const float scale2 = scale * SIG_LOG2E;
        const bool on_diag = !sim5_off_diagonal(p.s, m0, n0);        // (uniform)
        float dt = 0.f, db = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dl = m0 + wm * 128 + i * 32 + (lane & 31) + p.s.diag_off - (n0 + wn * 64 + 4 * h);
            float rawd = 0.f;
            if (on_diag) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) rawd = (dl == j * 32 + (r & 3) + 8 * (r >> 2)) ? acc[i][j][r] : rawd;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float raw = acc[i][j][r];
                    const float l2 = raw * scale2 + bias2;
                    const float e = fast_exp2(-fabsf(l2));
                    const float g = ((l2 >= 0.f) ? gc : gc * e) * fast_rcp(1.0f + e);
                    dt += g * raw;
                    db += g;
                    acc[i][j][r] = g;
                }
            if (on_diag) {
                const float gp_ = gc * sig_dterm(rawd * scale2 + bias2, true);
                float gold = 0.f;
                bool hit = false;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool sel = dl == j * 32 + (r & 3) + 8 * (r >> 2);
                        gold = sel ? acc[i][j][r] : gold;
                        hit = hit || sel;
                        acc[i][j][r] = sel ? gp_ : acc[i][j][r];
                    }
                dt += hit ? (gp_ - gold) * rawd : 0.f;
                db += hit ? gp_ - gold : 0.f;
            }
            sched_fence();
        }
        dt_acc += dt;
        db_acc += db;
    }
};

// the tiles SigGradEpilogue skips (Sim5EdgeTiles), through the general form on simloss3.h's loop: per-element range and diagonal tests,
// 16-byte row stores, rows of G padded to a whole chunk with zeros
struct SigGradEdgeEpilogue {
    const SigParams& p;
    float dto_acc = 0.f, dts_acc = 0.f, db_acc = 0.f;   // sum one * acc, sum small * acc (x gc scale in finish), sum G
    XC_DEV void finish() {
        const float gcs = (p.s.gmul != nullptr ? *p.s.gmul : 1.0f) * p.coef * sim_scale(p.s);
        const float dt = wave_sum(dto_acc + dts_acc) * gcs, db = wave_sum(db_acc);
        if ((threadIdx.x & 63) == 0) {
            if (p.s.dtau != nullptr) atomic_add(p.s.dtau, dt);
            if (p.dbias != nullptr) atomic_add(p.dbias, db);
        }
    }
    XC_DEV int operator()(f32x16 (&acc)[4][2], int m0, int n0) {
        const SimParams& s = p.s;
        const int lane = threadIdx.x & 63, h = lane >> 5;
        const int wave = uniform(threadIdx.x >> 6), wm = wave >> 2, wn = wave & 3;
        const float scale = sim_scale(s);
        const float scale2 = scale * SIG_LOG2E, bias2 = *p.bias * SIG_LOG2E;
        const float gc = (s.gmul != nullptr ? *s.gmul : 1.0f) * p.coef;
        const float gs = s.g_times_scale ? scale : 1.0f;
        const int nkp = (s.nk + 7) & ~7;                           // G rows are padded to a whole 16-byte chunk with zeros
        bf16_t* G = reinterpret_cast<bf16_t*>(s.G);
        float dto = 0.f, dts = 0.f, db = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 128 + i * 32 + (lane & 31);
            const bool row_ok = gm < s.nq;
            const int dcol = gm + s.diag_off;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nb = n0 + wn * 64 + j * 32;
                uint32_t pk[4][2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int gn = nb + 4 * h + 8 * q + k;
                        const float raw = acc[i][j][4 * q + k];
                        float v = 0.f;
                        if (row_ok && gn < s.nk) {
                            float one, small;
                            sig_dsplit(raw * scale2 + bias2, gn == dcol, one, small);
                            v = gc * sig_dterm(raw * scale2 + bias2, gn == dcol);
                            dto += one * raw;
                            dts += small * raw;
                            db += v;
                        }
                        g[k] = v * gs;
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
        dto_acc += dto;
        dts_acc += dts;
        db_acc += db;
        return 0;
    }
};

template <bool STREAM>
__global__ __launch_bounds__(G2_THREADS, 2) void sig5_grad_kernel(SigParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim5_g_gemm_params(p.s, STREAM);
    const float scale = sim_scale(p.s);
    const float gc = (p.s.gmul != nullptr ? *p.s.gmul : 1.0f) * p.coef * (p.s.g_times_scale ? scale : 1.0f);
    g5_run<false, false, SigGradEpilogue<STREAM>>(g, lds, SigGradEpilogue<STREAM>{p, g, scale, *p.bias * SIG_LOG2E, gc, reinterpret_cast<float*>(lds)});
}
__global__ __launch_bounds__(G2_THREADS, 2) void sig5_grad_edge_kernel(SigParams p) {
    XC_LDS_DYNAMIC(lds);
    const Gemm2Params g = sim3_gemm_params(p.s);
    g3_run<false, false, 0>(g, lds, SigGradEdgeEpilogue{p}, Sim5EdgeTiles{p.s});
}

// the general form (fp32, bf16 with other d, fewer than 128 rows or columns) on sim_grad_kernel's loop
template <typename T>
__global__ __launch_bounds__(256) void sig_grad_kernel(SigParams p) {
    constexpr int VEC = Elem<T>::VEC, LDC = GemmCfg<T>::LDC;
    XC_LDS_DYNAMIC(lds);
    const SimParams& s = p.s;
    const float* Cs = reinterpret_cast<const float*>(lds);
    const int tid = threadIdx.x;
    int m0, n0, tn;
    sim_general_tile<T>(s, lds, m0, n0, tn);
    constexpr int CPR = 128 / VEC;
    T* G = reinterpret_cast<T*>(s.G);
    const float scale = sim_scale(s);
    const float scale2 = scale * SIG_LOG2E, bias2 = *p.bias * SIG_LOG2E;
    const float gc = (s.gmul != nullptr ? *s.gmul : 1.0f) * p.coef;
    const float gs = s.g_times_scale ? scale : 1.0f;
    float dto = 0.f, dts = 0.f, db = 0.f;
    for (int id = tid; id < 128 * CPR; id += GEMM_THREADS) {
        const int row = id / CPR, col = (id % CPR) * VEC;
        const int gm = m0 + row, gn0 = n0 + col;
        if (gm < s.nq && gn0 < s.nk) {                      // G rows are padded to a whole chunk: columns >= nk get 0
            const int dcol = gm + s.diag_off;
            float g[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int gn = gn0 + k;
                const float raw = Cs[row * LDC + col + k];
                float v = 0.f;
                if (gn < s.nk) {
                    float one, small;
                    sig_dsplit(raw * scale2 + bias2, gn == dcol, one, small);
                    v = gc * sig_dterm(raw * scale2 + bias2, gn == dcol);
                    dto += one * raw;
                    dts += small * raw;
                    db += v;
                }
                g[k] = v * gs;
            }
            store_vec<T>(G + (long)gm * s.ldg + gn0, g);
        }
    }
    const float dt = wave_sum(dto + dts) * (gc * scale);
    db = wave_sum(db);
    if (lane_id() == 0) {
        if (s.dtau != nullptr) atomic_add(s.dtau, dt);
        if (p.dbias != nullptr) atomic_add(p.dbias, db);
    }
}

}  // namespace xc
