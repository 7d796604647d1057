// xclip_api.hip -- the extern "C" boundary (include/xclip.h): argument checks, dtype / shape dispatch and kernel
// launches.  No allocation, no synchronisation, no global mutable state besides the thread-local error string.
#include "xc_device.h"

#include "api_common.h"
#include "kernels/colnorm.h"
#include "kernels/filip.h"
#include "kernels/filip5.h"
#include "kernels/gemm.h"
#include "kernels/gemm2.h"
#include "kernels/gemm3.h"
#include "kernels/gemm4.h"
#include "kernels/gemm8.h"
#include "kernels/gemm9.h"
#include "kernels/gemm_small.h"
#include "kernels/optim.h"
#ifdef XCLIP_MEASURE                                             // negative-result experiments, measurement build only (DESIGN_APPENDIX.md 6b)
#include "kernels/measure/gemm6.h"
#include "kernels/measure/gemm7.h"
#endif
#include "kernels/rows.h"
#include "kernels/simloss.h"
#include "kernels/simloss5.h"
#include "kernels/simrank.h"
#include "kernels/simtopk.h"
#include "kernels/sigloss.h"
#include "kernels/vocabce.h"
#include "kernels/sort.h"
#include "kernels/tokens.h"
#include "kernels/embed_packed.h"

using namespace xc;
using namespace xcapi;

namespace xcapi {

thread_local char g_err[512] = "";

int fail(const char* fn, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, what);
    return 1;
}
int check_launch(const char* fn) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: HIP error: %s", fn, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

}  // namespace xcapi

namespace {

// smallest power of two >= ceil(dim / (64 * VEC)), i.e. 16-byte chunks per lane when one wave holds a row
inline int chunks_per_lane(int64_t dim, int vec) {
    const int64_t need = (dim / vec + 63) / 64;
    int c = 1;
    while (c < need) c <<= 1;
    return c;
}

// Non-temporal row accesses, per kernel (bit 1 GEGLU-LayerNorm backward, 2 GEGLU-LayerNorm forward, 4 LayerNorm forward, 8 LayerNorm backward,
// 16 chained forward, 32 chained backward).  Inside the step (profiles/r04_m_kernel_stats_nt{0,63}.txt): GEGLU forward -8 %, GEGLU backward -2 %,
// plain forward / backward / chained backward -1 ... -2 %, chained forward +1 % -- the hint stays off there.  XCLIP_ROWS_NT (measurement build)
// overrides the mask.
constexpr int ROWS_NT = 1 | 2 | 4 | 8 | 32;
inline bool rows_nt_flipped(int bit) { return ((measure_env("XCLIP_ROWS_NT", ROWS_NT) ^ ROWS_NT) & bit) != 0; }

struct LnFwdArgs {                                            // xclip_layernorm_fwd's arguments, in its order
    const void* x; int64_t ldx; const void* g; const void* res; void* y; int64_t ldy; int y_grp;
    float* mean; float* rstd; int rows, dim; float eps; int geglu;
};
template <typename T, int MAXC>
void launch_ln_fwd(const LnFwdArgs& a, hipStream_t st) {
    dim3 grid((a.rows + 3) / 4), block(256);
#ifdef XCLIP_MEASURE
    if constexpr (MAXC <= 2) {
        // measured and not kept (profiles/r03_k_ln_fwd_rows_per_wave.log): several rows per wave with all loads ahead of the reductions
        // (rows.h ln_fwd_rows_kernel; XCLIP_LN_FWD = 1 / 2 / 4 rows per wave).  263 k x 512: 108.7 us with the one-row kernel, 105 / 99 /
        // 117 us; with the residual 137 against 141 / 147 / 168 us; 1.18 M x 1024: 796 (6.1 TB/s) against 904 / 1000 / 1514 us.  The
        // one-row kernel is at the copy ceiling when it runs alone; its lower in-step figure is not a property of the kernel.
        static const int rpw = measure_env("XCLIP_LN_FWD", 0);
        if (!a.geglu && rpw > 0) {
#define XC_LNR(R) { dim3 g2((a.rows + 4 * R - 1) / (4 * R)); hipLaunchKernelGGL((ln_fwd_rows_kernel<T, MAXC, R>), g2, block, 0, st, (const T*)a.x, (long)a.ldx, (const T*)a.g, (const T*)a.res, (T*)a.y, a.mean, a.rstd, a.rows, a.dim, a.eps, (long)a.ldy, a.y_grp); return; }
            if (rpw == 1) XC_LNR(1)
            if (rpw == 4) XC_LNR(4)
            XC_LNR(2)
#undef XC_LNR
        }
    }
#endif
    constexpr bool NTG = (ROWS_NT & 2) != 0, NTP = (ROWS_NT & 4) != 0;
#define XC_LNF(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, 0, st, (const T*)a.x, (long)a.ldx, (const T*)a.g, (const T*)a.res, (T*)a.y, a.mean, a.rstd, a.rows, a.dim, a.eps, (long)a.ldy, a.y_grp)
#ifdef XCLIP_MEASURE
    if constexpr (sizeof(T) == 2 && MAXC <= 4) {
        if (a.geglu && rows_nt_flipped(2)) { XC_LNF((ln_fwd_kernel<T, MAXC, true, !NTG>)); return; }
        if (!a.geglu && rows_nt_flipped(4)) { XC_LNF((ln_fwd_kernel<T, MAXC, false, !NTP>)); return; }
    }
#endif
    if (a.geglu) XC_LNF((ln_fwd_kernel<T, MAXC, true, NTG>));
    else XC_LNF((ln_fwd_kernel<T, MAXC, false, NTP>));
#undef XC_LNF
}
constexpr int LN_BWD_MAX_BLOCKS = 4096;          // MI355X, 263k x 512 rows: 1024 work-groups 180 us, 2048: 189, 4096: 163, 8192: 165
inline int ln_bwd_blocks(int64_t rows) {
    const int64_t b = (rows + 3) / 4;
    return (int)(b > LN_BWD_MAX_BLOCKS ? LN_BWD_MAX_BLOCKS : b);
}
// the GEGLU variant: 80 VGPRs and 20 KB of LDS per work-group = six resident work-groups per CU; the grid is a whole number of such
// rounds (never more than ln_bwd_blocks(rows): the workspace is sized by that)
inline int ln_geglu_bwd_blocks(int64_t rows) {
    const int64_t b = (rows + 1) / 2, cap = ln_bwd_blocks(rows);
    const int per_round = 6 * xc_policy_cus();
    int64_t want = (int64_t)measure_env("XCLIP_LNG_BLOCKS", 2 * per_round);
    if (want > cap) want = cap;
    return (int)(b < want ? (b < 1 ? 1 : b) : want);
}

struct LnBwdArgs {                                            // xclip_layernorm_bwd's operands; dg: the rows of partial gain gradients
    const void* dy; const void* x; int64_t ldx; const void* g; const float* mean; const float* rstd;
    const void* dres; void* dx; int64_t lddx; float* dg; int rows, dim, geglu;
};
template <typename T, int MAXC>
int launch_ln_bwd(const LnBwdArgs& a, hipStream_t st) {
    const int blocks = ln_bwd_blocks(a.rows);
    dim3 grid(blocks), block(256);
    const size_t lds = (size_t)3 * a.dim * sizeof(float);
    constexpr bool NTG = (ROWS_NT & 1) != 0, NTP = (ROWS_NT & 8) != 0;
#define XC_LNB(KERNEL, GRID, LDS) do { XC_ALLOW_LDS((KERNEL), LDS); hipLaunchKernelGGL((KERNEL), GRID, block, LDS, st, (const T*)a.dy, (const T*)a.x, (long)a.ldx, (const T*)a.g, a.mean, a.rstd, (T*)a.dx, (long)a.lddx, a.dg, a.rows, a.dim); } while (0)
#define XC_LNB_RES(KERNEL, GRID, LDS) do { XC_ALLOW_LDS((KERNEL), LDS); hipLaunchKernelGGL((KERNEL), GRID, block, LDS, st, (const T*)a.dy, (const T*)a.x, (long)a.ldx, (const T*)a.g, a.mean, a.rstd, (const T*)a.dres, (T*)a.dx, (long)a.lddx, a.dg, a.rows, a.dim); } while (0)
    if (a.geglu) {
        // rows wider than 3 chunks per lane are shared by two waves (register budget: three waves per SIMD)
        constexpr int SPLIT = (MAXC >= 4 && MAXC % 2 == 0) ? 2 : 1;
        constexpr int C = MAXC / SPLIT;
        const bool split = SPLIT == 2 && (a.dim / Elem<T>::VEC) % 2 == 0;
        // four waves' dg partials of their column part + the row sums + gamma
        const size_t lds2 = ((size_t)4 * (a.dim / (split ? 2 : 1)) + 16) * sizeof(float) + (size_t)a.dim * sizeof(T)
                            + (measure_env("XCLIP_LNG_LDSPAD", 0) && split ? (size_t)2 * a.dim * sizeof(float) : 0);   // what rounds 1-3 requested
        dim3 ggrid(ln_geglu_bwd_blocks(a.rows));
        if (split) {
#ifdef XCLIP_MEASURE
            if (rows_nt_flipped(1)) {
                XC_LNB((ln_geglu_bwd_kernel<T, C, SPLIT, !NTG>), ggrid, lds2);
                return (int)ggrid.x;
            }
#endif
            XC_LNB((ln_geglu_bwd_kernel<T, C, SPLIT, NTG>), ggrid, lds2);
            return (int)ggrid.x;
        } else if (MAXC <= 4) {
            constexpr int C1 = MAXC <= 4 ? MAXC : 1;
            XC_LNB((ln_geglu_bwd_kernel<T, C1, 1, NTG>), ggrid, lds2);
            return (int)ggrid.x;
        } else {                                               // very wide rows with an odd chunk count: the generic two-pass kernel
            XC_LNB_RES((ln_bwd_kernel<T, MAXC, true, NTG>), grid, lds);
        }
    } else {
#ifdef XCLIP_MEASURE
        if constexpr (sizeof(T) == 2 && MAXC <= 2) {
            if (rows_nt_flipped(8)) {
                XC_LNB_RES((ln_bwd_kernel<T, MAXC, false, !NTP>), grid, lds);
                return blocks;
            }
        }
#endif
        XC_LNB_RES((ln_bwd_kernel<T, MAXC, false, NTP>), grid, lds);
    }
#undef XC_LNB
#undef XC_LNB_RES
    return blocks;
}

// dispatch on (dtype, chunks per lane); F is a macro taking (T, MAXC)
#define XC_DISPATCH_ROW(dtype, cpl, F)                                   \
    do {                                                                 \
        if ((dtype) == XCLIP_BF16) {                                     \
            switch (cpl) {                                               \
                case 1: F(bf16_t, 1); break;                             \
                case 2: F(bf16_t, 2); break;                             \
                case 4: F(bf16_t, 4); break;                             \
                case 8: F(bf16_t, 8); break;                             \
                default: return fail(__func__, "row too wide (bf16 rows up to 4096 elements)"); \
            }                                                            \
        } else {                                                         \
            switch (cpl) {                                               \
                case 1: F(float, 1); break;                              \
                case 2: F(float, 2); break;                              \
                case 4: F(float, 4); break;                              \
                case 8: F(float, 8); break;                              \
                case 16: F(float, 16); break;                            \
                default: return fail(__func__, "row too wide (fp32 rows up to 4096 elements)"); \
            }                                                            \
        }                                                                \
    } while (0)

// the three operand layouts in use as template arguments (api_common.h by_dtype): NT (false, false), NN (false, true), TN (true, true);
// (A k-major, B normal) is refused by the entry points and never instantiated
template <typename F> inline void by_layout(int a_kmajor, int b_kmajor, F&& f) {
    if (!a_kmajor && !b_kmajor) f(bool_tag<false>{}, bool_tag<false>{});
    else if (!a_kmajor) f(bool_tag<false>{}, bool_tag<true>{});
    else f(bool_tag<true>{}, bool_tag<true>{});
}

// the generic 128 x 128 kernel (gemm.h): grid.y = K slices, grid.z = problems of a batch
void launch_gemm(const GemmParams& p, int dtype, int a_kmajor, int b_kmajor, int splits, int64_t batch, hipStream_t st) {
    const dim3 grid(p.tiles_m * p.tiles_n, splits, (unsigned)batch), block(GEMM_THREADS);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        by_layout(a_kmajor, b_kmajor, [&](auto ak, auto bk) {
            constexpr bool AK = decltype(ak)::value, BK_ = decltype(bk)::value;
            XC_ALLOW_LDS((gemm_kernel<T, AK, BK_>), GemmCfg<T>::LDS_BYTES);
            hipLaunchKernelGGL((gemm_kernel<T, AK, BK_>), grid, block, GemmCfg<T>::LDS_BYTES, st, p);
        });
    });
}
// the fp32 slabs of a split-K product -> C = alpha * sum (+ residual: the row tail of a product with a skip term)
template <typename T>
void launch_splitk_reduce(const void* slabs, void* C, int64_t ldc, int64_t M, int64_t N, int splits, float alpha, const void* residual,
                          int64_t ldr, hipStream_t st) {
    int64_t blocks = (M * (N / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)slabs, (T*)C, (long)ldc, (int)M, (int)N,
                       splits, alpha, (const T*)residual, (long)ldr);
}

// Which bf16 GEMM runs.  Product (0): g5_run (A in a ring of three LDS stages) for the layouts whose B operand is a weight panel that
// lives in L2 -- forward (NT) and dgrad (NN): +2 ... +6 % there -- and g4_run for wgrad (TN), where BOTH operands stream from HBM and
// the deeper A ring measured 3-11 % SLOWER (profiles/r02_run5_gemm5_ring_probe.log).  Measurement build only (XCLIP_GEMM, read once;
// A/B runs): 2 = gemm2.h (two-phase), 3 = gemm3.h (first scheduled kernel), 4 = g4_run everywhere, 5 = g5_run everywhere, 6 / 7 = the
// experiments under kernels/measure/.
inline int gemm_generation() {
    static const int v = [] { const int e = measure_env("XCLIP_GEMM", 0); return (e >= 2 && e <= 7) ? e : 0; }();
    return v;
}
// gemm8.h on / off.  Product: G8_DEFAULT.  Measurement build: XCLIP_GEMM8=0 / 1 at load, xclip_measure_gemm8() at run time (same-process A/B).
constexpr int G8_DEFAULT = 1;
static int g_gemm8 = -1;
inline bool gemm8_on() {
    if (g_gemm8 < 0) g_gemm8 = measure_env("XCLIP_GEMM8", G8_DEFAULT);
    return XC_ASM_UNITS && g_gemm8 != 0;
}
template <bool AK, bool BK_, int MODE>
void launch_gemm4(const Gemm2Params& p, dim3 pgrid, bool ring3, hipStream_t st) {
#ifdef XCLIP_MEASURE
    if constexpr (!AK && !BK_ && MODE == G4_PLAIN) {             // measurement: XCLIP_GEMM5_ABL=<mask> (gemm4.h g5_run), NT plain only
        static const int abl = measure_env("XCLIP_GEMM5_ABL", 0);
        if (ring3 && abl) {
#define XC_ABL5(N) case N: XC_ALLOW_LDS((gemm5_kernel<false, false, G4_PLAIN, N>), G5_LDS_BYTES); hipLaunchKernelGGL((gemm5_kernel<false, false, G4_PLAIN, N>), pgrid, dim3(G2_THREADS), G5_LDS_BYTES, st, p); return;
            switch (abl) { XC_ABL5(1) XC_ABL5(2) XC_ABL5(4) XC_ABL5(8) XC_ABL5(9) XC_ABL5(10) XC_ABL5(11) XC_ABL5(14) XC_ABL5(16) XC_ABL5(32) XC_ABL5(48) XC_ABL5(12) XC_ABL5(6) XC_ABL5(26) XC_ABL5(58) XC_ABL5(64) XC_ABL5(74) XC_ABL5(128) XC_ABL5(256) XC_ABL5(512) XC_ABL5(1024) XC_ABL5(2560) XC_ABL5(4096) XC_ABL5(8192) XC_ABL5(526) XC_ABL5(522) default: break; }
#undef XC_ABL5
        }
    }
#endif
#ifdef XCLIP_MEASURE
    constexpr bool both = true;                                   // every layout on either loop (XCLIP_GEMM=4 / 5)
#else
    constexpr bool both = false;                                  // the product carries one loop per layout: ring for NT / NN, two-stage for TN
    (void)ring3;
#endif
    if constexpr (both || !AK) {
        if (both ? ring3 : true) {
            XC_ALLOW_LDS((gemm5_kernel<AK, BK_, MODE>), G5_LDS_BYTES);
            hipLaunchKernelGGL((gemm5_kernel<AK, BK_, MODE>), pgrid, dim3(G2_THREADS), G5_LDS_BYTES, st, p);
            return;
        }
    }
    if constexpr (both || AK) {
        XC_ALLOW_LDS((gemm4_kernel<AK, BK_, MODE>), G5_LDS_BYTES);   // two stages + 32 KiB of epilogue scratch (gemm4.h g4_run)
        hipLaunchKernelGGL((gemm4_kernel<AK, BK_, MODE>), pgrid, dim3(G2_THREADS), G5_LDS_BYTES, st, p);
    }
}
template <bool AK, bool BK_>
void launch_gemm2(const Gemm2Params& p, int splits, hipStream_t st) {
    dim3 grid(p.tiles_m * p.tiles_n, splits), block(G2_THREADS);
    const int gen = gemm_generation();
#ifdef XCLIP_MEASURE
    if (gen == 2) {
        XC_ALLOW_LDS((gemm2_kernel<AK, BK_>), G2_LDS_BYTES);
        hipLaunchKernelGGL((gemm2_kernel<AK, BK_>), grid, block, G2_LDS_BYTES, st, p);
        return;
    }
#endif
    // persistent: one work-group per CU walks the tiles (split-K problems are sized to ~one tile per work-group already)
    int gx = p.tiles_m * p.tiles_n;
    const int cus = xc_num_cus();
    if (gx * splits > cus && splits == 1) gx = gx < cus ? gx : cus;
    dim3 pgrid(gx, splits);
    // 32-bit in-tile byte offsets: leading dimensions below 2^22 elements (anything else is not a Linear of this model)
    const bool small_ld = p.lda < (1L << 22) && p.ldb < (1L << 22) && p.ldc < (1L << 22) && (long)p.N < (1L << 21);
    if (gen != 3 && small_ld) {
        const bool ring3 = gen == 5 || ((gen == 0 || gen >= 6) && !AK);   // (6, 7: gemm6.h / gemm7.h for the shapes they take, the default otherwise)
        // split-K on the two-stage loop (the weight gradients): a 1-D grid whose work-groups place themselves so that an XCD holds whole
        // K slices (gemm2.h g2_where); XCLIP_GEMM_SPLIT2D=1 (measurement build) keeps the (tile, slice) grid for the A/B
        static const int split2d = measure_env("XCLIP_GEMM_SPLIT2D", 0);
        if (splits > 1 && !ring3 && !split2d) {
            Gemm2Params q = p;
            q.split_lin = splits;
            const dim3 lgrid((unsigned)(8 * ((gx * splits + 7) / 8)), 1);
            if (q.partial != nullptr) launch_gemm4<AK, BK_, G4_SLAB>(q, lgrid, ring3, st);
            else launch_gemm4<AK, BK_, G4_PLAIN>(q, lgrid, ring3, st);
            return;
        }
        const bool terms = p.bias != nullptr || p.residual != nullptr || p.addrows != nullptr;
#ifdef XCLIP_MEASURE
        // experiment (XCLIP_GEMM=7): four waves of 128 x 128 per tile, one per SIMD (measure/gemm7.h)
        if (gen == 7 && !AK && !BK_ && !terms && p.partial == nullptr && splits == 1 && p.M % G2_BM == 0 && p.N % G2_BN == 0 && p.K / G2_BK >= 2) {
            XC_ALLOW_LDS(gemm7_kernel, G5_LDS_BYTES);
            hipLaunchKernelGGL(gemm7_kernel, pgrid, dim3(G7_THREADS), G5_LDS_BYTES, st, p);
            return;
        }
        // experiment (XCLIP_GEMM=6, XCLIP_GEMM6_MAXK=<K>): two 4-wave work-groups per CU on 256 x 128 tiles for the short-K forward products
        // whose tiles are all interior (gemm6.h)
        if (gen == 6 && !AK && !BK_ && !terms && p.partial == nullptr && splits == 1 && p.M % G6_BM == 0 && p.N % G6_BN == 0 &&
            p.K % G6_BK == 0 && p.K / G6_BK >= 4) {
            static const int maxk = measure_env("XCLIP_GEMM6_MAXK", 1024);
            if (p.K <= maxk) {
                const int tiles6 = (p.M / G6_BM) * (p.N / G6_BN);
                const int g6 = tiles6 < 2 * cus ? tiles6 : 2 * cus;
                XC_ALLOW_LDS(gemm6_kernel, G6_LDS_BYTES);
                hipLaunchKernelGGL(gemm6_kernel, dim3((unsigned)g6), dim3(G6_THREADS), G6_LDS_BYTES, st, p);
                return;
            }
        }
#endif
        // the hand-scheduled ring kernel (gemm8.h) for the plain interior products it takes
        if constexpr (!AK) {
            if (gemm8_on() && g8_takes(p, splits, gx)) {
#define XC_G8(V) do { XC_ALLOW_LDS((gemm8_kernel<BK_, V>), G5_LDS_BYTES); hipLaunchKernelGGL((gemm8_kernel<BK_, V>), dim3((unsigned)gx), dim3(G2_THREADS), G5_LDS_BYTES, st, p); } while (0)
#ifdef XCLIP_MEASURE
                switch (g_gemm8) { case 2: XC_G8(2); return; case 3: XC_G8(3); return; case 4: XC_G8(4); return; case 5: XC_G8(5); return; case 6: XC_G8(6); return; case 10: XC_G8(0); return; case 11: XC_G8(1); return; default: break; }
#endif
                if (p.stream_out) XC_G8(1); else XC_G8(0);
#undef XC_G8
                return;
            }
        }
        const bool res_only = p.residual != nullptr && p.bias == nullptr && p.addrows == nullptr && p.ldr < (1L << 22);
        if (p.partial != nullptr) launch_gemm4<AK, BK_, G4_SLAB>(p, pgrid, ring3, st);
        else if (res_only) launch_gemm4<AK, BK_, G4_RES>(p, pgrid, ring3, st);
        else if (terms) launch_gemm4<AK, BK_, G4_TERMS>(p, pgrid, ring3, st);
        else launch_gemm4<AK, BK_, G4_PLAIN>(p, pgrid, ring3, st);
        return;
    }
#ifdef XCLIP_MEASURE
    static const int abl = measure_env("XCLIP_GEMM_ABL", 0);
    if (abl != 0 && !AK && !BK_) {                      // measurement-only variants of the NT kernel
#define XC_ABL(N) case N: XC_ALLOW_LDS((gemm3_kernel<false, false, N>), G3_LDS_BYTES); hipLaunchKernelGGL((gemm3_kernel<false, false, N>), pgrid, block, G3_LDS_BYTES, st, p); return;
        switch (abl) { XC_ABL(1) XC_ABL(2) XC_ABL(4) XC_ABL(8) XC_ABL(3) XC_ABL(9) XC_ABL(10) XC_ABL(11) XC_ABL(14) XC_ABL(15) XC_ABL(25) XC_ABL(41) XC_ABL(64) XC_ABL(73) XC_ABL(105) default: break; }
#undef XC_ABL
    }
#endif
    XC_ALLOW_LDS((gemm3_kernel<AK, BK_>), G3_LDS_BYTES);
    hipLaunchKernelGGL((gemm3_kernel<AK, BK_>), pgrid, block, G3_LDS_BYTES, st, p);
}

// the 256x256 DMA-staged kernel (gemm2.h) takes every bf16 problem whose contraction is a multiple of its K step and
// whose output is at least a tile wide; everything else (fp32, ragged K, tiny outputs) goes to the 128x128 kernel
inline bool use_gemm2(int64_t M, int64_t N, int64_t K, int dtype) {
    return dtype == XCLIP_BF16 && K % G2_BK == 0 && M >= 128 && N >= 128 && M % 8 == 0;
}
int gemm2_splits(int64_t M, int64_t N, int64_t K) {
    const int64_t tiles = ((M + G2_BM - 1) / G2_BM) * ((N + G2_BN - 1) / G2_BN);
    int64_t s = xc_policy_cus() / tiles;                      // one 8-wave work-group per CU: enough K slices to fill the part that runs it
    static const int force = measure_env("XCLIP_GEMM_SPLITS", 0);     // (measurement build: a fixed slice count, for the sweep)
    if (force > 0) s = force;
    const int64_t maxs = K / (4 * G2_BK);
    if (s > maxs) s = maxs;
    if (s > 64) s = 64;
    return s < 2 ? 1 : (int)s;
}

// ---- the row tail of a persistent GEMM ------------------------------------------------------------------------------------------------
// One work-group per CU walks tiles_m x tiles_n tiles: the launch takes ceil(tiles / CUs) rounds of one tile time each, and a last round
// that fills a few CUs costs as much as a full one.  The text tower's rows are batch x 257 (the CLS token): 263,168 rows = 1028 row tiles,
// x 2 column tiles (every N = 512 product: out-projection, FF2, the QKV / FF1 input gradients) = 2056 tiles = 8 rounds + 8 tiles -- a NINTH
// round for 3 % of a round's work, 12 % of the launch (115 us of the FF1 input gradient's 940); the vision tower's 33,792 rows are
// 132 row tiles: 264 tiles = TWO rounds for 1.03.  So the rows are cut at the last whole round: the main launch takes `main_rows`, and the
// few row tiles behind it become a split-K problem of their own that fills the part for a few K steps -- fp32 slabs + the reduction
// (which also adds the skip term of an FF2 forward).  Worth it when a tile is long (>= 16 K steps) and the tail small (<= half a round).
// -> rows of the main launch (a multiple of the tile), 0 = no cut
int64_t gemm2_tail_cut(int64_t M, int64_t N, int64_t K) {
    static const int on = measure_env("XCLIP_GEMM_TAIL", 1);   // (measurement build: 0 = the uncut launch, for the A/B)
    if (!on) return 0;
    const int64_t cus = xc_policy_cus();
    const int64_t tm = (M + G2_BM - 1) / G2_BM, tn = (N + G2_BN - 1) / G2_BN, tiles = tm * tn;
    const int64_t rounds = tiles / cus;
    if (rounds < 1 || tiles % cus == 0 || K / G2_BK < 16 || M % 8 != 0) return 0;
    const int64_t tm_main = rounds * cus / tn;                 // the most row tiles `rounds` rounds can hold
    const int64_t tail_tiles = tiles - tm_main * tn;
    if (tm_main < 1 || tail_tiles * 2 > cus || M - tm_main * G2_BM < 128) return 0;      // (a tail the 256 x 256 kernels would not take)
    return tm_main * G2_BM;
}

// split-K policy shared by xclip_gemm and xclip_gemm_workspace_bytes: fill ~512 work-groups, keep >= 4 K steps each
int gemm_splits(int64_t M, int64_t N, int64_t K, int dtype) {
    const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
    const int bk = 8 * vec_of(dtype);
    int64_t s = 2 * xc_policy_cus() / tiles;                    // two 4-wave work-groups per CU
    const int64_t maxs = K / (4 * bk);
    if (s > maxs) s = maxs;
    if (s > 64) s = 64;
    return s < 2 ? 1 : (int)s;
}

// ---- one plan per product: xclip_gemm executes it, xclip_gemm_workspace_bytes reports its bytes ----------------------------------------
struct GemmArgs {                                             // xclip_gemm's arguments, in its order
    int a_kmajor, b_kmajor;
    const void* A; int64_t lda; const void* B; int64_t ldb; void* C; int64_t ldc;
    int64_t M, N, K; float alpha;
    const void* bias; const void* residual; int64_t ldr; const void* addrows; const int32_t* rowidx; int64_t ld_add;
    void* workspace; int64_t workspace_bytes;
};
enum GemmRoute { GEMM_SMALL, GEMM_256, GEMM_256_CUT, GEMM_GENERIC };   // gemm_small.h; gemm2.h ... gemm8.h (launch_gemm2); the same, row tail cut; gemm.h
struct GemmPlan {
    GemmRoute route;
    int splits, k_per_split;             // K slices (no empty ones) and their length; GEMM_256_CUT: of the tail (its main rows take one slice)
    int64_t main_rows, tail_rows;        // GEMM_256_CUT: rows of the main launch, rows of the split-K tail behind it
    int64_t workspace_bytes;             // the fp32 slabs the route wants; offered less, the product runs in one slice (and uncut)
};
// K in slices of whole `bk` steps: rounding the slice up can leave the last slices EMPTY (96 K steps over 17 slices -> 6 per slice, 16 slices
// cover them): a slice without work returns without touching its slab and the reduction would add whatever the workspace held before
inline void gemm_slices(GemmPlan& p, int s, int64_t K, int bk) {
    p.k_per_split = K > 0 ? (int)((((K + s - 1) / s) + bk - 1) / bk * bk) : 0;   // (K <= 0: the size query of a shape xclip_gemm refuses --
    p.splits = K > 0 ? (int)((K + p.k_per_split - 1) / p.k_per_split) : 1;       //  one slice of nothing)
}
// offer: the bytes of workspace at hand (0 without one); small_flop: the limit of the 64 x 64 kernel (xclip_gemm_small_limit)
GemmPlan gemm_plan(const GemmArgs& g, int dtype, int64_t offer, int64_t small_flop) {
    const int64_t M = g.M, N = g.N, K = g.K;
    const bool bias_or_rows = g.bias != nullptr || g.addrows != nullptr, plain = !bias_or_rows && g.residual == nullptr;
    GemmPlan p{};                                             // (route GEMM_SMALL)
    if (dtype == XCLIP_BF16 && gs_takes(M, N, K, bias_or_rows, g.lda, g.ldb, small_flop)) return p;      // GEMM_SMALL, no workspace
    const bool g2 = use_gemm2(M, N, K, dtype);
    p.route = g2 ? GEMM_256 : GEMM_GENERIC;
    const int bk = g2 ? G2_BK : 8 * vec_of(dtype);
    // the row tail as a split-K problem of its own (gemm2_tail_cut): normal-A layouts, no bias / gathered rows (the reduction adds the skip term)
    const int64_t cut = (g2 && !g.a_kmajor && !bias_or_rows) ? gemm2_tail_cut(M, N, K) : 0;
    if (cut > 0) {
        const int ts = gemm2_splits(M - cut, N, K);
        p.workspace_bytes = (int64_t)ts * (M - cut) * N * 4;
        if (ts > 1 && offer >= p.workspace_bytes) {
            gemm_slices(p, ts, K, bk);
            if (p.splits > 1) {                                 // (always: ts slices of >= 4 K steps each stay >= 2 after the rounding)
                p.route = GEMM_256_CUT;
                p.main_rows = cut; p.tail_rows = M - cut;
                return p;
            }
        }
    }
    int s = g2 ? gemm2_splits(M, N, K) : gemm_splits(M, N, K, dtype);
    if (cut == 0) p.workspace_bytes = s > 1 ? (int64_t)s * M * N * 4 : 0;
    if (s > 1 && (!plain || offer < (int64_t)s * M * N * 4)) s = 1;       // a short or missing workspace: one slice
    gemm_slices(p, s, K, bk);
    return p;
}

}  // namespace

extern "C" {

int xclip_abi_version(void) { return XCLIP_ABI_VERSION; }
const char* xclip_last_error(void) { return g_err; }
#ifndef XCLIP_BUILD_TOOLCHAIN
#define XCLIP_BUILD_TOOLCHAIN "unknown toolchain"
#endif
const char* xclip_build_info(void) { return XCLIP_BUILD_TOOLCHAIN; }

int xclip_layernorm_fwd(const void* x, int64_t ldx, const void* g, const void* res, void* y, int64_t ldy, int64_t y_grp,
                        float* mean, float* rstd, int64_t rows, int64_t dim, float eps, int geglu, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec == 0 && ldx % vec == 0, "dim / ldx must be multiples of the 16-byte chunk");
    XC_REQUIRE(ldx >= (geglu ? 2 * dim : dim), "ldx too small");
    XC_REQUIRE(ldy >= dim && ldy % vec == 0 && y_grp >= 0, "ldy must cover a row, chunk aligned; y_grp >= 0");
    XC_REQUIRE(aligned16(x) && aligned16(g) && aligned16(y) && aligned16(res), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    const LnFwdArgs a{x, ldx, g, res, y, ldy, (int)y_grp, mean, rstd, (int)rows, (int)dim, eps, geglu};
#define F(T, C) launch_ln_fwd<T, C>(a, (hipStream_t)stream)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int64_t xclip_layernorm_bwd_workspace_bytes(int64_t rows, int64_t dim) { return (int64_t)ln_bwd_blocks(rows) * dim * 4; }

int xclip_layernorm_bwd(const void* dy, const void* x, int64_t ldx, const void* g, const float* mean, const float* rstd,
                        const void* dres, void* dx, int64_t lddx, float* dg_accum, void* workspace, int64_t workspace_bytes,
                        int64_t rows, int64_t dim, int geglu, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec == 0 && ldx % vec == 0 && lddx % vec == 0, "dims must be multiples of the 16-byte chunk");
    XC_REQUIRE(ldx >= (geglu ? 2 * dim : dim) && lddx >= (geglu ? 2 * dim : dim), "leading dimension too small");
    XC_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(g) && aligned16(dx) && aligned16(dres), "pointers must be 16-byte aligned");
    XC_REQUIRE(!(geglu && dres != nullptr), "dres is not defined for the GEGLU variant");
    XC_REQUIRE(workspace != nullptr && workspace_bytes >= xclip_layernorm_bwd_workspace_bytes(rows, dim) && aligned16(workspace),
               "workspace of xclip_layernorm_bwd_workspace_bytes(rows, dim) bytes required");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    float* partial = (float*)workspace;
    int nblk = 0;                                              // rows of dg partials the kernel wrote
    const LnBwdArgs a{dy, x, ldx, g, mean, rstd, dres, dx, lddx, partial, (int)rows, (int)dim, geglu};
#define F(T, C) nblk = launch_ln_bwd<T, C>(a, (hipStream_t)stream)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    int slices = nblk / 64;
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((dim + 63) / 64), (unsigned)slices), dim3(256), 1024, (hipStream_t)stream,
                       (const float*)partial, (long)dim, dg_accum, nblk, (int)dim);
    return check_launch(__func__);
}

int xclip_layernorm_bwd_ffnstats(const void* dy, const void* x, int64_t ldx, const void* g, const float* mean, const float* rstd,
                                 const void* dres, void* dx, int64_t lddx, float* dg_accum, void* workspace, int64_t workspace_bytes,
                                 int64_t rows, int64_t dim, const void* x1_below, int64_t ld1, const float* wg, const float* mean4,
                                 const float* rstd4, float inv_f, float* rowc, int dtype, void* stream) {
    XC_REQUIRE(dtype == XCLIP_BF16, "bf16 only (the fused feed-forward backward the row constants feed)");
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % 8 == 0 && ldx % 8 == 0 && lddx % 8 == 0 && ld1 % 8 == 0, "dims must be multiples of the 16-byte chunk");
    XC_REQUIRE(ldx >= dim && lddx >= dim && ld1 >= dim, "leading dimension too small");
    XC_REQUIRE(dy && x && g && mean && rstd && dx && dg_accum && x1_below && wg && mean4 && rstd4 && rowc, "null pointer");
    XC_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(g) && aligned16(dx) && aligned16(dres) && aligned16(x1_below) && aligned16(wg) && aligned16(rowc),
               "pointers must be 16-byte aligned");
    XC_REQUIRE(workspace != nullptr && workspace_bytes >= xclip_layernorm_bwd_workspace_bytes(rows, dim) && aligned16(workspace),
               "workspace of xclip_layernorm_bwd_workspace_bytes(rows, dim) bytes required");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, 8);
    XC_REQUIRE(cpl == 1 || cpl == 2 || cpl == 4 || cpl == 8, "row too wide (bf16 rows up to 4096 elements)");
    float* partial = (float*)workspace;
    const int blocks = ln_bwd_blocks(rows);
    const size_t lds = (size_t)3 * dim * sizeof(float);
    constexpr bool NTP = (ROWS_NT & 8) != 0;
    const LnFfnStats fs{x1_below, (long)ld1, wg, mean4, rstd4, inv_f, rowc};
    hipStream_t st = (hipStream_t)stream;
#define XC_LNF(C) do { XC_ALLOW_LDS((ln_bwd_kernel<bf16_t, C, false, NTP, true>), lds); \
        hipLaunchKernelGGL((ln_bwd_kernel<bf16_t, C, false, NTP, true>), dim3((unsigned)blocks), dim3(256), lds, st, (const bf16_t*)dy, (const bf16_t*)x, (long)ldx, \
                           (const bf16_t*)g, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, (long)lddx, partial, (int)rows, (int)dim, fs); } while (0)
    switch (cpl) { case 1: XC_LNF(1); break; case 2: XC_LNF(2); break; case 4: XC_LNF(4); break; default: XC_LNF(8); break; }
#undef XC_LNF
    int slices = blocks / 64;
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((dim + 63) / 64), (unsigned)slices), dim3(256), 1024, st, (const float*)partial, (long)dim, dg_accum,
                       blocks, (int)dim);
    return check_launch(__func__);
}

int xclip_layernorm_chain_fwd(const void* p, const void* g1, const void* res, void* x1, float* mean1, float* rstd1, const void* g2,
                              void* h2, float* mean2, float* rstd2, int64_t rows, int64_t dim, float eps, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(p && g1 && res && x1 && g2 && h2 && mean1 && rstd1 && mean2 && rstd2, "null pointer");
    XC_REQUIRE(aligned16(p) && aligned16(g1) && aligned16(res) && aligned16(x1) && aligned16(g2) && aligned16(h2), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    constexpr bool NTC = (ROWS_NT & 16) != 0;
#ifdef XCLIP_MEASURE
    if (dtype == XCLIP_BF16 && cpl == 1 && rows_nt_flipped(16)) {
        hipLaunchKernelGGL((ln_chain_fwd_kernel<bf16_t, 1, !NTC>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)p, (const bf16_t*)g1, (const bf16_t*)res, (bf16_t*)x1, mean1, rstd1, (const bf16_t*)g2, (bf16_t*)h2, mean2, rstd2, (int)rows, (int)dim, eps);
        return check_launch(__func__);
    }
#endif
#define F(T, C) hipLaunchKernelGGL((ln_chain_fwd_kernel<T, C, NTC>), grid, block, 0, (hipStream_t)stream, (const T*)p, (const T*)g1, (const T*)res, (T*)x1, mean1, rstd1, (const T*)g2, (T*)h2, mean2, rstd2, (int)rows, (int)dim, eps)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int64_t xclip_layernorm_chain_bwd_workspace_bytes(int64_t rows, int64_t dim) { return (int64_t)ln_bwd_blocks(rows) * 2 * dim * 4; }

int xclip_layernorm_chain_bwd(const void* dh2, const void* x1, const void* g2, const float* mean2, const float* rstd2, const void* dres,
                              void* dx1, const void* p, const void* g1, const float* mean1, const float* rstd1, void* dp, float* dg2_accum,
                              float* dg1_accum, void* workspace, int64_t workspace_bytes, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(dh2 && x1 && g2 && mean2 && rstd2 && dres && dx1 && p && g1 && mean1 && rstd1 && dp && dg2_accum && dg1_accum, "null pointer");
    XC_REQUIRE(aligned16(dh2) && aligned16(x1) && aligned16(dres) && aligned16(dx1) && aligned16(p) && aligned16(dp) && aligned16(g1) && aligned16(g2),
               "pointers must be 16-byte aligned");
    XC_REQUIRE(workspace != nullptr && workspace_bytes >= xclip_layernorm_chain_bwd_workspace_bytes(rows, dim), "workspace too small");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    const int nblk = ln_bwd_blocks(rows);
    dim3 grid((unsigned)nblk), block(256);
    float* partial = (float*)workspace;
    const size_t lds = (size_t)6 * dim * sizeof(float);
    constexpr bool NTC = (ROWS_NT & 32) != 0;
#ifdef XCLIP_MEASURE
    if (dtype == XCLIP_BF16 && cpl == 1 && rows_nt_flipped(32)) {
        XC_ALLOW_LDS((ln_chain_bwd_kernel<bf16_t, 1, !NTC>), lds);
        hipLaunchKernelGGL((ln_chain_bwd_kernel<bf16_t, 1, !NTC>), grid, block, lds, (hipStream_t)stream, (const bf16_t*)dh2, (const bf16_t*)x1, (const bf16_t*)g2, mean2, rstd2, (const bf16_t*)dres, (bf16_t*)dx1, (const bf16_t*)p, (const bf16_t*)g1, mean1, rstd1, (bf16_t*)dp, partial, (int)rows, (int)dim);
    } else
#endif
#define F(T, C) do { XC_ALLOW_LDS((ln_chain_bwd_kernel<T, C, NTC>), lds); hipLaunchKernelGGL((ln_chain_bwd_kernel<T, C, NTC>), grid, block, lds, (hipStream_t)stream, (const T*)dh2, (const T*)x1, (const T*)g2, mean2, rstd2, (const T*)dres, (T*)dx1, (const T*)p, (const T*)g1, mean1, rstd1, (T*)dp, partial, (int)rows, (int)dim); } while (0)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    int slices = nblk / 64;
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL(colsum_fold2_kernel, dim3((unsigned)((dim + 63) / 64), (unsigned)slices, 2), dim3(256), 1024, (hipStream_t)stream,
                       (const float*)partial, dg2_accum, dg1_accum, nblk, (int)dim);      // both gains' partials in one launch
    return check_launch(__func__);
}

int xclip_l2norm_fwd(const void* x, void* y, float* rnorm, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(aligned16(x) && aligned16(y), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define F(T, C) hipLaunchKernelGGL((l2norm_fwd_kernel<T, C>), grid, block, 0, (hipStream_t)stream, (const T*)x, (T*)y, rnorm, (int)rows, (int)dim)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int xclip_l2norm_bwd(const void* dy, const void* y, const float* rnorm, void* dx, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(dx), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define F(T, C) hipLaunchKernelGGL((l2norm_bwd_kernel<T, C>), grid, block, 0, (hipStream_t)stream, (const T*)dy, (const T*)y, rnorm, (T*)dx, (int)rows, (int)dim)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int xclip_text_embed_fwd(const int64_t* tokens, const void* E, const void* P, const void* cls, void* out, int64_t batch,
                         int64_t n, int64_t dim, int64_t vocab, int32_t* bad_token_flag, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(vocab > 0, "vocab (rows of the embedding table) must be positive");
    XC_REQUIRE(dim > 0 && dim % vec_of(dtype) == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(aligned16(E) && aligned16(P) && aligned16(cls) && aligned16(out), "pointers must be 16-byte aligned");
    const int64_t rows = batch * (n + (cls ? 1 : 0));
    if (rows == 0) return 0;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((text_embed_fwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const long long*)tokens,
                           (const T*)E, (const T*)P, (const T*)cls, (T*)out, (int)batch, (int)n, (int)dim,
                           (long long)vocab, bad_token_flag);
    });
    return check_launch(__func__);
}

int xclip_text_embed_bwd(const void* dout, const int64_t* tokens, float* dE_accum, float* dP_accum, float* dcls_accum,
                         int64_t batch, int64_t n, int64_t dim, int64_t vocab, int has_cls, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(aligned16(dout), "pointers must be 16-byte aligned");
    XC_REQUIRE(has_cls == 0 || dcls_accum != nullptr, "dcls_accum required with a CLS row");
    if (batch == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    int ysplit = (int)((batch + 31) / 32);
    if (ysplit > 16) ysplit = 16;
    dim3 grid((unsigned)(n + (has_cls ? 1 : 0)), ysplit), block(256);
    const size_t red_bytes = (size_t)3 * dim * sizeof(float);
#define F(T, C) hipLaunchKernelGGL((text_embed_bwd_kernel<T, C>), grid, block, red_bytes, (hipStream_t)stream, (const T*)dout, (const long long*)tokens, dE_accum, dP_accum, dcls_accum, (int)batch, (int)n, (int)dim, has_cls ? 1 : 0, (long long)vocab)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int xclip_text_embed_packed_fwd(const int64_t* tok, const int32_t* pos, const void* E, const void* P, const void* cls, void* out,
                                int64_t rows, int64_t dim, int64_t vocab, int64_t npos, int32_t* bad_token_flag, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(vocab > 0 && rows >= 0 && npos >= 0, "vocab must be positive, rows and npos non-negative");
    XC_REQUIRE(dim > 0 && dim % vec_of(dtype) == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(aligned16(E) && aligned16(P) && aligned16(cls) && aligned16(out), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    XC_REQUIRE(tok && pos && E && out, "null pointer");
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((text_embed_packed_fwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const long long*)tok, (const int*)pos,
                           (const T*)E, (const T*)P, (const T*)cls, (T*)out, (long)rows, (int)dim, (long long)vocab, (int)npos, bad_token_flag);
    });
    return check_launch(__func__);
}

int xclip_text_embed_packed_bwd(const void* dout, const int32_t* cu, float* dcls_accum, int64_t batch, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(dout && cu && dcls_accum && aligned16(dout), "pointers must be non-null, dout 16-byte aligned");
    if (batch <= 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    int split = (int)((batch + 31) / 32);
    if (split > 16) split = 16;
    dim3 grid((unsigned)split), block(256);
    const size_t red_bytes = (size_t)3 * dim * sizeof(float);
#define F(T, C) hipLaunchKernelGGL((text_embed_packed_dcls_kernel<T, C>), grid, block, red_bytes, (hipStream_t)stream, (const T*)dout, (const int*)cu, dcls_accum, (int)batch, (int)dim)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int xclip_patchify(const void* image, const int32_t* keep, void* out, int64_t ldo, int64_t batch, int64_t channels,
                   int64_t height, int64_t width, int64_t patch, int64_t nkeep, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(patch > 0 && height % patch == 0 && width % patch == 0, "image must be divisible by the patch size");
    XC_REQUIRE(ldo % vec_of(dtype) == 0 && ldo >= patch * patch * channels, "ldo must cover a patch row, chunk aligned");
    XC_REQUIRE(aligned16(out), "pointers must be 16-byte aligned");
    const int64_t total = batch * nkeep * (ldo / vec_of(dtype));
    if (total == 0) return 0;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    dim3 grid((unsigned)blocks), block(256);
    // three bf16 channels, patch edge and image width multiples of 8, no padding behind a row: whole 16-byte pieces in and out
    static const int rgb8 = measure_env("XCLIP_PATCHIFY_RGB8", 1);     // (measurement build: 0 = the element-wise kernel, for the A/B)
    if (rgb8 && dtype == XCLIP_BF16 && channels == 3 && patch % 8 == 0 && width % 8 == 0 && ldo == patch * patch * 3 && aligned16(image)) {
        int64_t b8 = (batch * nkeep * patch * (patch / 8) + 255) / 256;
        if (b8 > 16384) b8 = 16384;
        hipLaunchKernelGGL(patchify_rgb8_kernel, dim3((unsigned)b8), block, 0, (hipStream_t)stream, (const bf16_t*)image, (const int*)keep,
                           (bf16_t*)out, (long)ldo, (int)batch, (int)height, (int)width, (int)patch, (int)nkeep);
        return check_launch(__func__);
    }
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((patchify_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)image, (const int*)keep, (T*)out, (long)ldo, (int)batch, (int)channels, (int)height, (int)width, (int)patch, (int)nkeep);
    });
    return check_launch(__func__);
}

int xclip_token_mean_fwd(const void* x, int64_t x_batch_stride, void* out, int64_t batch, int64_t n, int64_t dim, int dtype,
                         void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && n > 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(x_batch_stride >= n * dim && x_batch_stride % vec == 0, "batch stride must cover n rows, chunk aligned");
    XC_REQUIRE(aligned16(x) && aligned16(out), "pointers must be 16-byte aligned");
    if (batch == 0) return 0;
    dim3 grid((unsigned)batch, (unsigned)((dim / vec + 63) / 64)), block(64);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((token_mean_fwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, (long)x_batch_stride, (T*)out, (int)n, (int)dim);
    });
    return check_launch(__func__);
}

int xclip_token_mean_bwd(const void* dout, const void* dsrc, int64_t src_batch_stride, void* dx, int64_t batch, int64_t n,
                         int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && n > 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQUIRE(dsrc == nullptr || (src_batch_stride >= n * dim && src_batch_stride % vec == 0), "bad source batch stride");
    XC_REQUIRE(aligned16(dout) && aligned16(dx) && aligned16(dsrc), "pointers must be 16-byte aligned");
    if (batch == 0) return 0;
    dim3 grid((unsigned)((batch * n + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((token_mean_bwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)dout, (const T*)dsrc, (long)src_batch_stride, (T*)dx, (int)batch, (int)n, (int)dim);
    });
    return check_launch(__func__);
}

int xclip_copy_rows(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && lds % vec == 0 && ldd % vec == 0 && lds >= dim && ldd >= dim, "dim / strides must be chunk multiples covering a row");
    XC_REQUIRE(aligned16(src) && aligned16(dst), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    int64_t blocks = (rows * (dim / vec) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((copy_rows_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)src, (long)lds, (T*)dst, (long)ldd, (long)rows, (int)dim);
    });
    return check_launch(__func__);
}

int xclip_add(const void* a, const void* b, void* out, int64_t count, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(count >= 0 && aligned16(a) && aligned16(b) && aligned16(out), "pointers must be 16-byte aligned");
    if (count == 0) return 0;
    const int64_t n16 = count / vec_of(dtype);
    int64_t blocks = (n16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;                                      // (a count below one chunk: the scalar tail alone)
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((add_rows_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)a, (const T*)b, (T*)out, (long)n16, (long)count);
    });
    return check_launch(__func__);
}

// ---- column sum for rows of any width (tokens.h colsum_wide_kernel) ----
// work-groups of 4 waves over the rows: as many as there are rows to give every wave one, capped so that strips x row groups stays near
// 2048 work-groups (and the partial rows at 256).  A strip is the 64 chunks a wave's lanes hold: 64 * vec columns.
inline int64_t colsum_row_blocks(int64_t rows, int64_t dim, int vec) {
    int64_t cap = 2048 / ((dim / vec + 63) / 64);
    cap = cap < 1 ? 1 : (cap > 64 ? 64 : cap);
    const int64_t want = (rows + 3) / 4;
    return want < cap ? (want < 1 ? 1 : want) : cap;
}
static int colsum_wide(const char* fn, const void* src, int64_t lds, float* colsum_accum, int64_t rows, int64_t dim, void* workspace,
                                    int64_t workspace_bytes, int dtype, hipStream_t st) {
    const int vec = vec_of(dtype);
    const int64_t rb = colsum_row_blocks(rows, dim, vec);
    if (!(workspace != nullptr && workspace_bytes >= rb * 4 * dim * 4)) return fail(fn, "rows this wide need the workspace (xclip_colsum_workspace_bytes)");
    if (!(dim < (1LL << 31))) return fail(fn, "row too wide for 32-bit column indices");
    dim3 grid((unsigned)((dim / vec + 63) / 64), (unsigned)rb), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((colsum_wide_kernel<T>), grid, block, 0, st, (const T*)src, (long)lds, (long)rows, (int)dim, (float*)workspace);
    });
    // ONE slice: a column's partial rows are summed in a fixed order and meet the accumulator in one addition
    hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((dim + 63) / 64), 1), dim3(256), 1024, st, (const float*)workspace, (long)dim,
                       colsum_accum, (int)(rb * 4), (int)dim);
    return check_launch(fn);
}

// (no dtype here: the bf16 strip is the wider one, so its row-group count is the larger of the two)
int64_t xclip_colsum_workspace_bytes(int64_t rows, int64_t dim) { return colsum_row_blocks(rows, dim, 8) * 4 * dim * 4; }

int xclip_colsum(const void* src, int64_t lds, float* colsum_accum, int64_t rows, int64_t dim, void* workspace, int64_t workspace_bytes,
                 int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec == 0 && lds % vec == 0 && lds >= dim, "dim / lds must be chunk multiples covering a row");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(src != nullptr && colsum_accum != nullptr && aligned16(src), "null or misaligned pointer");
    return colsum_wide(__func__, src, lds, colsum_accum, rows, dim, workspace, workspace_bytes, dtype, (hipStream_t)stream);
}

int64_t xclip_rows_scatter_add_workspace_bytes(int64_t rows, int64_t dim) {
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 256) blocks = 256;
    return blocks * 4 * dim * 4;
}

int xclip_rows_scatter_add(const void* src, int64_t lds, const int32_t* idx, float* table_accum, float* colsum_accum, int64_t rows,
                           int64_t dim, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && lds % vec == 0 && lds >= dim, "dim / lds must be chunk multiples covering a row");
    XC_REQUIRE(aligned16(src), "pointers must be 16-byte aligned");
    XC_REQUIRE(table_accum == nullptr || idx != nullptr, "table_accum needs idx");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    // the column sum alone over rows wider than the dispatch below takes (the MLM head's bias gradient over a vocabulary): colsum_wide_kernel
    if (idx == nullptr && table_accum == nullptr && colsum_accum != nullptr && cpl > 4096 / 64 / vec)
        return colsum_wide(__func__, src, lds, colsum_accum, rows, dim, workspace, workspace_bytes, dtype, (hipStream_t)stream);
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 256) blocks = 256;
    // column sums go through per-wave partial rows + a fold (thousands of waves adding into the same `dim` floats serialise)
    float* partial = (colsum_accum != nullptr && workspace != nullptr && workspace_bytes >= blocks * 4 * dim * 4) ? (float*)workspace : nullptr;
    dim3 grid((unsigned)blocks), block(256);
#define F(T, C) hipLaunchKernelGGL((rows_scatter_add_kernel<T, C>), grid, block, 0, (hipStream_t)stream, (const T*)src, (long)lds, (const int*)idx, table_accum, colsum_accum, (long)rows, (int)dim, partial)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    if (partial != nullptr) {
        // every wave writes its row (waves without rows write zeros), so all blocks * 4 rows are defined
        hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((dim + 63) / 64), 4), dim3(256), 1024, (hipStream_t)stream,
                           (const float*)partial, (long)dim, colsum_accum, (int)(blocks * 4), (int)dim);
    }
    return check_launch(__func__);
}

int xclip_scatter_add_sorted(const void* src, int64_t lds, const int64_t* sorted_ids, const int64_t* perm, float* table_accum,
                             int64_t table_rows, int64_t count, int64_t dim, int64_t n_in, int64_t n_out, int64_t row_off, int dtype,
                             void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && lds % vec == 0 && lds >= dim, "dim / lds must be chunk multiples covering a row");
    XC_REQUIRE(aligned16(src) && sorted_ids != nullptr && perm != nullptr && table_accum != nullptr, "bad pointers");
    XC_REQUIRE(n_in > 0 && n_out > 0 && table_rows > 0, "bad row map");
    if (count == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    int64_t chunk = (count + 16383) / 16384;               // ~16k waves; at least 16 entries per wave
    if (chunk < 16) chunk = 16;
    const int64_t waves = (count + chunk - 1) / chunk;
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    // the flush is staged through LDS (one wave's row of fp32: coalesced atomics) where four rows fit the default 64 KiB
    const size_t stage_bytes = (size_t)4 * dim * sizeof(float) <= 64 * 1024 ? (size_t)4 * dim * sizeof(float) : 0;
    const int staged = measure_env("XCLIP_SCATTER_STAGED", 1) && stage_bytes > 0;
#define F(T, C) hipLaunchKernelGGL((scatter_add_sorted_kernel<T, C>), grid, block, staged ? stage_bytes : 0, (hipStream_t)stream, (const T*)src, (long)lds, (const long long*)sorted_ids, (const long long*)perm, table_accum, (long)count, (int)dim, (int)n_in, (int)n_out, (int)row_off, (int)chunk, (long long)table_rows, staged)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int64_t xclip_sort_ids_workspace_bytes(int64_t count) {
    if (count <= 0) return 0;
    const int64_t nblk = (count + SORT_BLOCK - 1) / SORT_BLOCK;
    return 2 * ((count * 8 + 15) & ~(int64_t)15) + 2 * nblk * SORT_BINS * 4;
}

int xclip_sort_ids(const int64_t* ids, int64_t count, int64_t id_limit, int64_t* sorted_ids, int64_t* perm, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    XC_REQUIRE(count >= 0 && count < ((int64_t)1 << 32) && id_limit >= 1 && id_limit <= ((int64_t)1 << 32), "count / id_limit out of range");
    if (count == 0) return 0;
    XC_REQUIRE(ids != nullptr && sorted_ids != nullptr && perm != nullptr, "bad pointers");
    XC_REQUIRE(workspace != nullptr && aligned16(workspace) && workspace_bytes >= xclip_sort_ids_workspace_bytes(count), "workspace too small or misaligned");
    const int64_t nblk = (count + SORT_BLOCK - 1) / SORT_BLOCK, half = (count * 8 + 15) & ~(int64_t)15;
    uint64_t* bufs[2] = {reinterpret_cast<uint64_t*>(workspace), reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(workspace) + half)};
    int* const hist = reinterpret_cast<int*>(static_cast<unsigned char*>(workspace) + 2 * half);
    int* const offs = hist + nblk * SORT_BINS;
    int bits = 0;
    while (((int64_t)1 << bits) < id_limit) ++bits;
    const int passes = bits <= 8 ? 1 : (bits + 7) / 8;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(256);
    const size_t lds = SORT_BINS * sizeof(int);
    const long long* src_ids = reinterpret_cast<const long long*>(ids);
    for (int ps = 0; ps < passes; ++ps) {
        const bool first = ps == 0, last = ps == passes - 1;
        const uint64_t* in = first ? nullptr : bufs[(ps - 1) & 1];
        uint64_t* out = last ? nullptr : bufs[ps & 1];
        const int shift = 8 * ps;
        if (first) hipLaunchKernelGGL((sort_hist_kernel<true>), grid, block, lds, st, src_ids, in, (long)count, shift, hist);
        else hipLaunchKernelGGL((sort_hist_kernel<false>), grid, block, lds, st, src_ids, in, (long)count, shift, hist);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 5 * lds, st, (const int*)hist, offs, (int)nblk);
#define S(F, L) hipLaunchKernelGGL((sort_scatter_kernel<F, L>), grid, block, lds, st, src_ids, in, out, (long long*)sorted_ids, (long long*)perm, (long)count, shift, (const int*)offs)
        if (first && last) S(true, true); else if (first) S(true, false); else if (last) S(false, true); else S(false, false);
#undef S
    }
    return check_launch(__func__);
}

int xclip_cast_from_f32(const float* src, void* dst, int64_t count, float scale, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    if (count == 0) return 0;
    int64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cast_from_f32_kernel<T>), grid, block, 0, (hipStream_t)stream, src, (T*)dst, (long)count, scale);
    });
    return check_launch(__func__);
}

int xclip_clock_sample(uint64_t* out2, int64_t ticks_10ns, void* stream) {
    XC_REQUIRE(out2 != nullptr && ticks_10ns > 0 && ticks_10ns <= 100000, "out2 must hold two uint64; 0 < ticks <= 100000 (1 ms)");
    hipLaunchKernelGGL(clock_sample_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out2, (long)ticks_10ns);
    return check_launch(__func__);
}

namespace {
inline int dwconv_bwd_blocks(int64_t batch, int64_t h, int64_t C, int dtype) {
    const int64_t items = batch * h * h * (C / vec_of(dtype));
    int64_t b = (items + 255) / 256;
    return (int)(b > 512 ? 512 : (b < 1 ? 1 : b));
}
}  // namespace
int64_t xclip_dwconv4s2_workspace_bytes(int64_t batch, int64_t h, int64_t C, int dtype) {
    return (int64_t)dwconv_bwd_blocks(batch, h, C, dtype) * 4 * C * 16 * 4;
}
int xclip_dwconv4s2_fwd(const void* x, const void* w, void* y, int64_t batch, int64_t h, int64_t C, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(batch >= 0 && h >= 2 && h % 2 == 0 && C > 0 && C % vec_of(dtype) == 0, "token grid must be even-sided, channels whole 16-byte chunks");
    XC_REQUIRE(x && w && y && aligned16(x) && aligned16(w) && aligned16(y), "null or misaligned pointer");
    if (batch == 0) return 0;
    const int64_t items = batch * (h / 2) * (h / 2) * (C / vec_of(dtype));
    int64_t blocks = (items + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((dwconv_fwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, (const T*)w, (T*)y, (int)batch, (int)h, (int)C);
    });
    return check_launch(__func__);
}
int xclip_dwconv4s2_bwd(const void* dy, const void* x, const void* w, void* dx, float* dw_accum, void* workspace, int64_t workspace_bytes,
                        int64_t batch, int64_t h, int64_t C, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(batch >= 0 && h >= 2 && h % 2 == 0 && C > 0 && C % vec_of(dtype) == 0, "token grid must be even-sided, channels whole 16-byte chunks");
    XC_REQUIRE(dy && x && w && dx && dw_accum && aligned16(dy) && aligned16(x) && aligned16(w) && aligned16(dx), "null or misaligned pointer");
    XC_REQUIRE(workspace != nullptr && workspace_bytes >= xclip_dwconv4s2_workspace_bytes(batch, h, C, dtype), "workspace too small");
    if (batch == 0) return 0;
    const int blocks = dwconv_bwd_blocks(batch, h, C, dtype);
    dim3 grid((unsigned)blocks), block(256);
    float* partial = (float*)workspace;
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((dwconv_bwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)dy, (const T*)x, (const T*)w, (T*)dx, partial, (int)batch, (int)h, (int)C);
    });
    hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((C * 16 + 63) / 64), 4), dim3(256), 1024, (hipStream_t)stream,
                       (const float*)partial, (long)(C * 16), dw_accum, blocks * 4, (int)(C * 16));
    return check_launch(__func__);
}

int xclip_gather_rows(const void* src, int64_t lds, const int32_t* idx, void* out, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec_of(dtype) == 0 && lds % vec_of(dtype) == 0, "dim / row stride must be whole 16-byte chunks");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(src && idx && out && aligned16(src) && aligned16(out), "null or misaligned pointer");
    int64_t blocks = (rows * (dim / vec_of(dtype)) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((gather_rows_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)src, (long)lds, idx, (T*)out, (long)rows, (int)dim);
    });
    return check_launch(__func__);
}
int xclip_rows_add_at(void* dst, int64_t ldd, const int32_t* idx, const void* src, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec_of(dtype) == 0 && ldd % vec_of(dtype) == 0, "dim / row stride must be whole 16-byte chunks");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(dst && idx && src && aligned16(dst) && aligned16(src), "null or misaligned pointer");
    int64_t blocks = (rows * (dim / vec_of(dtype)) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rows_add_at_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)dst, (long)ldd, idx, (const T*)src, (long)rows, (int)dim);
    });
    return check_launch(__func__);
}
int xclip_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t cols, float* lse, float* loss_accum,
                            int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && cols > 0 && ld >= cols && ld % vec_of(dtype) == 0, "row stride must cover the columns in whole 16-byte chunks");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(logits && labels && lse && loss_accum && aligned16(logits), "null or misaligned pointer");
    int64_t blocks = (rows + 3) / 4;
    if (blocks > ROWLOSS_MAX_BLOCKS) blocks = ROWLOSS_MAX_BLOCKS;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ce_fwd_kernel<T>), grid, block, 16, (hipStream_t)stream, (const T*)logits, (long)ld, (const long long*)labels, (int)rows, (int)cols, lse, loss_accum);
    });
    return check_launch(__func__);
}
int xclip_cross_entropy_bwd(void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* gmul, int64_t rows, int64_t cols,
                            int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && cols > 0 && ld >= cols && ld % vec_of(dtype) == 0, "row stride must cover the columns in whole 16-byte chunks");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(logits && labels && lse && gmul && aligned16(logits), "null or misaligned pointer");
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ce_bwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)logits, (long)ld, (const long long*)labels, lse, gmul, (int)rows, (int)cols);
    });
    return check_launch(__func__);
}

int xclip_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(n >= 0 && n % vec_of(dtype) == 0 && p >= 0.f && p < 1.f, "n must be a whole number of 16-byte chunks, p in [0, 1)");
    XC_REQUIRE(x && y && aligned16(x) && aligned16(y), "null or misaligned pointer");
    if (n == 0) return 0;
    int64_t blocks = (n / vec_of(dtype) + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const uint32_t th = drop_thresh(p);
    const float sc = 1.0f / (1.0f - p);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((dropout_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, (long)n, th, sc, seed);
    });
    return check_launch(__func__);
}

int xclip_rotary(void* x, int64_t ld, int64_t rows, int64_t n, int64_t slots, int64_t slot_width, int64_t rot, const float* inv_freq, int inverse,
                 int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(slot_width == 64 || slot_width == 128, "head slots are 64 or 128 wide");
    XC_REQUIRE(rot >= 2 && rot <= 32 && rot % 2 == 0, "rot = min(dim_head, 32) rotated features per head: even, 2 .. 32");
    XC_REQUIRE(rows >= 0 && n > 0 && slots > 0 && ld >= slots * slot_width && ld % vec_of(dtype) == 0, "bad shape");
    XC_REQUIRE(x && aligned16(x) && inv_freq, "null or misaligned pointer");
    if (rows == 0) return 0;
    const int64_t items = rows * slots * (16 / vec_of(dtype));
    int64_t blocks = (items + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    dim3 grid((unsigned)blocks), block(256);
    const float sign = inverse ? -1.0f : 1.0f;
    if (rot != 32) {                                             // narrow heads: element pairs
        int64_t pb = (rows * slots * (rot / 2) + 255) / 256;
        if (pb > 8192) pb = 8192;
        by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
            hipLaunchKernelGGL((rotary_pairs_kernel<T>), dim3((unsigned)pb), block, 0, (hipStream_t)stream, (T*)x, (long)ld, (long)rows, (int)n, (int)slots, (int)slot_width, (int)(rot / 2), inv_freq, sign);
        });
        return check_launch(__func__);
    }
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rotary_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)x, (long)ld, (long)rows, (int)n, (int)slots, (int)slot_width, inv_freq, sign);
    });
    return check_launch(__func__);
}

// xclip_rotary for rows that carry their own position (the packed text tower: pos = TextLayout.pos); the launch sizes of xclip_rotary
int xclip_rotary_pos(void* x, int64_t ld, int64_t rows, const int32_t* pos, int64_t slots, int64_t slot_width, int64_t rot, const float* inv_freq,
                     int inverse, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(slot_width == 64 || slot_width == 128, "head slots are 64 or 128 wide");
    XC_REQUIRE(rot >= 2 && rot <= 32 && rot % 2 == 0, "rot = min(dim_head, 32) rotated features per head: even, 2 .. 32");
    XC_REQUIRE(rows >= 0 && slots > 0 && ld >= slots * slot_width && ld % vec_of(dtype) == 0, "bad shape");
    if (rows == 0) return 0;                                         // (an empty packed batch: its arrays have no address)
    XC_REQUIRE(x && aligned16(x) && inv_freq && pos, "null or misaligned pointer");
    const int64_t per_slot = rot == 32 ? 16 / vec_of(dtype) : rot / 2;      // items of a head slot: 16-byte chunk pairs / element pairs
    int64_t blocks = (rows * slots * per_slot + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    dim3 grid((unsigned)blocks), block(256);
    const float sign = inverse ? -1.0f : 1.0f;
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (rot != 32)                                               // narrow heads: element pairs
            hipLaunchKernelGGL((rotary_pos_pairs_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)x, (long)ld, (long)rows, (const int*)pos, (int)slots, (int)slot_width, (int)(rot / 2), inv_freq, sign);
        else
            hipLaunchKernelGGL((rotary_pos_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)x, (long)ld, (long)rows, (const int*)pos, (int)slots, (int)slot_width, inv_freq, sign);
    });
    return check_launch(__func__);
}

// the 256 x 256 bf16 kernels behind xclip_gemm, on the plan's K slices.  reduce = false: a split-K problem leaves its fp32 slabs in
// g.workspace for the caller (alpha not applied).
static int gemm2_run(const GemmArgs& g, int splits, int k_per_split, bool reduce, hipStream_t st) {
    Gemm2Params q;
    q.A = (const bf16_t*)g.A; q.B = (const bf16_t*)g.B; q.C = (bf16_t*)g.C; q.lda = g.lda; q.ldb = g.ldb; q.ldc = g.ldc;
    q.M = (int)g.M; q.N = (int)g.N; q.K = (int)g.K; q.alpha = g.alpha;
    q.bias = (const bf16_t*)g.bias; q.residual = (const bf16_t*)g.residual; q.ldr = g.ldr;
    q.addrows = (const bf16_t*)g.addrows; q.rowidx = g.rowidx; q.ld_add = g.ld_add;
    q.tiles_m = (int)((g.M + G2_BM - 1) / G2_BM); q.tiles_n = (int)((g.N + G2_BN - 1) / G2_BN);
    // an output that cannot stay in the 8 x 4 MiB of L2 anyway is streamed past it: the A / B panels the sibling tiles share then
    // survive a round's 32 MiB of output (XCLIP_GEMM_NT=0 / 1 forces the policy, for measurement)
    static const int nt_env = measure_env("XCLIP_GEMM_NT", -1);
    q.stream_out = nt_env >= 0 ? nt_env : (g.M * g.N * 2 > (int64_t)(48 << 20) ? 1 : 0);
    // more than 8 N tiles (FF1: 16): banded tile order for the ring kernel (XCLIP_GEMM_BAND=<tiles per band>, 0 = off, for measurement)
    static const int band_env = measure_env("XCLIP_GEMM_BAND", -1);
    // FF1 forward in the step: 1227 -> 1155 us (profiles/r02_run22_gemm_banded_order.log); the widest band of 4..8 tiles that divides
    // the N tiles, none if there is none (9 tiles) or the operand fits anyway (<= 8 tiles)
    q.band_n = 0;
    if (band_env != 0 && q.tiles_n > 8)
        for (int b = band_env > 0 ? band_env : 8; b >= 4 && q.band_n == 0; --b)
            if (q.tiles_n % b == 0) q.band_n = b;
    q.k_per_split = k_per_split;
    q.partial = splits > 1 ? (float*)g.workspace : nullptr;
    by_layout(g.a_kmajor, g.b_kmajor, [&](auto ak, auto bk) { launch_gemm2<decltype(ak)::value, decltype(bk)::value>(q, splits, st); });
    if (splits > 1 && reduce) launch_splitk_reduce<bf16_t>(g.workspace, g.C, g.ldc, g.M, g.N, splits, g.alpha, nullptr, 0, st);
    return check_launch(__func__);
}

// the latency-built 64 x 64 kernel (gemm_small.h) for outputs of a few tiles and a few GFLOP
static int64_t g_small_flop = GS_MAX_FLOP;
int64_t xclip_gemm_small_limit(int64_t max_flop) {
    const int64_t was = g_small_flop;
    if (max_flop >= 0) g_small_flop = max_flop;
    return was;
}
static int gemm_small_run(const GemmArgs& g, hipStream_t st) {
    GemmSmallParams q;
    q.A = (const bf16_t*)g.A; q.B = (const bf16_t*)g.B; q.C = (bf16_t*)g.C; q.lda = g.lda; q.ldb = g.ldb; q.ldc = g.ldc;
    q.M = (int)g.M; q.N = (int)g.N; q.K = (int)g.K; q.alpha = g.alpha; q.residual = (const bf16_t*)g.residual; q.ldr = g.ldr;
    q.tiles_m = (int)(g.M / GS_BM); q.tiles_n = (int)(g.N / GS_BN);
    const int64_t tiles = (int64_t)q.tiles_m * q.tiles_n;
    q.stages = gs_stages(tiles, g.K / GS_BK);
    const int lds = q.stages * GS_STAGE_BYTES;
#define XC_GS(RES) do { XC_ALLOW_LDS((gemm_small_kernel<AK, BK_, RES>), GS_MAX_STAGES * GS_STAGE_BYTES); \
        hipLaunchKernelGGL((gemm_small_kernel<AK, BK_, RES>), dim3((unsigned)tiles), dim3(GS_THREADS), lds, st, q); } while (0)
    by_layout(g.a_kmajor, g.b_kmajor, [&](auto ak, auto bk) {
        constexpr bool AK = decltype(ak)::value, BK_ = decltype(bk)::value;
        if (g.residual != nullptr) XC_GS(true); else XC_GS(false);
    });
#undef XC_GS
    return check_launch(__func__);
}

// (Measured and not kept: the row tail of a SHORT-K persistent product -- fewer than 16 K steps, which gemm2_tail_cut leaves whole -- as a
//  second launch of the 64 x 64 kernel behind the whole rounds.  Bit-identical results (the same MFMA k-blocks in the same order), and the
//  round it saves is worth about what the dependent launch costs: text out-projection 153.8 -> 152.0 us, QKV 406 -> 403, FF1 1101 -> 1102
//  (profiles/r05_s_bench_shapes_short_k_tail_on_small_kernel.log against r05_r_bench_shapes_small_kernel.log).)

#ifdef XCLIP_MEASURE
// measurement build: gemm8.h on / off at run time (same-process A/B); -> the previous setting
extern "C" int xclip_measure_gemm8(int on) { const int was = gemm8_on() ? 1 : 0; g_gemm8 = on; return was; }
#endif

// the plan's bytes for the most demanding caller of the shape: no terms, normal A (the only layout that cuts the row tail: a k-major-A
// caller just gets a little more than it needs), a workspace as large as asked for, the 64 x 64 kernel turned off
int64_t xclip_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype) {
    GemmArgs g{}; g.M = M; g.N = N; g.K = K;
    return gemm_plan(g, dtype, INT64_MAX, -1).workspace_bytes;
}

// the route of the plan xclip_gemm would execute for a product of this description (a host query: the plan reads which optional terms are
// there, never through them -- a stand-in address marks them)
int xclip_gemm_route(int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int has_bias_or_rows,
                     int has_residual, int64_t workspace_bytes, int dtype) {
    if (!dtype_ok(dtype) || M <= 0 || N <= 0 || K <= 0 || workspace_bytes < 0) {      // (-1: a code of xclip_gemm's would read as a route)
        xcapi::fail(__func__, "bad dtype or shape");
        return -1;
    }
    static const char term = 0;
    GemmArgs g{};
    g.a_kmajor = a_kmajor; g.b_kmajor = b_kmajor; g.lda = lda; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.bias = has_bias_or_rows ? &term : nullptr;
    g.residual = has_residual ? &term : nullptr;
    return (int)gemm_plan(g, dtype, workspace_bytes, g_small_flop).route;
}

int xclip_gemm(int a_kmajor, int b_kmajor, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
               int64_t M, int64_t N, int64_t K, float alpha, const void* bias, const void* residual, int64_t ldr,
               const void* addrows, const int32_t* rowidx, int64_t ld_add, void* workspace, int64_t workspace_bytes,
               int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(M >= 0 && N > 0 && K > 0, "bad shape");
    XC_REQUIRE(N % vec == 0 && ldc % vec == 0, "N and ldc must be multiples of the 16-byte chunk");
    XC_REQUIRE(lda % vec == 0 && ldb % vec == 0, "lda / ldb must be multiples of the 16-byte chunk");
    // operands are read in whole 16-byte chunks: a row must be allocated (and, for a normal operand whose K is not a
    // chunk multiple, zero padded by the caller) up to the next chunk boundary
    const int64_t Kp = (K + vec - 1) / vec * vec, Mp = (M + vec - 1) / vec * vec;
    XC_REQUIRE(a_kmajor ? (lda >= Mp) : (lda >= Kp), "lda must cover A's contiguous dim rounded up to the 16-byte chunk");
    XC_REQUIRE(b_kmajor ? (ldb >= N) : (ldb >= Kp), "ldb must cover B's contiguous dim rounded up to the 16-byte chunk");
    XC_REQUIRE(!(a_kmajor && !b_kmajor), "layout (A k-major, B normal) is not used on this path");
    XC_REQUIRE(aligned16(A) && aligned16(B) && aligned16(C) && aligned16(bias) && aligned16(residual) && aligned16(addrows) && aligned16(workspace),
               "pointers must be 16-byte aligned");
    XC_REQUIRE(residual == nullptr || ldr % vec == 0, "ldr must be a multiple of the 16-byte chunk");
    XC_REQUIRE(addrows == nullptr || (rowidx != nullptr && ld_add % vec == 0), "addrows needs rowidx and an aligned ld");
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const GemmArgs g{a_kmajor, b_kmajor, A, lda, B, ldb, C, ldc, M, N, K, alpha, bias, residual, ldr, addrows, rowidx, ld_add, workspace, workspace_bytes};
    const GemmPlan plan = gemm_plan(g, dtype, workspace != nullptr ? workspace_bytes : 0, g_small_flop);
    switch (plan.route) {
    case GEMM_SMALL: return gemm_small_run(g, st);
    case GEMM_256: return gemm2_run(g, plan.splits, plan.k_per_split, true, st);
    case GEMM_256_CUT: {                                      // the main rows, then the tail's slabs, then the reduction that also applies alpha and the skip term
        GemmArgs main = g, tail = g;
        main.M = plan.main_rows;
        if (const int rc = gemm2_run(main, 1, (int)K, true, st)) return rc;
        tail.M = plan.tail_rows;
        tail.A = (const char*)A + plan.main_rows * lda * 2;   // (bf16: use_gemm2)
        tail.C = (char*)C + plan.main_rows * ldc * 2;
        tail.residual = nullptr; tail.ldr = 0;
        if (const int rc = gemm2_run(tail, plan.splits, plan.k_per_split, false, st)) return rc;
        const char* Rt = residual != nullptr ? (const char*)residual + plan.main_rows * ldr * 2 : nullptr;
        launch_splitk_reduce<bf16_t>(workspace, tail.C, ldc, tail.M, N, plan.splits, alpha, Rt, ldr, st);
        return check_launch(__func__);
    }
    case GEMM_GENERIC: break;
    }
    GemmParams p;
    p.A = A; p.B = B; p.C = C; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.alpha = alpha;
    p.bias = bias; p.residual = residual; p.ldr = ldr; p.addrows = addrows; p.rowidx = rowidx; p.ld_add = ld_add;
    p.tiles_m = (int)((M + 127) / 128); p.tiles_n = (int)((N + 127) / 128);
    p.k_per_split = plan.k_per_split;
    p.partial = plan.splits > 1 ? (float*)workspace : nullptr;
    launch_gemm(p, dtype, a_kmajor, b_kmajor, plan.splits, 1, st);
    if (plan.splits > 1)
        by_dtype(dtype, [&](auto t) { launch_splitk_reduce<typename decltype(t)::type>(workspace, C, ldc, M, N, plan.splits, alpha, nullptr, 0, st); });
    return check_launch(__func__);
}

int xclip_ffn_dgrad_geglu_ok(int64_t M, int64_t F, int64_t D, int dtype) {
    return dtype == XCLIP_BF16 && M > 0 && M % G2_BM == 0 && F % G2_BN == 0 && D % G2_BK == 0 && D >= 2 * G2_BK && D <= 4096 && F < (1L << 20) &&
           (M / G2_BM) * (F / G2_BN) < (1L << 30);
}
int64_t xclip_ffn_dgrad_geglu_workspace_bytes(int64_t M, int64_t F, int64_t D) {
    return ((D + 3) / 4 * 4 + 4 * M + 2 * (M / G2_BM) * F) * 4;
}
// rowc_in != nullptr: the rows' constants are already there (written by xclip_layernorm_bwd_ffnstats in the pass that produced dout);
// otherwise the weight vector and the row pass run here (x2 / x1 required)
struct FfnDgradArgs {                                         // xclip_ffn_dgrad_geglu's arguments, in its order, + rowc_in
    const void* dout; int64_t ldd; const void* w2; int64_t ldw; const void* x; int64_t ldx; const void* gamma;
    const float* mean; const float* rstd; const void* x2; int64_t ld2; const void* x1; int64_t ld1; const float* rowc_in;
    void* dx; int64_t lddx; float* dg_accum; void* workspace; int64_t workspace_bytes; int64_t M, F, D; int dtype; void* stream;
};
static int ffn_dgrad_geglu_run(const char* fn, const FfnDgradArgs& a) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(xclip_ffn_dgrad_geglu_ok(a.M, a.F, a.D, a.dtype), "shape / dtype not taken by the fused kernel (xclip_ffn_dgrad_geglu_ok)");
    XC_REQ(a.dout && a.w2 && a.x && a.gamma && a.dx && a.dg_accum, "null pointer");
    XC_REQ(a.rowc_in != nullptr || (a.mean && a.rstd && a.x2 && a.x1), "null pointer");
    XC_REQ(aligned16(a.dout) && aligned16(a.w2) && aligned16(a.x) && aligned16(a.gamma) && aligned16(a.x2) && aligned16(a.x1) && aligned16(a.dx) && aligned16(a.workspace) && aligned16(a.rowc_in),
           "pointers must be 16-byte aligned");
    XC_REQ(a.ldd % 8 == 0 && a.ldw % 8 == 0 && a.ldx % 8 == 0 && a.ld2 % 8 == 0 && a.ld1 % 8 == 0 && a.lddx % 8 == 0, "leading dimensions must be multiples of the 16-byte chunk");
    XC_REQ(a.ldd >= a.D && (a.rowc_in != nullptr || (a.ld2 >= a.D && a.ld1 >= a.D)) && a.ldw >= a.F && a.ldx >= 2 * a.F && a.lddx >= 2 * a.F, "leading dimension too small");
    XC_REQ(a.ldd < (1L << 22) && a.ldw < (1L << 22) && a.ldx < (1L << 22) && a.lddx < (1L << 22), "leading dimensions beyond the 32-bit tile offsets");
    XC_REQ(a.workspace != nullptr && a.workspace_bytes >= xclip_ffn_dgrad_geglu_workspace_bytes(a.M, a.F, a.D), "workspace too small");
#undef XC_REQ
    hipStream_t st = (hipStream_t)a.stream;
    float* wg = (float*)a.workspace;
    float* rowc = wg + (a.D + 3) / 4 * 4;
    float* slab = rowc + 4 * a.M;
    if (a.rowc_in == nullptr) {
        hipLaunchKernelGGL(ffn_wgamma_kernel, dim3((unsigned)((a.D + 3) / 4)), dim3(256), 0, st, (const bf16_t*)a.w2, (long)a.ldw, (const bf16_t*)a.gamma, wg, (int)a.D, (int)a.F);
        hipLaunchKernelGGL(ffn_rowstats_kernel, dim3((unsigned)((a.M + 3) / 4)), dim3(256), 0, st, (const bf16_t*)a.dout, (long)a.ldd, (const bf16_t*)a.x2, (long)a.ld2,
                           (const bf16_t*)a.x1, (long)a.ld1, (const float*)wg, a.mean, a.rstd, rowc, (int)a.M, (int)a.D, 1.0f / (float)a.F);
    } else {
        rowc = const_cast<float*>(a.rowc_in);
    }
    Gemm2Params q{};
    q.A = (const bf16_t*)a.dout; q.B = (const bf16_t*)a.w2; q.C = nullptr; q.lda = a.ldd; q.ldb = a.ldw; q.ldc = a.F;
    q.M = (int)a.M; q.N = (int)a.F; q.K = (int)a.D; q.alpha = 1.f;
    q.bias = nullptr; q.residual = nullptr; q.ldr = 0; q.addrows = nullptr; q.rowidx = nullptr; q.ld_add = 0; q.partial = nullptr;
    q.k_per_split = (int)a.D;
    q.tiles_m = (int)(a.M / G2_BM); q.tiles_n = (int)(a.F / G2_BN);
    q.band_n = 0;
    if (q.tiles_n > 8)
        for (int b = 8; b >= 4 && q.band_n == 0; --b)
            if (q.tiles_n % b == 0) q.band_n = b;
    q.stream_out = 1;
    GegluBwdArgs e;
    e.x = (const bf16_t*)a.x; e.ldx = a.ldx; e.dx = (bf16_t*)a.dx; e.lddx = a.lddx; e.gamma = (const bf16_t*)a.gamma;
    e.rowc = rowc; e.dg_partial = slab; e.F = (int)a.F;

    int gx = q.tiles_m * q.tiles_n;
    const int cus = xc_num_cus();
    if (gx > cus) gx = cus;
    // (round 5's two-work-groups-per-CU form of this kernel -- 256 x 128 tiles, four waves each -- measured slower, 1457 against 1277 us, and
    //  was not correct beyond one tile per work-group on the hardware; removed in round 6, log: profiles/r05_aa_gemm10_two_groups_ab.log)
    {
#define XC_G9(N) do { XC_ALLOW_LDS(gemm9_geglu_bwd_kernel<N>, G5_LDS_BYTES); \
        hipLaunchKernelGGL(gemm9_geglu_bwd_kernel<N>, dim3((unsigned)gx, 1), dim3(G2_THREADS), G5_LDS_BYTES, st, q, e); } while (0)
#ifdef XCLIP_MEASURE
    static const int abl = measure_env("XCLIP_GEMM9_ABL", 0);
    switch (abl) {
        case 1: XC_G9(1); break;
        case 2: XC_G9(2); break;
        case 4: XC_G9(4); break;
        case 8: XC_G9(8); break;
        case 14: XC_G9(14); break;
        default: XC_G9(0); break;
    }
#else
    XC_G9(0);
#endif
#undef XC_G9
    }
    const int nrows = 2 * q.tiles_m;
    int slices = nrows / 64;
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((a.F + 63) / 64), (unsigned)slices), dim3(256), 1024, st, (const float*)slab, (long)a.F, a.dg_accum,
                       nrows, (int)a.F);
    return check_launch(fn);
}
int xclip_ffn_dgrad_geglu(const void* dout, int64_t ldd, const void* w2, int64_t ldw, const void* x, int64_t ldx, const void* gamma,
                          const float* mean, const float* rstd, const void* x2, int64_t ld2, const void* x1, int64_t ld1, void* dx,
                          int64_t lddx, float* dg_accum, void* workspace, int64_t workspace_bytes, int64_t M, int64_t F, int64_t D,
                          int dtype, void* stream) {
    XC_REQUIRE(mean && rstd && x2 && x1, "null pointer");
    return ffn_dgrad_geglu_run(__func__, {dout, ldd, w2, ldw, x, ldx, gamma, mean, rstd, x2, ld2, x1, ld1, nullptr, dx, lddx, dg_accum, workspace,
                                          workspace_bytes, M, F, D, dtype, stream});
}
int xclip_ffn_dgrad_geglu_rowc(const void* dout, int64_t ldd, const void* w2, int64_t ldw, const void* x, int64_t ldx, const void* gamma,
                               const float* rowc, void* dx, int64_t lddx, float* dg_accum, void* workspace, int64_t workspace_bytes,
                               int64_t M, int64_t F, int64_t D, int dtype, void* stream) {
    XC_REQUIRE(rowc != nullptr, "null pointer");
    return ffn_dgrad_geglu_run(__func__, {dout, ldd, w2, ldw, x, ldx, gamma, nullptr, nullptr, nullptr, 0, nullptr, 0, rowc, dx, lddx, dg_accum, workspace,
                                          workspace_bytes, M, F, D, dtype, stream});
}
int xclip_ffn_wgamma(const void* w2, int64_t ldw, const void* gamma, float* wg, int64_t D, int64_t F, int dtype, void* stream) {
    XC_REQUIRE(dtype == XCLIP_BF16, "bf16 only (the fused feed-forward backward)");
    XC_REQUIRE(w2 && gamma && wg && aligned16(w2) && aligned16(gamma) && aligned16(wg), "null or misaligned pointer");
    XC_REQUIRE(D > 0 && F > 0 && F % 8 == 0 && ldw % 8 == 0 && ldw >= F, "bad shape");
    hipLaunchKernelGGL(ffn_wgamma_kernel, dim3((unsigned)((D + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w2, (long)ldw, (const bf16_t*)gamma, wg, (int)D, (int)F);
    return check_launch(__func__);
}

int xclip_gemm_batched(int a_kmajor, int b_kmajor, const void* A, int64_t lda, int64_t stride_a, const void* B, int64_t ldb, int64_t stride_b,
                       void* C, int64_t ldc, int64_t stride_c, int64_t batch, int64_t M, int64_t N, int64_t K, float alpha, int dtype,
                       void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(batch >= 0 && batch <= 65535 && M >= 0 && N > 0 && K > 0, "bad shape (up to 65535 problems per launch)");
    XC_REQUIRE(N % vec == 0 && ldc % vec == 0 && lda % vec == 0 && ldb % vec == 0 && stride_a % vec == 0 && stride_b % vec == 0 && stride_c % vec == 0,
               "N, the leading dimensions and the batch strides must be multiples of the 16-byte chunk");
    const int64_t Kp = (K + vec - 1) / vec * vec, Mp = (M + vec - 1) / vec * vec;
    XC_REQUIRE(a_kmajor ? (lda >= Mp) : (lda >= Kp), "lda must cover A's contiguous dim rounded up to the 16-byte chunk");
    XC_REQUIRE(b_kmajor ? (ldb >= N) : (ldb >= Kp), "ldb must cover B's contiguous dim rounded up to the 16-byte chunk");
    XC_REQUIRE(!(a_kmajor && !b_kmajor), "layout (A k-major, B normal) is not used on this path");
    XC_REQUIRE(aligned16(A) && aligned16(B) && aligned16(C), "pointers must be 16-byte aligned");
    if (M == 0 || batch == 0) return 0;
    GemmParams p;
    p.A = A; p.B = B; p.C = C; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.alpha = alpha;
    p.bias = nullptr; p.residual = nullptr; p.ldr = 0; p.addrows = nullptr; p.rowidx = nullptr; p.ld_add = 0; p.partial = nullptr;
    p.tiles_m = (int)((M + 127) / 128); p.tiles_n = (int)((N + 127) / 128);
    p.k_per_split = (int)((K + 8 * vec - 1) / (8 * vec) * (8 * vec));
    p.batch_a = stride_a; p.batch_b = stride_b; p.batch_c = stride_c;
    launch_gemm(p, dtype, a_kmajor, b_kmajor, 1, batch, (hipStream_t)stream);
    return check_launch(__func__);
}

int xclip_rowdot(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(dim > 0 && dim % vec == 0 && lda % vec == 0 && ldb % vec == 0 && lda >= dim && ldb >= dim, "dim / leading dimensions must be multiples of the 16-byte chunk");
    XC_REQUIRE(aligned16(a) && aligned16(b) && out, "null or misaligned pointer");
    if (rows == 0) return 0;
    const int cpl = chunks_per_lane(dim, vec);
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define F(T, C) hipLaunchKernelGGL((rowdot_kernel<T, C>), grid, block, 0, (hipStream_t)stream, (const T*)a, (long)lda, (const T*)b, (long)ldb, (T*)out, (int)rows, (int)dim)
    XC_DISPATCH_ROW(dtype, cpl, F);
#undef F
    return check_launch(__func__);
}

int xclip_filip_reduce(const void* S, int64_t lds, const uint8_t* mask, const float* log_temp, float* t2i, float* i2t, int64_t ldo,
                       int16_t* kmax, int16_t* tmax, float* cnt, int64_t bx, int64_t nt, int64_t yc, int64_t ni, int64_t y0,
                       int64_t ytotal, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(bx > 0 && nt > 0 && yc > 0 && ni > 0 && ni <= 256, "FILIP reductions support up to 256 image tokens");
    XC_REQUIRE(lds >= yc * ni && y0 >= 0 && y0 + yc <= ytotal && ldo >= ytotal, "bad chunk geometry");
    XC_REQUIRE(S && mask && log_temp && t2i && i2t && kmax && tmax && cnt, "null pointer");
    // chunk rows that fit the register budget of the row-coalesced kernel (the host sizes its chunks for it) take that one
    if (yc * ni <= 256 * vec_of(dtype) * FILIP_MAXCH && yc <= 2048 && ni >= vec_of(dtype) && lds % vec_of(dtype) == 0 && aligned16(S)) {
        // split the chunk's images over blockIdx.y only when there are fewer text samples than CUs; sub-ranges start on 16-byte chunks
        const int vec = vec_of(dtype);
        int64_t g = ni, h = vec;
        while (h) { const int64_t r = g % h; g = h; h = r; }          // gcd(ni, vec)
        const int64_t step = vec / g;
        int64_t nsplit = ((int64_t)xc_num_cus() + bx - 1) / bx;          // (more, shorter rows per work-group measured slower: the per-row cost is fixed)
        if (nsplit < 1) nsplit = 1;
        int64_t ysplit = ((yc + nsplit - 1) / nsplit + step - 1) / step * step;
        if (ysplit < step) ysplit = step;
        nsplit = (yc + ysplit - 1) / ysplit;
        const int64_t nchunks = (ysplit * ni + vec - 1) / vec;
        const size_t shm = (size_t)nchunks * 32 + (size_t)ysplit * 4;
        dim3 g2((unsigned)bx, (unsigned)nsplit), b2(256);
        by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
            XC_ALLOW_LDS((filip_reduce_rows_kernel<T>), 96 * 1024);
            hipLaunchKernelGGL((filip_reduce_rows_kernel<T>), g2, b2, shm, (hipStream_t)stream, (const T*)S, (long)lds, mask, log_temp, t2i, i2t, (long)ldo, kmax, tmax, cnt, (int)bx, (int)nt, (int)yc, (int)ni, (int)y0, (int)ytotal, (int)ysplit);
        });
        return check_launch(__func__);
    }
    dim3 grid((unsigned)((bx * yc + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((filip_reduce_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)S, (long)lds, mask, log_temp, t2i, i2t, (long)ldo, kmax, tmax, cnt, (int)bx, (int)nt, (int)yc, (int)ni, (int)y0, (int)ytotal);
    });
    return check_launch(__func__);
}

int xclip_filip_fused_ok(int64_t nt, int64_t ni, int64_t d, int dtype) {
    return dtype == XCLIP_BF16 && d > 0 && d % G2_BK == 0 && nt >= 32 && ni >= 32 && nt <= 32767 && ni <= 32767;
}
int64_t xclip_filip_fused_workspace_bytes(int64_t bx, int64_t nt, int64_t yc, int64_t ni) {
    const int64_t M = bx * nt, N = yc * ni;
    return (M * ((N + 63) / 64) * F5_SIDES + ((M + 127) / 128) * F5_SLOTS * N) * 4;
}
int xclip_filip_fused_fwd(const void* X, const uint8_t* mask, const void* Y, const float* log_temp, float* t2i, float* i2t, int64_t ldo,
                          int16_t* kmax, int16_t* tmax, float* cnt, void* workspace, int64_t workspace_bytes, int64_t bx, int64_t nt,
                          int64_t yc, int64_t ni, int64_t d, int64_t y0, int64_t ytotal, int dtype, void* stream) {
    XC_REQUIRE(xclip_filip_fused_ok(nt, ni, d, dtype), "the fused FILIP forward needs bf16, d % 64 == 0, nt >= 32, ni >= 32");
    XC_REQUIRE(bx > 0 && yc > 0 && y0 >= 0 && y0 + yc <= ytotal && ldo >= ytotal, "bad chunk geometry");
    XC_REQUIRE(bx * nt < (1LL << 31) && yc * ni < (1LL << 31), "problem too large for 32-bit tile indices");
    XC_REQUIRE(X && Y && mask && log_temp && t2i && i2t && kmax && tmax && cnt && aligned16(X) && aligned16(Y), "null or misaligned pointer");
    XC_REQUIRE(workspace && workspace_bytes >= xclip_filip_fused_workspace_bytes(bx, nt, yc, ni), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    Filip5Params f;
    f.mask = mask;
    f.M = (int)(bx * nt); f.N = (int)(yc * ni); f.nt = (int)nt; f.ni = (int)ni; f.nblk64 = (int)((f.N + 63) / 64);
    f.rowpart = (uint32_t*)workspace;
    f.colpart = f.rowpart + (int64_t)f.M * f.nblk64 * F5_SIDES;
    const int64_t tiles = ((f.M + G2_BM - 1) / G2_BM) * (int64_t)((f.N + G2_BN - 1) / G2_BN);
    const int cus = xc_num_cus();
    XC_ALLOW_LDS(filip5_kernel, G5_LDS_BYTES);
    hipLaunchKernelGGL(filip5_kernel, dim3((unsigned)(tiles < cus ? tiles : cus)), dim3(G2_THREADS), G5_LDS_BYTES, st, (const bf16_t*)X,
                       (const bf16_t*)Y, (int)d, f);
    hipLaunchKernelGGL(filip5_merge_rows_kernel, dim3((unsigned)bx, (unsigned)((yc + 255) / 256)), dim3(256), 0, st, f.rowpart, mask, log_temp, t2i,
                       (long)ldo, kmax, cnt, (int)nt, (int)ni, (int)yc, f.nblk64, (int)y0, (int)ytotal);
    const int ypb = (int)(256 / ni > 0 ? 256 / ni : 1);
    hipLaunchKernelGGL(filip5_merge_cols_kernel, dim3((unsigned)bx, (unsigned)((yc + ypb - 1) / ypb)), dim3(256), (size_t)ypb * ni * 4, st, f.colpart,
                       log_temp, i2t, (long)ldo, tmax, (int)nt, (int)ni, (int)yc, f.N, ypb, (int)y0, (int)ytotal);
    return check_launch(__func__);
}

int xclip_filip_route(void* P, int64_t ldp, int64_t pcols, const uint8_t* mask, const float* log_temp, const float* g1, const float* g2, int64_t ldg,
                      const int16_t* kmax, const int16_t* tmax, const float* cnt, int64_t bx, int64_t nt, int64_t yc, int64_t ni,
                      int64_t y0, int64_t ytotal, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(bx > 0 && nt > 0 && yc > 0 && ni > 0, "bad shape");
    XC_REQUIRE(ldp % vec_of(dtype) == 0 && pcols % vec_of(dtype) == 0 && pcols >= yc * ni && ldp >= pcols && aligned16(P),
               "pcols must cover a chunk row and ldp pcols, both 16-byte chunk aligned");
    XC_REQUIRE(P && mask && log_temp && g1 && g2 && kmax && tmax && cnt, "null pointer");
    XC_REQUIRE(bx * nt < (1LL << 31) && pcols / vec_of(dtype) < (1LL << 31) && bx <= 65535, "chunk too large for the launch grid");
    // one work-group per (text x, slice of 256 chunks): blockIdx.y = x
    dim3 grid((unsigned)((pcols / vec_of(dtype) + 255) / 256), (unsigned)bx), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        XC_ALLOW_LDS((filip_route_kernel<T>), ROUTE_LDS_BYTES);
        hipLaunchKernelGGL((filip_route_kernel<T>), grid, block, ROUTE_LDS_BYTES, (hipStream_t)stream, (T*)P, (long)ldp, (long)pcols, mask, log_temp, g1, g2, (long)ldg, kmax, tmax, cnt, (int)bx, (int)nt, (int)yc, (int)ni, (int)y0, (int)ytotal);
    });
    return check_launch(__func__);
}

int xclip_rowlse(const float* S, int64_t lds, int64_t rows, int64_t cols, int64_t diag_off, int dcl, float coef, float* lse,
                 float* loss_accum, void* stream) {
    XC_REQUIRE(S && lse && rows > 0 && cols > 0 && lds >= cols, "bad arguments");
    hipLaunchKernelGGL(rowlse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S, (long)lds, (int)rows, (int)cols, (int)diag_off, dcl, coef, lse, loss_accum);
    return check_launch(__func__);
}

int xclip_rowgrad(const float* S, int64_t lds, const float* lse, int64_t rows, int64_t cols, int64_t diag_off, int dcl, float coef,
                  const float* gmul, float* G, int64_t ldg, float* dtau_accum, void* stream) {
    XC_REQUIRE(S && lse && G && rows > 0 && cols > 0 && lds >= cols && ldg >= cols, "bad arguments");
    int64_t blocks = (rows * cols + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(rowgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, S, (long)lds, lse, (int)rows, (int)cols, (int)diag_off, dcl, coef, gmul, G, (long)ldg, dtau_accum);
    return check_launch(__func__);
}

int64_t xclip_simloss_workspace_bytes(int64_t nq, int64_t nk) { return 2 * ((nk + 63) / 64) * nq * 4; }

// the gemm3-based head kernels take bf16 problems at least a tile wide whose feature dim is a whole number of K steps
inline bool use_sim3(int64_t nq, int64_t nk, int64_t d, int dtype) {
    return dtype == XCLIP_BF16 && d % G2_BK == 0 && nq >= 128 && nk >= 128;
}
extern "C++" inline dim3 sim3_grid(int64_t nq, int64_t nk) {
    int64_t tiles = ((nq + G2_BM - 1) / G2_BM) * ((nk + G2_BN - 1) / G2_BN);
    const int cus = xc_num_cus();
    return dim3((unsigned)(tiles < cus ? tiles : cus));
}

// ---- what the six head entry points share (InfoNCE, rank and sigmoid; partial / pos / grad) ----
extern "C++" {
// -> what is wrong with the arguments, or null.  nq, nk and diag_off become int fields of SimParams.
static const char* sim_bad_args(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, int64_t diag_off, int dtype) {
    if (!dtype_ok(dtype)) return "bad dtype";
    if (!(nq > 0 && nk > 0 && d > 0 && d % vec_of(dtype) == 0)) return "bad shape (d must be a multiple of the 16-byte chunk)";
    if (!(aligned16(Q) && aligned16(K))) return "Q and K must be 16-byte aligned";
    if (!(nq < (1LL << 31) && nk < (1LL << 31) && d < (1LL << 31) && diag_off > -(1LL << 31) && diag_off < (1LL << 31)))
        return "problem too large for 32-bit indices";
    return nullptr;
}
// the same for G of the two grads
static const char* sim_bad_g(const void* G, int64_t ldg, int64_t nq, int64_t nk, int64_t d, int dtype) {
    const int vec = vec_of(dtype);
    if (!(ldg % vec == 0 && ldg >= (nk + vec - 1) / vec * vec)) return "ldg must cover nk rounded up to the chunk";
    if (!aligned16(G)) return "G must be 16-byte aligned";
    if (use_sim3(nq, nk, d, dtype) && !(255 * ldg * 2 + 512 < (1LL << 32))) return "ldg too large for the line stores";
    return nullptr;
}
#define XC_SIM_REQUIRE(what) do { if (const char* bad_ = (what)) return xcapi::fail(__func__, bad_); } while (0)

// the forward's fields; everything else zero
static SimParams sim_params(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                            int64_t diag_off, int dcl) {
    SimParams p;
    memset(&p, 0, sizeof(p));
    p.Q = Q; p.K = K; p.nq = (int)nq; p.nk = (int)nk; p.d = (int)d; p.scale = scale; p.log_scale = log_scale;
    p.diag_off = (int)diag_off; p.dcl = dcl;
    p.tiles_m = (int)((nq + 127) / 128); p.tiles_n = (int)((nk + 127) / 128);
    return p;
}

// one launch over every tile: the general kernel of the dtype.  (The kernels are template arguments: XC_ALLOW_LDS keeps one flag per kernel.)
template <typename P, void (*GENERAL_BF16)(P), void (*GENERAL_F32)(P)>
static void sim_launch_general(const P& p, const SimParams& s, int dtype, hipStream_t st) {
    dim3 grid(s.tiles_m * s.tiles_n), block(256);
    if (dtype == XCLIP_BF16) {
        XC_ALLOW_LDS(*GENERAL_BF16, GemmCfg<bf16_t>::LDS_BYTES);
        hipLaunchKernelGGL(GENERAL_BF16, grid, block, GemmCfg<bf16_t>::LDS_BYTES, st, p);
    } else {
        XC_ALLOW_LDS(*GENERAL_F32, GemmCfg<float>::LDS_BYTES);
        hipLaunchKernelGGL(GENERAL_F32, grid, block, GemmCfg<float>::LDS_BYTES, st, p);
    }
}
// ... or the ring kernel where use_sim3 takes the problem (the three partials)
template <typename P, void (*RING)(P), void (*GENERAL_BF16)(P), void (*GENERAL_F32)(P)>
static void sim_launch(const P& p, const SimParams& s, int dtype, hipStream_t st) {
    if (!use_sim3(s.nq, s.nk, s.d, dtype)) return sim_launch_general<P, GENERAL_BF16, GENERAL_F32>(p, s, dtype, st);
    XC_ALLOW_LDS(*RING, G5_LDS_BYTES);
    hipLaunchKernelGGL(RING, sim3_grid(s.nq, s.nk), dim3(G2_THREADS), G5_LDS_BYTES, st, p);
}

// G of a use_sim3 problem (simloss5.h): every full 256 x 256 tile (on the diagonal or off it) on the ring loop with a spill-free epilogue
// of its own -- streamed stores for a G larger than the L2s can hold anyway -- if there is a full tile at all; tiles at a ragged edge, if
// there are any, through the general epilogue over a tile list (Sim5EdgeTiles) in a second launch.
// (without_full / without_edge: the measurement build's split of the two)
template <typename P, void (*FULL_STREAMED)(P), void (*FULL)(P), void (*EDGE)(P)>
static void sim_launch_g(const P& p, const SimParams& s, hipStream_t st, bool without_full = false, bool without_edge = false) {
    const int64_t nq = s.nq, nk = s.nk;
    if (!without_full && nq >= G2_BM && nk >= G2_BN) {
        if (nq * s.ldg * 2 > (48LL << 20)) {
            XC_ALLOW_LDS(*FULL_STREAMED, G5_LDS_BYTES);
            hipLaunchKernelGGL(FULL_STREAMED, sim3_grid(nq, nk), dim3(G2_THREADS), G5_LDS_BYTES, st, p);
        } else {
            XC_ALLOW_LDS(*FULL, G5_LDS_BYTES);
            hipLaunchKernelGGL(FULL, sim3_grid(nq, nk), dim3(G2_THREADS), G5_LDS_BYTES, st, p);
        }
    }
    const int64_t tm = (nq + G2_BM - 1) / G2_BM, tn = (nk + G2_BN - 1) / G2_BN;
    const int64_t nedge = ((nk % G2_BN) ? tm : 0) + ((nq % G2_BM) ? tn : 0);    // Sim5EdgeTiles::count
    if (without_edge || nedge == 0) return;
    const int cus = xc_num_cus();
    XC_ALLOW_LDS(*EDGE, G2_LDS_BYTES);
    hipLaunchKernelGGL(EDGE, dim3((unsigned)(nedge < cus ? nedge : cus)), dim3(G2_THREADS), G2_LDS_BYTES, st, p);
}
}  // extern "C++"

int xclip_simloss_partial(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                          int64_t diag_off, int dcl, void* workspace, int64_t tile_slot0, int64_t tile_slots, float* pos, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_REQUIRE(workspace != nullptr, "workspace required");
    XC_REQUIRE(tile_slot0 >= 0 && tile_slot0 + (nk + 63) / 64 <= tile_slots, "column slots out of range");
    SimParams p = sim_params(Q, K, nq, nk, d, scale, log_scale, diag_off, dcl);
    p.part_m = (float*)workspace + tile_slot0 * nq; p.part_l = (float*)workspace + (tile_slots + tile_slot0) * nq; p.pos = pos;
    hipStream_t st = (hipStream_t)stream;
    static const int gen = measure_env("XCLIP_SIM", 5);          // measurement build: 3 = the round-1 two-stage loop (simloss3.h)
    if (gen == 3 && use_sim3(nq, nk, d, dtype)) {
        XC_ALLOW_LDS(sim3_lse_kernel, G2_LDS_BYTES);
        hipLaunchKernelGGL(sim3_lse_kernel, sim3_grid(nq, nk), dim3(G2_THREADS), G2_LDS_BYTES, st, p);
    } else {
        sim_launch<SimParams, sim5_lse_kernel, sim_lse_partial_kernel<bf16_t>, sim_lse_partial_kernel<float>>(p, p, dtype, st);
    }
    return check_launch(__func__);
}

int xclip_simloss_combine(const void* workspace, int64_t nq, int64_t tile_slots, const float* pos, float* lse, float* loss_accum,
                          float coef, void* stream) {
    XC_REQUIRE(nq > 0 && tile_slots > 0 && workspace != nullptr && pos != nullptr && lse != nullptr, "bad arguments");
    const float* part_m = (const float*)workspace;
    hipLaunchKernelGGL(sim_lse_combine_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(1024), 2 * 16 * 64 * 4, (hipStream_t)stream, part_m,
                       part_m + tile_slots * nq, pos, lse, loss_accum, (int)nq, (int)tile_slots, coef);
    return check_launch(__func__);
}

int xclip_simloss_fwd(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                      int64_t diag_off, int dcl, float coef, void* workspace, float* pos, float* lse, float* loss_accum, int dtype,
                      void* stream) {
    const int64_t slots = (nk + 63) / 64;
    const int rc = xclip_simloss_partial(Q, K, nq, nk, d, scale, log_scale, diag_off, dcl, workspace, 0, slots, pos, dtype, stream);
    if (rc != 0) return rc;
    return xclip_simloss_combine(workspace, nq, slots, pos, lse, loss_accum, coef, stream);
}

// ---- in-batch retrieval metrics on the head's tile loop (kernels/simrank.h; reference x_clip.py:813-847) ----
int64_t xclip_simrank_workspace_bytes(int64_t nq, int64_t nk) { return 3 * ((nk + 63) / 64) * nq * 4; }

int xclip_simrank_pos(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                      int64_t diag_off, float* thr, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_REQUIRE(thr != nullptr, "thr required");
    dim3 grid((unsigned)((nq + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((simrank_pos_kernel<T>), grid, block, 0, st, (const T*)Q, (const T*)K, (int)nq, (int)nk, (int)d, scale, log_scale, (int)diag_off, thr);
    });
    return check_launch(__func__);
}

int xclip_simrank_partial(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                          int64_t diag_off, int64_t col0, const float* thr, void* workspace, int64_t tile_slot0, int64_t tile_slots,
                          int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_REQUIRE(workspace != nullptr && thr != nullptr, "workspace and thr required");
    XC_REQUIRE(col0 >= 0 && col0 + nk < (1LL << 31), "problem too large for 32-bit column indices");
    XC_REQUIRE(tile_slot0 >= 0 && tile_slot0 + (nk + 63) / 64 <= tile_slots, "column slots out of range");
    SimRankParams p;
    memset(&p, 0, sizeof(p));
    p.s = sim_params(Q, K, nq, nk, d, scale, log_scale, diag_off, 0);
    p.thr = thr; p.col0 = (int)col0;
    p.cnt = (uint32_t*)workspace + tile_slot0 * nq;
    p.hmax = (float*)workspace + (tile_slots + tile_slot0) * nq;
    p.harg = (int*)workspace + (2 * tile_slots + tile_slot0) * nq;
    sim_launch<SimRankParams, sim5_rank_kernel, sim_rank_partial_kernel<bf16_t>, sim_rank_partial_kernel<float>>(p, p.s, dtype, (hipStream_t)stream);
    return check_launch(__func__);
}

int xclip_simrank_combine(const void* workspace, int64_t nq, int64_t tile_slots, int32_t* rank, float* hard_val, int32_t* hard_idx,
                          void* stream) {
    XC_REQUIRE(nq > 0 && tile_slots > 0 && workspace != nullptr && rank != nullptr && hard_val != nullptr && hard_idx != nullptr, "bad arguments");
    const uint32_t* cnt = (const uint32_t*)workspace;
    hipLaunchKernelGGL(simrank_combine_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(1024), 3 * 16 * 64 * 4, (hipStream_t)stream, cnt,
                       (const float*)workspace + tile_slots * nq, (const int*)workspace + 2 * tile_slots * nq, rank, hard_val, hard_idx,
                       (int)nq, (int)tile_slots);
    return check_launch(__func__);
}

// ---- retrieval / zero-shot top-k on the head's tile loop (kernels/simtopk.h; the logits of x_clip.py:813-847) ----
// workspace: the rank partial's three tables (cnt, hmax, harg: the first sweep IS xclip_simrank_partial), then the two mask words
int64_t xclip_simtopk_workspace_bytes(int64_t nq, int64_t nk) { return 5 * ((nk + 63) / 64) * nq * 4; }

int xclip_simtopk_select(const void* workspace, int64_t nq, int64_t tile_slots, int64_t k, float* tau, void* stream) {
    XC_REQUIRE(k >= 1 && k <= SIMTOPK_MAX_K, "k must lie in 1 .. 32");
    XC_REQUIRE(nq > 0 && tile_slots > 0 && nq < (1LL << 31) && tile_slots < (1LL << 31) && workspace != nullptr && tau != nullptr, "bad arguments");
    hipLaunchKernelGGL(simtopk_select_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace + tile_slots * nq, tau, (int)nq, (int)tile_slots, (int)k);
    return check_launch(__func__);
}

int xclip_simtopk_mask(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                       const float* tau, void* workspace, int64_t tile_slot0, int64_t tile_slots, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, 0, dtype));
    XC_REQUIRE(workspace != nullptr && tau != nullptr, "workspace and tau required");
    XC_REQUIRE(tile_slot0 >= 0 && tile_slot0 + (nk + 63) / 64 <= tile_slots, "column slots out of range");
    SimTopkParams p;
    memset(&p, 0, sizeof(p));
    // (diag_off: no row reaches it, so that every full tile takes the epilogue's plain form -- as in the first sweep)
    p.s = sim_params(Q, K, nq, nk, d, scale, log_scale, -(1LL << 30), 0);
    p.tau = tau;
    p.mlo = (uint32_t*)workspace + (3 * tile_slots + tile_slot0) * nq;
    p.mhi = (uint32_t*)workspace + (4 * tile_slots + tile_slot0) * nq;
    sim_launch<SimTopkParams, sim5_mask_kernel, sim_mask_partial_kernel<bf16_t>, sim_mask_partial_kernel<float>>(p, p.s, dtype, (hipStream_t)stream);
    return check_launch(__func__);
}

int xclip_simtopk_finish(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                         int64_t col0, const void* workspace, int64_t tile_slot0, int64_t tile_slots, int64_t k, float* values,
                         int32_t* indices, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, 0, dtype));
    XC_REQUIRE(k >= 1 && k <= SIMTOPK_MAX_K, "k must lie in 1 .. 32");
    XC_REQUIRE(workspace != nullptr && values != nullptr && indices != nullptr, "workspace, values and indices required");
    XC_REQUIRE(col0 >= 0 && col0 + nk < (1LL << 31), "problem too large for 32-bit column indices");
    XC_REQUIRE(tile_slot0 >= 0 && tile_slot0 + (nk + 63) / 64 <= tile_slots, "column slots out of range");
    const uint32_t* mlo = (const uint32_t*)workspace + (3 * tile_slots + tile_slot0) * nq;
    const uint32_t* mhi = (const uint32_t*)workspace + (4 * tile_slots + tile_slot0) * nq;
    dim3 grid((unsigned)((nq + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((simtopk_finish_kernel<T>), grid, block, 0, st, (const T*)Q, (const T*)K, (int)nq, (int)nk, (int)d, scale, log_scale, (int)col0, mlo, mhi, (int)k, values, indices);
    });
    return check_launch(__func__);
}

// ---- pairwise sigmoid (SigLIP) loss on the head's tile loop (kernels/sigloss.h; similarity of x_clip.py:813-817) ----
int64_t xclip_sigloss_workspace_bytes(int64_t nq, int64_t nk) { return ((nk + 63) / 64) * nq * 4; }

int xclip_sigloss_partial(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                          const float* bias, int64_t diag_off, void* workspace, int64_t tile_slot0, int64_t tile_slots, int dtype,
                          void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_REQUIRE(workspace != nullptr && bias != nullptr, "workspace and bias required");
    XC_REQUIRE(tile_slot0 >= 0 && tile_slot0 + (nk + 63) / 64 <= tile_slots, "column slots out of range");
    SigParams p;
    memset(&p, 0, sizeof(p));
    p.s = sim_params(Q, K, nq, nk, d, scale, log_scale, diag_off, 0);
    p.bias = bias;
    p.part = (float*)workspace + tile_slot0 * nq;
    sim_launch<SigParams, sig5_loss_kernel, sig_partial_kernel<bf16_t>, sig_partial_kernel<float>>(p, p.s, dtype, (hipStream_t)stream);
    return check_launch(__func__);
}

int xclip_sigloss_combine(const void* workspace, int64_t nq, int64_t tile_slots, float* rowloss, float* loss_accum, float coef,
                          void* stream) {
    XC_REQUIRE(nq > 0 && nq < (1LL << 31) && tile_slots > 0 && workspace != nullptr && rowloss != nullptr, "bad arguments");
    hipLaunchKernelGGL(sigloss_combine_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(1024), 16 * 64 * 4, (hipStream_t)stream,
                       (const float*)workspace, rowloss, (int)nq, (int)tile_slots);
    if (loss_accum != nullptr)
        hipLaunchKernelGGL(sigloss_total_kernel, dim3(1), dim3(1024), 16 * 4, (hipStream_t)stream, (const float*)rowloss, loss_accum, (int)nq, coef);
    return check_launch(__func__);
}

int xclip_sigloss_grad(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                       const float* bias, int64_t diag_off, float coef, const float* gmul, int g_times_scale, void* G, int64_t ldg,
                       float* dtau_accum, float* dbias_accum, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_SIM_REQUIRE(sim_bad_g(G, ldg, nq, nk, d, dtype));
    XC_REQUIRE(bias != nullptr, "bias required");
    SigParams p;
    memset(&p, 0, sizeof(p));
    p.s = sim_params(Q, K, nq, nk, d, scale, log_scale, diag_off, 0);
    p.s.gmul = gmul; p.s.g_times_scale = g_times_scale; p.s.G = G; p.s.ldg = ldg; p.s.dtau = dtau_accum;
    p.bias = bias; p.coef = coef; p.dbias = dbias_accum;
    hipStream_t st = (hipStream_t)stream;
    if (use_sim3(nq, nk, d, dtype))
        sim_launch_g<SigParams, sig5_grad_kernel<true>, sig5_grad_kernel<false>, sig5_grad_edge_kernel>(p, p.s, st);
    else
        sim_launch_general<SigParams, sig_grad_kernel<bf16_t>, sig_grad_kernel<float>>(p, p.s, dtype, st);
    return check_launch(__func__);
}

// ---- fused MLM vocabulary head on the head's tile loop (kernels/vocabce.h; mlm.py:100-107) ----
// workspace (floats): the bias row as fp32 padded to whole 256-column tiles | part_m, part_l [slots][rows] | zlab [rows] | rowloss [rows]
inline int64_t vocab_bias_cols(int64_t vocab) { return (vocab + 255) / 256 * 256; }
int64_t xclip_vocab_ce_workspace_bytes(int64_t rows, int64_t vocab) {
    return (vocab_bias_cols(vocab) + (2 * ((vocab + 63) / 64) + 2) * rows) * 4;
}
static void vocab_bias(const void* bias, float* out, int64_t vocab, int dtype, hipStream_t st) {
    const int64_t padded = vocab_bias_cols(vocab);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((vocab_bias_kernel<T>), dim3((unsigned)(padded / 256)), dim3(256), 0, st, (const T*)bias, out, (int)vocab, (int)padded);
    });
}

int xclip_vocab_ce_fwd(const void* x, const void* W, const void* bias, const int64_t* labels, int64_t rows, int64_t vocab, int64_t dim,
                       void* workspace, float* lse, float* loss_accum, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0, "bad shape");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_SIM_REQUIRE(sim_bad_args(x, W, rows, vocab, dim, 0, dtype));
    XC_REQUIRE(bias && labels && lse && loss_accum && workspace && aligned16(workspace), "null or misaligned pointer");
    VocabParams p;
    memset(&p, 0, sizeof(p));
    p.s = sim_params(x, W, rows, vocab, dim, 1.0f, nullptr, 0, 0);
    const int64_t slots = (vocab + 63) / 64;
    float* ws = (float*)workspace;
    p.bias = ws;
    p.s.part_m = ws + vocab_bias_cols(vocab); p.s.part_l = p.s.part_m + slots * rows; p.s.pos = p.s.part_l + slots * rows;
    float* rowloss = p.s.pos + rows;
    p.label = (const long long*)labels;
    hipStream_t st = (hipStream_t)stream;
    vocab_bias(bias, ws, vocab, dtype, st);
    sim_launch<VocabParams, vocab5_lse_kernel, vocab_lse_partial_kernel<bf16_t>, vocab_lse_partial_kernel<float>>(p, p.s, dtype, st);
    hipLaunchKernelGGL(vocab_combine_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(1024), 2 * 16 * 64 * 4, st, (const float*)p.s.part_m,
                       (const float*)p.s.part_l, (const float*)p.s.pos, lse, rowloss, (int)rows, (int)slots);
    hipLaunchKernelGGL(sigloss_total_kernel, dim3(1), dim3(1024), 16 * 4, st, (const float*)rowloss, loss_accum, (int)rows, 1.0f);
    return check_launch(__func__);
}

int xclip_vocab_ce_bwd(const void* x, const void* W, const void* bias, const int64_t* labels, const float* lse, const float* gmul,
                       int64_t rows, int64_t vocab, int64_t dim, void* G, int64_t ldg, void* workspace, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0, "bad shape");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_SIM_REQUIRE(sim_bad_args(x, W, rows, vocab, dim, 0, dtype));
    XC_SIM_REQUIRE(sim_bad_g(G, ldg, rows, vocab, dim, dtype));
    XC_REQUIRE(bias && labels && lse && gmul && workspace && aligned16(workspace), "null or misaligned pointer");
    VocabParams p;
    memset(&p, 0, sizeof(p));
    p.s = sim_params(x, W, rows, vocab, dim, 1.0f, nullptr, 0, 0);
    p.s.lse_q = lse; p.s.gmul = gmul; p.s.G = G; p.s.ldg = ldg;
    p.bias = (const float*)workspace;
    p.label = (const long long*)labels;
    hipStream_t st = (hipStream_t)stream;
    vocab_bias(bias, (float*)workspace, vocab, dtype, st);
    if (use_sim3(rows, vocab, dim, dtype))
        sim_launch_g<VocabParams, vocab5_grad_kernel<true>, vocab5_grad_kernel<false>, vocab5_grad_edge_kernel>(p, p.s, st);
    else
        sim_launch_general<VocabParams, vocab_grad_kernel<bf16_t>, vocab_grad_kernel<float>>(p, p.s, dtype, st);
    return check_launch(__func__);
}

int xclip_simloss_grad(const void* Q, const void* K, int64_t nq, int64_t nk, int64_t d, float scale, const float* log_scale,
                       int64_t diag_off, int dcl, float a, float c, float e, const float* gmul, int g_times_scale,
                       const float* lse_q, const float* lse_k, void* G, int64_t ldg, float* dtau_accum, int dtype, void* stream) {
    XC_SIM_REQUIRE(sim_bad_args(Q, K, nq, nk, d, diag_off, dtype));
    XC_SIM_REQUIRE(sim_bad_g(G, ldg, nq, nk, d, dtype));
    SimParams p = sim_params(Q, K, nq, nk, d, scale, log_scale, diag_off, dcl);
    p.gmul = gmul; p.g_times_scale = g_times_scale;
    p.lse_q = lse_q; p.lse_k = lse_k; p.a = a; p.c = c; p.e = e; p.G = G; p.ldg = ldg; p.dtau = dtau_accum;
    hipStream_t st = (hipStream_t)stream;
    if (!use_sim3(nq, nk, d, dtype)) {
        sim_launch_general<SimParams, sim_grad_kernel<bf16_t>, sim_grad_kernel<float>>(p, p, dtype, st);
        return check_launch(__func__);
    }
    // XCLIP_SIM (measurement build): 3 = simloss3.h alone (one launch, every tile through the general epilogue: 355 - 368 us at
    // 4096 x 32768 x 512), 5 = the first ring form (whole-line epilogue with the general tile in the same function: 423 us),
    // 7 = the full-tile launch alone, 8 = the edge launch alone (the split of the two)
    bool without_full = false, without_edge = false;
#ifdef XCLIP_MEASURE
    static const int gen = measure_env("XCLIP_SIM", 0);
    if (gen == 5) {
        XC_ALLOW_LDS(sim5_grad_kernel, G5_LDS_BYTES);
        hipLaunchKernelGGL(sim5_grad_kernel, sim3_grid(nq, nk), dim3(G2_THREADS), G5_LDS_BYTES, st, p);
        return check_launch(__func__);
    }
    if (gen == 3) {
        XC_ALLOW_LDS(sim3_grad_kernel, G2_LDS_BYTES);
        hipLaunchKernelGGL(sim3_grad_kernel, sim3_grid(nq, nk), dim3(G2_THREADS), G2_LDS_BYTES, st, p);
        return check_launch(__func__);
    }
    without_full = gen == 8;
    without_edge = gen == 7;
    static const int simg = measure_env("XCLIP_SIMG", 0);      // A/B of the additions to the G kernel (simloss5.h VAR), streamed form only
#define XC_SIMG(V) case V: sim_launch_g<SimParams, sim5_grad_fast_kernel<true, V>, sim5_grad_fast_kernel<false>, sim5_grad_edge_kernel>(p, p, st, without_full, without_edge); return check_launch(__func__);
    switch (simg) { XC_SIMG(1) XC_SIMG(2) XC_SIMG(3) XC_SIMG(4) }
#undef XC_SIMG
#endif
    sim_launch_g<SimParams, sim5_grad_fast_kernel<true>, sim5_grad_fast_kernel<false>, sim5_grad_edge_kernel>(p, p, st, without_full, without_edge);
    return check_launch(__func__);
}

int xclip_simreg_diff(const void* A, int64_t lda, const void* C, int64_t ldc, void* D, int64_t ldd, int64_t rows, int64_t cols,
                      int64_t diag_off, float* sumsq_accum, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    const int vec = vec_of(dtype);
    XC_REQUIRE(rows >= 0 && cols > 0 && cols % vec == 0 && lda % vec == 0 && ldc % vec == 0 && ldd % vec == 0,
               "cols and the row strides must be multiples of the 16-byte chunk");
    XC_REQUIRE(lda >= cols && ldc >= cols && ldd >= cols, "row stride smaller than the row");
    XC_REQUIRE(A && C && D && aligned16(A) && aligned16(C) && aligned16(D), "null or misaligned pointer");
    if (rows == 0) return 0;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((simreg_diff_kernel<T>), grid, block, 16, (hipStream_t)stream, (const T*)A, (long)lda, (const T*)C, (long)ldc, (T*)D, (long)ldd, (int)rows, (int)cols, (int)diag_off, sumsq_accum);
    });
    return check_launch(__func__);
}

namespace {
constexpr int BN_MAX_SLICES = 256;
inline ColNormGeom colnorm_geom(int64_t rows, int64_t cols, int dtype) {
    const int nch = (int)(cols / vec_of(dtype));
    ColNormGeom g;
    g.cw = 64;
    if (nch < 64) { g.cw = 1; while (g.cw < nch) g.cw *= 2; }
    g.slabs = (nch + g.cw - 1) / g.cw;
    const int64_t rows_per_wg = 4 * (64 / g.cw);
    int64_t slices = 2048 / g.slabs;
    const int64_t useful = (rows + rows_per_wg - 1) / rows_per_wg;
    if (slices > useful) slices = useful;
    if (slices > BN_MAX_SLICES) slices = BN_MAX_SLICES;
    if (slices < 1) slices = 1;
    g.slices = (int)slices;
    return g;
}
}  // namespace

int64_t xclip_batchnorm_workspace_bytes(int64_t rows, int64_t cols) {
    (void)rows;
    return (int64_t)(2 * BN_MAX_SLICES + 2) * cols * (int64_t)sizeof(float);
}

int xclip_batchnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, float* running_mean,
                        float* running_var, float momentum, float eps, int training, int relu, int64_t rows, int64_t cols,
                        void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows > 0 && cols > 0 && cols % vec_of(dtype) == 0 && rows < (1LL << 31) && cols < (1LL << 24), "cols must be a multiple of the 16-byte chunk");
    XC_REQUIRE(x && y && mean && rstd && aligned16(x) && aligned16(y), "null or misaligned pointer");
    XC_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var come together");
    XC_REQUIRE(training || running_mean, "evaluation mode needs the running statistics");
    XC_REQUIRE(!training || rows > 1, "Expected more than 1 value per channel when training");
    XC_REQUIRE(!training || (workspace && workspace_bytes >= xclip_batchnorm_workspace_bytes(rows, cols)), "workspace too small");
    const ColNormGeom g = colnorm_geom(rows, cols, dtype);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)g.slabs, (unsigned)g.slices), block(256);
    const int R = (int)rows, C = (int)cols;
    const int fin_blocks = (C + 63) / 64;              // finalize: 64 columns x 4 slice strips per work-group
    float* part = (float*)workspace;
    if (training) {
        const int lds = 256 * 2 * vec_of(dtype) * (int)sizeof(float);
        by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
            hipLaunchKernelGGL((bn_stats_kernel<T>), grid, block, lds, st, (const T*)x, part, R, C, g.cw);
            hipLaunchKernelGGL((bn_finalize_kernel<T>), dim3(fin_blocks), block, 2048, st, (const T*)x, part, g.slices, R, C, eps, momentum,
                               mean, rstd, running_mean, running_var);
        });
    } else {
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3(fin_blocks), block, 0, st, running_mean, running_var, eps, mean, rstd, C);
    }
#define BN_APPLY(RELU) hipLaunchKernelGGL((bn_apply_kernel<T, RELU>), grid, block, 0, st, (const T*)x, mean, rstd, gamma, beta, (T*)y, R, C, g.cw)
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (relu) BN_APPLY(true); else BN_APPLY(false);
    });
#undef BN_APPLY
    return check_launch(__func__);
}

int xclip_batchnorm_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        void* dx, float* dgamma, float* dbeta, int training, int relu, int64_t rows, int64_t cols, void* workspace,
                        int64_t workspace_bytes, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows > 0 && cols > 0 && cols % vec_of(dtype) == 0 && rows < (1LL << 31) && cols < (1LL << 24), "cols must be a multiple of the 16-byte chunk");
    XC_REQUIRE(x && dy && dx && mean && rstd && aligned16(x) && aligned16(dy) && aligned16(dx), "null or misaligned pointer");
    XC_REQUIRE(workspace && workspace_bytes >= xclip_batchnorm_workspace_bytes(rows, cols), "workspace too small");
    const ColNormGeom g = colnorm_geom(rows, cols, dtype);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)g.slabs, (unsigned)g.slices), block(256);
    const int R = (int)rows, C = (int)cols;
    float* part = (float*)workspace;
    float* coef = part + (int64_t)2 * BN_MAX_SLICES * cols;
    const BnCols cols_p{mean, rstd, gamma, beta};
    const int lds = 256 * 2 * vec_of(dtype) * (int)sizeof(float);
#define BN_BWD(RELU)                                                                                                                 \
    do {                                                                                                                             \
        hipLaunchKernelGGL((bn_bwd_sums_kernel<T, RELU>), grid, block, lds, st, (const T*)x, (const T*)dy, cols_p, part, R, C, g.cw); \
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), block, 2048, st, part, g.slices, R, C, training, dgamma, dbeta, coef); \
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, RELU>), grid, block, 0, st, (const T*)x, (const T*)dy, cols_p, coef, (T*)dx, R, C, g.cw); \
    } while (0)
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (relu) BN_BWD(true); else BN_BWD(false);
    });
#undef BN_BWD
    return check_launch(__func__);
}

int xclip_neg_cosine_fwd(const void* p, const void* z, int64_t rows, int64_t dim, float coef, float* cosv, float* rp, float* rz,
                         float* loss_accum, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec_of(dtype) == 0, "dim must be a multiple of the 16-byte chunk");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(p && z && cosv && rp && rz && loss_accum && aligned16(p) && aligned16(z), "null or misaligned pointer");
    int64_t blocks = (rows + 3) / 4;
    if (blocks > ROWLOSS_MAX_BLOCKS) blocks = ROWLOSS_MAX_BLOCKS;
    dim3 grid((unsigned)blocks), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((neg_cosine_fwd_kernel<T>), grid, block, 16, (hipStream_t)stream, (const T*)p, (const T*)z, (int)rows, (int)dim, coef, cosv, rp, rz, loss_accum);
    });
    return check_launch(__func__);
}

int xclip_neg_cosine_bwd(const void* p, const void* z, const float* cosv, const float* rp, const float* rz, const float* gmul, float coef,
                         void* dp, int64_t rows, int64_t dim, int dtype, void* stream) {
    XC_REQUIRE(dtype_ok(dtype), "bad dtype");
    XC_REQUIRE(rows >= 0 && dim > 0 && dim % vec_of(dtype) == 0, "dim must be a multiple of the 16-byte chunk");
    if (rows == 0) return 0;                                  // (an empty tensor has a null data pointer)
    XC_REQUIRE(p && z && cosv && rp && rz && gmul && dp && aligned16(p) && aligned16(z) && aligned16(dp), "null or misaligned pointer");
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((neg_cosine_bwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)p, (const T*)z, cosv, rp, rz, gmul, coef, (T*)dp, (int)rows, (int)dim);
    });
    return check_launch(__func__);
}

// ---- the optimizer step (kernels/optim.h) ---------------------------------------------------------------------------------------------
int xclip_gradnorm_partial(const void* table, int64_t chunk0, int64_t count, int g_dtype, float* partials, void* stream) {
    XC_REQUIRE(dtype_ok(g_dtype), "bad gradient dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 31), "bad chunk range");
    if (count == 0) return 0;
    XC_REQUIRE(table && partials && aligned16(table), "null or misaligned pointer");
    dim3 grid((unsigned)count), block(OPT_THREADS);
    by_dtype(g_dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((gradnorm_partial_kernel<T>), grid, block, 16, (hipStream_t)stream, (const OptChunk*)table, (int)chunk0, partials);
    });
    return check_launch(__func__);
}

int xclip_optim_prepare(const float* partials, int64_t n_chunks, float max_norm, int clip, void* state_block, int32_t* step_base,
                        const int32_t* absent, int64_t n_absent, void* stream) {
    XC_REQUIRE(n_chunks > 0 && n_chunks < (1ll << 31) && n_absent >= 0 && n_absent < (1ll << 31), "bad counts");
    XC_REQUIRE(partials && state_block && step_base && (n_absent == 0 || absent), "null pointer");
    XC_REQUIRE(!clip || (max_norm > 0.f && max_norm == max_norm), "max_norm must be positive");
    static_assert(sizeof(OptBlock) == 32 && sizeof(OptChunk) == 48, "x_clip_amd/optim.py builds these layouts");
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(OPT_THREADS), OPT_THREADS * 8, (hipStream_t)stream, partials, (int)n_chunks, max_norm,
                       clip ? 1 : 0, (OptBlock*)state_block, step_base, absent, (int)n_absent);
    return check_launch(__func__);
}

static AdamWArgs adamw_args(double lr, double beta1, double beta2, double eps, double weight_decay) {
    AdamWArgs a;
    a.decay = (float)(1.0 - lr * weight_decay);
    a.b1 = (float)beta1; a.omb1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2; a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
    return a;
}

int xclip_adamw_step(const void* table, int64_t chunk0, int64_t count, int p_dtype, int g_dtype, float* exp_avg, float* exp_avg_sq,
                     float* master, const void* state_block, int32_t* step_base, double lr, double beta1, double beta2, double eps,
                     double weight_decay, void* stream) {
    XC_REQUIRE(dtype_ok(p_dtype) && dtype_ok(g_dtype), "bad dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 31), "bad chunk range");
    XC_REQUIRE(lr >= 0.0 && lr < 1e30 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < 1e30 &&
               weight_decay >= 0.0 && weight_decay < 1e30, "bad hyper-parameter");
    if (count == 0) return 0;
    XC_REQUIRE(table && exp_avg && exp_avg_sq && state_block && step_base && aligned16(table) && aligned16(exp_avg) && aligned16(exp_avg_sq),
               "null or misaligned pointer");
    XC_REQUIRE(p_dtype == XCLIP_F32 || (master && aligned16(master)), "bf16 parameters need the fp32 master array");
    const AdamWArgs a = adamw_args(lr, beta1, beta2, eps, weight_decay);
    dim3 grid((unsigned)count), block(OPT_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define XC_ADAMW(P, G, M) hipLaunchKernelGGL((adamw_kernel<P, G, M>), grid, block, 0, st, (const OptChunk*)table, (int)chunk0, exp_avg, exp_avg_sq, master, (const OptBlock*)state_block, step_base, a)
    if (p_dtype == XCLIP_BF16) { if (g_dtype == XCLIP_BF16) XC_ADAMW(bf16_t, bf16_t, true); else XC_ADAMW(bf16_t, float, true); }
    else                       { if (g_dtype == XCLIP_BF16) XC_ADAMW(float, bf16_t, false); else XC_ADAMW(float, float, false); }
#undef XC_ADAMW
    return check_launch(__func__);
}

int xclip_adamw_ema_step(const void* table, int64_t chunk0, int64_t count, int p_dtype, int g_dtype, float* exp_avg, float* exp_avg_sq,
                         float* master, const void* state_block, int32_t* step_base, double lr, double beta1, double beta2, double eps,
                         double weight_decay, float* ema, double ema_decay, int ema_warmup, void* stream) {
    XC_REQUIRE(dtype_ok(p_dtype) && dtype_ok(g_dtype), "bad dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 31), "bad chunk range");
    XC_REQUIRE(lr >= 0.0 && lr < 1e30 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < 1e30 &&
               weight_decay >= 0.0 && weight_decay < 1e30, "bad hyper-parameter");
    XC_REQUIRE(ema_decay >= 0.0 && ema_decay < 1.0, "ema_decay must be in [0, 1)");
    if (count == 0) return 0;
    XC_REQUIRE(table && exp_avg && exp_avg_sq && ema && state_block && step_base && aligned16(table) && aligned16(exp_avg) &&
               aligned16(exp_avg_sq) && aligned16(ema), "null or misaligned pointer");
    XC_REQUIRE(p_dtype == XCLIP_F32 || (master && aligned16(master)), "bf16 parameters need the fp32 master array");
    const AdamWArgs a = adamw_args(lr, beta1, beta2, eps, weight_decay);
    dim3 grid((unsigned)count), block(OPT_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define XC_ADAMW_EMA(P, G, M) hipLaunchKernelGGL((adamw_ema_kernel<P, G, M>), grid, block, 0, st, (const OptChunk*)table, (int)chunk0, exp_avg, exp_avg_sq, master, ema, (const OptBlock*)state_block, step_base, a, ema_decay, ema_warmup ? 1 : 0)
    if (p_dtype == XCLIP_BF16) { if (g_dtype == XCLIP_BF16) XC_ADAMW_EMA(bf16_t, bf16_t, true); else XC_ADAMW_EMA(bf16_t, float, true); }
    else                       { if (g_dtype == XCLIP_BF16) XC_ADAMW_EMA(float, bf16_t, false); else XC_ADAMW_EMA(float, float, false); }
#undef XC_ADAMW_EMA
    return check_launch(__func__);
}

// param groups with trust_ratio / bounds (kernels/optim.h: lamb_norm_kernel, lamb_fold_kernel, optim_update_kernel)
static bool update_args(UpdateArgs& q, double lr, double beta1, double beta2, double eps, double weight_decay, double lo, double hi) {
    q.a = adamw_args(lr, beta1, beta2, eps, weight_decay);
    q.wd = (float)weight_decay;
    q.lo = (float)lo;
    q.hi = (float)hi;
    // the caller rounds the bounds to the parameter's storage type (lo up, hi down): a value float would round again is refused
    return (double)q.lo == lo && (double)q.hi == hi && q.lo <= q.hi;
}

int xclip_lamb_norm(const void* table, int64_t chunk0, int64_t count, int p_dtype, int g_dtype, const float* exp_avg, const float* exp_avg_sq,
                    const float* master, const void* state_block, const int32_t* step_base, double beta1, double beta2, double eps,
                    double weight_decay, float* pairs, void* stream) {
    XC_REQUIRE(dtype_ok(p_dtype) && dtype_ok(g_dtype), "bad dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 30), "bad chunk range");
    XC_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < 1e30 && weight_decay >= 0.0 &&
               weight_decay < 1e30, "bad hyper-parameter");
    if (count == 0) return 0;
    XC_REQUIRE(table && exp_avg && exp_avg_sq && state_block && step_base && pairs && aligned16(table) && aligned16(exp_avg) &&
               aligned16(exp_avg_sq), "null or misaligned pointer");
    XC_REQUIRE(p_dtype == XCLIP_F32 || (master && aligned16(master)), "bf16 parameters need the fp32 master array");
    UpdateArgs q;
    update_args(q, 0.0, beta1, beta2, eps, weight_decay, 0.0, 0.0);
    dim3 grid((unsigned)count), block(OPT_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define XC_LAMB_NORM(P, G, M) hipLaunchKernelGGL((lamb_norm_kernel<P, G, M>), grid, block, 32, st, (const OptChunk*)table, (int)chunk0, exp_avg, exp_avg_sq, master, (const OptBlock*)state_block, step_base, q, pairs)
    if (p_dtype == XCLIP_BF16) { if (g_dtype == XCLIP_BF16) XC_LAMB_NORM(bf16_t, bf16_t, true); else XC_LAMB_NORM(bf16_t, float, true); }
    else                       { if (g_dtype == XCLIP_BF16) XC_LAMB_NORM(float, bf16_t, false); else XC_LAMB_NORM(float, float, false); }
#undef XC_LAMB_NORM
    return check_launch(__func__);
}

int xclip_lamb_fold(const void* table, int64_t chunk0, int64_t count, const float* pairs, const void* state_block, float* ratio,
                    void* stream) {
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 30), "bad chunk range");
    if (count == 0) return 0;
    XC_REQUIRE(table && pairs && state_block && ratio && aligned16(table), "null or misaligned pointer");
    hipLaunchKernelGGL(lamb_fold_kernel, dim3((unsigned)((count + OPT_THREADS - 1) / OPT_THREADS)), dim3(OPT_THREADS), 0, (hipStream_t)stream,
                       (const OptChunk*)table, (int)chunk0, (int)count, pairs, (const OptBlock*)state_block, ratio);
    return check_launch(__func__);
}

int xclip_optim_update(const void* table, int64_t chunk0, int64_t count, int p_dtype, int g_dtype, float* exp_avg, float* exp_avg_sq,
                       float* master, const void* state_block, int32_t* step_base, double lr, double beta1, double beta2, double eps,
                       double weight_decay, const float* ratio, double lo, double hi, float* ema, double ema_decay, int ema_warmup,
                       void* stream) {
    XC_REQUIRE(dtype_ok(p_dtype) && dtype_ok(g_dtype), "bad dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 31), "bad chunk range");
    XC_REQUIRE(lr >= 0.0 && lr < 1e30 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < 1e30 &&
               weight_decay >= 0.0 && weight_decay < 1e30, "bad hyper-parameter");
    XC_REQUIRE(!ema || (ema_decay >= 0.0 && ema_decay < 1.0), "ema_decay must be in [0, 1)");
    UpdateArgs q;
    XC_REQUIRE(update_args(q, lr, beta1, beta2, eps, weight_decay, lo, hi), "bounds must be float values with lo <= hi (-inf / +inf: none)");
    if (count == 0) return 0;
    XC_REQUIRE(table && exp_avg && exp_avg_sq && state_block && step_base && aligned16(table) && aligned16(exp_avg) && aligned16(exp_avg_sq) &&
               (!ema || aligned16(ema)), "null or misaligned pointer");
    XC_REQUIRE(p_dtype == XCLIP_F32 || (master && aligned16(master)), "bf16 parameters need the fp32 master array");
    dim3 grid((unsigned)count), block(OPT_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define XC_UPDATE(P, G, M, T, E) hipLaunchKernelGGL((optim_update_kernel<P, G, M, T, E>), grid, block, 0, st, (const OptChunk*)table, (int)chunk0, exp_avg, exp_avg_sq, master, ema, ratio, (const OptBlock*)state_block, step_base, q, ema_decay, ema_warmup ? 1 : 0)
#define XC_UPDATE_PG(T, E)                                                                                                          \
    do {                                                                                                                            \
        if (p_dtype == XCLIP_BF16) { if (g_dtype == XCLIP_BF16) XC_UPDATE(bf16_t, bf16_t, true, T, E); else XC_UPDATE(bf16_t, float, true, T, E); } \
        else                       { if (g_dtype == XCLIP_BF16) XC_UPDATE(float, bf16_t, false, T, E); else XC_UPDATE(float, float, false, T, E); } \
    } while (0)
    if (ratio) { if (ema) XC_UPDATE_PG(true, true); else XC_UPDATE_PG(true, false); }
    else       { if (ema) XC_UPDATE_PG(false, true); else XC_UPDATE_PG(false, false); }
#undef XC_UPDATE_PG
#undef XC_UPDATE
    return check_launch(__func__);
}

int xclip_grad_accumulate(const void* table, int64_t chunk0, int64_t count, int g_dtype, float* acc, int materialise, void* stream) {
    XC_REQUIRE(dtype_ok(g_dtype), "bad gradient dtype");
    XC_REQUIRE(chunk0 >= 0 && count >= 0 && chunk0 + count < (1ll << 31), "bad chunk range");
    if (count == 0) return 0;
    XC_REQUIRE(table && acc && aligned16(table) && aligned16(acc), "null or misaligned pointer");
    dim3 grid((unsigned)count), block(OPT_THREADS);
    by_dtype(g_dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (materialise) hipLaunchKernelGGL((grad_accum_kernel<T, true>), grid, block, 0, (hipStream_t)stream, (const OptChunk*)table, (int)chunk0, acc);
        else hipLaunchKernelGGL((grad_accum_kernel<T, false>), grid, block, 0, (hipStream_t)stream, (const OptChunk*)table, (int)chunk0, acc);
    });
    return check_launch(__func__);
}

}  // extern "C"
