// xclip_attn.hip -- the attention entry points of include/xclip.h.  A translation unit of its own because it is compiled with
// -mllvm -amdgpu-mfma-vgpr-form: the attention kernels consume every MFMA result with VALU right away, and the default
// heuristic parked those accumulators in AGPRs (32 v_accvgpr_read per 12 MFMAs in the backward's inner loop); the same flag
// makes the contrastive-head kernels of the other unit spill.
#include "xc_device.h"

#include "api_common.h"
#include "kernels/attention.h"
#include "kernels/attention2.h"
#include "kernels/attention3.h"
#include "kernels/attention4.h"
#include "kernels/attention5.h"
#include "kernels/attention6.h"
#include "kernels/attention7.h"
#include "kernels/attention_pool.h"
#include "kernels/attention_varlen.h"
#include "kernels/pack_rows.h"

using namespace xc;
using namespace xcapi;

namespace {

template <typename T, int NW, int NH = 1>
void launch_attn_fwd(AttnParams p, hipStream_t st) {
    p.chunks = (p.n + NW * 32 - 1) / (NW * 32);
    constexpr int lds = attn_fwd_lds_bytes<T, NW, NH>();
    XC_ALLOW_LDS((attn_fwd_kernel<T, NW, NH>), lds);
    hipLaunchKernelGGL((attn_fwd_kernel<T, NW, NH>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds, st, p);
}
template <typename T, int NW, int NH = 1>
void launch_attn_bwd(AttnParams p, hipStream_t st) {
    p.chunks = (p.n + NW * 32 - 1) / (NW * 32);
    constexpr int lds_q = attn_dq_lds_bytes<T, NW, NH>(), lds_kv = attn_dkv_lds_bytes<T, NW, NH>();
    XC_ALLOW_LDS((attn_dq_kernel<T, NW, NH>), lds_q);
    XC_ALLOW_LDS((attn_dkv_kernel<T, NW, NH>), lds_kv);
    hipLaunchKernelGGL((attn_dq_kernel<T, NW, NH>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds_q, st, p);
    hipLaunchKernelGGL((attn_dkv_kernel<T, NW, NH>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds_kv, st, p);
}
template <int NW>
void launch_attn2_fwd(AttnParams p, hipStream_t st) {
    p.chunks = (p.n + NW * 32 - 1) / (NW * 32);
    constexpr int lds = attn2_lds_bytes<NW>();
    hipLaunchKernelGGL((attn2_fwd_kernel<NW>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds, st, p);
}
template <int NW>
void launch_attn2_bwd(AttnParams p, hipStream_t st) {
    p.chunks = (p.n + NW * 32 - 1) / (NW * 32);
    constexpr int lds = attn2_lds_bytes<NW>();
    hipLaunchKernelGGL((attn2_dq_kernel<NW>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds, st, p);
    hipLaunchKernelGGL((attn2_dkv_kernel<NW>), dim3(p.batch * p.heads * p.chunks), dim3(NW * 64), lds, st, p);
}
// waves per work-group: the NW in 1..4 that wastes the fewest padded rows (ties -> larger NW)
int attn_waves(int64_t n) {
    int best = 1;
    int64_t best_pad = -1;
    for (int nw = 1; nw <= 4; ++nw) {
        const int64_t rows = ((n + nw * 32 - 1) / (nw * 32)) * nw * 32;
        if (best_pad < 0 || rows <= best_pad) { best = nw; best_pad = rows; }
    }
    return best;
}

// the run-time wave count / causal flag as template arguments (api_common.h by_dtype)
template <typename F> inline void by_waves(int nw, F&& f) {
    switch (nw) { case 1: f(int_tag<1>{}); break; case 2: f(int_tag<2>{}); break; case 3: f(int_tag<3>{}); break; default: f(int_tag<4>{}); break; }
}
template <typename F> inline void by_causal(int causal, F&& f) {
    if (causal) f(bool_tag<true>{}); else f(bool_tag<false>{});
}

// ---- what xclip_attention_fwd and xclip_attention_bwd share ----
enum AttnRoute {
    ATTN_WIDE_RESIDENT,      // wide heads, head-resident (attention4.h)
    ATTN_WIDE_TILED,         // wide heads, long sequences / fp32 / dropout: the tiled kernels with two 64-wide halves per head
    ATTN_RESIDENT,           // head-resident kernels: one work-group per (batch, head) (attention3.h, attention5.h)
    ATTN_TILED_BF16,         // long bf16 sequences (attention2.h)
    ATTN_TILED,              // fp32, and bf16 with dropout (attention.h)
};
// tiled_only: dropout lives in the tiled kernels (attention.h)
inline AttnRoute attn_route(int64_t head_dim, int dtype, int64_t n, bool tiled_only) {
    const bool resident = dtype == XCLIP_BF16 && n <= A3_MAX_N && !tiled_only;
    if (head_dim == 128) return resident ? ATTN_WIDE_RESIDENT : ATTN_WIDE_TILED;
    if (resident) return ATTN_RESIDENT;
    return dtype == XCLIP_BF16 && !tiled_only ? ATTN_TILED_BF16 : ATTN_TILED;
}

struct AttnCall {                                             // the arguments both take
    const void* qkv; const uint8_t* mask; int64_t batch, n, heads, head_dim;
    float scale; int causal; float dropout_p; uint64_t dropout_seed; int dtype;
};
// the common checks (ptrs_aligned: the entry point's own pointers) and the common fields of AttnParams; -> 0, or 1 with the error recorded
// under the entry point's name `fn`.  An empty batch (the caller returns 0) stops before the dropout check, as it always has.
int attn_setup(const char* fn, const AttnCall& c, bool ptrs_aligned, AttnParams& p, AttnRoute& route) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(dtype_ok(c.dtype), "bad dtype");
    XC_REQ(c.batch >= 0 && c.n > 0 && c.heads > 0, "bad shape");
    XC_REQ(c.head_dim == 64 || c.head_dim == 128, "head_dim must be 64 or 128 (narrower / in-between widths are zero-padded by the caller)");
    XC_REQ(ptrs_aligned, "pointers must be 16-byte aligned");
    if (c.batch == 0) return 0;
    memset(&p, 0, sizeof(p));
    p.qkv = c.qkv; p.mask = c.mask;
    p.batch = (int)c.batch; p.n = (int)c.n; p.heads = (int)c.heads; p.scale = c.scale; p.causal = c.causal != 0;
    p.first_round = 2 * xc_num_cus();
    XC_REQ(c.dropout_p >= 0.f && c.dropout_p < 1.f, "dropout_p must lie in [0, 1)");
    p.drop_thresh = drop_thresh(c.dropout_p); p.drop_scale = 1.0f / (1.0f - c.dropout_p); p.drop_seed = c.dropout_seed;
    route = attn_route(c.head_dim, c.dtype, c.n, p.drop_thresh != 0);
    XC_REQ((route != ATTN_WIDE_RESIDENT && route != ATTN_RESIDENT) || c.scale > 0.f,
           "the head-resident kernels take the score maximum before scaling: scale must be positive");
    return 0;
#undef XC_REQ
}

// ---- the one-wave-per-unit kernel families (kernels/attention_pool.h: dense and packed pooled; kernels/attention_varlen.h: plain) ----
// F<T, HS>::fwd / ::bwd are the family's kernels; four waves to a work-group, `units` waves in all
template <template <typename, int> class F, typename T, typename P>
void launch_wave_per_unit(const P& p, int64_t units, int64_t head_dim, bool backward, hipStream_t st) {
    const dim3 grid((unsigned)((units + 3) / 4)), block(256);
    if (head_dim == 64) hipLaunchKernelGGL((backward ? F<T, 64>::bwd : F<T, 64>::fwd), grid, block, 0, st, p);
    else hipLaunchKernelGGL((backward ? F<T, 128>::bwd : F<T, 128>::fwd), grid, block, 0, st, p);
}
#define XC_WAVE_FAMILY(NAME, PARAMS, FWD, BWD) \
    template <typename T, int HS> struct NAME { static constexpr void (*fwd)(PARAMS) = FWD<T, HS>; static constexpr void (*bwd)(PARAMS) = BWD<T, HS>; }
XC_WAVE_FAMILY(PoolKernels, AttnPoolParams, attn_pool_fwd_kernel, attn_pool_bwd_kernel);
XC_WAVE_FAMILY(PoolVarlenKernels, AttnPoolVarlenParams, attn_pool_varlen_fwd_kernel, attn_pool_varlen_bwd_kernel);
XC_WAVE_FAMILY(VarlenPlainKernels, AttnVarlenParams, attn_varlen_plain_fwd_kernel, attn_varlen_plain_bwd_kernel);
#undef XC_WAVE_FAMILY
template <typename T, int HS> struct VarlenPlainCausalKernels {   // (the same kernel templates, CAUSAL = true)
    static constexpr void (*fwd)(AttnVarlenParams) = attn_varlen_plain_fwd_kernel<T, HS, true>;
    static constexpr void (*bwd)(AttnVarlenParams) = attn_varlen_plain_bwd_kernel<T, HS, true>;
};

// ---- one query row per (sample, head) (kernels/attention_pool.h) ----
// the common checks and fields of the dense pair; ptr_err: the entry point's own pointer complaint, or null; -> 0, or 1 with the error recorded
// under `fn`.  An empty batch passes every check (the caller returns 0)
int attn_pool_setup(const char* fn, const void* q, const void* kv, const uint8_t* mask, int64_t batch, int64_t n, int64_t heads, int64_t head_dim,
                    float scale, int64_t visible_keys, int dtype, const char* ptr_err, AttnPoolParams& p) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(dtype_ok(dtype), "bad dtype");
    XC_REQ(batch >= 0 && n > 0 && heads > 0 && visible_keys >= 1 && visible_keys <= n, "bad shape");
    XC_REQ(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128 (narrower / in-between widths are zero-padded by the caller)");
    XC_REQ(ptr_err == nullptr, ptr_err);
    memset(&p, 0, sizeof(p));
    p.q = q; p.kv = kv; p.mask = mask;
    p.batch = (int)batch; p.n = (int)n; p.heads = (int)heads; p.nvis = (int)visible_keys; p.scale = scale;
    return 0;
#undef XC_REQ
}
}  // namespace

extern "C" {

int xclip_attention_fwd(const void* qkv, const uint8_t* mask, void* out, float* lse, int64_t batch, int64_t n, int64_t heads,
                        int64_t head_dim, float scale, int causal, float dropout_p, uint64_t dropout_seed, int dtype, void* stream) {
    const AttnCall call{qkv, mask, batch, n, heads, head_dim, scale, causal, dropout_p, dropout_seed, dtype};
    AttnParams p; AttnRoute route;
    const int rc = attn_setup(__func__, call, aligned16(qkv) && aligned16(out), p, route);
    if (rc != 0 || batch == 0) return rc;
    p.out = out; p.lse = lse;
    hipStream_t st = (hipStream_t)stream;
    const dim3 hgrid((unsigned)(batch * heads));             // the head-resident kernels: one work-group per (batch, head)
    const int nw = attn_waves(n);                             // the tiled ones
    switch (route) {
    case ATTN_WIDE_RESIDENT: {
        const int nwq = a4_fwd_waves((int)n);
        XC_REQUIRE(attn4_fwd_lds_bytes((int)n) <= 160 * 1024, "internal: wide-head forward LDS");
        by_causal(causal, [&](auto c) {
            XC_ALLOW_LDS(attn4_fwd_kernel<decltype(c)::value>, 160 * 1024);
            hipLaunchKernelGGL(attn4_fwd_kernel<decltype(c)::value>, hgrid, dim3(nwq * 64), attn4_fwd_lds_bytes((int)n), st, p);
        });
        break;
    }
    case ATTN_WIDE_TILED:
        by_dtype(dtype, [&](auto t) { by_waves(nw, [&](auto w) { launch_attn_fwd<typename decltype(t)::type, decltype(w)::value, 2>(p, st); }); });
        break;
    case ATTN_RESIDENT: {
        const int nwq = a3_waves((int)n);
        // half a head's time (13 us at n = 257, growing with n^2) between the two work-groups of a CU: 0.413 -> 0.376 ms at
        // b = 1024, n = 257 (profiles/r02_run20_attention_stagger_sweep.log); XCLIP_ATTN_STAGGER_FWD=<10 ns ticks> overrides
        static const int stag = measure_env("XCLIP_ATTN_STAGGER_FWD", -1);
        const int half_head = (int)(1300.0 * (double)n * (double)n / (257.0 * 257.0));
        p.stagger_10ns = (attn3_fwd_lds_bytes((int)n) <= 80 * 1024 && batch * heads >= 1024) ? (stag >= 0 ? stag : half_head) : 0;
        static const int abl_f = measure_env("XCLIP_ATTN_ABL", 0);  // measurement build only: 4 = the tail row as a 33rd block (round-3 form)
        p.chunks = abl_f;
        by_causal(causal, [&](auto c) {
            XC_ALLOW_LDS(attn3_fwd_kernel<decltype(c)::value>, 160 * 1024);
            hipLaunchKernelGGL(attn3_fwd_kernel<decltype(c)::value>, hgrid, dim3(nwq * 64), attn3_fwd_lds_bytes((int)n), st, p);
        });
        break;
    }
    case ATTN_TILED_BF16:
        by_waves(nw, [&](auto w) { launch_attn2_fwd<decltype(w)::value>(p, st); });
        break;
    case ATTN_TILED:
        by_dtype(dtype, [&](auto t) { by_waves(nw, [&](auto w) { launch_attn_fwd<typename decltype(t)::type, decltype(w)::value>(p, st); }); });
        break;
    }
    return check_launch(__func__);
}

int xclip_attention_bwd(const void* qkv, const uint8_t* mask, const void* out, const void* dout, const float* lse,
                        float* delta_ws, void* dqkv, int64_t batch, int64_t n, int64_t heads, int64_t head_dim, float scale, int causal,
                        float dropout_p, uint64_t dropout_seed, int dtype, void* stream) {
    const AttnCall call{qkv, mask, batch, n, heads, head_dim, scale, causal, dropout_p, dropout_seed, dtype};
    AttnParams p; AttnRoute route;
    const int rc = attn_setup(__func__, call, aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv), p, route);
    if (rc != 0 || batch == 0) return rc;
    p.out = const_cast<void*>(out); p.lse = const_cast<float*>(lse); p.dout = dout; p.delta = delta_ws; p.dqkv = dqkv;
    hipStream_t st = (hipStream_t)stream;
    const dim3 hgrid((unsigned)(batch * heads));             // the head-resident kernels: one work-group per (batch, head)
    const dim3 dgrid((unsigned)((batch * n + 3) / 4)), dblock(256);   // the tiled ones' delta pass
    const int nw = attn_waves(n);
    switch (route) {
    case ATTN_WIDE_RESIDENT: {                                 // (computes delta itself)
        const int nwq = a3_bwd_waves((int)n);
        by_causal(causal, [&](auto c) {
            XC_ALLOW_LDS(attn4_bwd_kernel<decltype(c)::value>, 160 * 1024);
            hipLaunchKernelGGL(attn4_bwd_kernel<decltype(c)::value>, hgrid, dim3(nwq * 64), attn4_bwd_lds_bytes((int)n), st, p);
        });
        break;
    }
    case ATTN_WIDE_TILED:                                      // delta pass + the tiled dQ / dK, dV kernels on two halves
        XC_REQUIRE(delta_ws != nullptr, "wide heads need the [batch, heads, n] fp32 delta workspace");
        if (dtype == XCLIP_BF16)
            hipLaunchKernelGGL((attn_delta_kernel<bf16_t, 2>), dgrid, dblock, 0, st, (const bf16_t*)out, (const bf16_t*)dout, delta_ws, (int)batch, (int)n, (int)heads);
        else
            hipLaunchKernelGGL((attn_delta_kernel<float, 2>), dgrid, dblock, 0, st, (const float*)out, (const float*)dout, delta_ws, (int)batch, (int)n, (int)heads);
        by_dtype(dtype, [&](auto t) { by_waves(nw, [&](auto w) { launch_attn_bwd<typename decltype(t)::type, decltype(w)::value, 2>(p, st); }); });
        break;
    case ATTN_RESIDENT: {                                      // merged head-resident backward (computes delta itself)
        // the single-pass form (attention5.h) for the sequences it takes; XCLIP_ATTN_BWD=3 (measurement build) keeps the two-phase kernel for the A/B
        // (XCLIP_ATTN5_MIN=2: every sequence it can take, for the record of where it loses)
        // round 6: the streaming persistent form (attention6.h) for n = 256 / 257, XCLIP_ATTN_BWD=6 on the measurement build: correct on the
        // hardware and SLOWER than the single pass -- 975 against 813 us at n = 256, 1305 against 937 at n = 257 (b = 1024, 8 heads;
        // profiles/r06_f_attn_bwd_ab.log, ablations profiles/r06_g_attn6_abl.log) -- the product keeps attention5.h
        static const int bwd_gen = measure_env("XCLIP_ATTN_BWD", 5), min5 = measure_env("XCLIP_ATTN5_MIN", A5_MIN_BLOCKS);
        if (bwd_gen == 6 && a6_takes((int)n, causal)) {
            XC_ALLOW_LDS(attn6_bwd_kernel, 160 * 1024);
            const int64_t heads_total = batch * heads;
            const int cus = xc_num_cus();
            int64_t g6 = heads_total < cus ? heads_total : cus;
            static const int abl6 = measure_env("XCLIP_ATTN6_ABL", 0);    // measurement build only: attention6.h's ablation mask
            p.chunks = abl6;
            if (g6 >= 8) g6 &= ~(int64_t)7;                     // whole XCD rounds: a work-group's heads stay on one XCD's slice of the order
            hipLaunchKernelGGL(attn6_bwd_kernel, dim3((unsigned)g6), dim3(512), A6_LDS_BYTES, st, p);
            return check_launch(__func__);
        }
        if (bwd_gen == 7 && a5_takes((int)n, causal) && (n >> 5) >= min5 && attn5_bwd_lds_bytes((int)n) <= 160 * 1024) {
            // attention7.h (round 6, measurement build): attention5.h persistent, the next head's images requested (asm-issued DMA) under this
            // head's stores -- bit-identical, and SLOWER: 1018 against 942 us at n = 257, 846 against 808 at n = 256 (profiles/r06_n_attn7_ab.log);
            // requesting the images at the top of the head instead changes nothing (r06_o_attn7_abl.log, mask 2)
            XC_ALLOW_LDS(attn7_bwd_kernel, 160 * 1024);
            const int64_t heads_total = batch * heads;
            const int cus = xc_num_cus();
            int64_t g7 = heads_total < cus ? heads_total : cus;
            if (g7 >= 8) g7 &= ~(int64_t)7;
            static const int abl7 = measure_env("XCLIP_ATTN7_ABL", 0);    // measurement build only: attention7.h's ablation mask
            p.chunks = abl7;
            hipLaunchKernelGGL(attn7_bwd_kernel, dim3((unsigned)g7), dim3((unsigned)((n >> 5) * 64)), attn5_bwd_lds_bytes((int)n), st, p);
            return check_launch(__func__);
        }
        if (bwd_gen >= 5 && a5_takes((int)n, causal) && (n >> 5) >= min5 && attn5_bwd_lds_bytes((int)n) <= 160 * 1024) {
            XC_ALLOW_LDS(attn5_bwd_kernel, 160 * 1024);
            static const int var5 = measure_env("XCLIP_ATTN5_VAR", 0);     // measurement build only: attention5.h's variant mask
            p.chunks = var5;
            const int64_t g5 = batch * heads;
            hipLaunchKernelGGL(attn5_bwd_kernel, dim3((unsigned)g5), dim3((unsigned)((n >> 5) * 64)), attn5_bwd_lds_bytes((int)n), st, p);
            return check_launch(__func__);
        }
        const int nwq = a3_bwd_waves((int)n);
        static const int abl = measure_env("XCLIP_ATTN_ABL", 0);   // measurement build only
        p.chunks = abl;
        // (measured: no effect on the backward -- its two work-groups are latency-bound chains that already overlap)
        static const int stag = measure_env("XCLIP_ATTN_STAGGER_BWD", 0);
        p.stagger_10ns = (attn3_bwd_lds_bytes((int)n) <= 80 * 1024 && batch * heads >= 1024) ? stag : 0;
        by_causal(causal, [&](auto c) {
            XC_ALLOW_LDS(attn3_bwd_kernel<decltype(c)::value>, 160 * 1024);
            hipLaunchKernelGGL(attn3_bwd_kernel<decltype(c)::value>, hgrid, dim3(nwq * 64), attn3_bwd_lds_bytes((int)n), st, p);
        });
        break;
    }
    case ATTN_TILED_BF16:
    case ATTN_TILED:
        by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
            hipLaunchKernelGGL((attn_delta_kernel<T>), dgrid, dblock, 0, st, (const T*)out, (const T*)dout, delta_ws, (int)batch, (int)n, (int)heads);
        });
        if (route == ATTN_TILED_BF16) by_waves(nw, [&](auto w) { launch_attn2_bwd<decltype(w)::value>(p, st); });
        else by_dtype(dtype, [&](auto t) { by_waves(nw, [&](auto w) { launch_attn_bwd<typename decltype(t)::type, decltype(w)::value>(p, st); }); });
        break;
    }
    return check_launch(__func__);
}

int xclip_attention_pool_fwd(const void* q, const void* kv, const uint8_t* mask, void* out, float* lse, int64_t batch, int64_t n,
                             int64_t heads, int64_t head_dim, float scale, int64_t visible_keys, int dtype, void* stream) {
    AttnPoolParams p;
    const bool ptrs_ok = q && kv && out && lse && aligned16(q) && aligned16(kv) && aligned16(out);
    const int rc = attn_pool_setup(__func__, q, kv, mask, batch, n, heads, head_dim, scale, visible_keys, dtype,
                                   ptrs_ok ? nullptr : "pointers must be non-null and 16-byte aligned", p);
    if (rc != 0 || batch == 0) return rc;
    p.out = out; p.lse = lse;
    by_dtype(dtype, [&](auto t) { launch_wave_per_unit<PoolKernels, typename decltype(t)::type>(p, batch * heads, head_dim, false, (hipStream_t)stream); });
    return check_launch(__func__);
}

int xclip_attention_pool_bwd(const void* q, const void* kv, const uint8_t* mask, const void* out, const void* dout, const float* lse,
                             void* dq, void* dkv, int64_t batch, int64_t n, int64_t heads, int64_t head_dim, float scale,
                             int64_t visible_keys, int dtype, void* stream) {
    AttnPoolParams p;
    const bool nonnull = q && kv && out && dout && lse && dq && dkv;
    const bool aligned = aligned16(q) && aligned16(kv) && aligned16(out) && aligned16(dout) && aligned16(dq) && aligned16(dkv);
    const int rc = attn_pool_setup(__func__, q, kv, mask, batch, n, heads, head_dim, scale, visible_keys, dtype,
                                   !nonnull ? "null pointer" : !aligned ? "pointers must be 16-byte aligned" : nullptr, p);
    if (rc != 0 || batch == 0) return rc;
    p.out = const_cast<void*>(out); p.lse = const_cast<float*>(lse); p.dout = dout; p.dq = dq; p.dkv = dkv;
    by_dtype(dtype, [&](auto t) { launch_wave_per_unit<PoolKernels, typename decltype(t)::type>(p, batch * heads, head_dim, true, (hipStream_t)stream); });
    return check_launch(__func__);
}

}  // extern "C"

// ---- samples of different lengths laid end to end (kernels/attention_varlen.h) ----
// the common checks and fields of both entry points; -> 0, or 1 with the error recorded under `fn`
static int attn_varlen_setup(const char* fn, const void* qkv, const int32_t* cu, int64_t rows, int64_t batch, int64_t heads, int64_t head_dim,
                             int64_t max_len, float scale, int dtype, bool ptrs_ok, xc::AttnVarlenParams& p) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(xcapi::dtype_ok(dtype), "bad dtype");
    // (rows may exceed batch * max_len: the rows behind cu[batch] are filler, owned by no sample -- zeros are written there)
    XC_REQ(batch >= 0 && heads > 0 && rows >= batch && max_len >= 1, "bad shape: every sample has 1 .. max_len rows");
    XC_REQ(rows * heads < ((int64_t)1 << 31) && rows * 3 * heads * head_dim < ((int64_t)1 << 40), "too many rows");
    XC_REQ(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128 (narrower / in-between widths are zero-padded by the caller)");
    XC_REQ(ptrs_ok && cu != nullptr, "pointers must be non-null and 16-byte aligned");
    XC_REQ(scale > 0.f, "scale must be positive");
    memset(&p, 0, sizeof(p));
    p.qkv = qkv; p.cu = cu; p.rows = (int)rows; p.batch = (int)batch; p.heads = (int)heads; p.max_len = (int)max_len; p.scale = scale;
    return 0;
#undef XC_REQ
}
static inline bool attn_varlen_resident(int dtype, int64_t head_dim, int64_t max_len) {
    return dtype == XCLIP_BF16 && head_dim == 64 && max_len <= xc::A3_MAX_N;
}

// plain form: the family by the causal switch
template <bool CAUSAL, typename T>
static void launch_varlen_plain(const xc::AttnVarlenParams& p, int64_t units, int64_t head_dim, bool backward, hipStream_t st) {
    if (CAUSAL) launch_wave_per_unit<VarlenPlainCausalKernels, T>(p, units, head_dim, backward, st);
    else launch_wave_per_unit<VarlenPlainKernels, T>(p, units, head_dim, backward, st);
}
// both entry-point pairs: CAUSAL picks the kernels, everything else (checks, routing, launch sizes) is shared
template <bool CAUSAL>
static int attn_varlen_fwd(const char* fn, const void* qkv, const int32_t* cu, void* out, float* lse, int64_t rows, int64_t batch, int64_t heads,
                           int64_t head_dim, int64_t max_len, float scale, int dtype, void* stream) {
    AttnVarlenParams p;
    const int rc = attn_varlen_setup(fn, qkv, cu, rows, batch, heads, head_dim, max_len, scale, dtype,
                                     qkv && out && lse && aligned16(qkv) && aligned16(out), p);
    if (rc != 0 || batch == 0) return rc;
    p.out = out; p.lse = lse;
    hipStream_t st = (hipStream_t)stream;
    if (attn_varlen_resident(dtype, head_dim, max_len)) {
        const int lds = attn_varlen_fwd_lds_bytes((int)max_len);
        if (lds > 160 * 1024) return xcapi::fail(fn, "internal: varlen forward LDS");
        const dim3 grid((unsigned)(batch * heads)), block(attn_varlen_fwd_waves((int)max_len) * 64);
        if (CAUSAL) {
            XC_ALLOW_LDS(attn_varlen_causal_fwd_kernel, 160 * 1024);
            hipLaunchKernelGGL(attn_varlen_causal_fwd_kernel, grid, block, lds, st, p);
        } else {
            XC_ALLOW_LDS(attn_varlen_fwd_kernel, 160 * 1024);
            hipLaunchKernelGGL(attn_varlen_fwd_kernel, grid, block, lds, st, p);
        }
    } else {
        by_dtype(dtype, [&](auto t) { launch_varlen_plain<CAUSAL, typename decltype(t)::type>(p, rows * heads, head_dim, false, st); });
    }
    return check_launch(fn);
}

template <bool CAUSAL>
static int attn_varlen_bwd(const char* fn, const void* qkv, const int32_t* cu, const void* out, const void* dout, const float* lse, void* dqkv,
                           int64_t rows, int64_t batch, int64_t heads, int64_t head_dim, int64_t max_len, float scale, int dtype,
                           void* stream) {
    AttnVarlenParams p;
    const int rc = attn_varlen_setup(fn, qkv, cu, rows, batch, heads, head_dim, max_len, scale, dtype,
                                     qkv && out && dout && lse && dqkv && aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv), p);
    if (rc != 0 || batch == 0) return rc;
    p.out = const_cast<void*>(out); p.lse = const_cast<float*>(lse); p.dout = dout; p.dqkv = dqkv;
    hipStream_t st = (hipStream_t)stream;
    if (attn_varlen_resident(dtype, head_dim, max_len)) {
        const int lds = attn_varlen_bwd_lds_bytes((int)max_len);
        if (lds > 160 * 1024) return xcapi::fail(fn, "internal: varlen backward LDS");
        const dim3 grid((unsigned)(batch * heads)), block(attn_varlen_bwd_waves((int)max_len) * 64);
        if (CAUSAL) {
            XC_ALLOW_LDS(attn_varlen_causal_bwd_kernel, 160 * 1024);
            hipLaunchKernelGGL(attn_varlen_causal_bwd_kernel, grid, block, lds, st, p);
        } else {
            XC_ALLOW_LDS(attn_varlen_bwd_kernel, 160 * 1024);
            hipLaunchKernelGGL(attn_varlen_bwd_kernel, grid, block, lds, st, p);
        }
    } else {
        by_dtype(dtype, [&](auto t) { launch_varlen_plain<CAUSAL, typename decltype(t)::type>(p, rows * heads, head_dim, true, st); });
    }
    return check_launch(fn);
}

extern "C" {

int xclip_attention_varlen_fwd(const void* qkv, const int32_t* cu, void* out, float* lse, int64_t rows, int64_t batch, int64_t heads,
                               int64_t head_dim, int64_t max_len, float scale, int dtype, void* stream) {
    return attn_varlen_fwd<false>(__func__, qkv, cu, out, lse, rows, batch, heads, head_dim, max_len, scale, dtype, stream);
}
int xclip_attention_varlen_bwd(const void* qkv, const int32_t* cu, const void* out, const void* dout, const float* lse, void* dqkv,
                               int64_t rows, int64_t batch, int64_t heads, int64_t head_dim, int64_t max_len, float scale, int dtype,
                               void* stream) {
    return attn_varlen_bwd<false>(__func__, qkv, cu, out, dout, lse, dqkv, rows, batch, heads, head_dim, max_len, scale, dtype, stream);
}
int xclip_attention_varlen_causal_fwd(const void* qkv, const int32_t* cu, void* out, float* lse, int64_t rows, int64_t batch, int64_t heads,
                                      int64_t head_dim, int64_t max_len, float scale, int dtype, void* stream) {
    return attn_varlen_fwd<true>(__func__, qkv, cu, out, lse, rows, batch, heads, head_dim, max_len, scale, dtype, stream);
}
int xclip_attention_varlen_causal_bwd(const void* qkv, const int32_t* cu, const void* out, const void* dout, const float* lse, void* dqkv,
                                      int64_t rows, int64_t batch, int64_t heads, int64_t head_dim, int64_t max_len, float scale, int dtype,
                                      void* stream) {
    return attn_varlen_bwd<true>(__func__, qkv, cu, out, dout, lse, dqkv, rows, batch, heads, head_dim, max_len, scale, dtype, stream);
}

}  // extern "C"

// ---- one query row per (sample, head) over samples of different lengths (kernels/attention_pool.h, the packed wrappers) ----
// the common checks and fields of both entry points; -> 0, or 1 with the error recorded under `fn`
static int attn_pool_varlen_setup(const char* fn, const void* q, const void* kv, const int32_t* cu, int64_t rows, int64_t batch, int64_t heads,
                                  int64_t head_dim, float scale, int dtype, bool ptrs_ok, xc::AttnPoolVarlenParams& p) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(xcapi::dtype_ok(dtype), "bad dtype");
    XC_REQ(batch >= 0 && heads > 0 && rows >= 0, "bad shape");
    XC_REQ(rows < ((int64_t)1 << 31) && batch * heads < ((int64_t)1 << 31), "too many rows");
    XC_REQ(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128 (narrower / in-between widths are zero-padded by the caller)");
    XC_REQ(batch == 0 || ptrs_ok, "pointers must be non-null and 16-byte aligned");
    XC_REQ(scale > 0.f, "scale must be positive");
    memset(&p, 0, sizeof(p));
    p.q = q; p.kv = kv; p.cu = cu;
    p.batch = (int)batch; p.heads = (int)heads; p.rows = (int)rows; p.scale = scale;
    return 0;
#undef XC_REQ
}

extern "C" {

int xclip_attention_pool_varlen_fwd(const void* q, const void* kv, const int32_t* cu, void* out, float* lse, int64_t rows, int64_t batch,
                                    int64_t heads, int64_t head_dim, float scale, int dtype, void* stream) {
    // (kv may be null when no sample owns a row: nothing is read through it then)
    AttnPoolVarlenParams p;
    const int rc = attn_pool_varlen_setup(__func__, q, kv, cu, rows, batch, heads, head_dim, scale, dtype,
                                          q && (kv || rows == 0) && cu && out && lse && aligned16(q) && aligned16(kv) && aligned16(out), p);
    if (rc != 0 || batch == 0) return rc;
    p.out = out; p.lse = lse;
    by_dtype(dtype, [&](auto t) { launch_wave_per_unit<PoolVarlenKernels, typename decltype(t)::type>(p, batch * heads, head_dim, false, (hipStream_t)stream); });
    return check_launch(__func__);
}

int xclip_attention_pool_varlen_bwd(const void* q, const void* kv, const int32_t* cu, const void* out, const void* dout, const float* lse,
                                    void* dq, void* dkv, int64_t rows, int64_t batch, int64_t heads, int64_t head_dim, float scale, int dtype,
                                    void* stream) {
    AttnPoolVarlenParams p;
    const int rc = attn_pool_varlen_setup(__func__, q, kv, cu, rows, batch, heads, head_dim, scale, dtype,
                                          q && ((kv && dkv) || rows == 0) && cu && out && dout && lse && dq && aligned16(q) && aligned16(kv) &&
                                              aligned16(out) && aligned16(dout) && aligned16(dq) && aligned16(dkv), p);
    if (rc != 0 || batch == 0) return rc;
    p.out = const_cast<void*>(out); p.lse = const_cast<float*>(lse); p.dout = dout; p.dq = dq; p.dkv = dkv;
    by_dtype(dtype, [&](auto t) { launch_wave_per_unit<PoolVarlenKernels, typename decltype(t)::type>(p, batch * heads, head_dim, true, (hipStream_t)stream); });
    return check_launch(__func__);
}

}  // extern "C"

// ---- packed rows <-> dense (sample, position) rows (kernels/pack_rows.h; in this unit because the pack kernel finds a row's sample with
// attention_varlen.h's av_sample_of, and the attention headers define kernels that only one unit may hold) ----
static int pack_rows_check(const char* fn, const void* packed, const int32_t* cu, const int32_t* pos, const void* dense, int64_t rows, int64_t batch,
                           int64_t n_out, int64_t pos0, int64_t dim, int dtype) {
#define XC_REQ(cond, msg) do { if (!(cond)) return xcapi::fail(fn, msg); } while (0)
    XC_REQ(xcapi::dtype_ok(dtype), "bad dtype");
    XC_REQ(rows >= 0 && batch >= 0 && n_out >= 0 && pos0 >= 0, "bad shape");
    XC_REQ(dim > 0 && dim % xcapi::vec_of(dtype) == 0, "dim must be a multiple of the 16-byte chunk");
    XC_REQ(rows < ((int64_t)1 << 31) && batch * n_out < ((int64_t)1 << 31) && pos0 + n_out < ((int64_t)1 << 31) && dim < ((int64_t)1 << 31), "too many rows");
    XC_REQ(cu != nullptr, "cu must be non-null");
    XC_REQ((rows == 0 || (packed && pos)) && (batch * n_out == 0 || dense) && xcapi::aligned16(packed) && xcapi::aligned16(dense),
           "pointers must be non-null and 16-byte aligned");
    return 0;
#undef XC_REQ
}

extern "C" {

int xclip_unpack_rows(const void* packed, const int32_t* cu, const int32_t* pos, void* dense, int64_t rows, int64_t batch, int64_t n_out,
                      int64_t pos0, int64_t dim, int dtype, void* stream) {
    const int rc = pack_rows_check(__func__, packed, cu, pos, dense, rows, batch, n_out, pos0, dim, dtype);
    if (rc != 0 || batch * n_out == 0) return rc;
    dim3 grid((unsigned)((batch * n_out + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((unpack_rows_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)packed, (const int*)cu, (const int*)pos, (T*)dense,
                           (int)rows, (int)batch, (int)n_out, (int)pos0, (int)dim);
    });
    return check_launch(__func__);
}

int xclip_pack_rows(const void* dense, const int32_t* cu, const int32_t* pos, void* packed, int64_t rows, int64_t batch, int64_t n_out,
                    int64_t pos0, int64_t dim, int dtype, void* stream) {
    const int rc = pack_rows_check(__func__, packed, cu, pos, dense, rows, batch, n_out, pos0, dim, dtype);
    if (rc != 0 || rows == 0) return rc;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL((pack_rows_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)dense, (const int*)cu, (const int*)pos, (T*)packed,
                           (int)rows, (int)batch, (int)n_out, (int)pos0, (int)dim);
    });
    return check_launch(__func__);
}

}  // extern "C"
