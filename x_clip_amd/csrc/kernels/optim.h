// optim.h -- the step after the backward: clip-by-global-norm + AdamW over every parameter of a model as three kinds of launches
// (replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step; x_clip_amd/optim.py FusedAdamW).
//
// Multi-tensor, driven by a CHUNK TABLE in device memory: one OptChunk per piece of at most OPT_CHUNK elements of a parameter.  The
// parameters stay where nn.Module put them, the gradients where autograd / GradSync.claim put them; the optimizer's own state (exp_avg,
// exp_avg_sq and -- bf16 parameters -- the fp32 master weights) lives in flat fp32 arrays, a 128-byte aligned slice per parameter.
//
//   gradnorm_partial_kernel   one work-group per chunk: partials[chunk] = sum g^2 (fp32; fixed order, no atomics: bit-reproducible)
//   optim_prepare_kernel      ONE work-group: sums the partials in a fixed order and writes the device-resident state block
//                             (OptBlock): the norm, the clip factor, the non-finite flag, the step counter.  Nothing goes to the host.
//   adamw_kernel              one work-group per chunk: returns at once when the gradients were not finite (the step is skipped ON THE
//                             DEVICE); otherwise one streaming pass, fp32 arithmetic, in torch.optim.AdamW's operation order.
//   adamw_ema_kernel          the same pass with a weight EMA kept beside the moments (FusedAdamW(ema_decay=...)): + 8 bytes per parameter.
//   grad_accum_kernel         gradients of several backward passes summed into a flat fp32 array and rounded once into `.grad`
//                             (FusedAdamW.accumulate_begin / accumulate / accumulate_end; x_clip_amd/cached.py).
//   lamb_norm_kernel          param groups with `trust_ratio` (LAMB): one work-group per chunk forms the update direction u from the
//                             moments as they WILL be (nothing is stored) and writes the chunk's pair (sum w^2, sum u^2).
//   lamb_fold_kernel          one thread per parameter: its chunks' pairs summed in chunk order, in double -> ratio[param] = |w| / |u|.
//   optim_update_kernel       the update of a group with `trust_ratio` and / or `bounds`: AdamW's or LAMB's step, then the clamp of the
//                             fp32 weight, then the EMA if on, one streaming pass; stores the moments.
//
// Algorithmic HBM traffic per parameter: bf16 2 (g, norm pass) + 2 (g) + 12 (m, v, master in) + 12 (out) + 2 (p out) = 30 bytes;
// fp32 4 + 4 + 12 (m, v, p in) + 12 (out) = 32 bytes.  Everything is read once and written once: non-temporal hint, as in rows.h.
// With `trust_ratio`: + lamb_norm_kernel's 2 (g) + 12 (m, v, master in) = 44 bytes bf16, + 4 + 12 = 48 bytes fp32 (its 8 bytes per
// CHUNK out and the fold are noise); `bounds` alone move no byte more than adamw_kernel / adamw_ema_kernel.
#pragma once
#include "common.h"

namespace xc {

constexpr int OPT_CHUNK = 65536;          // elements per chunk at most
constexpr int OPT_THREADS = 256;

struct OptChunk {                         // 48 bytes; built on the host (x_clip_amd/optim.py _TABLE_DTYPE is the same layout)
    uint64_t p;                           // first element of the piece in the parameter
    uint64_t g;                           // ... in its gradient
    int64_t state_off;                    // ... in the flat fp32 state arrays (elements)
    int32_t n;                            // elements, 1 .. OPT_CHUNK
    int32_t dtypes;                       // parameter dtype | gradient dtype << 8   (0 fp32, 1 bf16)
    int32_t param;                        // index of the parameter (its entry of step_base)
    int32_t first;                        // 1: the parameter's first chunk (the one that records step_base)
    int32_t reserved[2];
};

struct OptBlock {                         // the device-resident state block, 32 bytes
    float grad_norm;                      // global l2 norm of the gradients of the last step() (inf / nan when the step was skipped)
    float clip_coef;                      // min(1, max_norm / (norm + 1e-6)), 1 without clipping
    int32_t found_nonfinite;              // 1: the last step() was skipped
    int32_t step;                         // successful steps so far
    int32_t skipped;                      // skipped steps so far
    int32_t reserved[3];
};

struct AdamWArgs {                        // per param group; the host rounds each coefficient once from the double it was given
    float decay;                          // 1 - lr * weight_decay
    float b1, omb1, b2, omb2, eps;
    double lr, beta1, beta2;              // (the bias corrections and lr / bc1 are formed in double, as torch forms them on the host)
};

template <typename T> struct OptDtype;
template <> struct OptDtype<float> { static constexpr int CODE = 0; };
template <> struct OptDtype<bf16_t> { static constexpr int CODE = 1; };

XC_DEV bool opt_nonfinite(float x) { return (f2u(x) & 0x7f800000u) == 0x7f800000u; }
XC_DEV bool opt_aligned16(uint64_t a) { return (a & 15u) == 0; }

// 8 consecutive elements <-> registers (bf16: one 16-byte access, fp32: two)
template <bool NT>
XC_DEV void opt_load8(const bf16_t* p, float (&f)[8]) { load_vec<bf16_t, NT>(p, f); }
template <bool NT>
XC_DEV void opt_load8(const float* p, float (&f)[8]) {
    float lo[4], hi[4];
    load_vec<float, NT>(p, lo);
    load_vec<float, NT>(p + 4, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
}
template <bool NT>
XC_DEV void opt_store8(bf16_t* p, const float (&f)[8]) { store_vec<bf16_t, NT>(p, f); }
template <bool NT>
XC_DEV void opt_store8(float* p, const float (&f)[8]) {
    const float lo[4] = {f[0], f[1], f[2], f[3]}, hi[4] = {f[4], f[5], f[6], f[7]};
    store_vec<float, NT>(p, lo);
    store_vec<float, NT>(p + 4, hi);
}

// ---- sum of squares of one chunk's gradient ----------------------------------------------------------------------------------------
template <typename G>
__global__ __launch_bounds__(OPT_THREADS) void gradnorm_partial_kernel(const OptChunk* __restrict__ table, int chunk0,
                                                                       float* __restrict__ partials) {
    XC_LDS_DYNAMIC(lds);                                       // 4 floats
    float* red = reinterpret_cast<float*>(lds);
    const int chunk = chunk0 + (int)blockIdx.x;
    const OptChunk c = table[chunk];
    const int tid = threadIdx.x;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (((c.dtypes >> 8) & 0xff) == OptDtype<G>::CODE) {       // (a table that disagrees with the launch reads nothing)
        const G* g = reinterpret_cast<const G*>(c.g);
        const int nvec = opt_aligned16(c.g) ? c.n / 8 : 0;
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            float f[8];
            opt_load8<false>(g + (long)i * 8, f);              // (no hint: the update pass reads the gradient again, from the L2 / MALL)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += f[j] * f[j];
        }
        for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {   // scalar tail / unaligned chunk
            const float f = to_f32(g[i]);
            acc[0] += f * f;
        }
    }
    const float s = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
    if (lane_id() == 0) red[wave_id()] = s;
    sync();
    if (tid == 0) partials[chunk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- partials -> the state block ---------------------------------------------------------------------------------------------------
// `absent`: parameters that hold optimizer state and have no gradient in this step: their own step count does not advance
// (torch semantics: step_base[p] is what the global counter read when p's count was 0).
__global__ __launch_bounds__(OPT_THREADS) void optim_prepare_kernel(const float* __restrict__ partials, int n_chunks, float max_norm,
                                                                    int clip, OptBlock* __restrict__ blk, int32_t* __restrict__ step_base,
                                                                    const int32_t* __restrict__ absent, int n_absent) {
    XC_LDS_DYNAMIC(lds);                                       // OPT_THREADS doubles
    double* red = reinterpret_cast<double*>(lds);
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n_chunks; i += OPT_THREADS) s += (double)partials[i];
    red[tid] = s;
    sync();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < OPT_THREADS; ++i) tot += red[i];
        red[0] = tot;
    }
    sync();
    const float sumsq = (float)red[0];
    const bool bad = opt_nonfinite(sumsq);
    if (tid == 0) {
        const float norm = bad ? sumsq : (float)sqrt(red[0]);
        float coef = 1.f;
        if (clip && !bad) {
            coef = max_norm / (norm + 1e-6f);
            coef = coef < 1.f ? coef : 1.f;
        }
        blk->grad_norm = norm;
        blk->clip_coef = coef;
        blk->found_nonfinite = bad ? 1 : 0;
        if (bad) blk->skipped = blk->skipped + 1;
        else blk->step = blk->step + 1;
    }
    if (!bad)
        for (int i = tid; i < n_absent; i += OPT_THREADS) {
            const int p = absent[i];
            if (step_base[p] >= 0) step_base[p] = step_base[p] + 1;
        }
}

XC_DEV double opt_ipow(double b, int t) {                      // b^t, t >= 0, by squaring
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

XC_DEV void adamw_elem(float g, float& w, float& m, float& v, const AdamWArgs& a, float clip, float step_size, float bc2_sqrt) {
    g *= clip;
    w *= a.decay;
    m = a.b1 * m + a.omb1 * g;
    v = a.b2 * v + a.omb2 * (g * g);
    w -= step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
}

// ---- the update ------------------------------------------------------------------------------------------------------------------------
// P / G: storage type of the parameter / of its gradient.  MASTER (P = bf16): w is the fp32 master weight (read, updated, stored) and the
// parameter is WRITTEN as its round-to-nearest-even bf16; without MASTER (P = fp32) w is the parameter itself.
template <typename P, typename G, bool MASTER>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(const OptChunk* __restrict__ table, int chunk0, float* __restrict__ exp_avg,
                                                            float* __restrict__ exp_avg_sq, float* __restrict__ master,
                                                            const OptBlock* __restrict__ blk, int32_t* __restrict__ step_base, AdamWArgs a) {
    const OptBlock b = *blk;
    if (b.found_nonfinite) return;                             // the step is skipped: parameters, moments and counters untouched
    const OptChunk c = table[chunk0 + (int)blockIdx.x];
    if ((c.dtypes & 0xff) != OptDtype<P>::CODE || ((c.dtypes >> 8) & 0xff) != OptDtype<G>::CODE) return;
    const int tid = threadIdx.x;
    // this parameter's own step count: the global counter minus what it read when the parameter got its first gradient.  Every chunk of
    // a fresh parameter (base < 0) derives the same value the parameter's first chunk stores, so the order of the two does not matter.
    int base = step_base[c.param];
    if (base < 0) {
        base = b.step - 1;
        if (tid == 0 && c.first) step_base[c.param] = base;
    }
    const int t = b.step - base;
    const double bc1 = 1.0 - opt_ipow(a.beta1, t), bc2 = 1.0 - opt_ipow(a.beta2, t);
    const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2), clip = b.clip_coef;

    P* p = reinterpret_cast<P*>(c.p);
    const G* g = reinterpret_cast<const G*>(c.g);
    float* m = exp_avg + c.state_off;
    float* v = exp_avg_sq + c.state_off;
    float* w = MASTER ? master + c.state_off : reinterpret_cast<float*>(c.p);
    const int nvec = (opt_aligned16(c.p) && opt_aligned16(c.g) && (c.state_off & 3) == 0) ? c.n / 8 : 0;
    for (int i = tid; i < nvec; i += OPT_THREADS) {
        const long o = (long)i * 8;
        float gv[8], mv[8], vv[8], wv[8];
        opt_load8<true>(g + o, gv);
        opt_load8<true>(m + o, mv);
        opt_load8<true>(v + o, vv);
        opt_load8<true>(w + o, wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) adamw_elem(gv[j], wv[j], mv[j], vv[j], a, clip, step_size, bc2_sqrt);
        opt_store8<true>(m + o, mv);
        opt_store8<true>(v + o, vv);
        opt_store8<true>(w + o, wv);
        if (MASTER) opt_store8<true>(p + o, wv);               // (rounds to the parameter's storage type)
    }
    for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {  // scalar tail / unaligned chunk
        float wi = w[i], mi = m[i], vi = v[i];
        adamw_elem(to_f32(g[i]), wi, mi, vi, a, clip, step_size, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        w[i] = wi;
        if (MASTER) p[i] = from_f32<P>(wi);
    }
}

// ---- the update with a weight EMA ----------------------------------------------------------------------------------------------------------
// adamw_kernel's streaming pass with one more flat fp32 array, `ema` (laid out as exp_avg): after adamw_elem has produced the new w,
// e += omd * (w - e) in fp32, on the fp32 master where there is one (an EMA of the rounded bf16 parameters stalls as bf16 AdamW does).
// omd = 1 - d_u is formed once per work-group, in double, from the device block: u = blk.step, the applied steps including this one
// (>= 1; a skipped step advances nothing), d_u = warmup ? min(decay, (1 + u) / (10 + u)) : decay.  A skipped step returns before it
// reads anything; chunks of parameters without a gradient are not in the table: their ema keeps its bits, as the parameter does.
XC_DEV void ema_elem(float w, float& e, float omd) { e += omd * (w - e); }

template <typename P, typename G, bool MASTER>
__global__ __launch_bounds__(OPT_THREADS) void adamw_ema_kernel(const OptChunk* __restrict__ table, int chunk0, float* __restrict__ exp_avg,
                                                                float* __restrict__ exp_avg_sq, float* __restrict__ master,
                                                                float* __restrict__ ema, const OptBlock* __restrict__ blk,
                                                                int32_t* __restrict__ step_base, AdamWArgs a, double ema_decay, int ema_warmup) {
    const OptBlock b = *blk;
    if (b.found_nonfinite) return;                             // the step is skipped: the EMA too keeps every bit
    const OptChunk c = table[chunk0 + (int)blockIdx.x];
    if ((c.dtypes & 0xff) != OptDtype<P>::CODE || ((c.dtypes >> 8) & 0xff) != OptDtype<G>::CODE) return;
    const int tid = threadIdx.x;
    int base = step_base[c.param];                             // (the parameter's own step count: as adamw_kernel)
    if (base < 0) {
        base = b.step - 1;
        if (tid == 0 && c.first) step_base[c.param] = base;
    }
    const int t = b.step - base;
    const double bc1 = 1.0 - opt_ipow(a.beta1, t), bc2 = 1.0 - opt_ipow(a.beta2, t);
    const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2), clip = b.clip_coef;
    const double ramp = (1.0 + (double)b.step) / (10.0 + (double)b.step);
    const float omd = (float)(1.0 - (ema_warmup && ramp < ema_decay ? ramp : ema_decay));

    P* p = reinterpret_cast<P*>(c.p);
    const G* g = reinterpret_cast<const G*>(c.g);
    float* m = exp_avg + c.state_off;
    float* v = exp_avg_sq + c.state_off;
    float* e = ema + c.state_off;
    float* w = MASTER ? master + c.state_off : reinterpret_cast<float*>(c.p);
    const int nvec = (opt_aligned16(c.p) && opt_aligned16(c.g) && (c.state_off & 3) == 0) ? c.n / 8 : 0;
    for (int i = tid; i < nvec; i += OPT_THREADS) {
        const long o = (long)i * 8;
        float gv[8], mv[8], vv[8], wv[8], ev[8];
        opt_load8<true>(g + o, gv);
        opt_load8<true>(m + o, mv);
        opt_load8<true>(v + o, vv);
        opt_load8<true>(w + o, wv);
        opt_load8<true>(e + o, ev);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            adamw_elem(gv[j], wv[j], mv[j], vv[j], a, clip, step_size, bc2_sqrt);
            ema_elem(wv[j], ev[j], omd);
        }
        opt_store8<true>(m + o, mv);
        opt_store8<true>(v + o, vv);
        opt_store8<true>(w + o, wv);
        opt_store8<true>(e + o, ev);
        if (MASTER) opt_store8<true>(p + o, wv);               // (rounds to the parameter's storage type)
    }
    for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {  // scalar tail / unaligned chunk
        float wi = w[i], mi = m[i], vi = v[i], ei = e[i];
        adamw_elem(to_f32(g[i]), wi, mi, vi, a, clip, step_size, bc2_sqrt);
        ema_elem(wi, ei, omd);
        m[i] = mi;
        v[i] = vi;
        w[i] = wi;
        e[i] = ei;
        if (MASTER) p[i] = from_f32<P>(wi);
    }
}

// ---- gradients of several backward passes, summed in fp32 ----------------------------------------------------------------------------------
// FusedAdamW.accumulate*(): `acc` is one more flat fp32 array laid out as exp_avg.  One work-group per chunk of the same table, G the
// gradient's storage type.  MATERIALISE = false: acc[state_off + i] += float(g[i]) (the gradient of one backward pass; a bf16 `.grad`
// summed by autograd's own += would round to 8 bits after every pass).  MATERIALISE = true: g[i] = acc[state_off + i] rounded to
// nearest even ONCE (fp32: a copy) -- what the norm pass and adamw_kernel then read.  Every element is owned by one thread: no atomics,
// the same bits on every run; inf / nan pass through the sum and the rounding, so the step is still skipped on the device.
// Traffic per bf16 gradient element: 2 (g) + 4 + 4 (acc in, out) = 10 bytes to add, 4 + 2 to materialise.
template <typename G, bool MATERIALISE>
__global__ __launch_bounds__(OPT_THREADS) void grad_accum_kernel(const OptChunk* __restrict__ table, int chunk0, float* __restrict__ acc) {
    const OptChunk c = table[chunk0 + (int)blockIdx.x];
    if (((c.dtypes >> 8) & 0xff) != OptDtype<G>::CODE) return;  // (a table that disagrees with the launch touches nothing)
    const int tid = threadIdx.x;
    G* g = reinterpret_cast<G*>(c.g);
    float* a = acc + c.state_off;
    const int nvec = (opt_aligned16(c.g) && (c.state_off & 3) == 0) ? c.n / 8 : 0;
    for (int i = tid; i < nvec; i += OPT_THREADS) {
        const long o = (long)i * 8;
        float av[8];
        opt_load8<true>(a + o, av);
        if (MATERIALISE) {
            opt_store8<false>(g + o, av);                      // (no hint: the norm pass reads the gradient next)
        } else {
            float gv[8];
            opt_load8<true>(g + o, gv);
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] += gv[j];
            opt_store8<true>(a + o, av);
        }
    }
    for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {  // scalar tail / unaligned chunk
        if (MATERIALISE) g[i] = from_f32<G>(a[i]);
        else a[i] += to_f32(g[i]);
    }
}

// ---- layer-wise trust ratio (LAMB) and bounds --------------------------------------------------------------------------------------------
// FusedAdamW param groups with `trust_ratio` and / or `bounds`.  LAMB as timm / apex state it, per parameter tensor:
//   g = clip g;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = (m / bc1) / (sqrt(v / bc2) + eps) + wd w   (decay INSIDE u)
//   r = |w| / |u| over the whole tensor (1 when either norm is 0);  w -= lr r u
// r needs every element of the tensor before any of them moves, so the step is three launches: lamb_norm_kernel forms u per chunk
// WITHOUT storing anything but the chunk's (sum w^2, sum u^2); lamb_fold_kernel adds a parameter's pairs in chunk order, in double
// (its chunks are adjacent in the table, `first` marks where they start), into ratio[param]; optim_update_kernel<.., TRUST = true>
// forms u again from the same inputs with the same function (lamb_elem) and stores m, v, w.  Both passes derive the parameter's own step
// count t the same way; only the update pass records step_base, and it runs after the norm pass, so a parameter with its first gradient
// gets one t in both.  `bounds`: lo <= w <= hi on the fp32 weight after the step (either kind), BEFORE the EMA reads it and before the
// bf16 parameter is rounded from it; the host hands lo rounded up and hi rounded down to the parameter's storage type, so the rounded
// parameter stays inside too; -inf / +inf: no bound.  Every kernel returns at once on a skipped step: ratio[] keeps its bits as well.
struct UpdateArgs {                       // per param group, for the kernels below
    AdamWArgs a;
    float wd;                             // weight_decay (LAMB adds wd w to the update; AdamW uses a.decay)
    float lo, hi;                         // bounds of the fp32 weight
};

// u of one element; m and v become the new moments (the norm pass drops them, the update pass stores them)
XC_DEV float lamb_elem(float g, float w, float& m, float& v, const UpdateArgs& q, float clip, float rbc1, float rbc2_sqrt) {
    g *= clip;
    m = q.a.b1 * m + q.a.omb1 * g;
    v = q.a.b2 * v + q.a.omb2 * (g * g);
    return (m * rbc1) / (sqrtf(v) * rbc2_sqrt + q.a.eps) + q.wd * w;
}

XC_DEV float opt_clamp(float w, float lo, float hi) {          // (comparisons: a nan stays a nan, +-inf bounds change no bit)
    w = w < lo ? lo : w;
    return w > hi ? hi : w;
}

template <typename P, typename G, bool MASTER>
__global__ __launch_bounds__(OPT_THREADS) void lamb_norm_kernel(const OptChunk* __restrict__ table, int chunk0,
                                                                const float* __restrict__ exp_avg, const float* __restrict__ exp_avg_sq,
                                                                const float* __restrict__ master, const OptBlock* __restrict__ blk,
                                                                const int32_t* __restrict__ step_base, UpdateArgs q,
                                                                float* __restrict__ pairs) {
    XC_LDS_DYNAMIC(lds);                                       // 8 floats
    float* red = reinterpret_cast<float*>(lds);
    const OptBlock b = *blk;
    if (b.found_nonfinite) return;                             // the step is skipped (uniform: nobody reaches the barrier)
    const int chunk = chunk0 + (int)blockIdx.x;
    const OptChunk c = table[chunk];
    const int tid = threadIdx.x;
    float aw[8], au[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) aw[j] = au[j] = 0.f;
    if ((c.dtypes & 0xff) == OptDtype<P>::CODE && ((c.dtypes >> 8) & 0xff) == OptDtype<G>::CODE) {   // (else: reads nothing, r = 1)
        int base = step_base[c.param];                         // (read only: optim_update_kernel records it)
        if (base < 0) base = b.step - 1;
        const int t = b.step - base;
        const double bc1 = 1.0 - opt_ipow(q.a.beta1, t), bc2 = 1.0 - opt_ipow(q.a.beta2, t);
        const float rbc1 = (float)(1.0 / bc1), rbc2_sqrt = (float)(1.0 / sqrt(bc2)), clip = b.clip_coef;
        const G* g = reinterpret_cast<const G*>(c.g);
        const float* m = exp_avg + c.state_off;
        const float* v = exp_avg_sq + c.state_off;
        const float* w = MASTER ? master + c.state_off : reinterpret_cast<const float*>(c.p);
        const int nvec = (opt_aligned16(c.p) && opt_aligned16(c.g) && (c.state_off & 3) == 0) ? c.n / 8 : 0;
        for (int i = tid; i < nvec; i += OPT_THREADS) {
            const long o = (long)i * 8;
            float gv[8], mv[8], vv[8], wv[8];
            opt_load8<false>(g + o, gv);                       // (no hints: the update pass reads all four again)
            opt_load8<false>(m + o, mv);
            opt_load8<false>(v + o, vv);
            opt_load8<false>(w + o, wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float u = lamb_elem(gv[j], wv[j], mv[j], vv[j], q, clip, rbc1, rbc2_sqrt);
                aw[j] += wv[j] * wv[j];
                au[j] += u * u;
            }
        }
        for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {   // scalar tail / unaligned chunk
            float mi = m[i], vi = v[i];
            const float wi = w[i], u = lamb_elem(to_f32(g[i]), wi, mi, vi, q, clip, rbc1, rbc2_sqrt);
            aw[0] += wi * wi;
            au[0] += u * u;
        }
    }
    const float sw = wave_sum(((aw[0] + aw[1]) + (aw[2] + aw[3])) + ((aw[4] + aw[5]) + (aw[6] + aw[7])));
    const float su = wave_sum(((au[0] + au[1]) + (au[2] + au[3])) + ((au[4] + au[5]) + (au[6] + au[7])));
    if (lane_id() == 0) {
        red[wave_id()] = sw;
        red[4 + wave_id()] = su;
    }
    sync();
    if (tid == 0) {
        pairs[2 * (long)chunk] = (red[0] + red[1]) + (red[2] + red[3]);
        pairs[2 * (long)chunk + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

// chunks [chunk0, chunk0 + count): the thread whose chunk is a parameter's first walks that parameter's chunks (adjacent, all inside the
// range: a parameter lies in one segment) and adds their pairs in chunk order, in double, as optim_prepare_kernel adds the global norm.
__global__ __launch_bounds__(OPT_THREADS) void lamb_fold_kernel(const OptChunk* __restrict__ table, int chunk0, int count,
                                                                const float* __restrict__ pairs, const OptBlock* __restrict__ blk,
                                                                float* __restrict__ ratio) {
    if (blk->found_nonfinite) return;                          // the step is skipped: the stored ratios keep their bits
    const int i = (int)blockIdx.x * OPT_THREADS + (int)threadIdx.x;
    if (i >= count) return;
    const int end = chunk0 + count, param = table[chunk0 + i].param;
    if (!table[chunk0 + i].first) return;
    double sw = 0.0, su = 0.0;
    for (int k = chunk0 + i; k < end && table[k].param == param; ++k) {
        sw += (double)pairs[2 * (long)k];
        su += (double)pairs[2 * (long)k + 1];
    }
    ratio[param] = (sw > 0.0 && su > 0.0) ? (float)(sqrt(sw) / sqrt(su)) : 1.f;
}

// TRUST: LAMB's step with ratio[param] (else adamw_elem: adamw_kernel's bits in front of the clamp).  EMA: as adamw_ema_kernel.
template <typename P, typename G, bool MASTER, bool TRUST, bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const OptChunk* __restrict__ table, int chunk0, float* __restrict__ exp_avg,
                                                                   float* __restrict__ exp_avg_sq, float* __restrict__ master,
                                                                   float* __restrict__ ema, const float* __restrict__ ratio,
                                                                   const OptBlock* __restrict__ blk, int32_t* __restrict__ step_base,
                                                                   UpdateArgs q, double ema_decay, int ema_warmup) {
    const OptBlock b = *blk;
    if (b.found_nonfinite) return;                             // the step is skipped
    const OptChunk c = table[chunk0 + (int)blockIdx.x];
    if ((c.dtypes & 0xff) != OptDtype<P>::CODE || ((c.dtypes >> 8) & 0xff) != OptDtype<G>::CODE) return;
    const int tid = threadIdx.x;
    int base = step_base[c.param];                             // (the parameter's own step count: as adamw_kernel)
    if (base < 0) {
        base = b.step - 1;
        if (tid == 0 && c.first) step_base[c.param] = base;
    }
    const int t = b.step - base;
    const double bc1 = 1.0 - opt_ipow(q.a.beta1, t), bc2 = 1.0 - opt_ipow(q.a.beta2, t);
    const float step_size = (float)(q.a.lr / bc1), bc2_sqrt = (float)sqrt(bc2), clip = b.clip_coef;              // AdamW's
    const float rbc1 = (float)(1.0 / bc1), rbc2_sqrt = (float)(1.0 / sqrt(bc2));                                 // LAMB's, as lamb_norm_kernel
    const float lr_r = TRUST ? (float)(q.a.lr * (double)ratio[c.param]) : 0.f;
    const double ramp = (1.0 + (double)b.step) / (10.0 + (double)b.step);
    const float omd = EMA ? (float)(1.0 - (ema_warmup && ramp < ema_decay ? ramp : ema_decay)) : 0.f;

    P* p = reinterpret_cast<P*>(c.p);
    const G* g = reinterpret_cast<const G*>(c.g);
    float* m = exp_avg + c.state_off;
    float* v = exp_avg_sq + c.state_off;
    float* e = EMA ? ema + c.state_off : nullptr;
    float* w = MASTER ? master + c.state_off : reinterpret_cast<float*>(c.p);
    const int nvec = (opt_aligned16(c.p) && opt_aligned16(c.g) && (c.state_off & 3) == 0) ? c.n / 8 : 0;
    for (int i = tid; i < nvec; i += OPT_THREADS) {
        const long o = (long)i * 8;
        float gv[8], mv[8], vv[8], wv[8], ev[8];
        opt_load8<true>(g + o, gv);
        opt_load8<true>(m + o, mv);
        opt_load8<true>(v + o, vv);
        opt_load8<true>(w + o, wv);
        if (EMA) opt_load8<true>(e + o, ev);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (TRUST) wv[j] -= lr_r * lamb_elem(gv[j], wv[j], mv[j], vv[j], q, clip, rbc1, rbc2_sqrt);
            else adamw_elem(gv[j], wv[j], mv[j], vv[j], q.a, clip, step_size, bc2_sqrt);
            wv[j] = opt_clamp(wv[j], q.lo, q.hi);
            if (EMA) ema_elem(wv[j], ev[j], omd);
        }
        opt_store8<true>(m + o, mv);
        opt_store8<true>(v + o, vv);
        opt_store8<true>(w + o, wv);
        if (EMA) opt_store8<true>(e + o, ev);
        if (MASTER) opt_store8<true>(p + o, wv);               // (rounds to the parameter's storage type)
    }
    for (int i = nvec * 8 + tid; i < c.n; i += OPT_THREADS) {  // scalar tail / unaligned chunk
        float wi = w[i], mi = m[i], vi = v[i];
        if (TRUST) wi -= lr_r * lamb_elem(to_f32(g[i]), wi, mi, vi, q, clip, rbc1, rbc2_sqrt);
        else adamw_elem(to_f32(g[i]), wi, mi, vi, q.a, clip, step_size, bc2_sqrt);
        wi = opt_clamp(wi, q.lo, q.hi);
        if (EMA) {
            float ei = e[i];
            ema_elem(wi, ei, omd);
            e[i] = ei;
        }
        m[i] = mi;
        v[i] = vi;
        w[i] = wi;
        if (MASTER) p[i] = from_f32<P>(wi);
    }
}

}  // namespace xc
