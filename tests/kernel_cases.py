"""Per-kernel parity cases, shared by tests/test_kernels_emu.py (CPU, wave64 emulator build of the kernel sources) and
tests/test_kernels_gpu.py (MI355X, libxclip_hip.so).  Every case calls through the C ABI (x_clip_amd.ops) and
compares against an fp32/fp64 torch-CPU expression taken from the oracle (oracle/clip_oracle.py).

Tolerances (`close` below): fp32 storage -> 2e-5 relative to the output scale (fp32 accumulation order differs from ATen's);
bf16 storage -> the reference is evaluated in fp64 on the bf16-rounded inputs and ROUNDED to bf16; kernels with fp32
arithmetic and one rounding on store are held to 1 bf16 ulp ELEMENT-WISE, kernels whose arithmetic itself passes through
bf16 (attention, chained GEMMs, backwards reading a rounded forward output) to 2 ulps of the output scale -- the per-kernel
reading of the north-star's "1e-3 bf16 / 1e-5 fp32" given in SURVEY.md section 0.  (`tol` is the coarse 1.5-ulp-of-scale
figure a few shape-only checks still use.)
"""
import math
import os

import numpy as np
import torch

from oracle import clip_oracle as O
from x_clip_amd import ops

DTYPES = [torch.float32, torch.bfloat16]


def tol(dtype):
    return 2e-5 if dtype == torch.float32 else 6e-3


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ref64(t):
    return t.detach().cpu().to(torch.float64)


# name -> [largest measured error, the bound it was held to, unit]: written out by tests/conftest.py at session end (the GPU run's
# table is committed under profiles/ and quoted in DESIGN_APPENDIX.md section 7 -- measured errors, not bounds)
REPORT = {}


def _record(name, dtype, measured, bound, unit):
    key = f"{name} [{'bf16' if dtype == torch.bfloat16 else 'fp32'}]"
    cur = REPORT.get(key)
    if cur is None or measured > cur[0]:
        REPORT[key] = [measured, bound, unit]


def bf16_ulp(x):
    """spacing of bfloat16 (8 significand bits) at |x|, elementwise, fp64 in / out"""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def close(got, want, dtype, name="", scale=None, mult=1.0, ulps=1.0, unit="elem"):
    """fp32 storage: max |got - want| <= 2e-5 * mult of the output scale (`mult` applies to fp32 only).
    bf16 storage (bound `ulps`), measured against the fp64 reference ROUNDED to bf16, in bf16 ulps, two ways:
      unit="elem"  (kernels with fp32 arithmetic and ONE rounding on store: every GEMM, LayerNorm forward, embeddings, means,
                   log-sum-exps ...): ELEMENT-WISE, |got_i - bf16(want_i)| <= `ulps` ulps of max(|want_i|, scale / 256) -- one ulp is
                   all such a kernel can differ by from the rounded exact value; elements below 1/256 of the output scale are held
                   to the ulp at scale / 256 = 1.5e-5 of the scale, the fp32 bar (an fp32 sum cancelling to ~0 is not exact to ITS
                   OWN bf16 ulp);
      unit="scale" (kernels whose arithmetic itself passes through bf16: attention rounds P and dS to feed the matrix cores, a
                   backward kernel reads the forward's ROUNDED output, two chained GEMMs round the intermediate): the error of
                   an output element is set by the magnitude of the terms summed into it, not by its own size, so the check is
                   max |got - bf16(want)| <= `ulps` ulps OF THE OUTPUT SCALE; each such case states its bound next to the measured
                   value (tests print both into gpurun_out/parity_report_*.txt)."""
    want = want.detach().to(torch.float64)                      # the arithmetic runs where the REFERENCE lives: a full-size reference built on
    got = got.detach().to(want.device, torch.float64)          # the GPU (attention_ref_blocked) is compared there, every element, nothing sampled
    assert got.shape == want.shape, (name, got.shape, want.shape)
    s = max(float(want.abs().max()) if scale is None else scale, 1e-30)       # the scale of the WHOLE tensor
    assert bool(torch.isfinite(got).all()), name
    if dtype == torch.float32:
        err = float((got - want).abs().max())
        _record(name, dtype, err / s, tol(dtype) * mult, "of the output scale")
        assert err <= tol(dtype) * mult * max(s, 1e-6), f"{name}: max err {err:.3e} vs scale {s:.3e} ({dtype})"
        return
    want_r = want.to(torch.bfloat16).to(torch.float64)
    diff = (got - want_r).abs()
    if unit == "elem":
        err_ulps = float((diff / bf16_ulp(torch.maximum(want.abs(), torch.full_like(want, s / 256)))).max())
        label = "bf16 ulp, element-wise"
    else:
        assert unit == "scale"
        err_ulps = float(diff.max()) / float(bf16_ulp(torch.tensor(s, dtype=torch.float64)))
        label = "bf16 ulp of the output scale"
    _record(name, dtype, err_ulps, ulps, label)
    if os.environ.get("XCLIP_TEST_MEASURE_ONLY") == "1":
        other = float(diff.max()) / float(bf16_ulp(torch.tensor(s, dtype=torch.float64)))
        _record(name + " {scale-ulp}", dtype, other, 0, "info")
        return
    assert err_ulps <= ulps, f"{name}: {err_ulps:.3f} {label} (bound {ulps}) at output scale {s:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
def case_layernorm(dev, dtype, rows, dim, geglu, with_res):
    width = 2 * dim if geglu else dim
    x = rnd((rows, width), dtype, 1)
    g = (1 + 0.1 * rnd((dim,), torch.float32, 2)).to(dtype)
    res = rnd((rows, dim), dtype, 3) if with_res else None
    dy = rnd((rows, dim), dtype, 4)
    y, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), None if res is None else res.to(dev), geglu)
    dx, dg = ops.layernorm_bwd(dy.to(dev), x.to(dev), g.to(dev), mean, rstd, geglu)

    x64 = ref64(x).requires_grad_(True)
    g64 = ref64(g).requires_grad_(True)
    eps = ops.ln_eps(dtype)
    v = O.geglu(x64) if geglu else x64
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    yr = (v - mu) * torch.rsqrt(var + eps) * g64
    if res is not None:
        yr = yr + ref64(res)
    yr.backward(ref64(dy))
    close(y, yr, dtype, "ln y")
    close(dx, x64.grad, dtype, "ln dx", mult=2.0)
    close(dg, g64.grad, dtype, "ln dg", mult=2.0)


def case_ffn_dgrad_geglu(dev, M, F, D, seed=41, resid_scale=1.0):
    """csrc/kernels/gemm9.h: net.4's input gradient + net.2's (GEGLU-LayerNorm) backward in one kernel, against fp64 autograd through
    h = LayerNorm(u gelu(t)) g ; y = h W2^T and against the two-kernel path (xclip_gemm + xclip_layernorm_bwd).  The fused kernel takes its second row
    statistic from x2 - x1 (the block's output minus its input, both rounded to bf16): x2 is built by the product's own forward"""
    dt = torch.bfloat16
    u = rnd((M, 2 * F), dt, seed)
    g = (1 + 0.1 * rnd((F,), torch.float32, seed + 1)).to(dt)
    w2 = (rnd((D, F), torch.float32, seed + 2) / math.sqrt(F)).to(dt)
    # resid_scale: the residual stream |x1| that many times the block's own output |y| ~ 1 (deep pre-norm layers): x2 = bf16(x1 + y)
    # then carries ulp(x2) / 2 of absolute error per element, i.e. x2 - x1 knows y only to resid_scale x 2^-9 of ITS scale -- the cancellation
    # the fused kernel's s2 = dOut . (x2 - x1) inherits and the two-kernel path (which reads the bf16-rounded d a instead) does not have
    x1 = (resid_scale * rnd((M, D), torch.float32, seed + 3)).to(dt)
    dout = rnd((M, D), dt, seed + 4)
    ud, gd, wd, x1d, dd = u.to(dev), g.to(dev), w2.to(dev), x1.to(dev), dout.to(dev)
    a, mean, rstd = ops.layernorm_fwd(ud, gd, None, True)
    x2 = ops.gemm(a, wd, M, D, F, residual=x1d)
    assert ops.ffn_dgrad_geglu_ok(M, F, D, dt)
    dx, dg = ops.ffn_dgrad_geglu(dd, wd, ud, gd, mean, rstd, x2, x1d)
    # the two-kernel path
    da = ops.gemm(dd, wd, M, F, D, b_kmajor=True)
    dx2k, dg2k = ops.layernorm_bwd(da, ud, gd, mean, rstd, True)
    # fp64 reference (plain torch autograd; on the device the kernels run on: at the text tower's size the CPU took 45 of the test's 49 s)
    rdev = dev if M * F >= (1 << 24) else torch.device("cpu")
    u64 = ref64(u).to(rdev).requires_grad_(True)
    g64 = ref64(g).to(rdev).requires_grad_(True)
    v = O.geglu(u64)
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    h = (v - mu) * torch.rsqrt(var + ops.ln_eps(dt)) * g64
    (h @ ref64(w2).to(rdev).t()).backward(ref64(dout).to(rdev))
    del v, mu, var, h
    ref_dx, ref_dg = u64.grad, g64.grad.cpu()
    scale = float(ref_dx.abs().max())
    e_f = float((dx.double().to(rdev) - ref_dx).abs().max()) / scale
    e_2 = float((dx2k.double().to(rdev) - ref_dx).abs().max()) / scale
    del ref_dx, u64
    # no worse than twice the two-kernel path's own error (it rounds d a to bf16; the fused kernel keeps it in fp32 but takes s2 from bf16 x2 - x1)
    # -- plus, for a residual stream R = |x1| / |y| > 1, the cancellation term of s2 (ops.FUSE_FFN_DGRAD's comment): x2 - x1 carries
    # R 2^-9 |y| of rounding per element, s2 / F moves by that x sqrt(D) / F x |dOut|, and the largest element of dx sees it amplified by
    # max |ahat| max |u| (~ 30 for Gaussian inputs; calibrated on the emulator: 4.2e-2 at R = 16, D = 128, F = 256) -- held to twice that
    bound = max(2.0 * e_2, 2.0 ** -7) + (0.0 if resid_scale == 1.0 else 60.0 * resid_scale * 2.0 ** -9 * math.sqrt(D) / F)
    _record("ffn_dgrad_geglu dx fused%s (two-kernel path: %.2e)" % ("" if resid_scale == 1.0 else " |x1|/|y| = %g" % resid_scale, e_2), dt, e_f, bound, "of the output scale")
    assert e_f <= bound, (e_f, e_2, bound)
    gs = float(ref_dg.abs().max())
    g_f = float((dg.double().cpu() - ref_dg).abs().max()) / gs
    g_2 = float((dg2k.double().cpu() - ref_dg).abs().max()) / gs
    assert g_f <= max(2.0 * g_2, 2.0 ** -7) + (0.0 if resid_scale == 1.0 else 60.0 * resid_scale * 2.0 ** -9 * math.sqrt(D) / F), (g_f, g_2)


def case_ffn_rowstats_in_layernorm_bwd(dev, M, F, D, seed=47):
    """round 6: the fused feed-forward backward's row pass inside the LayerNorm backward that writes its dOut (rows.h ln_bwd_kernel FFN,
    xclip_layernorm_bwd_ffnstats + xclip_ffn_dgrad_geglu_rowc) against the separate row pass: the same dx from the LayerNorm backward, the
    same row constants (dOut enters as stored, chunk for chunk as ffn_rowstats_kernel sums it), hence the same d(u | t) and gain gradient"""
    dt = torch.bfloat16
    u = rnd((M, 2 * F), dt, seed).to(dev)
    gi = (1 + 0.1 * rnd((F,), torch.float32, seed + 1)).to(dt).to(dev)
    w2 = (rnd((D, F), torch.float32, seed + 2) / math.sqrt(F)).to(dt).to(dev)
    x1 = rnd((M, D), dt, seed + 3).to(dev)
    a, m4, r4 = ops.layernorm_fwd(u, gi, None, True)
    x2 = ops.gemm(a, w2, M, D, F, residual=x1)                       # the block's output = the input row of the LayerNorm above it
    g = (1 + 0.1 * rnd((D,), torch.float32, seed + 4)).to(dt).to(dev)
    _, mean, rstd = ops.layernorm_fwd(x2, g)
    dy, dres = rnd((M, D), dt, seed + 5).to(dev), rnd((M, D), dt, seed + 6).to(dev)
    def same(a, b, what, frac=2e-3):
        """the two instantiations of one kernel: identical on the emulator; on the GPU the compiler contracts their fused multiply-adds
        differently, so a few elements may round the other way -- at most one bf16 ulp of the scale, on at most `frac` of the elements"""
        a, b = a.float(), b.float()
        scale = float(b.abs().max())
        bad = float((a != b).float().mean())
        err = float((a - b).abs().max())
        assert err <= scale * 2.0 ** -7 and bad <= frac, (what, err, scale, bad)

    for res in (dres, None):
        dx_ref, dg_ref = ops.layernorm_bwd(dy, x2, g, mean, rstd, dres=res)
        req = ops.ffn_stats_request(w2, gi, x1, m4, r4)
        assert req is not None
        dx, dg = ops.layernorm_bwd(dy, x2, g, mean, rstd, dres=res, ffn_stats=req)
        same(dx, dx_ref, "dx")
        assert float((dg - dg_ref).abs().max()) <= 1e-4 * float(dg_ref.abs().max())
        # the same dOut through both forms of the row pass
        du_ref, dgi_ref = ops.ffn_dgrad_geglu(dx, w2, u, gi, m4, r4, x2, x1)
        du, dgi = ops.ffn_dgrad_geglu(dx, w2, u, gi, m4, r4, None, None, rowc=req[5])
        assert torch.isfinite(du.float()).all()
        same(du, du_ref, "du", frac=2e-2)
        assert float((dgi - dgi_ref).abs().max()) <= 1e-3 * float(dgi_ref.abs().max())


def case_l2norm(dev, dtype, rows, dim):
    x = rnd((rows, dim), dtype, 5)
    dy = rnd((rows, dim), dtype, 6)
    y, rn = ops.l2norm_fwd(x.to(dev))
    dx = ops.l2norm_bwd(dy.to(dev), y, rn)
    x64 = ref64(x).requires_grad_(True)
    yr = O.l2_normalize(x64)
    yr.backward(ref64(dy))
    close(y, yr, dtype, "l2 y")
    # the backward consumes the (rounded) y the forward stored
    close(dx, x64.grad, dtype, "l2 dx", mult=3.0, ulps=2.0, unit="scale")


def case_text_embed(dev, dtype, batch, n, dim, vocab, has_pos=True, has_cls=True):
    g = torch.Generator().manual_seed(7)
    tok = torch.randint(0, vocab, (batch, n), generator=g)
    E = rnd((vocab, dim), dtype, 8)
    P = rnd((n, dim), dtype, 9) if has_pos else None
    cls = rnd((dim,), dtype, 10) if has_cls else None
    out = ops.text_embed_fwd(tok.to(dev), E.to(dev), None if P is None else P.to(dev), None if cls is None else cls.to(dev))
    E64 = ref64(E).requires_grad_(True)
    P64 = ref64(P).requires_grad_(True) if has_pos else None
    c64 = ref64(cls).requires_grad_(True) if has_cls else None
    r = E64[tok]
    if has_pos:
        r = r + P64[None]
    if has_cls:
        r = torch.cat([c64.expand(batch, 1, dim), r], dim=1)
    close(out, r, dtype, "embed out")
    dout = rnd(tuple(r.shape), dtype, 11)
    r.backward(ref64(dout))
    dE, dP, dcls = ops.text_embed_bwd(dout.to(dev), tok.to(dev), vocab, has_pos, has_cls)
    close(dE, E64.grad, torch.float32, "dE", mult=4.0)
    if has_pos:
        close(dP, P64.grad, torch.float32, "dP", mult=4.0)
    if has_cls:
        close(dcls, c64.grad, torch.float32, "dcls", mult=4.0)


def case_text_embed_bad_ids(dev, dtype):
    """token ids outside [0, vocab): the reference's nn.Embedding raises IndexError (x_clip.py:320); here nothing is read or written
    out of bounds, the offending rows come out NaN, the host raises IndexError (at once on the CPU build, at the next call on the GPU
    once the flag copy has landed -- no sync in the step), and the backward kernels drop those ids"""
    import pytest
    batch, n, dim, vocab = 3, 6, 64, 11
    g = torch.Generator().manual_seed(70)
    tok = torch.randint(0, vocab, (batch, n), generator=g)
    tok[1, 2], tok[2, 5] = vocab, -1
    E = rnd((vocab, dim), dtype, 71)
    P = rnd((n, dim), dtype, 72)
    gpu = torch.device(dev).type == "cuda"
    if gpu:
        out = ops.text_embed_fwd(tok.to(dev), E.to(dev), P.to(dev), None)      # launches; the flag copy is in flight
        torch.cuda.synchronize()
        assert torch.isnan(out[1, 2].float()).all() and torch.isnan(out[2, 5].float()).all()
        assert torch.isfinite(out[0].float()).all() and torch.isfinite(out[1, :2].float()).all()
        with pytest.raises(IndexError, match="index out of range"):
            ops.text_embed_fwd(tok.clamp(0, vocab - 1).to(dev), E.to(dev), P.to(dev), None)   # the NEXT call reports it
    else:
        with pytest.raises(IndexError, match="index out of range"):
            ops.text_embed_fwd(tok.to(dev), E.to(dev), P.to(dev), None)
    ok = ops.text_embed_fwd(tok.clamp(0, vocab - 1).to(dev), E.to(dev), P.to(dev), None)       # and the state is clean again
    assert torch.isfinite(ok.float()).all()
    dout = rnd((batch, n, dim), dtype, 73)
    good = (tok >= 0) & (tok < vocab)
    want = torch.zeros(vocab, dim, dtype=torch.float64)
    want.index_add_(0, tok[good], ref64(dout)[good])
    dE, dP, _ = ops.text_embed_bwd(dout.to(dev), tok.to(dev), vocab, True, False)
    close(dE, want, torch.float32, "dE with bad ids dropped", mult=4.0)
    st = torch.sort(tok.reshape(-1))
    dE2, _, _ = ops.text_embed_bwd(dout.to(dev), tok.to(dev), vocab, True, False, sorted_tokens=(st.values.to(dev), st.indices.to(dev)))
    close(dE2, want, torch.float32, "dE sorted with bad ids dropped", mult=4.0)


def case_patchify(dev, dtype, batch, c, size, p, keep_frac):
    img = rnd((batch, c, size, size), dtype, 12)
    npatch = (size // p) ** 2
    keep = None
    if keep_frac < 1.0:
        g = torch.Generator().manual_seed(13)
        nk = max(1, int(npatch * keep_frac))
        keep = torch.randn(batch, npatch, generator=g).topk(nk, dim=-1).indices.to(torch.int32)
    out = ops.patchify(img.to(dev), p, None if keep is None else keep.to(dev))
    r = O.patchify(img.float(), p)
    if keep is not None:
        r = torch.gather(r, 1, keep.long()[..., None].expand(-1, -1, r.shape[-1]))
    r = r.reshape(-1, r.shape[-1])
    got = out.cpu().float()
    assert torch.equal(got[:, : r.shape[1]], r), "patchify is a pure gather: must be bit exact"
    assert float(got[:, r.shape[1]:].abs().sum()) == 0.0


def case_token_mean(dev, dtype, batch, n, dim):
    x = rnd((batch, n, dim), dtype, 14)
    out = ops.token_mean_fwd(x.to(dev))
    close(out, ref64(x).mean(1), dtype, "mean")
    d = rnd((batch, dim), dtype, 15)
    dx = ops.token_mean_bwd(d.to(dev), n)
    close(dx, (ref64(d) / n)[:, None].expand(batch, n, dim), dtype, "mean bwd")
    # strided forms: the tokens sit behind a CLS slot of a [b, 1+n, D] buffer
    full = rnd((batch, n + 1, dim), dtype, 16)
    close(ops.token_mean_fwd(full.to(dev)[:, 1:]), ref64(full)[:, 1:].mean(1), dtype, "mean strided")
    acc = ops.token_mean_bwd(d.to(dev), n, add=full.to(dev)[:, 1:])
    close(acc, ref64(full)[:, 1:] + (ref64(d) / n)[:, None], dtype, "mean bwd + source")


def case_gemm(dev, dtype, M, N, K, layout, epilogue=False, alpha=1.0, residual_only=False, in_place=False):
    """layout: 'nt' forward, 'nn' dgrad, 'tn' wgrad; residual_only: C = alpha A B + R (the skip connection of the FF2 forward; in_place:
    R is the output buffer itself, as the accumulating GEMMs of the loss heads call it)"""
    a_k = layout == "tn"
    b_k = layout in ("nn", "tn")
    # asymmetric operands: a transposed / mirrored output cannot pass
    a = rnd((K, M) if a_k else (M, K), dtype, 17)
    b = rnd((K, N) if b_k else (N, K), dtype, 18)
    bias = res = addrows = rowidx = None
    if residual_only:
        res = rnd((M, N), dtype, 20)
    if epilogue:
        bias = rnd((N,), dtype, 19)
        res = rnd((M, N), dtype, 20)
        addrows = rnd((5, N), dtype, 21)
        rowidx = (torch.arange(M) * 3 % 5).to(torch.int32)
    res_dev = None if res is None else res.to(dev).clone()            # (clone: on the CPU build .to() aliases, and in_place overwrites it)
    c = ops.gemm(a.to(dev), b.to(dev), M, N, K, a_k, b_k, alpha, None if bias is None else bias.to(dev),
                 res_dev, None if addrows is None else addrows.to(dev),
                 None if rowidx is None else rowidx.to(dev), out=res_dev if in_place else None)
    A = ref64(a).t() if a_k else ref64(a)
    B = ref64(b) if b_k else ref64(b).t()
    r = alpha * (A @ B)
    scale = float(r.abs().max())
    if epilogue:
        r = r + ref64(bias) + ref64(res) + ref64(addrows)[rowidx.long()]
    if residual_only:
        r = r + ref64(res)
    close(c, r, dtype, f"gemm {layout} {M}x{N}x{K}", scale=max(scale, float(r.abs().max())))


def _attention_ref(qkv64, mask, heads, scale, causal=False, hd=64, drop=None, with_lse=False):
    """with_lse: also the natural log of the sum of exponentials of the scaled scores over the keys a query sees [b, heads, n] -- what
    xclip_attention_fwd saves for the backward (include/xclip.h): masked and hidden keys are not in the sum, dropout does not enter it"""
    b, n, _ = qkv64.shape
    q, k, v = qkv64.view(b, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (q * scale) @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], -torch.finfo(s.dtype).max)
    if causal:                                                  # x_clip.py:231-234
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), -torch.finfo(s.dtype).max)
    p = torch.softmax(s, dim=-1)
    if drop is not None:                                        # (p, seed): the product's keep-mask over (b, h, i, j), rebuilt on the host
        p = p * O.dropout_keep(drop[1], b * heads * n * n, drop[0]).view(b, heads, n, n).double() / (1.0 - float(np.float32(drop[0])))
    o = (p @ v).permute(0, 2, 1, 3).reshape(b, n, heads * hd)
    return (o, torch.logsumexp(s.detach(), dim=-1)) if with_lse else o


def case_attention(dev, dtype, batch, n, heads, masked, causal=False, hd=64, drop=None, mask_override=None):
    """hd = features per head slot: 64, or 128 (wide heads, reference Attention(dim_head > 64), x_clip.py:201-212); drop = (p, seed):
    attention dropout (x_clip.py:212,241) with the product's own stateless keep-mask"""
    qkv = rnd((batch, n, 3 * heads * hd), dtype, 22)
    dout = rnd((batch, n, heads * hd), dtype, 23)
    mask = None
    if masked:
        mask = torch.ones(batch, n, dtype=torch.bool)
        for bi in range(batch):
            k = (bi * 5 + 2) % max(1, n // 2)
            if k:
                mask[bi, n - k:] = False
            if n > 3:
                mask[bi, 2] = bi % 2 == 0           # a hole in the middle as well
    if mask_override is not None:
        mask = mask_override
    scale = hd ** -0.5
    dk = {} if drop is None else dict(dropout_p=drop[0], dropout_seed=drop[1])
    out, lse = ops.attention_fwd(qkv.to(dev), None if mask is None else mask.to(dev), heads, scale, causal, hd, **dk)
    q64 = ref64(qkv).requires_grad_(True)
    r, lse_r = _attention_ref(q64, mask, heads, scale, causal, hd, drop, with_lse=True)
    r.backward(ref64(dout))
    tag = ("" if hd == 64 else f" (head slot {hd})") + ("" if drop is None else " + dropout")
    close(out, r, dtype, "attn out" + tag, ulps=2.0, unit="scale")
    close(lse, lse_r, torch.float32, "attn lse" + tag + (" <- bf16" if dtype == torch.bfloat16 else ""))     # (an fp32 output for either storage type)
    dqkv = ops.attention_bwd(qkv.to(dev), None if mask is None else mask.to(dev), out, dout.to(dev), lse, heads, scale, causal, hd, **dk)
    close(dqkv, q64.grad, dtype, "attn dqkv" + tag, mult=3.0, ulps=2.0, unit="scale")


def case_attention_pool(dev, dtype, batch, n, heads, masked, hd=64, row=0, causal=False):
    """ONE query row per (sample, head) (attention_pool.h; the last text layer under the CLS head): against the fp64 attention of the dense
    packed qkv restricted to that query row -- output, and the gradients of the pooled query and of every key / value row"""
    qkv = rnd((batch, n, 3 * heads * hd), dtype, 28)
    dout = rnd((batch, heads * hd), dtype, 29)
    mask = None
    if masked:
        mask = torch.ones(batch, n, dtype=torch.bool)
        for bi in range(batch):
            k = (bi * 5 + 2) % max(1, n // 2)
            if k:
                mask[bi, n - k:] = False
            if n > 3 and row != 2:
                mask[bi, 2] = bi % 2 == 0
        mask[:, row] = True
    scale = hd ** -0.5
    inner = heads * hd
    q = qkv[:, row, :inner].contiguous()
    kv = qkv[:, :, inner:].contiguous()
    m_dev = None if mask is None else mask.to(dev)
    vis = row + 1 if causal else None
    out, lse = ops.attention_pool_fwd(q.to(dev), kv.to(dev), m_dev, heads, scale, hd, vis)
    q64 = ref64(qkv).requires_grad_(True)
    r, lse_r = _attention_ref(q64, mask, heads, scale, causal, hd, None, with_lse=True)
    r = r[:, row]
    r.backward(ref64(dout))
    tag = f" pooled row {row}" + ("" if hd == 64 else f" (head slot {hd})")
    close(out, r, dtype, "attn out" + tag, ulps=2.0, unit="scale")
    close(lse, lse_r[:, :, row], torch.float32, "attn lse" + tag + (" <- bf16" if dtype == torch.bfloat16 else ""))
    dq, dkv = ops.attention_pool_bwd(q.to(dev), kv.to(dev), m_dev, out, dout.to(dev), lse, heads, scale, hd, vis)
    g = q64.grad
    close(dq, g[:, row, :inner], dtype, "attn dq" + tag, mult=3.0, ulps=2.0, unit="scale")
    close(dkv, g[:, :, inner:], dtype, "attn dkv" + tag, mult=3.0, ulps=2.0, unit="scale")
    off = g[:, :, :inner].clone()
    off[:, row] = 0
    assert float(off.abs().max()) == 0.0                       # (the reference's dQ is zero off the pooled row)


def case_attention_single_tail(dev, dtype, n=257, heads=2):
    """n = 32 q + 1 (the text encoder's CLS + 256 tokens): the tail row enters the head-resident kernels as the INITIAL value of their
    accumulators (attention3.h a3_tail_dot / a3_tail_outer), not as a 33rd MFMA block.  Four samples: no mask at all; a hole in the middle
    with the tail key valid; the tail key itself padded; everything but the first three keys padded (the tail query then sees three keys)"""
    mask = torch.ones(4, n, dtype=torch.bool)
    mask[1, min(40, n // 2)] = False
    mask[2, n - 1] = False
    mask[2, 7] = False
    mask[3, 3:] = False
    case_attention(dev, dtype, 4, n, heads, True, mask_override=mask)
    case_attention(dev, dtype, 1, n, heads, False)


def case_attention_spike(dev, dtype):
    """forces the online-softmax rescale: one key scores far above everything in a LATER tile (guide rule 26)"""
    batch, n, heads = 1, 150, 1
    qkv = rnd((batch, n, 3 * 64), dtype, 24, scale=0.3)
    v = qkv.view(batch, n, 3, 64)
    v[0, :, 0, :] = v[0, :, 0, :] + 0.0
    v[0, 140, 1, :] = v[0, 5, 0, :] * 40.0           # key 140 (third tile) aligned with query 5
    v[0, 70, 1, :] = v[0, 5, 0, :] * 15.0            # and a smaller spike in the second tile
    scale = 64 ** -0.5
    out, lse = ops.attention_fwd(qkv.to(dev), None, heads, scale)
    r, lse_r = _attention_ref(ref64(qkv), None, heads, scale, with_lse=True)
    close(out, r, dtype, "attn spike", ulps=2.0, unit="scale")
    close(lse, lse_r, torch.float32, "attn lse spike" + (" <- bf16" if dtype == torch.bfloat16 else ""))


# ---- attention at full occupancy: a reference that scales to 8192 heads, text-like masks, every head checked ----------------------------
def dropout_keep_range(seed, start, count, p, device):
    """oracle.clip_oracle.dropout_keep (the product's stateless keep-mask, csrc/kernels/common.h drop_hash) for the element indices
    [start, start + count), in torch integer arithmetic on `device`: a block of the keep-mask over (b, h, i, j) without building the
    whole of it on the host.  Everything stays inside int64: 32 x 32-bit products are formed from 16-bit halves"""
    M = 0xFFFFFFFF

    def mul32(a, c):                                           # (a c) mod 2^32 for 0 <= a, c < 2^32
        return (((a & 0xFFFF) * c) + ((((a >> 16) * c) & M) << 16)) & M

    seed &= (1 << 64) - 1
    idx = torch.arange(start, start + count, dtype=torch.int64, device=device)
    h = mul32(idx & M, 0x9E3779B1) ^ mul32(idx >> 32, 0xC2B2AE3D) ^ ((seed & M) ^ (((seed >> 32) * 0x85EBCA77) & M))
    h = h ^ (h >> 16)
    h = mul32(h, 0x7FEB352D)
    h = h ^ (h >> 15)
    h = mul32(h, 0x846CA68B)
    h = h ^ (h >> 16)
    thresh = 0 if p <= 0 else int(np.float32(p).astype(np.float64) * 4294967296.0)
    return h >= thresh


def attention_ref_blocked(qkv, dout, mask, heads, scale, causal=False, hd=64, drop=None, query_row=None, block=None):
    """_attention_ref + autograd, evaluated in blocks of samples on the device of `qkv` (one score tensor of b = 1024, n = 257, 8 heads
    is 4.3 GB in fp64): the same expression -- scaled scores, mask fill, causal fill, softmax, the product's keep-mask, P V -- in plain
    torch fp64, the backward by autograd.  -> (out, lse, dqkv) in fp64 on that device; lse = log sum exp of the scaled scores a query
    sees [b, heads, n].  query_row = r: only query r of every sample (the pooled kernels): out [b, heads * hd], lse [b, heads], dout
    [b, heads * hd]; dqkv still covers every row (its q third is zero off row r)."""
    dev = qkv.device
    b, n, w = qkv.shape
    assert w == 3 * heads * hd
    nq = n if query_row is None else 1
    if block is None:                                          # <= 512 MB per score-sized tensor, <= 2 GB for a block of qkv in fp64
        block = max(1, min((1 << 26) // (heads * n * nq), (1 << 28) // (n * w)))
    neg = -torch.finfo(torch.float64).max
    out = torch.zeros(b, nq, heads * hd, dtype=torch.float64, device=dev)
    lse = torch.zeros(b, heads, nq, dtype=torch.float64, device=dev)
    grad = torch.zeros(b, n, w, dtype=torch.float64, device=dev)
    hidden = None
    if causal:
        hidden = torch.ones(n, n, dtype=torch.bool, device=dev).triu(1)
        if query_row is not None:
            hidden = hidden[query_row: query_row + 1]
    for b0 in range(0, b, block):
        x = qkv[b0: b0 + block].detach().to(torch.float64).requires_grad_(True)
        bb = x.shape[0]
        q, k, v = x.view(bb, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
        if query_row is not None:
            q = q[:, :, query_row: query_row + 1]
        s = (q * scale) @ k.transpose(-1, -2)
        if mask is not None:
            s = s.masked_fill(~mask[b0: b0 + bb, None, None, :], neg)
        if causal:
            s = s.masked_fill(hidden, neg)
        lse[b0: b0 + bb] = torch.logsumexp(s.detach(), dim=-1)
        p = torch.softmax(s, dim=-1)
        if drop is not None:
            assert query_row is None
            keep = dropout_keep_range(drop[1], b0 * heads * n * n, bb * heads * n * n, drop[0], dev).view(bb, heads, n, n)
            p = p * keep.double() / (1.0 - float(np.float32(drop[0])))
        o = (p @ v).permute(0, 2, 1, 3).reshape(bb, nq, heads * hd)
        out[b0: b0 + bb] = o.detach()
        o.backward(dout[b0: b0 + bb].detach().to(torch.float64).reshape(bb, nq, heads * hd))
        grad[b0: b0 + bb] = x.grad
        del x, q, k, v, s, p, o
    if query_row is not None:
        out, lse = out[:, 0], lse[:, :, 0]
    return out, lse, grad


def text_mask(batch, n, seed=0):
    """key validity shaped like padded text: position 0 (the CLS slot) always valid, then a valid prefix whose length differs per sample;
    sample 0 keeps the CLS slot alone, sample 1 every key, every fifth sample from the third on has a hole inside its prefix"""
    mask = torch.ones(batch, n, dtype=torch.bool)
    if n < 2:
        return mask
    g = torch.Generator().manual_seed(1000 + seed)
    L = torch.randint(2, n + 1, (batch,), generator=g)
    L[0] = 1
    if batch > 1:
        L[1] = n
    if batch > 2 and n > 3:
        L[2] = max(int(L[2]), 4)                               # (long enough for the first hole)
    mask = torch.arange(n)[None, :] < L[:, None]
    for bi in range(2, batch, 5):
        if int(L[bi]) > 3:
            mask[bi, 1 + int(torch.randint(0, int(L[bi]) - 2, (1,), generator=g))] = False
    return mask


def assert_every_query_sees_a_key(mask, causal=False, query_row=None):
    """the condition of the full-size cases: no query row with all of its visible keys masked -- there the product returns 0 where the reference's
    softmax over all-filled scores returns the uniform average (include/xclip.h; tests/test_kernels_emu.py test_edge_cases_of_the_row_kernels)"""
    if mask is None:
        return
    seen = mask.cumsum(1) > 0 if causal else mask.any(1, keepdim=True)        # [b, n] / [b, 1]: query i sees a valid key among 0 .. i / among all
    if query_row is not None and causal:
        seen = seen[:, query_row]
    assert bool(seen.all()), "a query row has every visible key masked"


def _worst_heads(got, want, heads, hd, bound_abs):
    """which (sample, head) slots of a [b, n, k * heads * hd] tensor exceed an absolute error -- the evidence a failing full-size case prints"""
    b, n, w = got.shape
    d = (got.to(want.device, torch.float64) - want).abs().nan_to_num(nan=float("inf")).view(b, n, w // (heads * hd), heads, hd).amax(dim=(1, 2, 4))
    bad = (d > bound_abs).nonzero()
    return f"{bad.shape[0]} of {b * heads} (sample, head) slots beyond the bound; first: {bad[:12].tolist()}; work-group slots (b * heads + h): {[int(r[0]) * heads + int(r[1]) for r in bad[:12]]}"


def _randn_nonzero(shape, g, dev, dtype):
    """standard normal values drawn on the device, none of them zero: among 4e8 draws a few dozen are exactly 0 (Box-Muller at an angle of 0
    or pi), and a zero dO or V element would let a misplaced one cancel -- those become 1"""
    x = torch.randn(*shape, generator=g, device=dev).to(dtype)
    x = torch.where(x == 0, torch.ones_like(x), x)
    assert bool((x != 0).all())
    return x


def case_attention_full(dev, dtype, batch, n, heads, hd=64, masked=True, causal=False, drop=None, tag="", seed=0, repeats=3):
    """every head of a launch that fills the chip: random qkv and dO (non-zero everywhere, different in every head: a work-group that
    read another head's image, a stale LDS image or an image still in flight cannot cancel), outputs allocated NaN-poisoned (an element
    no work-group wrote is NaN), out / lse / dqkv against the blocked fp64 reference under the bounds of case_attention -- in ulps of the
    scale of the WHOLE reference tensor -- and `repeats` more launches of forward and backward bit-identical (fixed summation order, no
    atomics: held to it under contention)."""
    from clip_cases import poisoned_empty
    g = torch.Generator(device=dev).manual_seed(7000 + seed)
    qkv = _randn_nonzero((batch, n, 3 * heads * hd), g, dev, dtype)
    dout = _randn_nonzero((batch, n, heads * hd), g, dev, dtype)
    mask = text_mask(batch, n, seed).to(dev) if masked else None
    assert_every_query_sees_a_key(mask, causal)
    scale = hd ** -0.5
    dk = {} if drop is None else dict(dropout_p=drop[0], dropout_seed=drop[1])

    def launch():
        with poisoned_empty():
            out, lse = ops.attention_fwd(qkv, mask, heads, scale, causal, hd, **dk)
            dqkv = ops.attention_bwd(qkv, mask, out, dout, lse, heads, scale, causal, hd, **dk)
        return out, lse, dqkv

    out, lse, dqkv = launch()
    again = [launch() for _ in range(repeats)]
    r_out, r_lse, r_grad = attention_ref_blocked(qkv, dout, mask, heads, scale, causal, hd, drop)
    tag = f" full size [{tag}]"
    for got, want, dt, name, kw in ((out, r_out, dtype, "attn out", dict(ulps=2.0, unit="scale")), (lse, r_lse, torch.float32, "attn lse", {}),
                                    (dqkv, r_grad, dtype, "attn dqkv", dict(mult=3.0, ulps=2.0, unit="scale"))):
        try:
            close(got, want, dt, name + tag + (" <- bf16" if dt != dtype else ""), **kw)
        except AssertionError as e:
            if got.dim() != 3 or got.shape[1] != n:
                raise
            s = float(want.abs().max())
            bound = 2.0 * float(bf16_ulp(torch.tensor(s, dtype=torch.float64))) if dt == torch.bfloat16 else tol(dt) * kw.get("mult", 1.0) * s
            raise AssertionError(f"{e}\n{name}: {_worst_heads(got, want, heads, hd, bound)}; first dispatch round = work-group slots below 2 x CUs") from None
    for i, (o2, l2, d2) in enumerate(again):
        assert torch.equal(o2, out), f"out differs between launch 0 and {i + 1}{tag}"
        assert torch.equal(l2, lse), f"lse differs between launch 0 and {i + 1}{tag}"
        assert torch.equal(d2, dqkv), f"dqkv differs between launch 0 and {i + 1}{tag}"


def case_attention_pool_full(dev, dtype, batch, n, heads, hd=64, row=0, causal=False, tag="", seed=0, repeats=3):
    """case_attention_pool with every CU busy (one wave per (sample, head), four to a work-group: 2048 work-groups at the benchmark's batch):
    text-like mask, poisoned outputs, every row of out / lse / dq / dkv against the blocked reference, `repeats` more launches bit-identical"""
    from clip_cases import poisoned_empty
    g = torch.Generator(device=dev).manual_seed(7100 + seed)
    inner = heads * hd
    qkv = _randn_nonzero((batch, n, 3 * inner), g, dev, dtype)
    dout = _randn_nonzero((batch, inner), g, dev, dtype)
    mask = text_mask(batch, n, seed).to(dev)
    assert_every_query_sees_a_key(mask, causal, row)
    scale = hd ** -0.5
    q = qkv[:, row, :inner].contiguous()
    kv = qkv[:, :, inner:].contiguous()
    vis = row + 1 if causal else None

    def launch():
        with poisoned_empty():
            out, lse = ops.attention_pool_fwd(q, kv, mask, heads, scale, hd, vis)
            dq, dkv = ops.attention_pool_bwd(q, kv, mask, out, dout, lse, heads, scale, hd, vis)
        return out, lse, dq, dkv

    out, lse, dq, dkv = launch()
    again = [launch() for _ in range(repeats)]
    r_out, r_lse, r_grad = attention_ref_blocked(qkv, dout, mask, heads, scale, causal, hd, None, query_row=row)
    tag = f" pooled row {row} full size [{tag}]"
    close(out, r_out, dtype, "attn out" + tag, ulps=2.0, unit="scale")
    close(lse, r_lse, torch.float32, "attn lse" + tag + (" <- bf16" if dtype == torch.bfloat16 else ""))
    close(dq, r_grad[:, row, :inner], dtype, "attn dq" + tag, mult=3.0, ulps=2.0, unit="scale")
    close(dkv, r_grad[:, :, inner:], dtype, "attn dkv" + tag, mult=3.0, ulps=2.0, unit="scale")
    off = r_grad[:, :, :inner].clone()
    off[:, row] = 0
    assert float(off.abs().max()) == 0.0                       # (the reference's dQ is zero off the pooled row)
    for i, (o2, l2, q2, k2) in enumerate(again):
        assert torch.equal(o2, out) and torch.equal(l2, lse), f"pooled forward differs between launch 0 and {i + 1}{tag}"
        assert torch.equal(q2, dq) and torch.equal(k2, dkv), f"pooled backward differs between launch 0 and {i + 1}{tag}"


def case_attention_random(dev, cases, seed, max_n=400, max_batch=5, max_heads=3):
    """a seeded sweep over what the fixed lists do not cross: storage type, head-slot width, dropout, key padding, causal masking, n from
    1 (legal in the reference) to beyond A3_MAX_N, batch 1 .. 5 -- every dispatch branch of xclip_attention_fwd / _bwd at lengths nobody chose"""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    for _ in range(cases):
        dtype = DTYPES[ri(0, 1)]
        hd = (64, 128)[ri(0, 1)]
        drop = (0.25, 0xC0FFEE1234567 + ri(0, 1 << 20)) if ri(0, 3) == 0 else None
        n, batch, heads = ri(1, max_n), ri(1, max_batch), ri(1, max_heads)
        masked, causal = bool(ri(0, 1)), ri(0, 2) == 0
        case_attention(dev, dtype, batch, n, heads, masked, causal=causal, hd=hd, drop=drop)


def case_simloss(dev, dtype, nq, nk, d, dcl, diag_off=0, tau=1.3):
    T = O.l2_normalize(rnd((nq, d), torch.float32, 25)).to(dtype)
    I = O.l2_normalize(rnd((nk, d), torch.float32, 26)).to(dtype)
    temp = math.exp(tau)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    lse, pos = ops.simloss_fwd(T.to(dev), I.to(dev), temp, diag_off, dcl, 0.5, loss)
    S = temp * ref64(T) @ ref64(I).t()
    rows = torch.arange(nq)
    diag = torch.zeros(nq, nk, dtype=torch.bool)
    valid = (rows + diag_off < nk) & (rows + diag_off >= 0)
    diag[rows[valid], (rows + diag_off)[valid]] = True
    E = S.exp()
    if dcl:
        E = E.masked_fill(diag, 0.0)
    lse_r = E.sum(1).log()
    close(lse, lse_r, dtype, "lse", scale=float(lse_r.abs().max()))
    pos_r = torch.zeros(nq, dtype=torch.float64)
    pos_r[valid] = S[diag]
    close(pos, pos_r, dtype, "pos", scale=float(S.abs().max()))
    close(loss.reshape(1), (0.5 * (lse_r - pos_r).sum()).reshape(1), dtype, "loss", mult=2.0)

    # gradient factor G and dtau with arbitrary coefficients
    a, c, e = 0.013, 0.021, 0.05
    g = torch.Generator().manual_seed(27)
    lse_k = (torch.rand(nk, generator=g) * 2 + float(S.max())).float()
    dtau = torch.zeros((), dtype=torch.float32, device=dev)
    G = ops.simloss_grad(T.to(dev), I.to(dev), temp, diag_off, dcl, a, c, e, lse.detach(), lse_k.to(dev), dtau)
    lq = lse.detach().cpu().double()
    off = (~diag).double() if dcl else torch.ones_like(S)
    Gr = (a * (S - lq[:, None]).exp() + c * (S - lse_k.double()[None, :]).exp()) * off - e * diag.double()
    close(G[:, :nk], Gr, dtype, "G", mult=2.0)
    assert float(G[:, nk:].abs().sum()) == 0.0
    close(dtau.reshape(1), (Gr * S).sum().reshape(1), dtype, "dtau", scale=float((Gr * S).abs().sum()), mult=2.0)


def case_simloss_spread(dev, dtype, nq, nk, d, dcl, diag_off=0, temp=200.0, matched=(0, 1, 2, 3)):
    """exp(tau) = 200 with a few PERFECTLY matched pairs among unrelated ones -- matched rows / columns have
    log-sum-exps of ~200, the rest ~10 - 60, so inside one 128 x 64 wave block the lse values spread by more than the ~88 a single
    reference point of the one-exponential form exp(s - R) exp(R - lse) can bridge in fp32 (0 x inf = NaN in nearly every entry of
    G with the round-3 kernel).  Forward and G with the REAL row / column log-sum-exps, InfoNCE and DCL (in DCL the positive is not
    part of its own lse and exceeds it by ~150: exp(s - lse) itself overflows there and must never be formed)."""
    T = O.l2_normalize(rnd((nq, d), torch.float32, 25)).to(dtype)
    I = O.l2_normalize(rnd((nk, d), torch.float32, 26)).to(dtype)
    for r in matched:
        if 0 <= r + diag_off < nk and r < nq:
            I[r + diag_off] = T[r]
            I[(r + diag_off + 7) % nk] = T[r]        # a duplicate of the positive off the diagonal: DCL rows / columns see a logit of `temp` too
    S = temp * ref64(T) @ ref64(I).t()
    rows = torch.arange(nq)
    diag = torch.zeros(nq, nk, dtype=torch.bool)
    valid = (rows + diag_off < nk) & (rows + diag_off >= 0)
    diag[rows[valid], (rows + diag_off)[valid]] = True
    Sm = S.masked_fill(diag, -math.inf) if dcl else S
    lse_r = torch.logsumexp(Sm, 1)
    lse_c = torch.logsumexp(Sm, 0)
    assert float(lse_r.max() - lse_r.min()) > 100.0 and float(lse_c.max() - lse_c.min()) > 100.0      # the case is the case
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    lse, pos = ops.simloss_fwd(T.to(dev), I.to(dev), temp, diag_off, dcl, 0.5, loss)
    close(lse, lse_r, dtype, "lse (spread)", scale=float(lse_r.abs().max()))
    a, c, e = 0.5 / nq, 0.5 / nq, 1.0 / nq
    for aa, cc in ((a, c), (a, 0.0), (0.0, c)):
        dtau = torch.zeros((), dtype=torch.float32, device=dev)
        G = ops.simloss_grad(T.to(dev), I.to(dev), temp, diag_off, dcl, aa, cc, e, lse_r.float().to(dev), lse_c.float().to(dev), dtau)
        off = (~diag).double() if dcl else torch.ones_like(S)
        lq, lk = lse_r.float().double(), lse_c.float().double()
        Gr = (aa * (Sm - lq[:, None]).exp() + cc * (Sm - lk[None, :]).exp()) * off - e * diag.double()
        assert bool(torch.isfinite(G.float()).all()), f"G not finite (a={aa}, c={cc}, dcl={dcl})"
        close(G[:, :nk], Gr, dtype, "G (spread)", mult=2.0)
        want = (Gr * S).sum()
        close(dtau.reshape(1), want.reshape(1), dtype, "dtau (spread)", scale=float((Gr * S).abs().sum()), mult=2.0)


def case_simloss_closed_form(dev, dtype, B, d, dcl):
    """full head (two LSE passes + G + two GEMMs) against the numpy closed form of SURVEY Appendix C"""
    T = O.l2_normalize(rnd((B, d), torch.float32, 28)).to(dtype)
    I = O.l2_normalize(rnd((B, d), torch.float32, 29)).to(dtype)
    tau = 0.7
    temp = math.exp(tau)
    w = 1.0 / (2 * B)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    lse_r, _ = ops.simloss_fwd(T.to(dev), I.to(dev), temp, 0, dcl, w, loss)
    lse_c, _ = ops.simloss_fwd(I.to(dev), T.to(dev), temp, 0, dcl, w, loss)
    dtau = torch.zeros((), dtype=torch.float32, device=dev)
    G = ops.simloss_grad(T.to(dev), I.to(dev), temp, 0, dcl, w, w, 1.0 / B, lse_r, lse_c, dtau)
    dT = ops.gemm(G[:, :B], I.to(dev), B, d, B, False, True, temp)
    dI = ops.gemm(G[:, :B], T.to(dev), B, d, B, True, True, temp)
    want = O.simloss_closed_form(T.double().numpy(), I.double().numpy(), tau, dcl)
    close(loss.reshape(1), torch.tensor([want["loss"]]), dtype, "loss", mult=2.0)
    close(dtau.reshape(1), torch.tensor([want["dtau"]]), dtype, "dtau", scale=1.0, mult=2.0)
    sc = float(np.abs(want["dT"]).max())
    close(dT, torch.tensor(want["dT"]), dtype, "dT", scale=sc, mult=4.0, ulps=2.0, unit="scale")
    close(dI, torch.tensor(want["dI"]), dtype, "dI", scale=sc, mult=4.0, ulps=2.0, unit="scale")


def case_layernorm_residual_paths(dev, dtype, rows, dim, grp):
    """LN forward writing behind a CLS slot of every `grp` rows + LN backward with the skip-path gradient added"""
    x = rnd((rows, dim), dtype, 30)
    g = (1 + 0.1 * rnd((dim,), torch.float32, 31)).to(dtype)
    dy = rnd((rows, dim), dtype, 32)
    dres = rnd((rows, dim), dtype, 33)
    nb = rows // grp
    out = torch.full((nb * (grp + 1), dim), 7.0, dtype=dtype).to(dev)
    y, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), out=out, out_group=grp)
    x64 = ref64(x).requires_grad_(True)
    g64 = ref64(g)
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    yr = (x64 - mu) * torch.rsqrt(var + ops.ln_eps(dtype)) * g64
    got = out.cpu().view(nb, grp + 1, dim)
    close(got[:, 1:].reshape(rows, dim), yr, dtype, "ln grouped y")
    assert float((got[:, 0].float() - 7.0).abs().max()) == 0.0, "CLS slots must stay untouched"
    yr.backward(ref64(dy))
    dx, _ = ops.layernorm_bwd(dy.to(dev), x.to(dev), g.to(dev), mean, rstd, dres=dres.to(dev))
    close(dx, x64.grad + ref64(dres), dtype, "ln dx + dres", mult=2.0)


def case_row_moves(dev, dtype):
    """copy_rows on strided views, rows_scatter_add (table + column sum)"""
    src = rnd((6, 5, 64), dtype, 34).to(dev)
    dst = torch.zeros(6, 64, dtype=dtype, device=dev)
    ops.copy_rows(src[:, 2], dst)
    assert torch.equal(dst.cpu(), src[:, 2].cpu())
    back = torch.zeros(6, 5, 64, dtype=dtype, device=dev)
    ops.copy_rows(dst, back[:, 3])
    assert torch.equal(back[:, 3].cpu(), dst.cpu()) and float(back[:, :3].abs().sum()) == 0.0
    rows, D, T = 300, 72 if dtype == torch.bfloat16 else 68, 7
    s = rnd((rows, D), dtype, 35)
    idx = (torch.arange(rows) * 5 % T).to(torch.int32)
    table = torch.zeros(T, D, dtype=torch.float32, device=dev)
    col = torch.zeros(D, dtype=torch.float32, device=dev)
    ops.rows_scatter_add(s.to(dev), idx.to(dev), table, col)
    want = torch.zeros(T, D, dtype=torch.float64).index_add_(0, idx.long(), ref64(s))
    close(table, want, torch.float32, "scatter table", mult=8.0)
    close(col, ref64(s).sum(0), torch.float32, "column sum", mult=8.0)


def case_simloss_chunked(dev, dtype, dcl):
    """K consumed in rank-sized chunks (local chunk first), temperature as a device scalar, gmul + scale folded into G"""
    nq, d, sizes, rank = 24, 64, [24, 16, 24], 2
    B = sum(sizes)
    off = sum(sizes[:rank])
    T = O.l2_normalize(rnd((nq, d), torch.float32, 36)).to(dtype)
    I = O.l2_normalize(rnd((B, d), torch.float32, 37)).to(dtype)
    tau = torch.tensor([0.9], dtype=torch.float32)
    temp = math.exp(0.9)
    offs = [sum(sizes[:r]) for r in range(len(sizes))]
    order = [rank] + [r for r in range(len(sizes)) if r != rank]
    chunks = [(I[offs[r]: offs[r] + sizes[r]].contiguous().to(dev), offs[r]) for r in order]
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    seen = []
    lse, pos = ops.simloss_chunked_fwd(T.to(dev), chunks, 1.0, off, dcl, 0.25, loss, log_scale=tau.to(dev),
                                       before_chunk=lambda c: seen.append(c))
    assert seen == [0, 1, 2]
    lse1, pos1 = ops.simloss_fwd(T.to(dev), I.to(dev), temp, off, dcl, 0.25, None)
    close(lse, lse1.cpu(), dtype, "chunked lse", scale=float(lse1.abs().max()))
    close(pos, pos1.cpu(), dtype, "chunked pos", scale=float(pos1.abs().max()) + 1e-6)
    S = temp * ref64(T) @ ref64(I).t()
    diag = torch.zeros(nq, B, dtype=torch.bool)
    diag[torch.arange(nq), torch.arange(nq) + off] = True
    E = S.exp().masked_fill(diag, 0.0) if dcl else S.exp()
    close(loss, (0.25 * (E.sum(1).log() - S[diag]).sum()).reshape(1), dtype, "chunked loss", mult=2.0)
    # G written chunk-wise into a wide buffer, pre-multiplied by temp and by a device-side upstream gradient
    a, c = 0.02, 0.0
    gm = torch.tensor([1.7], dtype=torch.float32)
    v = ops.vec(dtype)
    G = torch.zeros(nq, B, dtype=dtype, device=dev)
    dtau = torch.zeros(1, dtype=torch.float32, device=dev)
    lk = torch.zeros(B, dtype=torch.float32, device=dev)
    for (K, col0) in chunks:
        ops.simloss_grad(T.to(dev), K, 1.0, off - col0, dcl, a, c, a + c, lse, lk[col0: col0 + K.shape[0]].contiguous(), dtau,
                         log_scale=tau.to(dev), gmul=gm.to(dev), times_scale=True, out=G[:, col0: col0 + K.shape[0]])
    lq = lse.cpu().double()
    offm = (~diag).double() if dcl else torch.ones_like(S)
    Gr = 1.7 * (a * (S - lq[:, None]).exp() * offm - (a + c) * diag.double())
    close(G, temp * Gr, dtype, "chunked G", mult=2.0)
    close(dtau, (Gr * S).sum().reshape(1), dtype, "chunked dtau", scale=float((Gr * S).abs().sum()), mult=2.0)


def case_scatter_sorted(dev, dtype):
    """sorted segmented scatter-add == index_add, incl. the text row map (rows behind a CLS slot) and runs crossing chunks"""
    b, n, D, vocab = 9, 37, 64, 23
    g = torch.Generator().manual_seed(41)
    tok = torch.randint(0, vocab, (b, n), generator=g)
    tok[:, :5] = 7                                          # a long run spanning several wave chunks
    dout = rnd((b, n + 1, D), dtype, 42)
    st = torch.sort(tok.reshape(-1))
    table = torch.zeros(vocab, D, dtype=torch.float32, device=dev)
    ops.scatter_add_sorted(dout.to(dev).view(b * (n + 1), D), st.values.to(dev), st.indices.to(dev), table, n_in=n, n_out=n + 1, row_off=1)
    want = torch.zeros(vocab, D, dtype=torch.float64).index_add_(0, tok.reshape(-1), ref64(dout)[:, 1:].reshape(-1, D))
    close(table, want, torch.float32, "sorted scatter", mult=8.0)
    dE, dP, dcls = ops.text_embed_bwd(dout.to(dev), tok.to(dev), vocab, True, True, sorted_tokens=ops.sort_ids(tok.reshape(-1).to(dev), vocab))
    close(dE, want, torch.float32, "dE sorted", mult=8.0)
    close(dP, ref64(dout)[:, 1:].sum(0), torch.float32, "dP", mult=8.0)
    close(dcls, ref64(dout)[:, 0].sum(0), torch.float32, "dcls", mult=8.0)


def case_sort_ids(dev, sizes=((1, 2), (63, 5), (64, 256), (1000, 7), (1024, 49408), (1025, 300), (4099, 49408), (5000, 262144), (9000, 1 << 20))):
    """sort.h against torch.sort(stable=True): one / two / three radix passes (id_limit up to 2^8 / 2^16 / 2^24), counts around the 1024-pair
    work-group and the 64-lane slice, long runs of one id (a padded batch), ids that differ only in a high digit; the result is the STABLE
    order -- and running it twice gives the same bits, which is what the segment sums behind it need"""
    for (n, limit) in sizes:
        g = torch.Generator().manual_seed(n * 31 + limit)
        ids = torch.randint(0, limit, (n,), generator=g)
        if n > 200:
            ids[n // 3: n // 3 + 150] = limit - 1                # a run crossing slices, rounds and (n > 1024) work-groups
            ids[::17] = 0
            if limit > 300:
                ids[5::19] = 256 * ((limit - 1) // 256)          # equal low digit, different high digit
        want = torch.sort(ids, stable=True)
        got, perm = ops.sort_ids(ids.to(dev), limit)
        assert torch.equal(got.cpu(), want.values), (n, limit, "ids")
        assert torch.equal(perm.cpu(), want.indices), (n, limit, "perm")
        again = ops.sort_ids(ids.to(dev), limit)
        assert torch.equal(again[0], got) and torch.equal(again[1], perm)
    e = ops.sort_ids(torch.empty(0, dtype=torch.int64, device=dev), 10)
    assert e[0].numel() == 0 and e[1].numel() == 0


def case_gelu_accuracy(dev, dtype):
    """the shared-exponential erf GELU stays within fp32 round-off class of the exact one, forward and backward"""
    rows, dim = 64, 64
    x = torch.linspace(-9, 9, rows * 2 * dim).reshape(rows, 2 * dim).to(dtype)
    x[:, :dim] = 1.0                                        # value = 1 -> the LN input is gelu(gate) itself
    g = torch.ones(dim, dtype=dtype)
    y, mean, rstd = ops.layernorm_fwd(x.to(dev), g.to(dev), None, True)
    x64 = ref64(x)
    v = O.geglu(x64)
    mu = v.mean(-1, keepdim=True)
    yr = (v - mu) * torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + ops.ln_eps(dtype))
    close(y, yr, dtype, "gelu via geglu-ln")


def case_simreg_diff(dev, dtype, rows, cols, diag_off):
    """D = A - C off the global diagonal + sum of squares (x_clip.py:773-784)"""
    A = rnd((rows, cols), dtype, 41)
    Cm = rnd((rows, cols), dtype, 42)
    acc = torch.zeros(1, dtype=torch.float32, device=dev)
    D = ops.simreg_diff(A.to(dev).clone(), Cm.to(dev), diag_off, acc)
    ref = ref64(A) - ref64(Cm)
    for r in range(rows):
        if 0 <= r + diag_off < cols:
            ref[r, r + diag_off] = 0
    close(D, ref, dtype, "simreg D")
    want = float((ref ** 2).sum())
    assert abs(float(acc) - want) <= 1e-4 * max(1.0, want), (float(acc), want)


def case_rotary(dev, dtype, batch, n, heads, hd=64):
    """rotary embedding on packed q | k | v head slots (hd = 64 or 128 features each), forward and its transposed (backward) form
    (x_clip.py:155-176)"""
    slots = 3 * heads
    x = rnd((batch * n, slots * hd), dtype, 51)
    inv_freq = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).to(dev)
    y = ops.rotary_(x.to(dev).clone(), n, inv_freq, head_dim=hd)
    fr = O.rotary_freqs(n, hd, torch.float64)                                  # [n, 32]
    x64 = ref64(x).view(batch, n, slots, hd)
    ref = O.apply_rotary(fr[None, :, None, :], x64).reshape(batch * n, slots * hd)
    close(y, ref, dtype, "rotary fwd")
    z = ops.rotary_(y.clone(), n, inv_freq, inverse=True, head_dim=hd)         # R^T R = identity
    close(z, ref64(x), dtype, "rotary inverse", mult=2.0, ulps=2.0, unit="scale")


def case_dwconv(dev, dtype, batch, h, C):
    """depthwise 4x4 / stride 2 / pad 1 convolution over the token grid, forward and both gradients (x_clip.py:560-568)"""
    x = rnd((batch, h * h, C), dtype, 61)
    w = rnd((C, 1, 4, 4), dtype, 62) * 0.25
    dy = rnd((batch, (h // 2) ** 2, C), dtype, 63)
    y = ops.dwconv4s2_fwd(x.to(dev), w.to(dev).view(C, 16))
    dwa = torch.zeros(C * 16, dtype=torch.float32, device=dev)
    dx = ops.dwconv4s2_bwd(dy.to(dev), x.to(dev), w.to(dev).view(C, 16), dwa)
    x64 = ref64(x).requires_grad_(True)
    w64 = ref64(w).requires_grad_(True)
    img = x64.transpose(1, 2).reshape(batch, C, h, h)
    ref = torch.nn.functional.conv2d(img, w64, None, stride=2, padding=1, groups=C).flatten(2).transpose(1, 2)
    ref.backward(ref64(dy))
    close(y, ref, dtype, "dwconv y", mult=2.0)
    close(dx, x64.grad, dtype, "dwconv dx", mult=2.0)
    close(dwa.view(C, 1, 4, 4), w64.grad, torch.float32 if dtype == torch.float32 else dtype, "dwconv dw", mult=4.0)


def case_cross_entropy(dev, dtype, rows, cols, ld):
    """gathered rows -> softmax cross-entropy with labels, forward + in-place gradient; padding columns [cols, ld) ignored / zeroed"""
    g = torch.Generator().manual_seed(71)
    src = rnd((rows * 3, ld), dtype, 72) * 3.0
    idx = torch.randperm(rows * 3, generator=g)[:rows].to(torch.int32)
    x = ops.gather_rows(src.to(dev), idx.to(dev))
    assert torch.equal(x.cpu(), src[idx.long()])
    labels = torch.randint(0, cols, (rows,), generator=g)
    acc = torch.zeros(1, dtype=torch.float32, device=dev)
    lse = ops.cross_entropy_fwd(x, cols, labels.to(dev), acc)
    x64 = ref64(src)[idx.long()][:, :cols].clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(x64, labels, reduction="sum")
    assert abs(float(acc) - float(ref.detach())) <= 2e-4 * max(1.0, abs(float(ref.detach()))), (float(acc), float(ref.detach()))
    (ref / rows * 0.7).backward()
    gm = torch.full((1,), 0.7, dtype=torch.float32, device=dev)
    d = ops.cross_entropy_bwd_(x, cols, labels.to(dev), lse, gm)
    close(d[:, :cols], x64.grad, dtype, "ce grad", mult=2.0)
    assert float(d[:, cols:].abs().max()) == 0.0 if ld > cols else True


def case_layernorm_chain(dev, dtype, rows, dim):
    """x1 = LN(p) g1 + res, h2 = LN(x1) g2 in one pass, and its backward, against the two-call composition in fp64"""
    p_ = rnd((rows, dim), dtype, 81)
    res = rnd((rows, dim), dtype, 82)
    g1 = (1.0 + 0.1 * rnd((dim,), torch.float32, 83)).to(dtype)
    g2 = (1.0 + 0.1 * rnd((dim,), torch.float32, 84)).to(dtype)
    dh2 = rnd((rows, dim), dtype, 85)
    dres = rnd((rows, dim), dtype, 86)
    x1, m1, r1, h2, m2, r2 = ops.layernorm_chain_fwd(p_.to(dev), g1.to(dev), res.to(dev), g2.to(dev))
    dg2 = torch.zeros(dim, dtype=torch.float32, device=dev)
    dg1 = torch.zeros(dim, dtype=torch.float32, device=dev)
    dx1, dp = ops.layernorm_chain_bwd(dh2.to(dev), x1, g2.to(dev), m2, r2, dres.to(dev), p_.to(dev), g1.to(dev), m1, r1, dg2, dg1)
    eps = 1e-5 if dtype == torch.float32 else 1e-3
    p64, g164, g264 = ref64(p_).requires_grad_(True), ref64(g1).requires_grad_(True), ref64(g2).requires_grad_(True)

    def ln(t, g):
        return (t - t.mean(-1, keepdim=True)) * torch.rsqrt(t.var(-1, unbiased=False, keepdim=True) + eps) * g

    x1r = ln(p64, g164) + ref64(res)
    x1r.retain_grad()
    h2r = ln(x1r, g264)
    (h2r * ref64(dh2)).sum().backward(retain_graph=True)
    close(x1, x1r, dtype, "chain x1")
    close(h2, h2r, dtype, "chain h2", mult=3.0, ulps=2.0, unit="scale")                    # (h2 is computed from the ROUNDED x1, like two separate calls)
    # total gradient of x1 = through LN2 + the skip path; dp = through LN1
    want_dx1 = x1r.grad + ref64(dres)
    close(dx1, want_dx1, dtype, "chain dx1", mult=3.0, ulps=2.0, unit="scale")
    gp, = torch.autograd.grad((ln(p64, g164) * want_dx1.detach()).sum(), p64)
    close(dp, gp, dtype, "chain dp", mult=4.0, ulps=2.0, unit="scale")
    close(dg2, g264.grad, torch.float32 if dtype == torch.float32 else dtype, "chain dg2", mult=4.0, ulps=2.0, unit="scale")
    xh1 = ((p64 - p64.mean(-1, keepdim=True)) * torch.rsqrt(p64.var(-1, unbiased=False, keepdim=True) + eps)).detach()
    close(dg1, (want_dx1.detach() * xh1).sum(0), torch.float32 if dtype == torch.float32 else dtype, "chain dg1", mult=4.0, ulps=2.0, unit="scale")


def case_batchnorm(dev, dtype, rows, cols, relu, affine, training, offset=0.0):
    """BatchNorm1d (+ReLU) over the rows, forward, running-statistics update and backward against torch's F.batch_norm in fp64
    (reference visual_ssl.py:112-136).  `offset` shifts the columns far from zero (the shifted-variance accumulation)."""
    F = torch.nn.functional
    x = (rnd((rows, cols), dtype, 91).float() * (0.5 + rnd((cols,), torch.float32, 92).abs()) + offset + rnd((cols,), torch.float32, 93)).to(dtype)
    dy = rnd((rows, cols), dtype, 94)
    gamma = (1.0 + 0.2 * rnd((cols,), torch.float32, 95)) if affine else None
    beta = 0.3 * rnd((cols,), torch.float32, 96) if affine else None
    rm0 = 0.1 * rnd((cols,), torch.float32, 97) + offset
    rv0 = 1.0 + 0.2 * rnd((cols,), torch.float32, 98).abs()
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    eps, mom = 1e-5, 0.1
    to = lambda t: None if t is None else t.to(dev)
    y, mean, rstd = ops.batchnorm_fwd(x.to(dev), to(gamma), to(beta), rm, rv, mom, eps, training, relu)
    dx, dg, db = ops.batchnorm_bwd(x.to(dev), dy.to(dev), to(gamma), to(beta), mean, rstd, training, relu, affine)
    x64 = ref64(x).requires_grad_(True)
    g64 = None if gamma is None else ref64(gamma).requires_grad_(True)
    b64 = None if beta is None else ref64(beta).requires_grad_(True)
    rm64, rv64 = ref64(rm0).clone(), ref64(rv0).clone()
    z = F.batch_norm(x64, rm64, rv64, g64, b64, training, mom, eps)
    # a pre-activation within rounding of 0 may take either side of the ReLU (at 70000 x 4096 a handful do, and each moves a column sum
    # by O(1)): the reference uses the side the kernel took
    want = z * (y.detach().cpu() > 0).double() if relu else z
    if relu:
        assert float((torch.relu(z.detach()) - want.detach()).abs().max()) < (1e-5 if dtype == torch.float32 else 1e-2)
    (want * ref64(dy)).sum().backward()
    close(y, want, dtype, "bn y", mult=2.0)
    if training:
        close(rm, rm64, torch.float32, "bn running_mean", scale=max(1.0, abs(offset)))
        close(rv, rv64, torch.float32, "bn running_var", mult=5.0)
    else:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    close(dx, x64.grad, dtype, "bn dx", mult=4.0)
    if affine:
        close(dg, g64.grad, dtype, "bn dgamma", mult=4.0)
        close(db, b64.grad, dtype, "bn dbeta", mult=4.0)


def case_neg_cosine(dev, dtype, rows, dim):
    """SimSiam loss_fn (visual_ssl.py:104-107), mean over rows accumulated through coef, and its gradient w.r.t. the prediction"""
    F = torch.nn.functional
    p_, z_ = rnd((rows, dim), dtype, 101), rnd((rows, dim), dtype, 102)
    acc = torch.zeros(1, dtype=torch.float32, device=dev)
    coef = 1.0 / rows
    st = ops.neg_cosine_fwd(p_.to(dev), z_.to(dev), coef, acc)
    p64 = ref64(p_).requires_grad_(True)
    want = (2 - 2 * (F.normalize(p64, dim=-1) * F.normalize(ref64(z_), dim=-1)).sum(-1)).mean()
    assert abs(float(acc) - float(want.detach())) < 2e-5 * max(1.0, abs(float(want.detach()))), (float(acc), float(want.detach()))
    (want * 0.6).backward()
    gm = torch.full((1,), 0.6, dtype=torch.float32, device=dev)
    dp = ops.neg_cosine_bwd(p_.to(dev), z_.to(dev), st, gm, coef)
    close(dp, p64.grad, dtype, "cosine dp", mult=2.0)


def case_nt_xent(dev, dtype, rows, dim, temperature):
    """NT-Xent between two sets of projections (nt_xent_loss, visual_ssl.py:90-102) built from the contrastive head's kernels, against
    the oracle's restatement in fp64; both gradients"""
    from x_clip_amd.visual_ssl import nt_xent_loss
    scale = 1.0 if dtype == torch.float32 else 0.5
    q_, k_ = rnd((rows, dim), dtype, 111, scale), rnd((rows, dim), dtype, 112, scale)
    q, k = q_.to(dev).requires_grad_(True), k_.to(dev).requires_grad_(True)
    loss = nt_xent_loss(q, k, temperature)
    (loss * 0.7).backward()
    q64, k64 = ref64(q_).requires_grad_(True), ref64(k_).requires_grad_(True)
    want = O.nt_xent(q64, k64, temperature)
    (want * 0.7).backward()
    assert abs(float(loss.detach()) - float(want.detach())) < (2e-5 if dtype == torch.float32 else 2e-2) * max(1.0, abs(float(want.detach()))), (float(loss.detach()), float(want.detach()))
    gs = max(float(q64.grad.abs().max()), float(k64.grad.abs().max()))
    close(q.grad, q64.grad, dtype, "nt-xent dq", scale=gs, mult=4.0, ulps=2.0, unit="scale")
    close(k.grad, k64.grad, dtype, "nt-xent dk", scale=gs, mult=4.0, ulps=2.0, unit="scale")


def case_gemm_splitk_uneven(dev, M=1248, N=768, K=6144):
    """split-K with a slice count that does not divide the K steps (96 steps over 17 slices: rounding the slice up to 6 steps leaves the
    17th slice empty).  The scratch is poisoned first: a slice that returns without writing its slab would put NaN into every output."""
    dtype = torch.bfloat16
    a = rnd((M, K), dtype, 121, 0.1)
    b = rnd((K, N), dtype, 122, 0.1)
    ws = ops.workspace(dev, 80 << 20)
    ws.fill_(0xFF)
    c = ops.gemm(a.to(dev), b.to(dev), M, N, K, b_kmajor=True)
    close(c, ref64(a) @ ref64(b), dtype, "gemm split-K uneven")


def case_gemm_fuzz(dev, cases=150, seed=1):
    """random shapes / layouts / epilogue terms of xclip_gemm against fp32 torch: interior and ragged tiles, split-K slabs, the residual
    form, alpha -- the paths whose hardware-only store hazards (DESIGN_APPENDIX.md section 6d) neither the emulator nor a fixed shape list shows"""
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    for _ in range(cases):
        lay = ["nt", "nn", "tn"][ri(0, 2)]
        M = 8 * ri(16, 200) if ri(0, 3) else 256 * ri(1, 6)
        N = 8 * ri(16, 200) if ri(0, 3) else 256 * ri(1, 6)
        K = 64 * ri(1, 40) if lay != "tn" else 64 * ri(4, 300)
        res = lay == "nt" and ri(0, 2) == 0
        alpha = [1.0, 0.5, 0.125][ri(0, 2)] if not res else 1.0
        ak, bk = lay[0] == "t", lay[1] == "n"
        a = torch.randn((K, M) if ak else (M, K), generator=g).to(torch.bfloat16).to(dev)
        b = torch.randn((K, N) if bk else (N, K), generator=g).to(torch.bfloat16).to(dev)
        r = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev) if res else None
        got = ops.gemm(a, b, M, N, K, ak, bk, alpha=alpha, residual=r).float()
        want = alpha * ((a.float().t() if ak else a.float()) @ (b.float() if bk else b.float().t()))
        if res:
            want = want + r.float()
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert bool(torch.isfinite(got).all()) and err <= scale * 2.0 ** -7, f"gemm {lay} {M}x{N}x{K} res={res} alpha={alpha}: {err:.3e} vs {scale:.3e}"


def case_filip_fused(dev, bx, nt, by, ni, d, seed=61, chunks=1):
    """the FILIP forward with its reductions inside the token-similarity GEMM (filip5.h, x_clip.py:797-811) against an fp64 evaluation of
    the same bf16 latents: t2i / i2t to the bf16 ulp of the scores they average, the arg-max maps up to ties within that ulp; and against
    the chunked form (materialised similarities + filip_reduce) whose t2i / i2t it must reproduce to the same bar"""
    dtype = torch.bfloat16
    X = O.l2_normalize(rnd((bx, nt, d), torch.float32, seed)).to(dtype)
    Y = O.l2_normalize(rnd((by, ni, d), torch.float32, seed + 1)).to(dtype)
    g = torch.Generator().manual_seed(seed + 2)
    mask = torch.ones(bx, nt, dtype=torch.bool)
    for x in range(bx):                                          # ragged text lengths, one text with a hole, one with a single token
        L = nt if x == 0 else int(torch.randint(1, nt + 1, (1,), generator=g))
        mask[x, L:] = False
    if bx > 2:
        mask[2, 1] = False
    if bx > 1:
        mask[1, 1:] = False
    assert ops.filip_fused_ok(nt, ni, d, dtype)
    tau = torch.tensor([0.37], dtype=torch.float32)
    temp = math.exp(0.37)
    t2i = torch.full((bx, by), float("nan"), dtype=torch.float32, device=dev)
    i2t = torch.full((bx, by), float("nan"), dtype=torch.float32, device=dev)
    kmax = torch.full((bx, nt, by), -1, dtype=torch.int16, device=dev)
    tmax = torch.full((bx, by, ni), -1, dtype=torch.int16, device=dev)
    cnt = torch.zeros(bx, dtype=torch.float32, device=dev)
    yc = (by + chunks - 1) // chunks
    need = ops.filip_fused_workspace_bytes(bx, nt, yc, ni)
    guard = 1 << 16                                              # canary behind the workspace: a partial written past its end shows here
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
    ws = buf[:need]
    m8 = mask.to(torch.uint8).to(dev)
    for y0 in range(0, by, yc):
        ops.filip_fused_fwd(X.to(dev), m8, Y[y0: y0 + yc].contiguous().to(dev), tau.to(dev), t2i, i2t, kmax, tmax, cnt, ws, y0)
    assert bool((buf[need:] == 0xA5).all()), "the fused FILIP forward wrote past its workspace"
    S = temp * torch.einsum("xtd,yid->xyti", ref64(X), ref64(Y))                     # [bx, by, nt, ni]
    w = mask.double()
    rowmax, rowarg = S.max(dim=-1)                                                    # [bx, by, nt]
    t2i_r = (rowmax * w[:, None, :]).sum(-1) / w.sum(-1).clamp_min(1e-6)[:, None]
    Sm = S.masked_fill(~mask[:, None, :, None], -float("inf"))
    colmax, colarg = Sm.max(dim=2)                                                    # [bx, by, ni]
    i2t_r = colmax.mean(-1)
    ulp = temp * 2.0 ** -8                                                            # a bf16 ulp of a score of magnitude <= 1
    assert float((t2i.double().cpu() - t2i_r).abs().max()) <= 0.75 * ulp, float((t2i.double().cpu() - t2i_r).abs().max())
    assert float((i2t.double().cpu() - i2t_r).abs().max()) <= 0.75 * ulp, float((i2t.double().cpu() - i2t_r).abs().max())
    assert torch.equal(cnt.cpu(), mask.sum(-1).float())
    # arg-max maps: the chosen position's score is within a bf16 ulp of the true maximum (ties under rounding may pick a neighbour)
    km = kmax.cpu().long().permute(0, 2, 1)                                           # [bx, by, nt]
    assert int(km.min()) >= 0 and int(km.max()) < ni
    got = S.gather(-1, km[..., None]).squeeze(-1)
    live = mask[:, None, :].expand_as(got)
    assert float(((rowmax - got) * live).max()) <= ulp, float(((rowmax - got) * live).max())
    exact = float(((km == rowarg) | ~live).double().mean())
    tm = tmax.cpu().long()                                                            # [bx, by, ni]
    assert int(tm.min()) >= 0 and int(tm.max()) < nt
    assert bool(mask.gather(1, tm.reshape(bx, -1)).all()), "a padding token was chosen as arg-max"
    got = S.gather(2, tm[:, :, None, :]).squeeze(2)
    assert float((colmax - got).max()) <= ulp, float((colmax - got).max())
    _record("filip fused t2i", dtype, float((t2i.double().cpu() - t2i_r).abs().max()) / ulp, 0.75, "bf16 ulp of a score")
    _record("filip fused i2t", dtype, float((i2t.double().cpu() - i2t_r).abs().max()) / ulp, 0.75, "bf16 ulp of a score")
    if ni > 256 or (by * ni) % 8 != 0:                             # the chunked form holds at most 256 image tokens / whole 16-byte chunks
        return exact
    # the chunked form on the same operands
    S16 = ops.gemm(X.to(dev).view(bx * nt, d), Y.to(dev).view(by * ni, d), bx * nt, by * ni, d)
    t2i_c, i2t_c = torch.empty_like(t2i), torch.empty_like(i2t)
    kmax_c, tmax_c, cnt_c = torch.empty_like(kmax), torch.empty_like(tmax), torch.zeros_like(cnt)
    ops.filip_reduce(S16, m8, tau.to(dev), t2i_c, i2t_c, kmax_c, tmax_c, cnt_c, nt, ni, by, 0)
    assert float((t2i - t2i_c).abs().max()) <= 0.75 * ulp and float((i2t - i2t_c).abs().max()) <= 0.75 * ulp
    return exact


def case_dropout(dev, dtype, n=4096 + 8 * 37, p=0.3, seed=0x1234567890ABCDEF):
    """the feed-forward dropout kernel (x_clip.py:193-194): element i kept iff the stateless hash of (seed, i) says so -- compared with
    the numpy rebuild of that hash; kept fraction near 1 - p; the same call on a gradient is the backward; in place"""
    x = rnd((n,), dtype, 71)
    y = ops.dropout(x.to(dev), p, seed)
    keep = O.dropout_keep(seed, n, p)
    want = ref64(x) * keep.double() / (1.0 - float(np.float32(p)))
    close(y, want, dtype, "dropout")
    assert abs(float(keep.double().mean()) - (1 - p)) < 0.03
    z = x.to(dev).clone()
    ops.dropout(z, p, seed, out=z)
    assert torch.equal(z, y)
    assert torch.equal(ops.dropout(x.to(dev), 0.0, seed), x.to(dev))


# ---- the chunked FILIP head (filip.h) and the inference-return products (gemm.h batched, rows.h rowdot), kernel by kernel -----------------
def _roundup(n, m):
    return (n + m - 1) // m * m


def filip_mask(bx, nt, seed=63):
    """text 0 full; ragged lengths for the rest; text 1 a single token; text 2 (if there is one) with a hole at position 1"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones(bx, nt, dtype=torch.bool)
    for x in range(1, bx):
        mask[x, int(torch.randint(min(3, nt), nt + 1, (1,), generator=g)):] = False
    if bx > 2:
        mask[2, 1] = False
    if bx > 1:
        mask[1, 1:] = False
    return mask


def filip_route_ref(mask, g1, g2, kmax, tmax, cnt, temp, ni, yc, y0, width):
    """include/xclip.h: P[(x,t),(y,k)] = temp (g1[x,y0+y] w[x,t] / cnt[x] [k == kmax[x,t,y0+y]] + g2[x,y0+y] / ni [t == tmax[x,y0+y,k]]) in fp64,
    zero in the padding columns [yc ni, width) -> (P [bx nt, width], how many elements carry BOTH families)"""
    bx, nt = mask.shape
    w = mask.double()
    ys = slice(y0, y0 + yc)
    assert bool(mask.gather(1, tmax.long().reshape(bx, -1)).all()), "tmax names a padding token: not a map xclip_filip_reduce can produce"
    hit1 = kmax[:, :, ys].long()[..., None] == torch.arange(ni)                          # [bx, nt, yc, ni]
    hit2 = tmax[:, ys].long()[:, None] == torch.arange(nt)[None, :, None, None]          # [bx, nt, yc, ni]
    a1 = g1[:, ys].double()[:, None, :, None] * (w / cnt.double()[:, None])[:, :, None, None]
    a2 = g2[:, ys].double()[:, None, :, None] / ni
    P = temp * (a1 * hit1 + a2 * hit2)
    out = torch.zeros(bx * nt, width, dtype=torch.float64)
    out[:, : yc * ni] = P.reshape(bx * nt, yc * ni)
    return out, int((hit1 & hit2 & mask[:, :, None, None]).sum())


def filip_route_check(dev, dtype, mask, g1, g2, maps_dev, maps_ref, ni, yc, y0, ldp_extra, name):
    """one xclip_filip_route call on the maps `maps_dev` = (kmax, tmax, cnt) against the header's formula evaluated on `maps_ref`: exact zeros
    wherever the formula is zero (padding rows, padding columns up to the width of P, unselected elements), one rounding elsewhere, and nothing
    written outside P -- P is a view [:bx nt, :ldp] of a NaN-filled [bx nt + 2, ldp + 16] buffer"""
    bx, nt = mask.shape
    v = ops.vec(dtype)
    ldp = _roundup(yc * ni, v) + ldp_extra
    tau = torch.tensor([0.37], dtype=torch.float32)
    full = torch.full((bx * nt + 2, ldp + 16), float("nan"), dtype=dtype, device=dev)
    P = full[: bx * nt, :ldp]
    ops.filip_route(P, mask.to(torch.uint8).to(dev), tau.to(dev), g1.to(dev), g2.to(dev), *maps_dev, nt, ni, yc, y0)
    ref, both = filip_route_ref(mask, g1, g2, *maps_ref, math.exp(float(tau)), ni, yc, y0, ldp)
    assert both > 0, "no element where the two families add"
    got = full.cpu()
    assert bool(torch.isnan(got[bx * nt:].float()).all()), f"{name}: the rows behind P were written"
    assert bool(torch.isnan(got[:, ldp:].float()).all()), f"{name}: the columns behind P's width were written"
    got = got[: bx * nt, :ldp].double()
    zero = ref == 0
    assert bool((got[zero] == 0).all()), f"{name}: {int((got[zero] != 0).sum())} elements that must be exactly zero are not (first: {(zero & (got != 0)).nonzero()[:4].tolist()})"
    assert int((~zero).sum()) > 0
    close(got, ref, dtype, name)
    return both


def case_filip_route(dev, dtype, bx, nt, ni, yc, y0, ytotal, ldp_extra):
    """filip.h filip_route_kernel on inputs made directly (no forward pass): kmax random in [0, ni) -- also in the rows of padding tokens, which
    the row-coalesced reduction never writes and the route kernel must not use; tmax random among the REAL tokens of its text (a subset of
    [0, nt): the header's second family carries no w[x, t] because xclip_filip_reduce takes tmax over real tokens only); elements where both
    families hit are planted at the first and last column, on both sides of the first slice boundary, and in every text"""
    v = ops.vec(dtype)
    g = torch.Generator().manual_seed(6100 + ni * 7 + yc + y0)
    mask = filip_mask(bx, nt)
    cnt = mask.sum(-1).float()
    kmax = torch.randint(0, ni, (bx, nt, ytotal), generator=g).to(torch.int16)
    tmax = torch.empty(bx, ytotal, ni, dtype=torch.int16)
    ncols = yc * ni
    plant = sorted({0, ncols - 1, ncols // 2} | ({256 * v - 1, 256 * v} if 256 * v < ncols else set()))
    for x in range(bx):
        real = mask[x].nonzero().flatten()
        tmax[x] = real[torch.randint(0, real.numel(), (ytotal, ni), generator=g)].to(torch.int16)
        for j, c in enumerate(plant):
            t, y, k = int(real[(real.numel() - 1 - j) % real.numel()]), c // ni, c % ni
            kmax[x, t, y0 + y] = k
            tmax[x, y0 + y, k] = t
    g1 = torch.randn(bx, ytotal, generator=g)
    g2 = torch.randn(bx, ytotal, generator=g)
    maps = (kmax, tmax, cnt)
    return filip_route_check(dev, dtype, mask, g1, g2, tuple(m.to(dev) for m in maps), maps, ni, yc, y0, ldp_extra, "filip route P")


def case_filip_reduce(dev, dtype, bx, nt, ni, by, chunks, lds_extra, chain=False):
    """filip.h filip_reduce_rows_kernel (ni >= the 16-byte chunk) / filip_reduce_kernel (below it) on a similarity matrix made directly, ties
    everywhere: values on the bf16 grid in both storage types (distinct values stay distinct and equal ones equal under the multiplication by
    temp), every other row quantised to 33 levels, one constant row, one constant column.  One call per chunk of ceil(by / chunks) images,
    each from a buffer of its own whose columns behind the chunk hold +1e30.  The arg-max maps are compared EXACTLY with numpy's
    first-occurrence arg-max of the fp64 matrix.  chain: the kernel's own maps then go through xclip_filip_route, against the header's formula
    on the REFERENCE maps"""
    v = ops.vec(dtype)
    g = torch.Generator().manual_seed(6200 + ni * 5 + by)
    mask = filip_mask(bx, nt)
    S = torch.randn(bx * nt, by * ni, generator=g).to(torch.bfloat16).float()
    S[::2] = (S[::2] * 4).round().clamp(-16, 16) / 4
    S[:, ni + min(3, ni - 1)] = 6.0                                  # a constant column at the top: every token ties in it
    S[nt + 0] = 6.0                                                  # a constant row (text 1's only real token): every k ties, in every image
    S[2] = -6.0                                                      # and one of text 0's at the bottom
    S = S.to(dtype)
    tau = torch.tensor([0.37], dtype=torch.float32)
    temp = math.exp(float(tau))
    nan = float("nan")
    t2i = torch.full((bx, by), nan, dtype=torch.float32, device=dev)
    i2t = torch.full((bx, by), nan, dtype=torch.float32, device=dev)
    kmax = torch.full((bx, nt, by), -1, dtype=torch.int16, device=dev)
    tmax = torch.full((bx, by, ni), -1, dtype=torch.int16, device=dev)
    cnt = torch.full((bx,), -1.0, dtype=torch.float32, device=dev)
    m8 = mask.to(torch.uint8).to(dev)
    yc = (by + chunks - 1) // chunks
    for y0 in range(0, by, yc):
        ycc = min(yc, by - y0)
        buf = torch.full((bx * nt, _roundup(ycc * ni, v) + lds_extra), 1e30, dtype=dtype)
        buf[:, : ycc * ni] = S[:, y0 * ni: (y0 + ycc) * ni]
        ops.filip_reduce(buf.to(dev), m8, tau.to(dev), t2i, i2t, kmax, tmax, cnt, nt, ni, ycc, y0)
    S4 = ref64(S).view(bx, nt, by, ni)
    kmax_r = torch.from_numpy(np.argmax(S4.numpy(), axis=3))                            # [bx, nt, by], first occurrence
    Sm = S4.masked_fill(~mask[:, :, None, None], -float("inf"))
    tmax_r = torch.from_numpy(np.argmax(Sm.numpy(), axis=1))                            # [bx, by, ni], first occurrence among the real tokens
    w = mask.double()
    t2i_r = (temp * S4.amax(3) * w[:, :, None]).sum(1) / w.sum(1).clamp_min(1e-6)[:, None]
    i2t_r = (temp * Sm.amax(1)).mean(-1)
    km, tm = kmax.cpu().long(), tmax.cpu().long()
    live = mask[:, :, None].expand_as(km)
    assert int((km[live] == -1).sum()) == 0 and int((tm == -1).sum()) == 0, "an arg-max entry was never written"
    assert torch.equal(km[live], kmax_r[live]), f"kmax differs from the first-occurrence arg-max at {int((km != kmax_r)[live].sum())} real (token, image) pairs"
    assert bool(mask.gather(1, tm.clamp(0, nt - 1).reshape(bx, -1)).all()), "tmax names a padding token"
    assert torch.equal(tm, tmax_r), f"tmax differs from the first-occurrence arg-max over the real tokens at {int((tm != tmax_r).sum())} columns"
    assert torch.equal(cnt.cpu(), mask.sum(-1).float())
    close(t2i, t2i_r, torch.float32, "filip reduce t2i" + (" <- bf16" if dtype == torch.bfloat16 else ""))
    close(i2t, i2t_r, torch.float32, "filip reduce i2t" + (" <- bf16" if dtype == torch.bfloat16 else ""))
    if chain:
        g1 = torch.randn(bx, by, generator=g)
        g2 = torch.randn(bx, by, generator=g)
        kmax_ref = kmax_r.to(torch.int16)
        for y0 in range(0, by, yc):
            filip_route_check(dev, dtype, mask, g1, g2, (kmax, tmax, cnt), (kmax_ref, tmax_r.to(torch.int16), mask.sum(-1).float()), ni,
                              min(yc, by - y0), y0, 0, "filip reduce -> route P")


def case_rowlse_rowgrad(dev, rows, cols, diag_off, dcl, lds_extra, spread):
    """filip.h rowlse_kernel / rowgrad_kernel against the two lines of include/xclip.h in fp64, rows whose diagonal column r + diag_off lies
    outside [0, cols) included (no positive term, nothing left out).  S is a view of a buffer whose extra columns hold +1e30, G a view of a
    NaN-filled buffer four columns wider; both accumulators start non-zero (the contract is +=).  A row that sums nothing (cols = 1, dcl,
    row 0) has lse = log(1e-20) (filip.h: `l > 0 ? m + logf(l) : logf(1e-20f)`; the header's sum is empty there) and G = -gmul coef at its
    diagonal.  rowgrad is given the lse rowlse produced -- its input -- and the reference G is formed from those same fp32 values; fast_exp
    (__expf: exp2 of x log2(e), an argument error of 2^-24 |x| log2(e)) stays below 1e-7 of the largest element for any x > -88, so the wide
    spread needs no wider bar.  loss / dtau increments: sums through float atomics in arbitrary order, held to the fp32 bar of the sum of
    the absolute values of their terms"""
    g = torch.Generator().manual_seed(6300 + rows + cols)
    Sb = torch.full((rows, cols + lds_extra), 1e30, dtype=torch.float32)
    Sb[:, :cols] = torch.randn(rows, cols, generator=g) * spread
    coef, gmul, loss0, dtau0 = 0.5 / rows, 0.7, 0.5, -0.25
    loss = torch.full((1,), loss0, dtype=torch.float32, device=dev)
    dtau = torch.full((1,), dtau0, dtype=torch.float32, device=dev)
    Sd = Sb.to(dev)[:, :cols]
    lse = ops.rowlse(Sd, diag_off, dcl, coef, loss)
    Gb = torch.full((rows, cols + 4), float("nan"), dtype=torch.float32, device=dev)
    G = ops.rowgrad(Sd, lse, diag_off, dcl, coef, torch.tensor([gmul], dtype=torch.float32).to(dev), dtau, out=Gb[:, :cols])
    assert bool(torch.isnan(Gb[:, cols:]).all()), "rowgrad wrote behind its columns"
    S = ref64(Sb[:, :cols])
    r = torch.arange(rows)
    valid = (r + diag_off >= 0) & (r + diag_off < cols)
    diag = torch.zeros(rows, cols, dtype=torch.bool)
    diag[r[valid], (r + diag_off)[valid]] = True
    lse_r = torch.logsumexp(S.masked_fill(diag, -float("inf")) if dcl else S, 1)
    empty = torch.isinf(lse_r)
    assert int(empty.sum()) == (1 if (dcl and cols == 1 and diag_off == 0) else 0)
    lse_r[empty] = math.log(1e-20)
    tag = f" (spread {spread})"
    close(lse, lse_r, torch.float32, "rowlse lse" + tag)
    pos = torch.zeros(rows, dtype=torch.float64)
    pos[valid] = S[diag]
    terms = coef * (lse_r - pos)
    got = loss.cpu().double() - loss0
    assert float(got.abs()) > 0 or float(terms.abs().sum()) == 0
    close(got, terms.sum().reshape(1), torch.float32, "rowlse loss increment" + tag, scale=float(terms.abs().sum()))
    lq = lse.cpu().double()
    Gr = gmul * coef * ((S - lq[:, None]).exp() * ((~diag).double() if dcl else 1.0) - diag.double())
    close(G, Gr, torch.float32, "rowgrad G" + tag, scale=abs(gmul * coef))
    got = dtau.cpu().double() - dtau0
    close(got, (Gr * S).sum().reshape(1), torch.float32, "rowgrad dtau increment" + tag, scale=float((Gr * S).abs().sum()))
    assert float(loss.cpu()) != float(terms.sum().float()) and float(dtau.cpu()) != float((Gr * S).sum().float()), "an accumulator was overwritten, not added to"


def _strided_operand(dtype, B, rows, cols, ld, gap, seed, zero_to=None):
    """a [B, rows, cols] view (row stride ld, problem stride rows ld + gap) into a NaN-filled buffer with NaN in front of problem 0, behind
    problem B - 1, between the problems and between a row's `cols` elements and ld -- except columns [cols, zero_to), which hold zeros"""
    v = ops.vec(dtype)
    stride, front = rows * ld + gap, 2 * v
    buf = torch.full((front + B * stride + 2 * v,), float("nan"), dtype=dtype)
    view = torch.as_strided(buf, (B, rows, cols), (stride, ld, 1), front)
    view.copy_(rnd((B, rows, cols), dtype, seed))
    if zero_to is not None and zero_to > cols:
        torch.as_strided(buf, (B, rows, zero_to - cols), (stride, ld, 1), front + cols).zero_()
    return buf, (lambda b: torch.as_strided(b, (B, rows, cols), (stride, ld, 1), front))


def case_bmm(dev, dtype, B, M, N, K, layout, alpha=1.0):
    """gemm.h gemm_kernel over blockIdx.z (xclip_gemm_batched) against a per-problem fp64 product.  Asymmetric operands, each a view into a
    NaN-filled buffer.  The pad contract of include/xclip.h, both halves: a NORMAL operand's columns [K, K rounded up to the chunk) hold zeros
    (load_normal reads the straddling chunk whole), NaN behind them up to the leading dimension; a K-MAJOR operand has NaN in everything
    behind its row K - 1 (the gap to the next problem: load_kmajor masks by contraction row) and behind its M (or N) columns up to the
    leading dimension (columns [M, M rounded up) are read, and reach only output rows that are never stored)"""
    v = ops.vec(dtype)
    a_k, b_k = layout == "tn", layout in ("nn", "tn")
    Kp = _roundup(K, v)
    if a_k:
        abuf, aview = _strided_operand(dtype, B, K, M, _roundup(M, v) + v, 2 * (_roundup(M, v) + v), 171)
    else:
        abuf, aview = _strided_operand(dtype, B, M, K, Kp + v, 2 * v, 171, zero_to=Kp)
    if b_k:
        bbuf, bview = _strided_operand(dtype, B, K, N, N + v, 2 * (N + v), 172)
    else:
        bbuf, bview = _strided_operand(dtype, B, N, K, Kp + v, 2 * v, 172, zero_to=Kp)
    c = ops.bmm(aview(abuf.to(dev)), bview(bbuf.to(dev)), M, N, K, a_k, b_k, alpha)
    A, Bm = ref64(aview(abuf)), ref64(bview(bbuf))
    r = alpha * ((A.transpose(1, 2) if a_k else A) @ (Bm if b_k else Bm.transpose(1, 2)))
    assert tuple(c.shape) == (B, M, N)
    close(c, r, dtype, f"bmm {layout}" + ("" if alpha == 1.0 else f" alpha {alpha}"))


def case_bmm_rejects_tt(dev, dtype):
    """(A k-major, B normal) is the one layout xclip_gemm_batched does not carry: an error, not a wrong product"""
    import pytest
    a, b = rnd((2, 16, 8), dtype, 173).to(dev), rnd((2, 8, 16), dtype, 174).to(dev)
    with pytest.raises(RuntimeError, match="xclip_gemm_batched"):
        ops.bmm(a, b, 8, 8, 16, True, False)


def case_bmm_many(dev, B=65536 + 2, M=8, N=8, K=8):
    """more problems than one launch carries (ops.bmm splits at 65535): every problem against fp64"""
    a, b = rnd((B, M, K), torch.float32, 175), rnd((B, N, K), torch.float32, 176)
    c = ops.bmm(a.to(dev), b.to(dev), M, N, K)
    close(c, ref64(a) @ ref64(b).transpose(1, 2), torch.float32, "bmm nt across the launch split")


def case_rowdot(dev, dtype, rows):
    """rows.h rowdot_kernel at every chunks-per-lane dispatch (bf16 rows of 8 .. 4096 elements: 1, 1, 1, 2, 4, 8 chunks per lane; fp32 rows of
    4 .. 4096: 1, 1, 1, 2, 4, 8, 16), contiguous and as row-strided views into NaN-filled buffers (ops.rowdot reads such views in place),
    against the fp64 dot product; each element to one rounding of a sum whose terms add up to max_r sum |a b|"""
    v = ops.vec(dtype)
    dims = (8, 24, 512, 1024, 2048, 4096) if dtype == torch.bfloat16 else (4, 12, 256, 512, 1024, 2048, 4096)
    for dim in dims:
        a, b = rnd((rows, dim), dtype, 181), rnd((rows, dim), dtype, 182)
        want = (ref64(a) * ref64(b)).sum(-1)
        scale = float((ref64(a) * ref64(b)).abs().sum(-1).max())
        close(ops.rowdot(a.to(dev), b.to(dev)), want, dtype, "rowdot", scale=scale)
        ab = torch.full((rows, dim + v), float("nan"), dtype=dtype)
        bb = torch.full((rows, dim + 3 * v), float("nan"), dtype=dtype)
        ab[:, :dim], bb[:, :dim] = a, b
        close(ops.rowdot(ab.to(dev)[:, :dim], bb.to(dev)[:, :dim]), want, dtype, "rowdot strided", scale=scale)


def _cast_inputs():
    """fp32 bit patterns around every rounding decision of the bf16 conversion"""
    bits = [0x00000000, 0x80000000,
            0x3F808000, 0x3F808001, 0x3F807FFF,                      # halfway above an EVEN bf16 (ties to it), just above, just below
            0x3F818000, 0x3F818001, 0x3F817FFF,                      # halfway above an ODD bf16 (ties away from it), just above, just below
            0xBF808000, 0xBF808001, 0xBF807FFF, 0xBF818000, 0xBF818001, 0xBF817FFF,
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,          # the largest finite bf16, just below its halfway point, the halfway point, FLT_MAX
            0xFF7F0000, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF,
            0x7F800000, 0xFF800000, 0x7FC00000]                      # +-inf, NaN
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def case_cast_and_add(dev, dtype):
    """tokens.h cast_from_f32_kernel and add_rows_kernel, bit for bit against the CPU's fp32 arithmetic and round-to-nearest-even conversion, at
    counts that are no multiple of anything (1, 7, 4096 + 37)"""
    ints = torch.int16 if dtype == torch.bfloat16 else torch.int32
    special = _cast_inputs()
    for count in (1, 7, 4096 + 37):
        for scale in (1.0, 0.125, 1.0 / 3.0):
            src = torch.cat([special, rnd((4096 + 37,), torch.float32, 191, 3.0)])
            src = src[2:3] if count == 1 else (src[2: 2 + count] if count == 7 else src[:count])
            if count > 7:
                assert bool(torch.isnan(src).any()) and bool(torch.isinf(src).any())
            got = ops.cast_from_f32(src.to(dev).contiguous(), dtype, scale).cpu()
            want = (src * torch.tensor(scale, dtype=torch.float32)).to(dtype)
            nan = torch.isnan(want.float())
            assert torch.equal(torch.isnan(got.float()), nan), "NaN must map to NaN, and nothing else may"
            assert torch.equal(got.view(ints)[~nan], want.view(ints)[~nan]), (count, scale, int((got.view(ints) != want.view(ints))[~nan].sum()))
        a, b = rnd((count,), dtype, 192, 3.0), rnd((count,), dtype, 193, 3.0)
        got = ops.add_rows(a.to(dev), b.to(dev)).cpu()
        assert torch.equal(got.view(ints), (a.float() + b.float()).to(dtype).view(ints)), count


# The parameter sets of the cases above, shared by the emulator and the GPU suite (the shapes are the smallest that reach each branch;
# nothing here gets larger on the GPU).  Each id names the branch its set exists for.
BF, FP = torch.bfloat16, torch.float32
FILIP_ROUTE_SETS = {   # id: (dtype, bx, nt, ni, yc, y0, ytotal, ldp_extra)
    "bf16-2450cols-two-slices-boundary-inside-an-image-odd-ni-both-tbase-parities": (BF, 3, 12, 49, 50, 0, 50, 0),
    "bf16-chunk-in-mid-batch-y0-3-tbase-parity-moves-with-x-and-y0": (BF, 3, 12, 49, 50, 3, 57, 0),
    "bf16-last-partial-chunk-in-the-full-row-stride-trailing-padding-and-a-padding-only-slice": (BF, 3, 12, 49, 7, 50, 57, 2456 - 344),
    "bf16-even-ni-64-wide-tmax-load-always-chunks-never-straddle-images": (BF, 3, 9, 64, 40, 0, 40, 0),
    "bf16-ni-3-chunk-spans-3-to-4-images-683-images-kmax-staged-in-batches-of-23-rows": (BF, 2, 50, 3, 700, 0, 700, 0),
    "bf16-third-slice-padding-only-live_slice-false": (BF, 3, 12, 49, 50, 0, 50, 4104 - 2456),
    "fp32-vec-4-1024-column-slices-1170cols-two-slices": (FP, 2, 7, 9, 130, 0, 130, 0),
    "fp32-ni-98-five-images-y0-2": (FP, 3, 12, 98, 5, 2, 9, 0),
}
FILIP_REDUCE_SETS = {  # id: (dtype, bx, nt, ni, by, chunks, lds_extra, chain)
    "bf16-rows-kernel-ni-49-one-chunk-image-split-over-blockIdx.y-then-route": (BF, 3, 12, 49, 12, 1, 0, True),
    "bf16-rows-kernel-ni-49-three-chunks-y0-above-0-chunks-straddle-segments-then-route": (BF, 3, 12, 49, 12, 3, 0, True),
    "bf16-rows-kernel-ni-64-aligned-segments": (BF, 3, 12, 64, 9, 1, 0, False),
    "bf16-rows-kernel-ni-9-chunk-columns-no-whole-number-of-16-byte-chunks": (BF, 3, 12, 9, 5, 2, 0, False),
    "bf16-per-pair-kernel-ni-5-below-the-chunk": (BF, 3, 12, 5, 6, 2, 0, False),
    "fp32-rows-kernel-ni-49-vec-4": (FP, 3, 12, 49, 6, 1, 0, False),
    "fp32-per-pair-kernel-ni-3": (FP, 3, 12, 3, 4, 2, 0, False),
    "bf16-rows-kernel-ni-49-row-stride-8-columns-wider-than-the-chunk": (BF, 3, 12, 49, 12, 3, 8, False),
}
ROWLSE_SETS = {        # id: (rows, cols, diag_off, lds_extra)
    "5x70": (5, 70, 0, 3),
    "7x63-diag-off-2": (7, 63, 2, 0),
    "6x65-diag-off-minus-3-rows-0-to-2-have-no-diagonal": (6, 65, -3, 1),
    "4x1-one-column-dcl-row-0-sums-nothing": (4, 1, 0, 2),
    "3x200-diag-off-190-diagonal-falls-off-the-right-edge": (3, 200, 190, 0),
    "1500x1500-rowgrad-capped-at-8192-work-groups-grid-stride-loop": (1500, 1500, 0, 4),
}
BMM_SETS = {           # id: (layout, M, N, K, alpha)
    "nt-77x104x512-several-k-steps": ("nt", 77, 104, 512, 1.0),
    "nt-257x200x64-three-m-tiles-two-n-tiles": ("nt", 257, 200, 64, 1.0),
    "nn-77x512x98-k-tail-four-n-tiles": ("nn", 77, 512, 98, 1.0),
    "nn-9x64x49-k-below-one-step": ("nn", 9, 64, 49, 1.0),
    "tn-98x512x77-ragged-m-and-k-lda-m-rounded-up": ("tn", 98, 512, 77, 1.0),
    "tn-49x64x9": ("tn", 49, 64, 9, 1.0),
    "nn-77x512x98-alpha-0.5": ("nn", 77, 512, 98, 0.5),
}
