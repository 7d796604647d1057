"""Shared cases of the packed text tower (x_clip_amd.packing, CLIP.pack_text): the varlen attention and packed embedding kernels against
fp64 references, and the public interface end to end.  tests/test_packed_emu.py runs them on the CPU emulator build, tests/test_packed_gpu.py
on an MI355X -- the same cases; the GPU file adds the launches that fill the chip.

Bars: attention out / dqkv within 2 bf16 ulps of the tensor's scale in bf16, 2e-5 / 6e-5 of the scale in fp32 (the bars of
kernel_cases.case_attention), lse within 2e-5 of its scale; end to end fp32 loss 1e-5 and gradients 3e-4 relative, bf16 loss 3e-4 and
gradients 8 % with cosine 0.999."""
import math

import pytest
import torch

import clip_cases as C
import kernel_cases as K
from oracle import clip_oracle as O
from x_clip_amd import CLIP, _lib, ops, text_layout
from x_clip_amd.packing import TextLayout

F32, BF16 = torch.float32, torch.bfloat16
LENS_A = (1, 2, 31, 32, 33, 63, 64, 65, 257)       # the offsets cu[s] fall on no tile or sub-tile boundary
LENS_B = (1, 1, 1, 288)
LENS_LONG = (289, 5)                               # beyond the head-resident limit (A3_MAX_N = 288)
GUARD = 64
# (slot, dim_head): 64-wide slots with a full and a narrow head, a 128-wide slot
WIDTHS = ((64, 64), (64, 24), (128, 80))


def _cu(lens, dev):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    return cu.to(dev)


def _nonzero_randn(shape, g, dtype):
    x = torch.randn(*shape, generator=g).to(dtype)
    return torch.where(x == 0, torch.ones_like(x), x)


def _poison(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def varlen_launch(qkv, dout, cu, max_len, heads, slot, scale):
    """both entry points through the C ABI into NaN-poisoned buffers with GUARD rows behind row R -> (out, lse, dqkv) on the R rows, after
    checking that every guard element kept its poison bit for bit"""
    L = _lib.lib()
    R, dev, dt = qkv.shape[0], qkv.device, qkv.dtype
    inner = heads * slot
    out = _poison((R + GUARD, inner), dt, dev)
    lse = _poison((heads * R + GUARD,), F32, dev)
    dqkv = _poison((R + GUARD, 3 * inner), dt, dev)
    want = [_bits(t).clone() for t in (out[R:], lse[heads * R:], dqkv[R:])]
    code = ops.dtype_code(qkv)
    st = ops._stream(qkv)
    _lib.check(L.xclip_attention_varlen_fwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), R, cu.numel() - 1, heads, slot, max_len,
                                            scale, code, st), "xclip_attention_varlen_fwd")
    _lib.check(L.xclip_attention_varlen_bwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), R,
                                            cu.numel() - 1, heads, slot, max_len, scale, code, st), "xclip_attention_varlen_bwd")
    for name, t, w in zip(("out", "lse", "dqkv"), (out[R:], lse[heads * R:], dqkv[R:]), want):
        assert torch.equal(_bits(t), w), f"varlen attention wrote behind row R of {name}"
    return out[:R], lse[:heads * R].view(heads, R), dqkv[:R]


def varlen_data(lens, heads, slot, dim_head, dtype, dev, seed=0):
    g = torch.Generator().manual_seed(9100 + seed)
    R = sum(lens)
    qkv = _nonzero_randn((R, 3, heads, slot), g, dtype)
    qkv[..., dim_head:] = 0                                     # a head narrower than its slot: zero columns (Transformer.stack_params)
    dout = _nonzero_randn((R, heads * slot), g, dtype)
    return qkv.view(R, 3 * heads * slot).to(dev), dout.to(dev)


def varlen_reference(qkv, dout, lens, heads, slot, scale):
    """kernel_cases.attention_ref_blocked per group of equal-length samples, on their own rows -> (out [R, inner], lse [heads, R], dqkv) fp64"""
    R, w = qkv.shape
    dev = qkv.device
    out = torch.zeros(R, heads * slot, dtype=torch.float64, device=dev)
    lse = torch.zeros(heads, R, dtype=torch.float64, device=dev)
    grad = torch.zeros(R, w, dtype=torch.float64, device=dev)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    for n in sorted(set(lens)):
        rows = torch.cat([torch.arange(starts[s], starts[s] + n) for s in range(len(lens)) if lens[s] == n]).to(dev)
        o, l, gq = K.attention_ref_blocked(qkv[rows].view(-1, n, w), dout[rows].view(-1, n, heads * slot), None, heads, scale, hd=slot)
        out[rows] = o.reshape(-1, heads * slot)
        lse[:, rows] = l.permute(1, 0, 2).reshape(heads, -1)
        grad[rows] = gq.reshape(-1, w)
    return out, lse, grad


def check_varlen(got, want, dtype, tag):
    (out, lse, dqkv), (r_out, r_lse, r_grad) = got, want
    for t in (out, lse, dqkv):
        assert bool(torch.isfinite(t).all()), f"{tag}: a row below R is not finite (never written?)"
    K.close(out, r_out, dtype, f"varlen attn out {tag}", ulps=2.0, unit="scale")
    K.close(lse, r_lse, F32, f"varlen attn lse {tag}")
    K.close(dqkv, r_grad, dtype, f"varlen attn dqkv {tag}", mult=3.0, ulps=2.0, unit="scale")


def case_varlen_attention(dev, dtype, lens, heads, slot, dim_head, seed=0, max_len=None, tag=None):
    """max_len = None: the longest sample's length, as text_layout counts it; larger: the launch sized for a sample the batch does not hold
    (cat_layouts).  `tag` names the check in the parity report (a sweep keeps one line, the worst of its cases); -> (got, want)"""
    qkv, dout = varlen_data(lens, heads, slot, dim_head, dtype, dev, seed)
    scale = dim_head ** -0.5
    got = varlen_launch(qkv, dout, _cu(lens, dev), max(lens) if max_len is None else max_len, heads, slot, scale)
    want = varlen_reference(qkv, dout, lens, heads, slot, scale)
    check_varlen(got, want, dtype, tag or f"lens {lens[:4]}.. h{heads} slot{slot}/{dim_head}")
    return got, want


def case_varlen_equals_dense(dev, dtype, B, n, heads, slot):
    """B samples of one length: the dense kernels without a mask on the same data reshaped to [B, n, ...], within the kernel bars"""
    qkv, dout = varlen_data((n,) * B, heads, slot, slot, dtype, dev, seed=3)
    scale = slot ** -0.5
    out, lse, dqkv = varlen_launch(qkv, dout, _cu((n,) * B, dev), n, heads, slot, scale)
    d_out, d_lse = ops.attention_fwd(qkv.view(B, n, -1), None, heads, scale, False, slot)
    d_dqkv = ops.attention_bwd(qkv.view(B, n, -1), None, d_out, dout.view(B, n, -1), d_lse, heads, scale, False, slot)
    tag = f"== dense B{B} n{n} slot{slot}"
    K.close(out, d_out.view(B * n, -1).double(), dtype, "varlen attn out " + tag, ulps=2.0, unit="scale")
    K.close(lse, d_lse.permute(1, 0, 2).reshape(heads, B * n).double(), F32, "varlen attn lse " + tag)
    K.close(dqkv, d_dqkv.view(B * n, -1).double(), dtype, "varlen attn dqkv " + tag, mult=3.0, ulps=2.0, unit="scale")


EQUAL_BITS_NS = (33, 65, 66, 97)          # one wave with an ordinary tail, a single tail, a two-row tail, three waves past a dip


def case_varlen_equals_dense_bits(dev, n, B=2, heads=3, slot=64):
    """bf16, B samples of one length, max_len = n, no mask: the head-resident packed kernels ARE the dense ones (one body in attention3.h, the
    unit's rows found from cu instead of (sample, n)) -- out, lse and dqkv bit for bit"""
    qkv, dout = varlen_data((n,) * B, heads, slot, slot, BF16, dev, seed=3)
    scale = slot ** -0.5
    out, lse, dqkv = varlen_launch(qkv, dout, _cu((n,) * B, dev), n, heads, slot, scale)
    d_out, d_lse = ops.attention_fwd(qkv.view(B, n, -1), None, heads, scale, False, slot)
    d_dqkv = ops.attention_bwd(qkv.view(B, n, -1), None, d_out, dout.view(B, n, -1), d_lse, heads, scale, False, slot)
    for name, a, b in (("out", out, d_out.view(B * n, -1)), ("lse", lse, d_lse.permute(1, 0, 2).reshape(heads, B * n)),
                       ("dqkv", dqkv, d_dqkv.view(B * n, -1))):
        assert torch.equal(_bits(a), _bits(b.contiguous())), f"{name}: packed and dense differ in bits at n {n}"


def case_varlen_full(dev, dtype=BF16, samples=256, heads=8, slot=64, repeats=3):
    """GPU: >= 1024 (sample, head) units, every head checked against the fp64 reference evaluated on the device, three launches bit-identical"""
    lens = tuple(LENS_A[i % len(LENS_A)] for i in range(samples))
    qkv, dout = varlen_data(lens, heads, slot, slot, dtype, dev, seed=5)
    scale, cu = slot ** -0.5, _cu(lens, dev)
    got = varlen_launch(qkv, dout, cu, max(lens), heads, slot, scale)
    check_varlen(got, varlen_reference(qkv, dout, lens, heads, slot, scale), dtype, f"full {samples} x {heads}")
    for i in range(repeats - 1):
        again = varlen_launch(qkv, dout, cu, max(lens), heads, slot, scale)
        for a, b, name in zip(got, again, ("out", "lse", "dqkv")):
            assert torch.equal(a, b), f"{name} differs between launch 0 and {i + 1}"


# ---- packed embedding ---------------------------------------------------------------------------------------------------------------------
def embed_tokens(B=6, n=9, vocab=50, seed=77):
    """the first six samples are one of each kind; the ones behind them have padded tails of every length"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, vocab, (B, n), generator=g)
    tok[0, 5:] = 0                                              # a padded tail
    if B > 1:
        tok[1] = 0                                              # all padding: the CLS row alone
    if B > 2:
        tok[2, 3] = 0                                           # a hole
    if B > 3:
        tok[3, :4] = 7                                          # a repeated id (and again in another sample)
    if B > 4:
        tok[4, 0] = 7
        tok[4, 6:] = 0
    for r in range(6, B):                                       # (sample 5: full)
        tok[r, 1 + (r * 5) % n:] = 0
    return tok


def _segmented(keys, size, d64):
    """fp64 index_add_ of the rows whose key lies inside the table -> (sum, k 2^-24 sum |terms|: the fp32-summation bound of k terms, as
    cached_cases.case_accumulate derives it -- k roundings of at most half an fp32 ulp of a partial sum that never exceeds sum |terms|)"""
    live = (keys >= 0) & (keys < size)
    dim = d64.shape[1]
    want = torch.zeros(size, dim, dtype=torch.float64).index_add_(0, keys[live], d64[live])
    mag = torch.zeros(size, dim, dtype=torch.float64).index_add_(0, keys[live], d64[live].abs())
    cnt = torch.zeros(size, dtype=torch.float64).index_add_(0, keys[live], torch.ones(int(live.sum()), dtype=torch.float64))
    return want, cnt[:, None] * 2.0 ** -24 * mag


def _within(name, dtype, got, want, bound, factor=1.0):
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    K._record(f"packed embedding {name}", dtype, ratio, factor, "of k 2^-24 sum |terms|, element-wise")
    assert bool((err <= factor * bound).all()), f"packed embedding {name}: worst error / bound {ratio:.3f} (allowed {factor})"


def case_packed_embedding(dev, dtype, B=6, n=9, dim=64, vocab=50, has_pos=True, has_cls=True):
    """forward: the bits of the kept rows of text_embed_fwd, and the bits of E[tok] + P[pos] formed in fp32 and rounded once (cls on the CLS
    rows) -- which does not lean on the dense kernel.  backward: dE, dP, dcls against fp64 within the derived fp32-summation bound, and against
    text_embed_bwd on the dense gradient that is zero on the dropped rows (two fp32 sums of the same terms: twice that bound; at the first
    shape of this case also the 1e-6 of the scale it has always held)"""
    tok = embed_tokens(B, n, vocab)
    if not has_cls and B > 1:
        with pytest.raises(ValueError, match="at least one kept token"):
            text_layout(tok, pad_id=0, has_cls=False)            # sample 1 is all padding: without a CLS row it would own no row at all
        tok[1, 2] = 3
    c = int(has_cls)
    E, P, cls = K.rnd((vocab, dim), dtype, 1), K.rnd((n, dim), dtype, 2) if has_pos else None, K.rnd((dim,), dtype, 3) if has_cls else None
    E_d, P_d, cls_d = E.to(dev), None if P is None else P.to(dev), None if cls is None else cls.to(dev)
    lay = text_layout(tok, pad_id=0, has_cls=has_cls).to(dev)
    keep = (torch.cat([torch.ones(B, 1, dtype=torch.bool), tok != 0], dim=1) if has_cls else tok != 0)
    assert lay.R == int(keep.sum()) and lay.max_len == int(keep.sum(1).max()) and lay.batch == B
    if B > 5:
        assert lay.max_len == n + c                              # sample 5 is full
    if B > 1 and has_cls:
        assert int(lay.cu[2] - lay.cu[1]) == 1
    keep = keep.reshape(-1)
    dense = ops.text_embed_fwd(tok.to(dev), E_d, P_d, cls_d).view(B * (n + c), dim)
    with C.poisoned_empty():
        packed = ops.text_embed_packed_fwd(lay.tok, lay.pos, E_d, P_d, cls_d)
    assert torch.equal(packed, dense[keep.to(dev)]), "packed embedding forward is not bit-equal to the kept rows of text_embed_fwd"
    tk, ps = lay.tok.cpu(), lay.pos.cpu().long()
    want = E.float()[tk]
    if has_pos:
        want = want + P.float()[(ps - c).clamp_min(0)]
    want = want.to(dtype)
    if has_cls:
        want[ps == 0] = cls
        assert bool((ps[lay.cu[:-1].cpu().long()] == 0).all()) and int((ps == 0).sum()) == B
    assert torch.equal(_bits(packed.cpu()), _bits(want)), "packed embedding forward is not E[tok] + P[pos] rounded once"

    d_packed = K.rnd((lay.R, dim), dtype, 4).to(dev)
    d_dense = torch.zeros(B * (n + c), dim, dtype=dtype, device=dev)
    d_dense[keep.to(dev)] = d_packed                             # a dense gradient that is zero on the dropped rows
    st = ops.sort_ids(tok.to(dev).reshape(-1), vocab)
    wE, wP, wc = ops.text_embed_bwd(d_dense.view(B, n + c, dim), tok.to(dev), vocab, has_pos, has_cls, sorted_tokens=st)
    tkey, pkey = lay.keys(vocab, n)
    gE, gP, gc = ops.text_embed_packed_bwd(d_packed, tkey, pkey, lay.cu, vocab, n if has_pos else 0, has_cls)
    assert (gP is None) == (not has_pos) and (gc is None) == (not has_cls) and (wP is None) == (gP is None) and (wc is None) == (gc is None)
    d64 = d_packed.cpu().double()
    refs = {"dE": (gE, wE) + _segmented(tkey.cpu(), vocab, d64)}
    if has_pos:
        refs["dP"] = (gP, wP) + _segmented(pkey.cpu(), n, d64)
    if has_cls:
        first = d64[lay.cu[:-1].cpu().long()]
        refs["dcls"] = (gc, wc, first.sum(0), B * 2.0 ** -24 * first.abs().sum(0))
    tag = f"B{B} dim{dim}" + ("" if has_pos else " no pos") + ("" if has_cls else " no cls")
    for name, (got, dense_got, ref, bound) in refs.items():
        assert got.dtype == F32 and got.shape == ref.shape, name
        _within(f"{name} vs fp64 {tag}", dtype, got, ref, bound)
        _within(f"{name} vs text_embed_bwd {tag}", dtype, got, dense_got.detach().cpu().double(), bound, factor=2.0)
        if B <= 6:
            s = float(dense_got.abs().max())
            err = float((got - dense_got).abs().max())
            assert err <= 1e-6 * s, f"packed embedding {name}: {err:.3e} against scale {s:.3e}"
    assert float(gE[0].abs().max()) == 0.0                       # the pad id owns no kept row


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
def case_layout(dev):
    tok = embed_tokens()
    a, b = text_layout(tok, pad_id=0), text_layout(tok.to(dev), pad_id=0)
    assert isinstance(a, TextLayout) and a.cu.dtype == torch.int32 and a.pos.dtype == torch.int32 and a.tok.dtype == torch.int64
    assert (a.R, a.max_len) == (b.R, b.max_len) and isinstance(a.R, int) and isinstance(a.max_len, int)
    for f in ("cu", "pos", "tok"):
        assert torch.equal(getattr(a, f), getattr(b, f).cpu()), f
    lens = (tok != 0).sum(1) + 1
    assert torch.equal(a.cu[1:].long(), lens.cumsum(0)) and int(a.cu[0]) == 0
    assert bool((a.pos[a.cu[:-1].long()] == 0).all())            # position 0 = the CLS row, first of every sample
    m = text_layout(tok, mask=tok != 0)
    assert torch.equal(m.pos, a.pos) and torch.equal(m.tok, a.tok)
    s = 2                                                        # the hole at token 3 = position 4 is simply a dropped row
    assert a.pos[a.cu[s]: a.cu[s + 1]].tolist() == [0, 1, 2, 3] + list(range(5, tok.shape[1] + 1))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def padded_text(cfg, text):
    """a padded tail per sample, sample 0 all padding, sample 1 full, sample 2 with a hole"""
    text = text.clone()
    B, n = text.shape
    text = torch.where(text == cfg.text_pad_id, torch.ones_like(text), text)
    for r in range(B):
        text[r, 3 + (r * 5) % (n - 4):] = cfg.text_pad_id
    text[0] = cfg.text_pad_id
    text[1] = torch.where(text[1] == cfg.text_pad_id, torch.full_like(text[1], 5), text[1])
    text[2, 1] = cfg.text_pad_id
    return text


VARIANTS = {
    "infonce": dict(cfg=O.CFG1, aug=(0, 0), sigmoid=False),
    "dcl_multiview": dict(cfg=O.ClipConfig(**dict(O.CFG1.__dict__, decoupled_contrastive_learning=True)), aug=(1, 1), sigmoid=False),
    "sigmoid": dict(cfg=O.CFG1, aug=(0, 0), sigmoid=True),
}


# DESIGN section 7 states the bf16 end-to-end bars (loss 3e-4, gradients 8 % / cosine 0.999) for the dim-512 model; the dim-64 toy CFG1 is held to a
# bf16 loss of 1.4e-3 by the suite's own oracle cases (test_clip_bf16_vs_oracle: "the dim-64 toy model").  So the bf16 oracle cases run a dim-512
# model -- the width of tests/test_clip_gpu.py's MID, cut to one layer per tower, 16 tokens and four patches so that the emulator twin stays short
# -- and the fp32 ones the two-layer CFG1.
WIDE = O.ClipConfig(dim_text=512, dim_image=512, dim_latent=512, num_text_tokens=2000, text_enc_depth=1, text_seq_len=16, text_heads=8,
                    visual_enc_depth=1, visual_image_size=64, visual_patch_size=32, visual_heads=8)


def small_setup(variant, dtype, batch=None, seed=11, wide=False, cfg=None, pad=None):
    """batch 8 by default: every kind of sample (all padding, full, a hole, padded tails of five lengths) at an emulator time of seconds.
    cfg / pad: another model (with the variant's loss) and another padding of its tokens"""
    v = VARIANTS[variant]
    if cfg is not None:
        cfg = O.ClipConfig(**dict(cfg.__dict__, decoupled_contrastive_learning=v["cfg"].decoupled_contrastive_learning))
    else:
        cfg = v["cfg"]
    pad_text = padded_text if pad is None else pad
    if wide:
        cfg = O.ClipConfig(**dict(WIDE.__dict__, decoupled_contrastive_learning=cfg.decoupled_contrastive_learning))
    if batch is None:
        batch = 8
    sd = O.make_state_dict(cfg, seed, F32)
    extra = {}
    if v["sigmoid"]:
        sd = dict(sd, temperature=torch.tensor(math.log(10.0)), logit_bias=torch.tensor(-10.0))
        extra["sigmoid_loss"] = True
    sd = {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items()}
    text, image, aug_t, aug_i = O.make_inputs(cfg, batch, seed + 1, *v["aug"])
    text, aug_t = pad_text(cfg, text), [pad_text(cfg, a.roll(1, 0)) for a in aug_t]
    return cfg, sd, extra, text, image.to(dtype), aug_t, [a.to(dtype) for a in aug_i]


def run_model(dev, dtype, variant, pack, layout_from=None, batch=None, wide=False, cfg=None, pad=None, **ctor):
    cfg, sd, extra, text, image, aug_t, aug_i = small_setup(variant, dtype, batch, wide=wide, cfg=cfg, pad=pad)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **extra, **ctor)
    if pack is not None:
        model.pack_text = pack
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    if layout_from is not None:
        kw["text_layout"] = text_layout(text if layout_from == "cpu" else text.to(dev), pad_id=cfg.text_pad_id)
    loss = model(text.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def oracle(variant, dtype, batch=None, wide=False, cfg=None, pad=None):
    cfg, sd, _, text, image, aug_t, aug_i = small_setup(variant, dtype, batch, wide=wide, cfg=cfg, pad=pad)
    sd64 = {k: (t.double().clone().requires_grad_(True) if t.is_floating_point() else t) for k, t in sd.items()}
    with O.layer_norm_eps(1e-5 if dtype == F32 else 1e-3):
        if VARIANTS[variant]["sigmoid"]:
            import sigloss_cases as S
            lat = O.clip_forward({k: v for k, v in sd64.items() if k != "logit_bias"}, cfg, text, image.double(), return_latents=True)
            loss = S.dense_loss(lat[0][None], lat[1][None], sd64["temperature"], sd64["logit_bias"], 1.0, 0.0)
        else:
            loss = O.clip_forward(sd64, cfg, text, image.double(), aug_t, [a.double() for a in aug_i])
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd64.items() if v.is_floating_point()}


_ORACLE = {}


def case_vs_oracle(dev, dtype, variant, cfg=None, pad=None):
    """pack_text = True against the fp64 oracle on the same (dtype-rounded) parameters and padded tokens; the pad id's embedding gradient is exactly zero.
    bf16 runs the dim-512 model the bf16 bars are stated for (WIDE above), fp32 the two-layer CFG1 -- or the model `cfg` with its tokens padded
    by `pad` (packed_sweep_cases.case_vs_oracle_mid)"""
    wide = dtype != F32 and cfg is None
    setup = dict(wide=wide, cfg=cfg, pad=pad)
    key = (variant, dtype, repr(cfg), getattr(pad, "__name__", None))
    if key not in _ORACLE:
        _ORACLE[key] = oracle(variant, dtype, **setup)
    ref_loss, ref_grads = _ORACLE[key]
    model, loss, grads = run_model(dev, dtype, variant, True, **setup)
    fp32 = dtype == F32
    err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    print(f"packed {variant} {dtype}: loss err {err:.2e}")
    assert err < (1e-5 if fp32 else 3e-4), (float(loss), ref_loss)
    for k, g in grads.items():
        rg = ref_grads.get(k)
        if rg is None or float(rg.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        g = g.double().cpu()
        assert bool(torch.isfinite(g).all()), k
        rel = float((g - rg).norm() / rg.norm())
        cos = float((g * rg).sum() / (g.norm() * rg.norm()))
        print(f"packed {variant} {dtype} {k}: rel {rel:.2e} cos {cos:.6f}")
        assert (rel < 3e-4) if fp32 else (rel < 0.08 and cos > 0.999), (k, rel, cos)
    pad_row = grads["text_transformer.token_emb.weight"][(cfg or O.CFG1).text_pad_id]
    assert float(pad_row.abs().max()) == 0.0, "the pad id's embedding row received a gradient"


EQ_BATCH = 6          # the run-against-run equality cases hold at any batch: the smallest with every kind of sample (emulator time)


def case_checkpoint(dev, dtype, bitwise):
    _, la, ga = run_model(dev, dtype, "infonce", True, batch=EQ_BATCH)
    _, lb, gb = run_model(dev, dtype, "infonce", True, batch=EQ_BATCH, checkpoint_during_training=True)
    assert torch.equal(la, lb)
    _same_grads(ga, gb, bitwise, "checkpoint")


def _atomic_sum(k):
    """gradients the backward accumulates with float atomics (LayerNorm gains, embedding tables, the CLS token, biases, the temperature): their
    summation order differs between two runs of the SAME launches, on the MI355X and -- its work-groups run on host threads -- on the emulator too
    (test_checkpointing_is_bit_identical[fp32] of the emulator file passed and failed on `temperature` / `cls_token` in consecutive runs before this
    rule).  tests/test_clip_gpu.py test_checkpointing_is_bit_identical holds exactly these to 1e-4 / 1e-6 and everything else to its bits; so do we."""
    return "token_emb" in k or k.endswith(".g") or "pos_emb" in k or "cls_token" in k or k.endswith("bias") or k == "temperature"


def _same_grads(g0, g1, bitwise, tag):
    for k in g0:
        if g0[k] is None or g1[k] is None:
            assert g0[k] is None and g1[k] is None, (tag, k)
        elif _atomic_sum(k):
            torch.testing.assert_close(g0[k], g1[k], rtol=1e-4, atol=1e-6)
        else:
            assert torch.equal(g0[k], g1[k]), (tag, k)


def case_layout_passed_in(dev, dtype, bitwise=True, variants=("infonce", "dcl_multiview")):
    """a layout built from CPU tokens, one built from device tokens and the implicit one: the same bits (also with augmented texts)"""
    for variant in variants:
        _, l0, g0 = run_model(dev, dtype, variant, True, batch=EQ_BATCH)
        for src in ("cpu", "dev"):
            _, l1, g1 = run_model(dev, dtype, variant, True, layout_from=src, batch=EQ_BATCH)
            assert torch.equal(l0, l1), (variant, src)
            _same_grads(g0, g1, bitwise, (variant, src))


def case_off_is_unchanged(dev, dtype, bitwise=True):
    _, l0, g0 = run_model(dev, dtype, "infonce", None, batch=EQ_BATCH)             # the attribute never touched
    model, l1, g1 = run_model(dev, dtype, "infonce", False, batch=EQ_BATCH)
    assert torch.equal(l0, l1)
    _same_grads(g0, g1, bitwise, "off")
    with pytest.raises(ValueError, match="pack_text"):
        cfg, _, _, text, image, _, _ = small_setup("infonce", dtype)
        model(text.to(dev), image.to(dev), return_loss=True, text_layout=text_layout(text))


def case_embed_text(dev, dtype):
    cfg, sd, extra, text, image, _, _ = small_setup("infonce", dtype)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype).eval()
    model.pack_text = True
    with torch.no_grad():
        tl, _ = model(text.to(dev), image.to(dev), return_latents=True)
    assert torch.equal(model.embed_text(text.to(dev)), tl)


def case_rejected(dev):
    """every combination out of scope raises, with the option's name in the message"""
    base = O.CFG1.ctor_kwargs()
    for over, name in ((dict(use_all_token_embeds=True), "use_all_token_embeds"), (dict(use_mlm=True), "use_mlm"),
                       (dict(text_causal_mask=True, text_eos_id=3), "text_causal_mask"), (dict(text_rotary_pos_emb=True), "text_rotary_pos_emb"),
                       (dict(text_has_cls_token=False), "text_has_cls_token"), (dict(text_encode_without_mask=True), "text_encode_without_mask")):
        model = CLIP(**dict(base, **over))
        with pytest.raises(NotImplementedError, match=name):
            model.pack_text = True
        assert model.pack_text is False
    from x_clip_amd import TextTransformer
    cfg = O.CFG1
    for kw, name in ((dict(attn_dropout=0.1), "attn_dropout"), (dict(ff_dropout=0.1), "ff_dropout")):
        enc = TextTransformer(dim=cfg.dim_text, num_tokens=cfg.num_text_tokens, max_seq_len=cfg.text_seq_len, depth=1, heads=2, dim_head=32, **kw)
        model = CLIP(**dict(base, text_encoder=enc)).train()
        with pytest.raises(NotImplementedError, match=name):
            model.pack_text = True

    class Plug(torch.nn.Module):
        def forward(self, x, mask=None):
            return torch.zeros(x.shape[0], x.shape[1] + 1, cfg.dim_text)
    with pytest.raises(NotImplementedError, match="text_encoder"):
        CLIP(**dict(base, text_encoder=Plug())).pack_text = True
    model = CLIP(**base).to(dev).train()
    model.pack_text = True
    _, _, _, text, image, _, _ = small_setup("infonce", F32)
    with pytest.raises(NotImplementedError, match="return_encodings"):
        model(text.to(dev), image.to(dev), return_encodings=True)


def case_adamw_steps(dev):
    from x_clip_amd import FusedAdamW
    cfg, sd, extra, text, image, _, _ = small_setup("infonce", BF16)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, BF16)
    model.pack_text = True
    opt = FusedAdamW(FusedAdamW.default_param_groups(model), lr=1e-3)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        model(text.to(dev), image.to(dev), return_loss=True).backward()
        opt.step()
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if p in opt.state and "master" in opt.state[p]:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16)), k


def case_default_architecture(dev, batch=64, fill=1 / 8):
    """GPU: the default architecture (dim 512, depth 6, n = 256) in bf16 at fill ~ 1/8: loss and gradient norms against the pack_text = False run of
    the same tokens within the bf16 bars, and a lower peak of allocated memory"""
    torch.manual_seed(5)
    model = CLIP(visual_patch_dropout=0.0).to(BF16).to(dev).train()
    g = torch.Generator().manual_seed(6)
    n = model.text_seq_len
    text = torch.randint(1, 10000, (batch, n), generator=g)
    lens = torch.randint(1, int(2 * fill * n), (batch,), generator=g)
    text[torch.arange(n)[None] >= lens[:, None]] = 0
    text, image = text.to(dev), torch.randn(batch, 3, 256, 256, generator=g).to(BF16).to(dev)
    res = {}
    for pack in (False, True):
        model.pack_text = pack
        model.zero_grad(set_to_none=True)
        for _ in range(2):                                       # (the first pass warms the allocator and the workspaces)
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            loss = model(text, image, return_loss=True)
            loss.backward()
            torch.cuda.synchronize()
        res[pack] = (float(loss.detach()), {k: p.grad.double().clone() for k, p in model.named_parameters() if p.grad is not None},
                     torch.cuda.max_memory_allocated())
    (l0, g0, m0), (l1, g1, m1) = res[False], res[True]
    print(f"default architecture b={batch} fill~{fill}: loss {l0:.6f} / {l1:.6f}; peak allocated {m0 / 2**20:.0f} -> {m1 / 2**20:.0f} MiB")
    assert abs(l0 - l1) / max(1.0, abs(l0)) < 3e-4, (l0, l1)
    for k in g0:
        n0, n1 = float(g0[k].norm()), float(g1[k].norm())
        if n0 < 1e-12:
            continue
        assert abs(n0 - n1) / n0 < 0.08, (k, n0, n1)
    assert m1 < m0, (m0, m1)
