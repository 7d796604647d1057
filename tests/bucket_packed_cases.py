"""Shared cases of the row-bucketed packed layout (packing.text_layout(row_multiple=), CLIP.pack_text_row_multiple): the array row count R is
the kept row count rounded up to a multiple, and the surplus FILLER rows [kept, R) belong to no sample.  tests/test_bucket_packed_emu.py runs
them on the CPU emulator build, tests/test_bucket_packed_gpu.py on an MI355X.

What is held:
  * layout: R, kept, cu, max_len, the filler's pos / tok, cat_layouts, the refused values;
  * kernel contract: the varlen entry points write EVERY row [0, rows) -- the kept rows the bits of the launch with rows = kept, the filler rows
    exact zeros (out, lse, dqkv; dkv of the one-query backward) -- through the C ABI into NaN-poisoned buffers with guard rows behind them;
  * routes: xclip_gemm_route for the default text layer's products at a ragged and at a bucketed row count;
  * end to end: loss and every gradient against the fp64 oracle at the bars of packed_cases.case_vs_oracle (fp32 loss 1e-5, gradients 3e-4
    relative; bf16 loss 3e-4, gradients 8 % with cosine 0.999), and the parameters filler rows could leak into -- token-embedding row 0, position
    row 0, cls_token, the first layer's to_qkv -- at the same bars against the unbucketed packed run.  Not bit-equality against that run: the
    GEMM route and the split-K cut change with M."""
import pytest
import torch

import cached_cases as CC
import causal_packed_cases as CP
import clip_cases as C
import packed_cases as P
import pooled_packed_cases as Q
import rotary_packed_cases as RP
from oracle import clip_oracle as O
from x_clip_amd import CLIP, CachedContrastiveStep, FusedAdamW, _lib, ops, text_layout
from x_clip_amd.packing import cat_layouts

F32, BF16 = P.F32, P.BF16
GUARD = P.GUARD
FILLERS = (0, 1, 5, 255)
LENS_ONE = (37,)                                    # a one-sample batch: the last sample is the first


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
def lens_tokens(lens, n=40, seed=3):
    """[len(lens), n] tokens whose sample s keeps lens[s] rows with the CLS row counted: lens[s] - 1 ids, then padding"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, 50, (len(lens), n), generator=g)
    for s, ln in enumerate(lens):
        tok[s, ln - 1:] = 0
    return tok


def _same_layout(a, b, fields=("cu", "pos", "tok")):
    for f in fields:
        assert torch.equal(getattr(a, f).cpu(), getattr(b, f).cpu()), f
    assert (a.R, a.kept, a.max_len, a.batch, a.n, a.has_cls, a.ends_at_eos) == (b.R, b.kept, b.max_len, b.batch, b.n, b.has_cls, b.ends_at_eos)


def case_layout(dev):
    tok = lens_tokens((1, 2, 31, 33))
    plain = text_layout(tok, pad_id=0)
    assert (plain.R, plain.kept, plain.row_multiple) == (67, 67, None)
    for m, R in ((8, 72), (64, 128), (256, 256)):
        a = text_layout(tok, pad_id=0, row_multiple=m)
        assert (a.R, a.kept, a.row_multiple, a.max_len, a.batch) == (R, 67, m, plain.max_len, 4) and isinstance(a.R, int)
        assert torch.equal(a.cu, plain.cu) and int(a.cu[-1]) == 67
        assert a.pos.shape == (R,) and a.tok.shape == (R,) and a.pos.dtype == torch.int32 and a.tok.dtype == torch.int64
        assert torch.equal(a.pos[:67], plain.pos) and torch.equal(a.tok[:67], plain.tok)
        assert int(a.pos[67:].abs().max()) == 0 and int(a.tok[67:].abs().max()) == 0
        b = text_layout(tok.to(dev), pad_id=0, row_multiple=m)                      # device-built equals CPU-built
        assert b.cu.device.type == dev.type
        _same_layout(a, b)
        _same_layout(a, a.to(dev))
        tk, pk = a.keys(50, 40)                                                     # filler is dropped like a CLS row
        assert bool((tk[67:] == 50).all()) and bool((pk[67:] == 40).all())
    # kept already a multiple: no filler, the unbucketed layout's tensors
    tok8 = lens_tokens((1, 2, 31, 30))
    a, b = text_layout(tok8, pad_id=0, row_multiple=8), text_layout(tok8, pad_id=0)
    assert a.R == a.kept == 64
    _same_layout(a, b)
    # an empty batch
    e = text_layout(torch.zeros(0, 40, dtype=torch.int64), pad_id=0, row_multiple=256)
    assert (e.R, e.kept, e.batch) == (0, 0, 0) and e.pos.numel() == 0
    # the causal form
    t = CP.eos_tokens()
    c0, c1 = text_layout(t, pad_id=0, has_cls=False, eos_id=CP.EOS), text_layout(t, pad_id=0, has_cls=False, eos_id=CP.EOS, row_multiple=8)
    assert c1.ends_at_eos and not c1.has_cls and c1.kept == c0.R == 15 and c1.R == 16 and torch.equal(c1.cu, c0.cu) and c1.max_len == c0.max_len
    assert torch.equal(c1.pos[:15], c0.pos) and torch.equal(c1.tok[:15], c0.tok) and int(c1.pos[15]) == 0 and int(c1.tok[15]) == 0
    tk, pk = c1.keys(50, 6)
    assert int(tk[15]) == 0 and int(pk[15]) == 0                                    # (row 0 of both tables: zeros are added there)
    for bad in (0, -8, 2.0, "256", True, 8.5):
        with pytest.raises(ValueError, match="row_multiple"):
            text_layout(tok, pad_id=0, row_multiple=bad)
        with pytest.raises(ValueError, match="row_multiple"):
            CLIP(**O.CFG1.ctor_kwargs()).pack_text_row_multiple = bad
    model = CLIP(**O.CFG1.ctor_kwargs())
    assert model.pack_text_row_multiple is None
    model.pack_text_row_multiple = 256
    assert model.pack_text_row_multiple == 256
    model.pack_text_row_multiple = None


def case_cat_layouts(dev):
    ta, tb = lens_tokens((1, 2, 31, 33)), lens_tokens((5, 9), seed=4)
    pa, pb = text_layout(ta, pad_id=0), text_layout(tb, pad_id=0)
    want = cat_layouts([pa, pb])                                                     # 67 + 14 = 81 kept rows
    for ma, mb, R in ((8, 64, 128), (64, 8, 128), (8, None, 88), (None, 8, 88), (8, 8, 88)):
        a, b = text_layout(ta.to(dev), pad_id=0, row_multiple=ma), text_layout(tb.to(dev), pad_id=0, row_multiple=mb)
        c = cat_layouts([a, b])
        assert (c.R, c.kept, c.batch, c.max_len, c.row_multiple) == (R, 81, 6, want.max_len, max(m for m in (ma, mb) if m))
        assert torch.equal(c.cu.cpu(), want.cu) and int(c.cu[-1]) == 81
        assert torch.equal(c.pos[:81].cpu(), want.pos) and torch.equal(c.tok[:81].cpu(), want.tok)      # filler never sits between samples
        assert c.pos.shape == (R,) and int(c.pos[81:].abs().max()) == 0 and int(c.tok[81:].abs().max()) == 0
    _same_layout(cat_layouts([pa, pb]), want)
    assert cat_layouts([pa, pb]).row_multiple is None


# ---- kernel contract ------------------------------------------------------------------------------------------------------------------------
def _filler_data(lens, filler, heads, slot, dtype, dev, seed):
    """packed_cases.varlen_data on the kept rows with `filler` finite, non-zero rows behind them (what a bucketed tower's qkv GEMM leaves there)"""
    qkv, dout = P.varlen_data(tuple(lens) + ((filler,) if filler else ()), heads, slot, slot, dtype, dev, seed)
    return qkv, dout


def _launch(names, qkv, dout, cu, rows, max_len, heads, slot, scale):
    """forward and backward entry points `names` through the C ABI on the first `rows` rows into NaN-poisoned buffers with GUARD rows behind row
    `rows`; every guard element keeps its poison bit for bit -> (out, lse [heads, rows], dqkv)"""
    L = _lib.lib()
    dev, dt, inner = qkv.device, qkv.dtype, heads * slot
    out, lse, dqkv = P._poison((rows + GUARD, inner), dt, dev), P._poison((heads * rows + GUARD,), F32, dev), P._poison((rows + GUARD, 3 * inner), dt, dev)
    guards = lambda: (out[rows:], lse[heads * rows:], dqkv[rows:])
    want = [P._bits(t).clone() for t in guards()]
    code, st, B = ops.dtype_code(qkv), ops._stream(qkv), cu.numel() - 1
    q, do = qkv[:rows].contiguous(), dout[:rows].contiguous()
    _lib.check(getattr(L, names[0])(q.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), rows, B, heads, slot, max_len, scale, code, st), names[0])
    _lib.check(getattr(L, names[1])(q.data_ptr(), cu.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), rows, B, heads, slot,
                                    max_len, scale, code, st), names[1])
    for name, t, w in zip(("out", "lse", "dqkv"), guards(), want):
        assert torch.equal(P._bits(t), w), f"{names[0]}: wrote behind row `rows` of {name}"
    return out[:rows], lse[:heads * rows].view(heads, rows), dqkv[:rows]


PLAIN = ("xclip_attention_varlen_fwd", "xclip_attention_varlen_bwd")
CAUSAL = ("xclip_attention_varlen_causal_fwd", "xclip_attention_varlen_causal_bwd")
# (dtype, slot): the head-resident form; the plain form by fp32, by a 128-wide slot and (with a sample longer than 288 rows) by max_len
FORMS = {"resident": (BF16, 64), "plain_fp32": (F32, 64), "plain_wide": (BF16, 128), "plain_long": (BF16, 64)}


def case_filler_rows(dev, form, lens, filler, causal, heads=3, seed=0):
    """rows = kept + filler: the kept rows of out / lse / dqkv are the bits of the launch with rows = kept, the filler rows exactly zero, the
    guards intact.  (On a library whose kernels write owned rows only, the filler rows keep their NaN poison.)"""
    dtype, slot = FORMS[form]
    kept = sum(lens)
    qkv, dout = _filler_data(lens, filler, heads, slot, dtype, dev, seed)
    cu, names, scale = P._cu(lens, dev), CAUSAL if causal else PLAIN, slot ** -0.5
    base = _launch(names, qkv, dout, cu, kept, max(lens), heads, slot, scale)
    got = _launch(names, qkv, dout, cu, kept + filler, max(lens), heads, slot, scale)
    for name, a, b in zip(("out", "lse", "dqkv"), base, got):
        kept_part = b[:, :kept] if name == "lse" else b[:kept]
        fill_part = b[:, kept:] if name == "lse" else b[kept:]
        assert bool(torch.isfinite(a).all()), f"{name}: a kept row is not finite"
        assert torch.equal(P._bits(kept_part), P._bits(a)), f"{name}: the kept rows changed with {filler} filler rows behind them"
        assert torch.equal(fill_part, torch.zeros_like(fill_part)), f"{name}: {filler} filler rows are not exactly zero"
    return got


def case_pool_filler_rows(dev, dtype, slot, lens, filler, heads=3, seed=1):
    """the one-query varlen backward: dkv's filler rows are zero, everything else the bits of the launch with rows = kept"""
    kept = sum(lens)
    _, q, kv, dout = Q.pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed)
    g = torch.Generator().manual_seed(77 + seed)
    kv_f = torch.cat([kv, P._nonzero_randn((filler, kv.shape[1]), g, dtype).to(dev)]) if filler else kv
    cu, scale = P._cu(lens, dev), slot ** -0.5
    base = Q.pool_varlen_launch(q, kv, dout, cu, heads, slot, scale)                 # (checks its guards and that everything is finite)
    got = Q.pool_varlen_launch(q, kv_f, dout, cu, heads, slot, scale)
    for name, a, b in zip(("out", "lse", "dq"), base, got):
        assert torch.equal(P._bits(a), P._bits(b)), name
    assert torch.equal(P._bits(got[3][:kept]), P._bits(base[3])), "dkv: the kept rows changed"
    assert torch.equal(got[3][kept:], torch.zeros_like(got[3][kept:])), f"dkv: {filler} filler rows are not exactly zero"


# ---- routes ---------------------------------------------------------------------------------------------------------------------------------
ROUTE_RAGGED, ROUTE_BUCKETED = 69276, 69376          # a measured row count at fill 1/4 (69,276 % 8 = 4) and the next multiple of 256
BIG = 1 << 40                                        # workspace on offer: whatever the plan asks for


def text_layer_products(R):
    """(tag, a_kmajor, b_kmajor, M, N, K, lda, ldb) of the default text layer (dim 512, inner 512, feed-forward 4 x 512 with GEGLU): forward,
    input gradient and weight gradient of to_qkv, to_out, FF1 and FF2"""
    out = []
    for name, n_out, k_in in (("to_qkv", 1536, 512), ("to_out", 512, 512), ("ff1", 4096, 512), ("ff2", 512, 2048)):
        out.append((name + " fwd", 0, 0, R, n_out, k_in, k_in, k_in))
        out.append((name + " dgrad", 0, 1, R, k_in, n_out, n_out, k_in))
        out.append((name + " wgrad", 1, 1, n_out, k_in, R, n_out, k_in))
    return out


def case_routes():
    L = _lib.lib()
    route = lambda p, dtype=1: L.xclip_gemm_route(p[1], p[2], p[3], p[4], p[5], p[6], p[7], 0, 0, BIG, dtype)
    for ragged, bucketed in zip(text_layer_products(ROUTE_RAGGED), text_layer_products(ROUTE_BUCKETED)):
        assert route(ragged) == 3, (ragged[0], route(ragged))
        assert route(bucketed) in (1, 2), (bucketed[0], route(bucketed))
    fwd = text_layer_products(ROUTE_BUCKETED)[0]
    assert route(fwd, 0) == 3                                                        # fp32 has the generic kernel alone
    assert L.xclip_gemm_route(0, 0, 256, 512, 512, 512, 512, 0, 0, 0, 1) == 0        # a [256, 512] x 512 product: the 64 x 64 latency kernel
    assert L.xclip_gemm_route(0, 0, 256, 512, 512, 512, 512, 1, 0, 0, 1) == 1        # ... which takes no bias
    assert L.xclip_gemm_route(0, 0, 0, 512, 512, 512, 512, 0, 0, 0, 1) == -1 and b"xclip_gemm_route" in L.xclip_last_error()
    assert L.xclip_gemm_route(0, 0, 256, 512, 512, 512, 512, 0, 0, 0, 7) == -1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
KINDS = {"cls": "pack_text", "causal": "pack_text_causal", "rotary": "pack_text_rotary"}


def _setup(kind, variant, dtype, batch=None):
    if kind == "cls":
        return P.small_setup(variant, dtype, batch, wide=dtype != F32)
    if kind == "causal":
        return P.small_setup(variant, dtype, batch, cfg=CP._cfg_for(dtype), pad=CP.eos_text)
    return P.small_setup(variant, dtype, batch, cfg=RP._cfg_for(dtype))


_ORACLE = {}


def _oracle(kind, variant, dtype, batch):
    """computed once per (encoder, loss, storage type, batch) and shared, unchanged, by the cases that need it"""
    key = (kind, variant, dtype, batch)
    if key not in _ORACLE:
        how = dict(wide=dtype != F32) if kind == "cls" else dict(cfg=CP._cfg_for(dtype), pad=CP.eos_text) if kind == "causal" else dict(cfg=RP._cfg_for(dtype))
        _ORACLE[key] = P.oracle(variant, dtype, batch, **how)
    return _ORACLE[key]


def _kept_rows(kind, variant, dtype, batch):
    cfg, _, _, text, _, aug_t, _ = _setup(kind, variant, dtype, batch)
    causal = dict(has_cls=False, eos_id=cfg.text_eos_id) if kind == "causal" else {}
    return sum(text_layout(t, pad_id=cfg.text_pad_id, **causal).kept for t in [text] + list(aug_t))


def batch_with_filler(kind, variant, dtype):
    """the largest batch <= 8 whose kept row count is no multiple of 8: every multiple the cases use then leaves filler rows"""
    return next(b for b in (8, 7, 6, 5) if _kept_rows(kind, variant, dtype, b) % 8 != 0)


def run(dev, dtype, kind, variant, multiple, pool_last=False, how="attr", batch=None, **ctor):
    """how = "attr": the implicit path, CLIP.pack_text_row_multiple = multiple; "layout": text_layout(..., row_multiple=multiple) passed in and the
    attribute never touched (with augmented texts their layout is then unbucketed: cat_layouts pads the whole to the passed layout's multiple)
    -> (loss, grads, the layout the tower saw)"""
    cfg, sd, extra, text, image, aug_t, aug_i = _setup(kind, variant, dtype, batch)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **extra, **ctor)
    setattr(model, KINDS[kind], True)
    model.pack_text_pool_last = pool_last
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    if how == "attr":
        model.pack_text_row_multiple = multiple
    else:
        causal = dict(has_cls=False, eos_id=cfg.text_eos_id) if kind == "causal" else {}
        kw["text_layout"] = text_layout(text, pad_id=cfg.text_pad_id, row_multiple=multiple, **causal)
    seen = []
    real = model.text_transformer.forward

    def spy(*a, **k):
        seen.append(k.get("layout"))
        return real(*a, **k)
    model.text_transformer.forward = spy
    loss = model(text.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    assert len(seen) >= 1 and seen[0] is not None
    return loss.detach(), {k: p.grad for k, p in model.named_parameters()}, seen[0]


def leak_prone(grads):
    """the gradients filler rows (tok 0, pos 0) could leak into: token-embedding row 0, position row 0, cls_token, the first layer's to_qkv"""
    out = {}
    for k, g in grads.items():
        if not k.startswith("text_transformer.") or g is None:
            continue
        if k.endswith("token_emb.weight") or k.endswith("abs_pos_emb.weight"):
            out[k + "[0]"] = g[0]
        elif k.endswith("cls_token"):
            out[k] = g
        elif k.endswith("to_qkv.weight") and not any(n.endswith("to_qkv.weight") for n in out):
            out[k] = g
    assert any(n.endswith("to_qkv.weight") for n in out) and any("token_emb" in n for n in out)
    return out


_PLAIN = {}


def case_vs_oracle(dev, dtype, kind, variant, multiple, pool_last, how="attr", **ctor):
    """loss and every gradient against the fp64 oracle; the leak-prone gradients against the unbucketed packed run of the same model and batch"""
    tag = f"bucketed {kind} {variant} {dtype} m{multiple} pool_last={pool_last} {how}" + ("".join(f" {k}" for k in ctor))
    batch = batch_with_filler(kind, variant, dtype)
    loss, grads, lay = run(dev, dtype, kind, variant, multiple, pool_last, how, batch, **ctor)
    assert lay.R % multiple == 0 and lay.row_multiple == multiple and 0 <= lay.R - lay.kept < multiple and int(lay.cu[-1]) == lay.kept, (lay.R, lay.kept)
    assert lay.R > lay.kept, "the case has no filler row: choose another batch"
    ref_loss, ref_grads = _oracle(kind, variant, dtype, batch)
    CP._compare(tag, dtype, loss, grads, ref_loss, ref_grads)
    key = (kind, variant, dtype, pool_last, dev.type) + tuple(sorted(ctor.items()))
    if key not in _PLAIN:
        l0, g0, lay0 = run(dev, dtype, kind, variant, None, pool_last, "attr", batch, **ctor)
        assert lay0.R == lay0.kept == lay.kept and lay0.row_multiple is None
        _PLAIN[key] = (float(l0), {k: g.double().cpu() for k, g in leak_prone(g0).items()})
    l0, g0 = _PLAIN[key]
    CP._compare(tag + " vs unbucketed", dtype, loss, leak_prone(grads), l0, g0)
    if kind != "causal":
        pad_row = grads["text_transformer.token_emb.weight"][0]
        assert float(pad_row.abs().max()) == 0.0, "the pad id's embedding row received a gradient"


def case_off_is_unchanged(dev, dtype, bitwise=True):
    """pack_text_row_multiple = None: the layout and the loss bits of a model whose attribute was never touched; the attribute is ignored while
    all three packing attributes are off"""
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype, P.EQ_BATCH)
    a, b = text_layout(text, pad_id=cfg.text_pad_id), text_layout(text, pad_id=cfg.text_pad_id, row_multiple=None)
    _same_layout(a, b)
    assert a.R == a.kept and a.row_multiple is None
    res = []
    for pack, multiple in ((True, "untouched"), (True, None), (False, "untouched"), (False, 256)):
        model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype)
        model.pack_text = pack
        if multiple != "untouched":
            model.pack_text_row_multiple = multiple
        loss = model(text.to(dev), image.to(dev), return_loss=True)
        loss.backward()
        res.append((loss.detach(), {k: p.grad for k, p in model.named_parameters()}))
    for i in (0, 2):
        assert torch.equal(res[i][0], res[i + 1][0]), i
        P._same_grads(res[i][1], res[i + 1][1], bitwise, f"row_multiple off {i}")


def case_no_filler_same_bits(dev, dtype, multiple=8):
    """a kept row count that is a multiple already (batch 8 of small_setup keeps 136 rows): the same layout tensors, hence the same launches --
    the loss bits of the unbucketed run"""
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype)
    assert text_layout(text, pad_id=cfg.text_pad_id).kept % multiple == 0
    losses = []
    for m in (None, multiple):
        model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype)
        model.pack_text = True
        model.pack_text_row_multiple = m
        losses.append(model(text.to(dev), image.to(dev), return_loss=True).detach())
    assert torch.equal(losses[0], losses[1])


def case_cached_and_adamw(dev, dtype, cfg, multiple=8, b=8):
    """one CachedContrastiveStep step (two slices) with its FusedAdamW step on a bucketed packed tower: clean and finite"""
    model = CC.build(dev, dtype, cfg, "infonce")
    model.pack_text = True
    model.pack_text_pool_last = True
    model.pack_text_row_multiple = multiple
    opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
    step = CachedContrastiveStep(model, opt, micro_batch=b // 2)
    text, image = CC.batch(cfg, b, dtype)
    loss = step.step(P.padded_text(cfg, text).to(dev), image.to(dev))
    assert bool(torch.isfinite(torch.as_tensor(float(loss))))
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
    # and a plain FusedAdamW step of forward + backward
    opt.zero_grad(set_to_none=True)
    loss = model(P.padded_text(cfg, text).to(dev), image.to(dev), return_loss=True)
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), k
    opt.step()
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k


def case_embed_text(dev, dtype, multiple=8):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype).eval()
    model.pack_text = True
    model.pack_text_row_multiple = multiple
    with torch.no_grad():
        tl, _ = model(text.to(dev), image.to(dev), return_latents=True)
        got = model.embed_text(text.to(dev))
    assert torch.equal(got, tl) and bool(torch.isfinite(got).all())
