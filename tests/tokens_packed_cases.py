"""Shared cases of the packed text tower for the heads that read TOKEN rows (CLIP.pack_text_tokens: the fine-grained FILIP head, the MLM head,
return_encodings): xclip_unpack_rows / xclip_pack_rows through the C ABI against a torch index reference (copies: torch.equal, no tolerance),
and the public interface end to end.  tests/test_tokens_packed_emu.py runs them on the CPU emulator build, tests/test_tokens_packed_gpu.py on
an MI355X.

Bars: the kernels copy -- bits.  End to end the bars the dense cases of the same variant and dtype are held to (tests/clip_cases.py
case_vs_oracle and its callers in tests/test_clip_gpu.py): fp32 loss 1e-5 and every gradient 2e-4 relative; bf16 loss 3e-4, gradients 8 % with
cosine 0.999 (MLM: test_mid_mlm_vs_oracle), and 16 % with cosine 0.985 wherever the fine-grained head routes through bf16 arg-max ties
(test_filip_mid_vs_oracle).  bf16 runs the dim-512 model those bars are stated for (packed_cases.WIDE), fp32 the two-layer CFG1.  Run against
run of the same launches: packed_cases._same_grads."""
import dataclasses

import pytest
import torch

import clip_cases as C
import packed_cases as P
from oracle import clip_oracle as O
from packed_cases import BF16, F32, GUARD, _bits, _poison
from x_clip_amd import CLIP, FusedAdamW, _lib, ops, packing, text_layout
from x_clip_amd import functional as XF


# ---- the two kernels, through the C ABI -------------------------------------------------------------------------------------------------------
def widths(dtype):
    """one 16-byte chunk, one chunk per lane of a wave's first half / whole wave, and a width that is no multiple of 64 lanes' worth"""
    return (8, 64, 520) if dtype == BF16 else (4, 64, 516)


def _tok(rows):
    return torch.tensor(rows, dtype=torch.int64)


def layouts():
    """name -> (tokens [B, n], row_multiple).  `kinds`: one of every kind of sample in one batch -- CLS only, full, a hole in mid-sequence, only
    the last position kept, a padded tail; `one`: batch = 1; `long`: samples of 65 and 129 kept rows (both sides of a 64-row search step) with
    holes, beside a CLS-only one; `filler`: rows > cu[batch]"""
    kinds = _tok([[0] * 8, [3, 4, 5, 6, 7, 8, 9, 10], [3, 4, 0, 0, 7, 8, 9, 10], [0] * 7 + [5], [3, 4, 5, 0, 0, 0, 0, 0]])
    long = torch.ones(3, 140, dtype=torch.int64)
    long[0, 64:] = 0                                            # 64 tokens + CLS = 65 rows
    long[1, 1::13] = 0                                          # holes: 140 - 11 = 129 tokens ...
    long[1, 137] = 0                                            # ... - 1 = 128 + CLS = 129 rows
    long[2] = 0
    lay = text_layout(long)
    assert (lay.cu[1:] - lay.cu[:-1]).tolist() == [65, 129, 1]
    return {"kinds": (kinds, None), "one": (kinds[2:3], None), "long": (long, None), "filler": (kinds, 16)}


def windows(n):
    """(pos0, n_out): `[:, 1:]` (the CLS row dropped), the whole encoding, the CLS row alone and one position in mid-sequence (n_out = 1)"""
    return ((1, n), (0, n + 1), (0, 1), (3, 1))


def _launch(fn_name, src, lay, out_rows, out_shape, batch, n_out, pos0):
    """src -> a NaN-poisoned output with GUARD rows in front and behind, through the C ABI; the guards keep their poison bit for bit"""
    L = _lib.lib()
    D, dev, dt = src.shape[-1], src.device, src.dtype
    buf = _poison((GUARD + out_rows + GUARD, D), dt, dev)
    before = _bits(buf).clone()
    body = buf[GUARD: GUARD + out_rows]
    # (both entry points: source, cu, pos, destination)
    _lib.check(getattr(L, fn_name)(src.data_ptr(), lay.cu.data_ptr(), lay.pos.data_ptr(), body.data_ptr(), lay.R, batch, n_out, pos0, D,
                                   ops.dtype_code(src), ops._stream(src)), fn_name)
    after = _bits(buf)
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + out_rows:], before[GUARD + out_rows:]), f"{fn_name} wrote a guard row"
    out = body.clone().view(out_shape)
    assert not bool(torch.isnan(out).any()), f"{fn_name} left an output row unwritten (poison)"
    return out


def unpack(x, lay, pos0, n_out):
    return _launch("xclip_unpack_rows", x, lay, lay.batch * n_out, (lay.batch, n_out, x.shape[1]), lay.batch, n_out, pos0)


def pack(y, lay, pos0):
    return _launch("xclip_pack_rows", y.contiguous(), lay, lay.R, (lay.R, y.shape[2]), lay.batch, y.shape[1], pos0)


def _selection(lay, pos0, n_out):
    """-> (owned: bool [R], the packed rows with a place in the window; flat: int64 [owned.sum()], their dense row s n_out + pos - pos0), on the CPU"""
    cu, pos = lay.cu.cpu().long(), lay.pos.cpu().long()
    r = torch.arange(lay.R)
    sample = torch.searchsorted(cu[1:], r, right=True).clamp_max(max(lay.batch - 1, 0))
    owned = (r < lay.kept) & (pos >= pos0) & (pos < pos0 + n_out)
    return owned, (sample * n_out + pos - pos0)[owned]


def _int_data(shape, dtype, seed):
    """small non-zero integers (exact in bf16, and every sum of their products exact in fp64)"""
    g = torch.Generator().manual_seed(8800 + seed)
    v = torch.randint(1, 9, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    return v.to(dtype)


def case_kernels(dev, dtype, name, D):
    """both kernels on one layout, every window: the torch index reference bit for bit (the reference's untouched rows are +0, so the sign bit
    of every zero row is checked), every output row written once (no poison left, guards intact), and adjointness -- pack(unpack(x)) is x on the
    owned rows and +0 elsewhere; <unpack(x), y> == <x, pack(y)> exactly, in fp64 sums of small-integer data"""
    tok, multiple = layouts()[name]
    lay = text_layout(tok, row_multiple=multiple).to(dev)
    assert (lay.R > lay.kept) == (name == "filler")
    B, n = tok.shape
    x = _int_data((lay.R, D), dtype, D + B).to(dev)
    for pos0, n_out in windows(n):
        owned, flat = _selection(lay, pos0, n_out)
        want = torch.zeros(B * n_out, D, dtype=dtype)
        want[flat] = x.cpu()[owned]
        got = unpack(x, lay, pos0, n_out)
        assert torch.equal(_bits(got.cpu().view(B * n_out, D)), _bits(want)), f"unpack_rows {name} D{D} window ({pos0}, {n_out})"
        y = _int_data((B, n_out, D), dtype, D + n_out).to(dev)
        want_p = torch.zeros(lay.R, D, dtype=dtype)
        want_p[owned] = y.cpu().view(B * n_out, D)[flat]
        got_p = pack(y, lay, pos0)
        assert torch.equal(_bits(got_p.cpu()), _bits(want_p)), f"pack_rows {name} D{D} window ({pos0}, {n_out})"
        back = pack(got, lay, pos0).cpu()
        assert torch.equal(_bits(back[owned]), _bits(x.cpu()[owned])) and not bool(_bits(back[~owned]).any()), "pack(unpack(x)) != x on the owned rows, +0 elsewhere"
        lhs = float((got.double() * y.double()).sum())
        rhs = float((x.double() * got_p.double()).sum())
        assert lhs == rhs, ("<unpack(x), y> != <x, pack(y)>", lhs, rhs)


def case_kernel_edges(dev, dtype):
    """nothing to do is success with nothing launched; a width that is no whole number of 16-byte chunks is refused"""
    L = _lib.lib()
    tok, _ = layouts()["kinds"]
    lay = text_layout(tok).to(dev)
    x = _int_data((lay.R, 16), dtype, 1).to(dev)
    code, st = ops.dtype_code(x), ops._stream(x)
    assert L.xclip_unpack_rows(x.data_ptr(), lay.cu.data_ptr(), lay.pos.data_ptr(), None, lay.R, lay.batch, 0, 1, 16, code, st) == 0
    assert L.xclip_pack_rows(None, lay.cu.data_ptr(), lay.pos.data_ptr(), None, 0, lay.batch, 0, 1, 16, code, st) == 0
    out = torch.zeros(lay.batch, 2, 16, dtype=dtype, device=dev)
    assert L.xclip_unpack_rows(x.data_ptr(), lay.cu.data_ptr(), lay.pos.data_ptr(), out.data_ptr(), lay.R, lay.batch, 2, 1, 15, code, st) != 0
    assert b"16-byte" in L.xclip_last_error()
    assert L.xclip_pack_rows(out.data_ptr(), lay.cu.data_ptr(), lay.pos.data_ptr(), x.data_ptr(), lay.R, lay.batch, 2, 1, 15, code, st) != 0


def case_functional_pair(dev, dtype):
    """functional.unpack_rows / pack_rows: each one's backward is the other (autograd through both, against the index reference)"""
    tok, _ = layouts()["kinds"]
    lay = text_layout(tok, row_multiple=16).to(dev)
    B, n = tok.shape
    owned, flat = _selection(lay, 1, n)
    x = _int_data((lay.R, 16), dtype, 3).to(dev).requires_grad_(True)
    g = _int_data((B, n, 16), dtype, 4).to(dev)
    d = XF.unpack_rows(x, lay, 1, n)
    d.backward(g)
    want = torch.zeros(lay.R, 16, dtype=dtype)
    want[owned] = g.cpu().view(B * n, 16)[flat]
    assert torch.equal(_bits(x.grad.cpu()), _bits(want))
    y = g.clone().requires_grad_(True)
    p = XF.pack_rows(y, lay, 1)
    assert torch.equal(_bits(p.detach().cpu()), _bits(want))
    p.backward(x.detach())
    assert torch.equal(_bits(y.grad.cpu()), _bits(d.detach().cpu()))
    with pytest.raises(ValueError, match="packed rows"):
        XF.unpack_rows(x[:-1], lay, 1, n)


def case_layout_helpers(dev):
    """TextLayout.with_tokens / row_of: index arithmetic only -- no text_layout call, the values of a layout built from the other tokens"""
    tok, _ = layouts()["kinds"]
    other = torch.where(tok != 0, tok + 100, tok)
    for multiple in (None, 16):
        lay = text_layout(tok.to(dev), row_multiple=multiple)
        want = text_layout(other.to(dev), row_multiple=multiple)
        got = lay.with_tokens(other.to(dev))
        assert got.cu is lay.cu and got.pos is lay.pos and (got.R, got.kept, got.max_len) == (lay.R, lay.kept, lay.max_len)
        assert torch.equal(got.tok, want.tok) and got.tok.dtype == torch.int64 and got.tok.shape == (lay.R,)
        row_of = lay.row_of().cpu()
        assert row_of.dtype == torch.int32 and row_of.shape == (tok.shape[0], tok.shape[1] + 1)
        keep = torch.cat([torch.ones(tok.shape[0], 1, dtype=torch.bool), tok != 0], dim=1)
        assert torch.equal(row_of[keep].long(), torch.arange(lay.kept)) and bool((row_of[~keep] == -1).all())
    with pytest.raises(TypeError, match="with_tokens"):
        lay.with_tokens(other[:, :-1])


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def text_for_filip(cfg, text):
    """packed_cases.padded_text with one token in sample 0: the fine-grained head averages over a sample's kept tokens, and a sample without
    any divides by zero in the reference too (x_clip.py:805-811).  Sample 0 is then CLS + one token, sample 1 full, sample 2 has a hole"""
    text = P.padded_text(cfg, text)
    text[0, 0] = 7
    return text


# kind -> (config flags, loss variant of packed_cases.VARIANTS, bf16 bars as the dense case of the variant holds them)
FILIP_BARS = dict(bf16_rel=0.16, bf16_cos=0.985)                # tests/test_clip_gpu.py test_filip_mid_vs_oracle
CLS_BARS = dict(bf16_rel=0.08, bf16_cos=0.999)                  # clip_cases.case_vs_oracle's defaults (test_mid_mlm_vs_oracle)
KINDS = {
    "filip": (dict(use_all_token_embeds=True), "infonce", FILIP_BARS),
    "filip_dcl_multiview": (dict(use_all_token_embeds=True), "dcl_multiview", FILIP_BARS),
    "mlm": (dict(use_mlm=True, text_ssl_loss_weight=0.3), "infonce", CLS_BARS),
    "mlm_filip": (dict(use_mlm=True, text_ssl_loss_weight=0.3, use_all_token_embeds=True), "infonce", FILIP_BARS),
    "filip_rotary": (dict(use_all_token_embeds=True, text_rotary_pos_emb=True), "infonce", FILIP_BARS),
}


# bf16: packed_cases.WIDE with the 16 image patches of the model the fine-grained bf16 bars were measured on (tests/test_clip_gpu.py MID): the head
# routes every text token through its arg-max patch, and with WIDE's four patches one tie that bf16 scores break the other way moves a quarter of
# a sample's image side -- the DENSE model then misses the bars by itself (measured, mlm_filip: 25 %, cosine 0.968, the same bits packed or not)
WIDE16 = dataclasses.replace(P.WIDE, visual_image_size=128)


def cfg_for(kind, dtype):
    return dataclasses.replace(O.CFG1 if dtype == F32 else WIDE16, **KINDS[kind][0])


def setup(kind, dtype, batch=None, pad=None):
    cfg = cfg_for(kind, dtype)
    if pad is None:
        pad = text_for_filip if cfg.use_all_token_embeds else P.padded_text
    cfg, sd, extra, text, image, aug_t, aug_i = P.small_setup(KINDS[kind][1], dtype, batch, cfg=cfg, pad=pad)
    mlm = None
    if cfg.use_mlm:                                             # clip_cases.case_vs_oracle's stand-in for the random masking: every 5th real token
        chosen = (text != cfg.text_pad_id) & ((torch.arange(text.shape[1])[None] + torch.arange(text.shape[0])[:, None]) % 5 == 0)
        mlm = (text.masked_fill(chosen, 2), text.masked_fill(~chosen, cfg.text_pad_id))
    return cfg, sd, text, image, aug_t, aug_i, mlm


def build(dev, dtype, kind, batch=None, pad=None, **ctor):
    cfg, sd, text, image, aug_t, aug_i, mlm = setup(kind, dtype, batch, pad)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **ctor)
    if mlm is not None:
        model.mlm.masked_override = (mlm[0].to(dev), mlm[1].to(dev))
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    return model, cfg, text, image, kw


def run(dev, dtype, kind, pack, layout_from=None, batch=None, pad=None, row_multiple=None, pool_last=False, **ctor):
    """pack: True / False set the attribute, None leaves it untouched -> (model, loss, grads)"""
    model, cfg, text, image, kw = build(dev, dtype, kind, batch, pad, **ctor)
    if pack is not None:
        model.pack_text_tokens = pack
    model.pack_text_row_multiple = row_multiple
    model.pack_text_pool_last = pool_last
    if layout_from is not None:
        kw["text_layout"] = text_layout(text if layout_from == "cpu" else text.to(dev), pad_id=cfg.text_pad_id, row_multiple=row_multiple)
    loss = model(text.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}


_ORACLE = {}


def oracle(kind, dtype):
    if (kind, dtype) not in _ORACLE:
        cfg, sd, text, image, aug_t, aug_i, mlm = setup(kind, dtype)
        sd64 = {k: (t.double() if t.is_floating_point() else t) for k, t in sd.items()}
        with O.layer_norm_eps(1e-5 if dtype == F32 else 1e-3):
            loss, grads = C.oracle_run(cfg, sd64, text, image.double(), aug_t, [a.double() for a in aug_i], None, mlm)
        _ORACLE[kind, dtype] = (float(loss), grads)
    return _ORACLE[kind, dtype]


def case_vs_oracle(dev, dtype, kind, pool_last=False):
    """pack_text_tokens = True against the fp64 oracle on the same (dtype-rounded) parameters, padded tokens and MLM masking: the loss and every
    gradient under clip_cases.case_vs_oracle's bars for the variant; the pad id's embedding-gradient row is exactly zero"""
    ref_loss, ref_grads = oracle(kind, dtype)
    model, loss, grads = run(dev, dtype, kind, True, pool_last=pool_last)
    bars, fp32 = KINDS[kind][2], dtype == F32
    err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    print(f"packed tokens {kind} {dtype}: loss {float(loss):.6f} oracle {ref_loss:.6f} err {err:.2e}")
    failures = [] if err < (1e-5 if fp32 else 3e-4) else [("loss", float(loss), ref_loss)]
    for k, g in grads.items():
        rg = ref_grads[k]
        if rg is None or float(rg.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        g = g.double().cpu()
        assert bool(torch.isfinite(g).all()), k
        rel = float((g - rg).norm() / rg.norm())
        cos = float((g * rg).sum() / (g.norm() * rg.norm()))
        print(f"packed tokens {kind} {dtype} {k}: rel {rel:.2e} cos {cos:.6f}")
        if not ((rel < 2e-4) if fp32 else (rel < bars["bf16_rel"] and cos > bars["bf16_cos"])):
            failures.append((k, rel, cos))
    assert not failures, failures
    pad_row = grads["text_transformer.token_emb.weight"][cfg_for(kind, dtype).text_pad_id]
    assert float(pad_row.abs().max()) == 0.0, "the pad id's embedding row received a gradient"


def case_encodings_equal_dense(dev, dtype, kind="mlm"):
    """return_encodings=True at EQ_BATCH: the kept rows are the dense tower's (prune_unused_rows = False) bit for bit, the padded rows +0.

    bf16: the head-resident varlen attention runs the dense kernels' body, and a masked key contributes exactly 0 there -- every kept row, the
    sample with a hole included.  fp32: the varlen entry points would take their plain form (one wave per (row, head)), which sums a row's
    probabilities and P V in another order than the dense blocked kernel (7.7e-7 on the attention output alone, 1.5e-6 on the encodings); the
    rows path therefore runs the DENSE attention kernels on the rows put back by position (functional._attn_dense_on_packed), counted here.
    Every GEMM and row kernel gives the dense bits on the kept rows in both types."""
    calls = []
    real = XF._attn_dense_on_packed

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    XF._attn_dense_on_packed = counted
    try:
        _encodings_equal_dense(dev, dtype, kind)
    finally:
        XF._attn_dense_on_packed = real
    assert len(calls) == (cfg_for(kind, dtype).text_enc_depth if dtype == F32 else 0), len(calls)


def _encodings_equal_dense(dev, dtype, kind):
    model, cfg, text, image, _ = build(dev, dtype, kind, batch=P.EQ_BATCH)
    model.prune_unused_rows = False
    with torch.no_grad():
        want, want_i = model(text.to(dev), image.to(dev), return_encodings=True)
        model.pack_text_tokens = True
        got, got_i = model(text.to(dev), image.to(dev), return_encodings=True)
    assert got.shape == want.shape == (text.shape[0], text.shape[1] + 1, cfg.dim_text) and torch.equal(got_i, want_i)
    keep = torch.cat([torch.ones(text.shape[0], 1, dtype=torch.bool), text != cfg.text_pad_id], dim=1).to(dev)
    assert bool((~keep).any()) and not bool(_bits(got[~keep]).any()), "a padded row of the packed encoding is not +0"
    diff = ((got.float() - want.float()).abs() * keep[..., None]).amax(dim=(1, 2))
    print(f"encodings packed vs dense {dtype}: worst element per sample {diff.tolist()}, kept rows per sample {keep.sum(1).tolist()}")
    assert torch.equal(_bits(got[keep]), _bits(want[keep])), f"kept rows differ from the dense tower's: worst element per sample {diff.tolist()}"


def case_encodings_grad(dev, dtype=F32):
    """return_encodings=True stays differentiable: a gradient on the encoding reaches the tower through pack_rows; padded rows carry none"""
    model, cfg, text, image, _ = build(dev, dtype, "mlm", batch=P.EQ_BATCH)
    model.pack_text_tokens = True
    et, _ = model(text.to(dev), image.to(dev), return_encodings=True)
    et.float().square().sum().backward()
    dE = model.text_transformer.token_emb.weight.grad
    assert float(dE[cfg.text_pad_id].abs().max()) == 0.0 and float(dE[int(text[1, 0])].abs().max()) > 0.0


def case_inference_return(dev, dtype=F32):
    """eval(): the fine-grained similarity [b, t, i] goes through the same unpack -- the dense model's on the kept tokens, 0 on the padded ones"""
    model, cfg, text, image, _ = build(dev, dtype, "filip", batch=P.EQ_BATCH)
    model.eval()
    with torch.no_grad():
        want = model(text.to(dev), image.to(dev))
        model.pack_text_tokens = True
        got = model(text.to(dev), image.to(dev))
        tl, il = model(text.to(dev), image.to(dev), return_latents=True)
    keep = (text != cfg.text_pad_id).to(dev)
    assert got.shape == want.shape and tl.shape == (text.shape[0], text.shape[1], cfg.dim_latent)
    assert float(got[~keep].abs().max()) == 0.0 and float(tl[~keep].abs().max()) == 0.0
    torch.testing.assert_close(got[keep], want[keep], rtol=1e-4, atol=1e-5)           # (clip_cases.case_freeze_and_early_returns' similarity bar)


def _same_run(kind, l0, g0, l1, g1, tag):
    """two runs of the same launches.  The CLS and MLM heads: the loss bit for bit, gradients per packed_cases._same_grads.  The fine-grained head
    sums its loss -- and the per-sample segment sums every gradient behind it depends on -- with float atomics (csrc/kernels/filip.h: seg_sum,
    loss), whose order differs between two runs of the SAME launches on the MI355X (the dense model with the attribute never touched against set
    to False gave two different bf16 loss bits there): its loss and all of its gradients are held to _same_grads' rule for atomically summed
    tensors, in fp32 -- in bf16 a last-bit difference of an fp32 sum is either invisible or a whole bf16 ulp, so those kinds run in fp32 here"""
    if not KINDS[kind][0].get("use_all_token_embeds"):
        assert torch.equal(l0, l1), tag
        P._same_grads(g0, g1, True, tag)
        return
    assert l0.dtype == F32 and all(g is None or g.dtype == F32 for g in g0.values()), "fine-grained kinds: fp32 (see above)"
    torch.testing.assert_close(l0, l1, rtol=1e-4, atol=1e-6)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), (tag, k)
        if g0[k] is not None:
            torch.testing.assert_close(g0[k], g1[k], rtol=1e-4, atol=1e-6)


def case_layout_passed_in(dev, dtype, kind, bitwise=True):
    """a layout built from CPU tokens, one built from device tokens and the implicit one: the same run (_same_run)"""
    _, l0, g0 = run(dev, dtype, kind, True, batch=P.EQ_BATCH)
    for src in ("cpu", "dev"):
        _, l1, g1 = run(dev, dtype, kind, True, layout_from=src, batch=P.EQ_BATCH)
        _same_run(kind, l0, g0, l1, g1, ("tokens layout", kind, src))


def case_checkpoint(dev, dtype, kind, bitwise=True):
    _, la, ga = run(dev, dtype, kind, True, batch=P.EQ_BATCH)
    _, lb, gb = run(dev, dtype, kind, True, batch=P.EQ_BATCH, checkpoint_during_training=True)
    _same_run(kind, la, ga, lb, gb, ("tokens checkpoint", kind))


def text_256_rows(cfg, text):
    """batch 8 of CFG1 (32 tokens): kept tokens 32, 30, 31, 31, 32, 30, 31, 31 + 8 CLS rows = 256 rows exactly"""
    text = torch.where(text == cfg.text_pad_id, torch.ones_like(text), text)
    for r, drop in enumerate((0, 2, 1, 1, 0, 2, 1, 1)):
        if drop:
            text[r, -drop:] = cfg.text_pad_id
    return text


def case_row_multiple(dev, dtype=F32, kind="mlm_filip"):
    """row_multiple = 256 with a kept count that is a multiple already: the unbucketed layout tensors, loss bits and gradients; and with filler
    rows (row_multiple = 256 on the ragged batch) the fp32 oracle bars (loss 1e-5, gradients 2e-4): the products contract over another row
    count, so their fp32 sums may be split elsewhere -- filler rows reach neither head"""
    cfg, _, text, _, _, _, _ = setup(kind, dtype, 8, text_256_rows)
    a, b = text_layout(text, pad_id=cfg.text_pad_id), text_layout(text, pad_id=cfg.text_pad_id, row_multiple=256)
    assert a.R == a.kept == b.R == b.kept == 256 and all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("cu", "pos", "tok"))
    _, l0, g0 = run(dev, dtype, kind, True, batch=8, pad=text_256_rows)
    _, l1, g1 = run(dev, dtype, kind, True, batch=8, pad=text_256_rows, row_multiple=256)
    _same_run(kind, l0, g0, l1, g1, "tokens row_multiple, no filler")
    _, l2, g2 = run(dev, dtype, kind, True, batch=P.EQ_BATCH)
    _, l3, g3 = run(dev, dtype, kind, True, batch=P.EQ_BATCH, row_multiple=256)
    assert abs(float(l2) - float(l3)) <= 1e-5 * max(1.0, abs(float(l2))), (float(l2), float(l3))
    for k in g2:
        if g2[k] is not None:
            rel = float((g2[k].double() - g3[k].double()).norm() / g2[k].double().norm().clamp_min(1e-30))
            assert rel < 2e-4 or float(g2[k].abs().max()) == 0.0, (k, rel)


def case_off_is_unchanged(dev, dtype, kind, bitwise=True):
    """the attribute never touched against set to False: the same bits; a layout passed with it off is refused"""
    _, l0, g0 = run(dev, dtype, kind, None, batch=P.EQ_BATCH)
    model, l1, g1 = run(dev, dtype, kind, False, batch=P.EQ_BATCH)
    assert model.pack_text_tokens is False
    _same_run(kind, l0, g0, l1, g1, ("tokens off", kind))
    _, cfg, text, image, kw = build(dev, dtype, kind, batch=P.EQ_BATCH)
    with pytest.raises(ValueError, match="pack_text"):
        model(text.to(dev), image.to(dev), return_loss=True, text_layout=text_layout(text), **kw)


def case_one_layout(dev, dtype=F32, kind="mlm"):
    """one layout serves the MLM pass and the contrastive pass: with text_layout= built from CPU tokens the step builds none (no read of a
    row count) and the MLM pass receives that layout with the masked ids; implicit, the step builds exactly one"""
    model, cfg, text, image, kw = build(dev, dtype, kind, batch=P.EQ_BATCH)
    model.pack_text_tokens = True
    passed = text_layout(text, pad_id=cfg.text_pad_id)
    seen, built = [], []
    real_mlm, real_layout = model.mlm.forward, packing.text_layout

    def mlm_forward(seq, layout=None, **k):
        seen.append(layout)
        return real_mlm(seq, layout=layout, **k)

    def counted(*a, **k):
        built.append(1)
        return real_layout(*a, **k)

    model.mlm.forward = mlm_forward
    packing.text_layout = counted
    try:
        model(text.to(dev), image.to(dev), return_loss=True, text_layout=passed, **kw).backward()
        assert built == [] and len(seen) == 1
        got = seen[0]
        assert got is passed or all(torch.equal(getattr(got, f).cpu(), getattr(passed, f)) for f in ("cu", "pos", "tok"))
        assert (got.R, got.kept, got.max_len, got.batch, got.n) == (passed.R, passed.kept, passed.max_len, passed.batch, passed.n)
        model.zero_grad(set_to_none=True)
        model(text.to(dev), image.to(dev), return_loss=True, **kw).backward()
        assert built == [1] and len(seen) == 2 and seen[1] is not None
    finally:
        packing.text_layout = real_layout
        del model.mlm.forward


def case_mlm_only_pool_last(dev, dtype=F32):
    """an MLM-only model: the contrastive pass is the CLS head and follows pack_text_pool_last (one pooled packed last layer per step), the MLM
    pass does not; against the oracle under the variant's bars"""
    calls = []
    real = XF._layer_forward_pooled

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    XF._layer_forward_pooled = counted
    try:
        case_vs_oracle(dev, dtype, "mlm", pool_last=True)
    finally:
        XF._layer_forward_pooled = real
    assert len(calls) == 1, len(calls)


def case_switches(dev):
    """every raise of the interface, by message"""
    base = O.CFG1.ctor_kwargs()
    filip = CLIP(**dict(base, use_all_token_embeds=True))
    assert filip.pack_text_tokens is False
    with pytest.raises(NotImplementedError, match="use_all_token_embeds"):
        filip.pack_text = True                                   # pack_text itself goes on refusing these models
    filip.pack_text_tokens = True
    assert filip.pack_text_tokens is True and filip.pack_text is False
    for other in ("pack_text", "pack_text_causal", "pack_text_rotary"):      # a second packing attribute
        with pytest.raises(ValueError, match="pack_text_tokens"):
            setattr(filip, other, True)
        assert getattr(filip, other) is False
    plain = CLIP(**base)
    with pytest.raises(ValueError, match="pack_text"):
        plain.pack_text_tokens = True                            # neither head: pointed at pack_text
    plain.pack_text = True
    with pytest.raises(ValueError, match="pack_text"):
        plain.pack_text_tokens = True
    assert plain.pack_text_tokens is False
    rot = CLIP(**dict(base, use_mlm=True, text_rotary_pos_emb=True))
    rot.pack_text_tokens = True                                  # rotary positions are accepted
    for over, name in ((dict(text_has_cls_token=False), "text_has_cls_token"), (dict(text_encode_without_mask=True), "text_encode_without_mask")):
        m = CLIP(**dict(base, use_all_token_embeds=True, **over))
        with pytest.raises(NotImplementedError, match=name):
            m.pack_text_tokens = True
        assert m.pack_text_tokens is False

    class Plug(torch.nn.Module):
        def forward(self, x, mask=None):
            return torch.zeros(x.shape[0], x.shape[1] + 1, O.CFG1.dim_text)
    with pytest.raises(NotImplementedError, match="text_encoder"):
        CLIP(**dict(base, use_all_token_embeds=True, text_encoder=Plug())).pack_text_tokens = True
    from x_clip_amd import TextTransformer
    cfg, _, text, image, _, _, _ = setup("filip", F32)
    for kw, name in ((dict(attn_dropout=0.1), "attn_dropout"), (dict(ff_dropout=0.1), "ff_dropout")):
        enc = TextTransformer(dim=cfg.dim_text, num_tokens=cfg.num_text_tokens, max_seq_len=cfg.text_seq_len, depth=1, heads=2, dim_head=32, **kw)
        m = CLIP(**dict(base, use_all_token_embeds=True, text_encoder=enc)).train()
        with pytest.raises(NotImplementedError, match=name):
            m.pack_text_tokens = True
        m.eval()
        m.pack_text_tokens = True                                # (no dropout in eval mode) ... and checked again at the call, in train mode
        m.train()
        with pytest.raises(NotImplementedError, match=name):
            m.to(dev)(text.to(dev), image.to(dev), return_loss=True)
    with pytest.raises(ValueError, match="text_layout was built"):
        filip.to(dev).train()(text.to(dev), image.to(dev), return_loss=True, text_layout=text_layout(text[:, :-1]))


def case_adamw_step(dev):
    """one FusedAdamW step on the bf16 FILIP model: finite, bf16 parameters equal their rounded masters (packed_cases.case_adamw_steps)"""
    model, cfg, text, image, kw = build(dev, BF16, "filip")
    model.pack_text_tokens = True
    opt = FusedAdamW(FusedAdamW.default_param_groups(model), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    model(text.to(dev), image.to(dev), return_loss=True, **kw).backward()
    opt.step()
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if p in opt.state and "master" in opt.state[p]:
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16)), k
