"""Shared cases of the packed CAUSAL text tower (CLIP.pack_text_causal; text_layout(eos_id=)): the causal varlen attention kernels against fp64,
against the dense causal kernels and against their own definition (what a row may not see does not move it), the layout that ends every sample
at its first EOS token, and the public interface end to end.  tests/test_causal_packed_emu.py runs them on the CPU emulator build,
tests/test_causal_packed_gpu.py on an MI355X.

Bars: the kernel family's (packed_cases.check_varlen: out 2 ulps of the scale, lse fp32, dqkv mult 3 / 2 ulps) and DESIGN section 7's end to
end (fp32 loss 1e-5, gradients 3e-4; bf16 loss 3e-4, gradients 8 % with cosine 0.999), as packed_cases.case_vs_oracle applies them."""
import dataclasses

import pytest
import torch

import cached_cases as CC
import clip_cases as C
import kernel_cases as K
import packed_cases as P
from oracle import clip_oracle as O
from packed_cases import BF16, F32, GUARD, _bits, _cu, _poison
from packed_sweep_cases import A3_MAX_N, a3_bwd_waves, a3_waves
from x_clip_amd import CLIP, CachedContrastiveStep, FusedAdamW, _lib, ops, text_layout
from x_clip_amd.packing import cat_layouts

EOS = 3


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
def causal_launch(qkv, dout, cu, max_len, heads, slot, scale):
    """packed_cases.varlen_launch for the causal entry points: through the C ABI into NaN-poisoned buffers with GUARD rows behind row R"""
    L = _lib.lib()
    R, dev, dt = qkv.shape[0], qkv.device, qkv.dtype
    inner = heads * slot
    out = _poison((R + GUARD, inner), dt, dev)
    lse = _poison((heads * R + GUARD,), F32, dev)
    dqkv = _poison((R + GUARD, 3 * inner), dt, dev)
    want = [_bits(t).clone() for t in (out[R:], lse[heads * R:], dqkv[R:])]
    code, st = ops.dtype_code(qkv), ops._stream(qkv)
    _lib.check(L.xclip_attention_varlen_causal_fwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), R, cu.numel() - 1, heads, slot,
                                                   max_len, scale, code, st), "xclip_attention_varlen_causal_fwd")
    _lib.check(L.xclip_attention_varlen_causal_bwd(qkv.data_ptr(), cu.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                                   R, cu.numel() - 1, heads, slot, max_len, scale, code, st), "xclip_attention_varlen_causal_bwd")
    for name, t, w in zip(("out", "lse", "dqkv"), (out[R:], lse[heads * R:], dqkv[R:]), want):
        assert torch.equal(_bits(t), w), f"causal varlen attention wrote behind row R of {name}"
    return out[:R], lse[:heads * R].view(heads, R), dqkv[:R]


def causal_reference(qkv, dout, lens, heads, slot, scale):
    """packed_cases.varlen_reference with causal=True: kernel_cases.attention_ref_blocked per group of equal lengths, fp64"""
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
        o, l, gq = K.attention_ref_blocked(qkv[rows].view(-1, n, w), dout[rows].view(-1, n, heads * slot), None, heads, scale, causal=True, hd=slot)
        out[rows] = o.reshape(-1, heads * slot)
        lse[:, rows] = l.permute(1, 0, 2).reshape(heads, -1)
        grad[rows] = gq.reshape(-1, w)
    return out, lse, grad


def case_causal_attention(dev, dtype, lens, heads, slot, dim_head, seed=0, max_len=None, tag=None):
    qkv, dout = P.varlen_data(lens, heads, slot, dim_head, dtype, dev, seed)
    scale = dim_head ** -0.5
    got = causal_launch(qkv, dout, _cu(lens, dev), max(lens) if max_len is None else max_len, heads, slot, scale)
    want = causal_reference(qkv, dout, lens, heads, slot, scale)
    P.check_varlen(got, want, dtype, "causal " + (tag or f"lens {lens[:4]}.. h{heads} slot{slot}/{dim_head}"))
    return qkv, got, want


# every launch size: max_len HELD ABOVE every unit (cat_layouts), through every forward wave count and both sides of each cooperative-tail dip
SIZE_LENS = (1, 33, 65, 2, 64)


def size_max_lens(all_sizes):
    from packed_sweep_cases import FIXED_MAX_LENS, SWEEP_EMU, SWEEP_MAX_LENS
    every = tuple(m for m in SWEEP_MAX_LENS + FIXED_MAX_LENS if m > max(SIZE_LENS))
    assert {a3_waves(m) for m in every} == set(range(2, 10)) and {66, 97, 288} <= set(every)
    return every if all_sizes else tuple(m for m in every if m in SWEEP_EMU or m in (288,))


def case_causal_launch_size(dev, max_len, heads=3):
    """bf16 head-resident launch sized for max_len over units (1, 33, 65, 2, 64) all shorter than it; the unit of length 1 sees one key:
    out = v and lse = scale q.k, whatever the launch"""
    print(f"max_len {max_len}: fwd waves {a3_waves(max_len)}, bwd waves {a3_bwd_waves(max_len)}")
    qkv, (out, lse, _), _ = case_causal_attention(dev, BF16, SIZE_LENS, heads, 64, 64, seed=max_len, max_len=max_len, tag="launch sizes above every unit")
    _check_unit_of_one(qkv, out, lse, 0, heads, 64, 64 ** -0.5)


def _check_unit_of_one(qkv, out, lse, row, heads, slot, scale):
    inner = heads * slot
    q, k, v = (qkv[row, i * inner:(i + 1) * inner] for i in range(3))
    assert torch.equal(_bits(out[row]), _bits(v)), "a query that sees one key returns that key's value, bit for bit"
    want = (q.double().view(heads, slot) * k.double().view(heads, slot)).sum(1) * scale
    K.close(lse[:, row], want, F32, "causal varlen lse of a one-row unit")


def case_causal_length_one_first(dev, dtype, slot):
    """units of length 1 alone and beside longer ones, both forms"""
    for lens in ((1,), (1, 1, 5), (1, 289)):
        if dtype == BF16 and slot == 64 and max(lens) > A3_MAX_N:
            continue
        qkv, (out, lse, _), _ = case_causal_attention(dev, dtype, lens, 2, slot, slot, seed=41)
        _check_unit_of_one(qkv, out, lse, 0, 2, slot, slot ** -0.5)


def case_causal_equals_dense_bits(dev, n, B=2, heads=3, slot=64):
    """bf16, B samples of one length n, max_len = n: out, lse, dqkv of the packed causal kernels equal the dense causal kernels' bit for bit"""
    qkv, dout = P.varlen_data((n,) * B, heads, slot, slot, BF16, dev, seed=3)
    scale = slot ** -0.5
    out, lse, dqkv = causal_launch(qkv, dout, _cu((n,) * B, dev), n, heads, slot, scale)
    d_out, d_lse = ops.attention_fwd(qkv.view(B, n, -1), None, heads, scale, True, slot)
    d_dqkv = ops.attention_bwd(qkv.view(B, n, -1), None, d_out, dout.view(B, n, -1), d_lse, heads, scale, True, slot)
    for name, a, b in (("out", out, d_out.view(B * n, -1)), ("lse", lse, d_lse.permute(1, 0, 2).reshape(heads, B * n)),
                       ("dqkv", dqkv, d_dqkv.view(B * n, -1))):
        assert torch.equal(_bits(a), _bits(b.contiguous())), f"{name}: packed causal and dense causal differ in bits at n {n}"


FORMS = {"resident": (BF16, 64), "plain_fp32": (F32, 64), "plain_wide": (BF16, 128)}


def case_causality(dev, form, n, heads=2):
    """the rule itself, against no reference.  A unit of n rows between two others.
    (a) q, k, v of every row BEHIND row r replaced: out and lse of the rows <= r keep their bits;
    (b) dout non-zero on row i alone: dK, dV of every row > i are exactly zero, and dQ of every row != i"""
    dtype, slot = FORMS[form]
    lens = (5, n, 3)
    lo = lens[0]
    qkv, dout = P.varlen_data(lens, heads, slot, slot, dtype, dev, seed=n)
    other, _ = P.varlen_data(lens, heads, slot, slot, dtype, dev, seed=n + 1000)
    cu, scale, inner = _cu(lens, dev), slot ** -0.5, heads * slot
    out, lse, _ = causal_launch(qkv, dout, cu, max(lens), heads, slot, scale)
    for r in sorted({0, 1, 30, 31, 32, n - 2} & set(range(n - 1))):
        moved = qkv.clone()
        moved[lo + r + 1: lo + n] = other[lo + r + 1: lo + n]
        o2, l2, _ = causal_launch(moved, dout, cu, max(lens), heads, slot, scale)
        keep = slice(0, lo + r + 1)
        assert torch.equal(_bits(o2[keep]), _bits(out[keep])) and torch.equal(_bits(l2[:, keep]), _bits(lse[:, keep])), \
            f"{form} n {n}: rows behind row {r} moved a row at or in front of it"
        assert torch.equal(_bits(o2[lo + n:]), _bits(out[lo + n:])), "another sample moved"
    for i in sorted({0, 31, 32, n - 2, n - 1} & set(range(n))):
        one = torch.zeros_like(dout)
        one[lo + i] = dout[lo + i]
        _, _, dqkv = causal_launch(qkv, one, cu, max(lens), heads, slot, scale)
        dq, dk, dv = (dqkv[lo: lo + n, j * inner:(j + 1) * inner] for j in range(3))
        assert float(dk[i + 1:].abs().max() if i + 1 < n else 0.0) == 0.0 and float(dv[i + 1:].abs().max() if i + 1 < n else 0.0) == 0.0, \
            f"{form} n {n}: a key behind query {i} received a gradient"
        rest = torch.cat([dq[:i], dq[i + 1:]])
        assert float(rest.abs().max()) == 0.0, f"{form} n {n}: a query other than {i} received a gradient"
        assert float(dq[i].abs().max()) > 0.0 or i == 0          # (row 0 sees one key: its softmax is constant, dQ = 0)
        assert float(dqkv[:lo].abs().max()) == 0.0 and float(dqkv[lo + n:].abs().max()) == 0.0, "another sample received a gradient"


def case_plain_and_resident_agree(dev, heads=2):
    """the same bf16 data through both forms: one launch with max_len each side of A3_MAX_N, each within the bars of the fp64 reference"""
    lens = (70, 1, 33)
    for max_len in (A3_MAX_N, A3_MAX_N + 1):
        case_causal_attention(dev, BF16, lens, heads, 64, 64, seed=8, max_len=max_len, tag=f"both forms, max_len {max_len}")


def case_causal_full(dev, dtype=BF16, samples=256, heads=8, slot=64, repeats=3):
    """GPU: packed_cases.case_varlen_full's shape -- every CU busy, every head against fp64 on the device, three launches bit-identical"""
    lens = tuple(P.LENS_A[i % len(P.LENS_A)] for i in range(samples))
    qkv, dout = P.varlen_data(lens, heads, slot, slot, dtype, dev, seed=5)
    scale, cu = slot ** -0.5, _cu(lens, dev)
    got = causal_launch(qkv, dout, cu, max(lens), heads, slot, scale)
    P.check_varlen(got, causal_reference(qkv, dout, lens, heads, slot, scale), dtype, f"causal full {samples} x {heads}")
    for i in range(repeats - 1):
        again = causal_launch(qkv, dout, cu, max(lens), heads, slot, scale)
        for a, b, name in zip(got, again, ("out", "lse", "dqkv")):
            assert torch.equal(_bits(a), _bits(b)), f"{name} differs between launch 0 and {i + 1}"


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
def eos_tokens(E=EOS):
    return torch.tensor([[5, 6, 7, 8, 9, E],        # the EOS is the last token: full length
                         [E, 5, 6, 0, 0, 0],        # the EOS is the first token: a unit of length 1
                         [5, 0, 6, E, 0, 0],        # a pad hole in front of the EOS
                         [5, E, 6, E, 0, 0],        # two EOS tokens: the first wins
                         [5, 6, E, 7, 8, 0]])       # non-pad tokens behind the EOS: dropped


def case_layout(dev):
    tok = eos_tokens()
    a = text_layout(tok, pad_id=0, has_cls=False, eos_id=EOS)
    assert a.cu.tolist() == [0, 6, 7, 10, 12, 15] and a.ends_at_eos and not a.has_cls and (a.R, a.max_len, a.batch, a.n) == (15, 6, 5, 6)
    assert a.pos.tolist() == [0, 1, 2, 3, 4, 5, 0, 0, 2, 3, 0, 1, 0, 1, 2]
    assert a.tok.tolist() == [5, 6, 7, 8, 9, EOS, EOS, 5, 6, EOS, 5, EOS, 5, 6, EOS]
    assert a.pos[(a.cu[1:] - 1).long()].tolist() == [5, 0, 3, 1, 2]      # every sample's first-EOS position
    b = text_layout(tok.to(dev), pad_id=0, has_cls=False, eos_id=EOS)
    assert (a.R, a.max_len, a.ends_at_eos) == (b.R, b.max_len, b.ends_at_eos) and b.cu.device.type == dev.type
    for f in ("cu", "pos", "tok"):
        assert torch.equal(getattr(a, f), getattr(b, f).cpu()), f
    assert a.to(dev).ends_at_eos
    tk, ps = a.keys(10, 6)
    assert torch.equal(tk, a.tok) and torch.equal(ps, a.pos.long())
    for t in (tok, tok.to(dev)):
        no_eos = t.clone()
        no_eos[4, 2] = 9
        with pytest.raises(ValueError, match="eos_id"):
            text_layout(no_eos, pad_id=0, has_cls=False, eos_id=EOS)
        hidden = t != 0
        hidden[3, 1] = False                                     # the mask hides the FIRST EOS of sample 3 (its second one does not count)
        with pytest.raises(ValueError, match="eos_id"):
            text_layout(t, pad_id=0, mask=hidden, has_cls=False, eos_id=EOS)
        with pytest.raises(ValueError, match="has_cls"):
            text_layout(t, pad_id=0, eos_id=EOS)
    two = cat_layouts([a, text_layout(tok[:2], pad_id=0, has_cls=False, eos_id=EOS)])
    assert two.ends_at_eos and two.cu.tolist() == [0, 6, 7, 10, 12, 15, 21, 22] and two.batch == 7
    plain = text_layout(torch.where(tok == 0, tok, tok), pad_id=0, has_cls=False)
    assert not plain.ends_at_eos
    with pytest.raises(ValueError, match="ends_at_eos"):
        cat_layouts([a, plain])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def causal(cfg):
    return dataclasses.replace(cfg, text_causal_mask=True, text_eos_id=EOS, text_has_cls_token=False)


CFG = causal(O.CFG1)
WIDE = causal(P.WIDE)
DEAD_ID = 7            # in the batches below this id stands behind an EOS token only


def eos_text(cfg, text):
    """the five kinds of sample of `eos_tokens`, tiled over the batch, on the random ids of `text` (so an augmented batch differs); the last
    column is padding in every sample -- a position no kept row has -- and DEAD_ID only ever stands behind an EOS"""
    B, n = text.shape
    E, pad = cfg.text_eos_id, cfg.text_pad_id
    t = text.clone()
    t[(t == E) | (t == pad) | (t == DEAD_ID)] = 11
    t[:, n - 1] = pad
    for r in range(B):
        kind = r % 5
        if kind == 0:
            t[r, n - 2] = E                                      # as long as it gets
        elif kind == 1:
            t[r, 0] = E
            t[r, 3:] = pad
        elif kind == 2:
            t[r, 1] = pad
            t[r, 3 + r % 3] = E
            t[r, 4 + r % 3:] = pad
        elif kind == 3:
            t[r, 1 + r % 2] = E
            t[r, 4] = E
            t[r, 5:] = pad
        else:
            t[r, 2] = E
            t[r, 3] = DEAD_ID
            t[r, 5:] = pad
    return t


def _cfg_for(dtype):
    return CFG if dtype == F32 else WIDE


def run(dev, dtype, variant, pack, pool_last=False, layout_from=None, batch=None, cfg=None, **ctor):
    """pack: True / False set the attribute, None leaves it untouched -> (model, loss, grads)"""
    cfg, sd, extra, text, image, aug_t, aug_i = P.small_setup(variant, dtype, batch, cfg=cfg or _cfg_for(dtype), pad=eos_text)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **extra, **ctor)
    if pack is not None:
        model.pack_text_causal = pack
    model.pack_text_pool_last = pool_last
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    if layout_from is not None:
        kw["text_layout"] = text_layout(text if layout_from == "cpu" else text.to(dev), pad_id=cfg.text_pad_id, has_cls=False, eos_id=cfg.text_eos_id)
    loss = model(text.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}, text


_ORACLE = {}


def _oracle(variant, dtype):
    if (variant, dtype) not in _ORACLE:
        _ORACLE[(variant, dtype)] = P.oracle(variant, dtype, cfg=_cfg_for(dtype), pad=eos_text)
    return _ORACLE[(variant, dtype)]


def _compare(tag, dtype, loss, grads, ref_loss, ref_grads):
    fp32 = dtype == F32
    err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    print(f"{tag}: loss err {err:.2e}")
    assert err < (1e-5 if fp32 else 3e-4), (tag, float(loss), ref_loss)
    for k, g in grads.items():
        rg = ref_grads.get(k)
        if rg is None or float(rg.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, (tag, k)
            continue
        g, rg = g.double().cpu(), rg.double().cpu()
        assert bool(torch.isfinite(g).all()), (tag, k)
        rel = float((g - rg).norm() / rg.norm())
        cos = float((g * rg).sum() / (g.norm() * rg.norm()))
        print(f"{tag} {k}: rel {rel:.2e} cos {cos:.6f}")
        assert (rel < 3e-4) if fp32 else (rel < 0.08 and cos > 0.999), (tag, k, rel, cos)


def case_vs_oracle(dev, dtype, variant, pool_last):
    ref_loss, ref_grads = _oracle(variant, dtype)
    _, loss, grads, _ = run(dev, dtype, variant, True, pool_last)
    _compare(f"packed causal {variant} {dtype} pool_last={pool_last}", dtype, loss, grads, ref_loss, ref_grads)


def _dead_rows(cfg, texts):
    """(token ids, positions) that only rows behind an EOS, or padded rows, hold"""
    live_tok, live_pos = set(), set()
    all_tok = set()
    for text in texts:
        for row in text.tolist():
            all_tok.update(row)
            for p, t in enumerate(row[: row.index(cfg.text_eos_id) + 1]):
                if t != cfg.text_pad_id:
                    live_tok.add(t)
                    live_pos.add(p)
    return sorted(all_tok - live_tok), sorted(set(range(cfg.text_seq_len)) - live_pos)


def case_vs_dense(dev, dtype, pool_last):
    """the attribute on against off on one model and batch: DESIGN section 7's bars, and zero gradient in BOTH on what only dead rows touch"""
    _, l0, g0, text = run(dev, dtype, "infonce", False)
    _, l1, g1, _ = run(dev, dtype, "infonce", True, pool_last)
    _compare(f"packed causal vs dense causal {dtype} pool_last={pool_last}", dtype, l1, g1, float(l0), {k: v for k, v in g0.items() if v is not None})
    cfg = _cfg_for(dtype)
    dead_tok, dead_pos = _dead_rows(cfg, [text])
    assert DEAD_ID in dead_tok and cfg.text_pad_id in dead_tok and cfg.text_seq_len - 1 in dead_pos
    for g in (g0, g1):
        assert float(g["text_transformer.token_emb.weight"][dead_tok].abs().max()) == 0.0, "a token only dead rows hold received a gradient"
        assert float(g["text_transformer.abs_pos_emb.weight"][dead_pos].abs().max()) == 0.0, "a position only dead rows hold received a gradient"
        assert float(g["text_transformer.token_emb.weight"][cfg.text_eos_id].abs().max()) > 0.0


def case_checkpoint(dev, dtype, bitwise=True):
    _, la, ga, _ = run(dev, dtype, "infonce", True, batch=P.EQ_BATCH)
    _, lb, gb, _ = run(dev, dtype, "infonce", True, batch=P.EQ_BATCH, checkpoint_during_training=True)
    assert torch.equal(la, lb)
    P._same_grads(ga, gb, bitwise, "causal checkpoint")


def case_layout_passed_in(dev, dtype, bitwise=True):
    for variant in ("infonce", "dcl_multiview"):
        _, l0, g0, _ = run(dev, dtype, variant, True, batch=P.EQ_BATCH)
        _, l1, g1, _ = run(dev, dtype, variant, True, layout_from="cpu", batch=P.EQ_BATCH)
        assert torch.equal(l0, l1), variant
        P._same_grads(g0, g1, bitwise, ("causal layout", variant))


def case_embed_text(dev, dtype):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype, cfg=_cfg_for(dtype), pad=eos_text)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype).eval()
    model.pack_text_causal = True
    with torch.no_grad():
        tl, _ = model(text.to(dev), image.to(dev), return_latents=True)
        assert tl.shape == (text.shape[0], cfg.dim_latent) and torch.equal(model.embed_text(text.to(dev)), tl)


def case_cached_step(dev, dtype, head="infonce", b=8):
    """one CachedContrastiveStep.step (two slices) against the one-pass step of the same packed model, cached_cases' bars"""
    cfg = _cfg_for(dtype)
    res = []
    for micro in (None, b // 2):
        model = CC.build(dev, dtype, cfg, head)
        model.pack_text_causal = True
        text, image = CC.batch(cfg, b, dtype)
        text = eos_text(cfg, text)
        if micro is None:
            loss = model(text.to(dev), image.to(dev), return_loss=True)
            loss.backward()
        else:
            opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
            loss = CachedContrastiveStep(model, opt, micro_batch=micro).step(text.to(dev), image.to(dev))
        res.append((float(loss.detach()), CC.grads_of(model)))
    (l1, g1), (l2, g2) = res
    CC.compare(f"packed causal cached {head} vs one pass", dtype, l2, g2, l1, g1)


def case_adamw_steps(dev):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", BF16, cfg=CFG, pad=eos_text)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, BF16)
    model.pack_text_causal = True
    model.pack_text_pool_last = True
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = FusedAdamW(FusedAdamW.default_param_groups(model), lr=1e-3)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        model(text.to(dev), image.to(dev), return_loss=True).backward()
        opt.step()
    for k, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), k
    for k in ("text_transformer.token_emb.weight", "text_transformer.transformer.layers.0.0.fn.to_qkv.weight", "to_text_latent.weight"):
        assert not torch.equal(before[k], dict(model.named_parameters())[k].detach()), f"{k} did not move"


def case_switches(dev):
    base = CFG.ctor_kwargs()
    model = CLIP(**base)
    with pytest.raises(NotImplementedError, match="text_causal_mask"):
        model.pack_text = True                                   # pack_text itself goes on refusing a causal model
    assert model.pack_text is False and model.pack_text_causal is False
    model.pack_text_causal = True
    assert model.pack_text_causal is True
    with pytest.raises(ValueError, match="pack_text"):
        CLIP(**O.CFG1.ctor_kwargs()).pack_text_causal = True     # a CLS-token model

    class Plug(torch.nn.Module):
        def forward(self, x, mask=None):
            return torch.zeros(x.shape[0], x.shape[1], CFG.dim_text)
    with pytest.raises(ValueError, match="pack_text"):
        CLIP(**dict(base, text_encoder=Plug())).pack_text_causal = True
    m = CLIP(**dict(base, text_encode_without_mask=True))
    with pytest.raises(NotImplementedError, match="text_encode_without_mask"):
        m.pack_text_causal = True
    assert m.pack_text_causal is False
    from x_clip_amd import TextTransformer
    for kw, name in ((dict(attn_dropout=0.1), "attn_dropout"), (dict(ff_dropout=0.1), "ff_dropout")):
        enc = TextTransformer(dim=CFG.dim_text, num_tokens=CFG.num_text_tokens, max_seq_len=CFG.text_seq_len, depth=1, heads=2, dim_head=32,
                              causal=True, **kw)
        m = CLIP(**dict(base, text_encoder=enc)).train()
        with pytest.raises(NotImplementedError, match=name):
            m.pack_text_causal = True
        m.eval()
        m.pack_text_causal = True                                # (no dropout in eval mode) ... and checked again at the call, in train mode
        m.train()
        _, _, _, text, image, _, _ = P.small_setup("infonce", F32, cfg=CFG, pad=eos_text)
        with pytest.raises(NotImplementedError, match=name):
            m.to(dev)(text.to(dev), image.to(dev), return_loss=True)
    model = model.to(dev).train()
    _, _, _, text, image, _, _ = P.small_setup("infonce", F32, cfg=CFG, pad=eos_text)
    with pytest.raises(NotImplementedError, match="return_encodings"):
        model(text.to(dev), image.to(dev), return_encodings=True)
    model.pack_text_causal = False
    with pytest.raises(ValueError, match="pack_text"):
        model(text.to(dev), image.to(dev), return_loss=True, text_layout=text_layout(text, has_cls=False, eos_id=EOS))


def case_off_is_unchanged(dev, dtype, bitwise=True):
    _, l0, g0, _ = run(dev, dtype, "infonce", None, batch=P.EQ_BATCH)
    _, l1, g1, _ = run(dev, dtype, "infonce", False, batch=P.EQ_BATCH)
    assert torch.equal(l0, l1)
    P._same_grads(g0, g1, bitwise, "causal off")
