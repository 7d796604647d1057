"""Shared cases of the packed ROTARY text tower (CLIP.pack_text_rotary): xclip_rotary_pos through the C ABI against xclip_rotary (bit for bit on
the kept rows of a ragged layout), against fp64 and against its own definition; the stack and the public interface end to end.
tests/test_rotary_packed_emu.py runs them on the CPU emulator build, tests/test_rotary_packed_gpu.py on an MI355X.

Bars: the kernel is held to xclip_rotary's bits (torch.equal) and, for inverse after forward, to a bound derived below from the roundings it
makes (`inverse_bound`); end to end DESIGN section 7's (fp32 loss 1e-5, gradients 3e-4; bf16 loss 3e-4, gradients 8 % with cosine 0.999), as
packed_cases.case_vs_oracle and causal_packed_cases._compare apply them; run against run of the same launches packed_cases._same_grads."""
import dataclasses
import math

import pytest
import torch

import cached_cases as CC
import clip_cases as C
import packed_cases as P
from causal_packed_cases import _compare
from oracle import clip_oracle as O
from packed_cases import BF16, F32, GUARD, _bits, _poison
from x_clip_amd import CLIP, CachedContrastiveStep, FusedAdamW, _lib, ops, text_layout

GRID_CAP, BLOCK = 8192, 256          # the launch: min(ceil(items / 256), 8192) work-groups of 256 threads, grid-stride beyond


# ---- the kernel, through the C ABI ----------------------------------------------------------------------------------------------------------
def inv_freq(rot, dev):
    return (1.0 / (10000 ** (torch.arange(0, rot, 2).float() / rot))).contiguous().to(dev)


def ragged_tokens():
    """B = 5, 8 tokens behind the CLS row (9 dense rows per sample): kept lengths 1 (all padding), 2, 9, 4 (with a hole in mid-sequence), 9"""
    tok = torch.arange(1, 41).view(5, 8).clone()
    tok[0] = 0
    tok[1, 1:] = 0
    tok[3, 4:] = 0
    tok[3, 1] = 0                                               # the hole: the rows behind it keep their positions
    return tok


def ragged(dev):
    """-> (layout on dev, flat indices of the kept rows in the dense [B n] order, dense rows per sample)"""
    tok = ragged_tokens()
    lay = text_layout(tok, pad_id=0)
    n = tok.shape[1] + 1
    assert (lay.cu[1:] - lay.cu[:-1]).tolist() == [1, 2, 9, 4, 9] and lay.pos[lay.cu[3]: lay.cu[4]].tolist() == [0, 1, 3, 4]
    sample = torch.repeat_interleave(torch.arange(lay.batch), (lay.cu[1:] - lay.cu[:-1]).long())
    return lay.to(dev), (sample * n + lay.pos.long()).to(dev), n


def _launch(fn_name, x, where, slots, w, rot, inverse, ld):
    """x [rows, slots w] copied into the middle of a NaN-poisoned [GUARD + rows + GUARD, ld] buffer and rotated in place through the C ABI;
    the guard rows on both sides and the columns from slots w to ld keep their poison bit for bit -> the rotated [rows, slots w]"""
    L = _lib.lib()
    rows, dev, dt = x.shape[0], x.device, x.dtype
    buf = _poison((GUARD + rows + GUARD, ld), dt, dev)
    buf[GUARD: GUARD + rows, : slots * w] = x
    before = _bits(buf).clone()
    body = buf[GUARD:]
    freq = inv_freq(rot, dev)                                   # (held until the result has been read back)
    args = (body.data_ptr(), ld, rows, where, slots, w, rot, freq.data_ptr(), int(inverse), ops.dtype_code(x), ops._stream(x))
    _lib.check(getattr(L, fn_name)(*args), fn_name)
    after = _bits(buf)
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + rows:], before[GUARD + rows:]), f"{fn_name} wrote a guard row"
    assert torch.equal(after[:, slots * w:], before[:, slots * w:]), f"{fn_name} wrote a padding column"
    out = buf[GUARD: GUARD + rows, : slots * w].clone()
    del freq
    return out


def rotary_pos(x, pos, slots, w, rot, inverse=False, ld=None):
    assert pos.dtype == torch.int32 and pos.numel() == x.shape[0]
    return _launch("xclip_rotary_pos", x, pos.data_ptr(), slots, w, rot, inverse, ld or slots * w)


def rotary_dense(x, n, slots, w, rot, inverse=False, ld=None):
    return _launch("xclip_rotary", x, n, slots, w, rot, inverse, ld or slots * w)


def _data(rows, slots, w, dtype, dev, seed):
    return P._nonzero_randn((rows, slots * w), torch.Generator().manual_seed(7300 + seed), dtype).to(dev)


SHAPES = ((64, 32), (128, 32), (64, 16), (64, 24))              # (slot_width, rot): the chunk path at both widths, the pair path twice


def case_equals_dense_on_kept_rows(dev, dtype, w, rot, slots, pad):
    """the exact bar: xclip_rotary on the dense [B n, slots w] array, its kept rows gathered == xclip_rotary_pos on the same rows packed with
    pos = layout.pos -- forward and inverse, bit for bit; features from rot on pass through bit for bit"""
    lay, kept, n = ragged(dev)
    ld = slots * w + pad
    x = _data(lay.batch * n, slots, w, dtype, dev, seed=w + rot + slots)
    packed = x[kept].contiguous()
    for inverse in (False, True):
        want = rotary_dense(x, n, slots, w, rot, inverse, ld)[kept]
        got = rotary_pos(packed, lay.pos, slots, w, rot, inverse, ld)
        assert torch.equal(_bits(got), _bits(want)), f"xclip_rotary_pos != xclip_rotary on the kept rows ({dtype}, w {w}, rot {rot}, slots {slots}, inverse {inverse})"
        g3, p3 = got.view(-1, slots, w), packed.view(-1, slots, w)
        assert torch.equal(_bits(g3[..., rot:]), _bits(p3[..., rot:])), "a feature at rot or above moved"
        assert not torch.equal(_bits(g3[..., :rot]), _bits(p3[..., :rot]))


def _half_ulp(v, dtype):
    """half the spacing of the storage type at |v| (fp64 in / out): 24 significand bits in fp32, 8 in bf16"""
    p = 24 if dtype == F32 else 8
    return 0.5 * torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - (p - 1))


def inverse_bound(x64, rot, dtype):
    """x64 [rows, slots, w] fp64 -> element-wise bound on |R^T R x - x| as the kernel computes it, two applications.

    One application forms y1 = x1 c - x2 s, y2 = x2 c + x1 s in fp32 -- two products and a sum, three roundings of at most u = 2^-24 relative
    to a magnitude of at most m = |x1| + |x2|: a = 3 u m -- and stores it: half an ulp of the storage type at the stored value.  With
    r = sqrt(x1^2 + x2^2): |y1|, |y2| <= r whatever the angle, and |y1| + |y2| <= sqrt(2) r.
      - the first application's errors (a + half an ulp at r + a, per element of the pair) pass through the second rotation with weights
        |c| + |s| <= sqrt(2) for a and at most 1 each for the two store roundings:   sqrt(2) a + 2 hu(r + a)
      - the second application's arithmetic, on stored values of magnitude <= sqrt(2) r + 2 a + 2 hu(r + a):   3 u (sqrt(2) r + 2 a + 2 hu(r + a))
      - c and s come from one sincosf call per application with the same argument, each within 2 ulps of a value <= 1 (2 u absolute; the bound
        both the device library and glibc document), so R^T R = (c^2 + s^2) I is the identity within 2 (|c| + |s|) 2 u <= 4 sqrt(2) u:
        4 sqrt(2) u |x_i|
      - and the final store: half an ulp at |x_i| + everything above."""
    half = rot // 2
    u = 2.0 ** -24
    x1, x2 = x64[..., :half], x64[..., half:rot]
    m, r = x1.abs() + x2.abs(), torch.sqrt(x1 * x1 + x2 * x2)
    a = 3 * u * m
    hu = _half_ulp(r + a, dtype)
    pair = math.sqrt(2.0) * a + 2 * hu + 3 * u * (math.sqrt(2.0) * r + 2 * a + 2 * hu)
    rest = torch.cat([pair, pair], dim=-1) + 4 * math.sqrt(2.0) * u * x64[..., :rot].abs()
    return rest + _half_ulp(x64[..., :rot].abs() + rest, dtype)


def case_inverse_after_forward(dev, dtype, w, rot, slots=6):
    """R^T R x against x in fp64, element-wise within `inverse_bound`; the features from rot on keep their bits"""
    lay, _, _ = ragged(dev)
    x = _data(lay.R, slots, w, dtype, dev, seed=11 * rot + w)
    y = rotary_pos(x, lay.pos, slots, w, rot)
    z = rotary_pos(y, lay.pos, slots, w, rot, inverse=True)
    x64, z64 = x.double().cpu().view(-1, slots, w), z.double().cpu().view(-1, slots, w)
    bound = inverse_bound(x64, rot, dtype)
    err = (z64[..., :rot] - x64[..., :rot]).abs()
    ratio = float((err / bound).max())
    print(f"rotary_pos inverse after forward {dtype} w {w} rot {rot}: worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"worst error / bound {ratio:.3f}"
    assert torch.equal(_bits(z.view(-1, slots, w)[..., rot:]), _bits(x.view(-1, slots, w)[..., rot:]))
    moved = lay.pos.cpu() > 0                                    # the check sees rotated rows: position 0 alone is the identity
    assert bool(moved.any()) and not torch.equal(_bits(y[moved.to(dev)]), _bits(x[moved.to(dev)]))


def case_position_zero_is_identity(dev, dtype, w, rot, slots=4, rows=7):
    x = _data(rows, slots, w, dtype, dev, seed=rot)
    pos = torch.zeros(rows, dtype=torch.int32, device=dev)
    for inverse in (False, True):
        assert torch.equal(_bits(rotary_pos(x, pos, slots, w, rot, inverse)), _bits(x)), "the angle 0 is the identity: sincosf(0) = (0, 1)"


def case_no_rows(dev, dtype):
    """rows = 0: success, nothing launched, nothing written -- with a real address and with none (an empty tensor's)"""
    x = _data(0, 4, 64, dtype, dev, seed=1)
    pos = torch.zeros(0, dtype=torch.int32, device=dev)
    assert rotary_pos(x, pos, 4, 64, 32).shape == (0, 256)
    assert ops.rotary_pos_(x, pos, inv_freq(32, dev)) is x
    L = _lib.lib()
    assert L.xclip_rotary_pos(None, 256, 0, None, 4, 64, 32, None, 0, ops.dtype_code(x), ops._stream(x)) == 0


def per_slot(dtype, rot):
    """work items of one head slot: pairs of 16-byte chunks on the chunk path (rot 32), element pairs below"""
    return (16 // (8 if dtype == BF16 else 4)) if rot == 32 else rot // 2


def wrap_rows(dtype, rot, slots=2):
    """the smallest row count at which the grid is capped and the grid-stride loop takes a second turn, plus two rows"""
    return GRID_CAP * BLOCK // (slots * per_slot(dtype, rot)) + 3


def case_launch_sizes(dev, dtype, rot, rows, slots=2, w=64, n=77):
    """one row (a single partly filled work-group), or enough rows that the capped grid wraps: every row is rotated once and by its own
    position -- the bits of xclip_rotary with pos[r] = r % n on the same array"""
    items = rows * slots * per_slot(dtype, rot)
    print(f"rows {rows}: {items} items, {min((items + BLOCK - 1) // BLOCK, GRID_CAP)} work-groups, wraps: {items > GRID_CAP * BLOCK}")
    x = _data(rows, slots, w, dtype, dev, seed=rows % 1000)
    pos = (torch.arange(rows, device=dev) % n).to(torch.int32)
    got = rotary_pos(x, pos, slots, w, rot)
    want = rotary_dense(x, n, slots, w, rot)
    assert torch.equal(_bits(got), _bits(want))


def case_ops_wrapper(dev, dtype):
    """ops.rotary_pos_ on a strided view ([R, 2 inner] out of a wider array): in place, the bits of the C call, the neighbour columns untouched"""
    lay, _, _ = ragged(dev)
    full = _data(lay.R, 6, 64, dtype, dev, seed=5)
    view = full[:, 128:]                                        # slots 2 .. 5: ld = 384 > 4 * 64
    want = rotary_pos(view.contiguous(), lay.pos, 4, 64, 32)
    keep = full[:, :128].clone()
    assert ops.rotary_pos_(view, lay.pos, inv_freq(32, dev)) is view
    assert torch.equal(_bits(full[:, 128:]), _bits(want)) and torch.equal(_bits(full[:, :128]), _bits(keep))


# ---- the stack and the model ------------------------------------------------------------------------------------------------------------------
def rotary(cfg, **over):
    return dataclasses.replace(cfg, text_rotary_pos_emb=True, **over)


CFG = rotary(O.CFG1)                                             # fp32: the two-layer dim-64 toy, 64-wide heads (rot 32)
WIDE = rotary(P.WIDE, text_enc_depth=2)                          # bf16: the dim-512 model the bf16 bars are stated for, at depth 2
NARROW = rotary(O.CFG1, text_dim_head=16)                        # rot 16: the pair kernels
SLOT128 = rotary(O.CFG1, text_dim_head=128, text_heads=2)        # 128-wide head slots


def _cfg_for(dtype, cfg=None):
    return cfg if cfg is not None else (CFG if dtype == F32 else WIDE)


def run(dev, dtype, variant, pack, pool_last=False, layout_from=None, batch=None, cfg=None, prune=True, text_edit=None, **ctor):
    """pack: True / False set the attribute, None leaves it untouched; prune = False: the dense last layer (CLIP.prune_unused_rows);
    text_edit(text) -> the token batch handed to forward beside a layout built from the unedited one -> (model, loss, grads, text)"""
    cfg, sd, extra, text, image, aug_t, aug_i = P.small_setup(variant, dtype, batch, cfg=_cfg_for(dtype, cfg))
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **extra, **ctor)
    if pack is not None:
        model.pack_text_rotary = pack
    model.pack_text_pool_last = pool_last
    model.prune_unused_rows = prune
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    if layout_from is not None:
        kw["text_layout"] = text_layout(text if layout_from == "cpu" else text.to(dev), pad_id=cfg.text_pad_id)
    fed = text if text_edit is None else text_edit(text)
    loss = model(fed.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}, text


_ORACLE = {}


def _oracle(variant, dtype, cfg=None):
    key = (variant, dtype, repr(cfg))
    if key not in _ORACLE:
        _ORACLE[key] = P.oracle(variant, dtype, cfg=_cfg_for(dtype, cfg))
    return _ORACLE[key]


def case_vs_oracle(dev, dtype, variant, pool_last, cfg=None):
    """pack_text_rotary against the fp64 oracle (which restates rotary) on the same parameters and padded tokens; the pad id's embedding
    gradient is exactly zero"""
    ref_loss, ref_grads = _oracle(variant, dtype, cfg)
    _, loss, grads, _ = run(dev, dtype, variant, True, pool_last, cfg=cfg)
    _compare(f"packed rotary {variant} {dtype} pool_last={pool_last} dim_head={_cfg_for(dtype, cfg).text_dim_head}", dtype, loss, grads, ref_loss, ref_grads)
    assert float(grads["text_transformer.token_emb.weight"][_cfg_for(dtype, cfg).text_pad_id].abs().max()) == 0.0, "the pad id's embedding row received a gradient"


def case_vs_dense(dev, dtype, pool_last, cfg=None, variant="infonce"):
    """the attribute on against the dense rotary tower with the dense last layer (prune_unused_rows = False), one model and batch"""
    _, l0, g0, _ = run(dev, dtype, variant, False, prune=False, cfg=cfg)
    _, l1, g1, _ = run(dev, dtype, variant, True, pool_last, cfg=cfg)
    _compare(f"packed rotary vs dense rotary {variant} {dtype} pool_last={pool_last} dim_head={_cfg_for(dtype, cfg).text_dim_head}", dtype, l1, g1, float(l0),
             {k: v.double().cpu() for k, v in g0.items() if v is not None})


def case_checkpoint(dev, dtype, bitwise=True):
    _, la, ga, _ = run(dev, dtype, "infonce", True, batch=P.EQ_BATCH)
    _, lb, gb, _ = run(dev, dtype, "infonce", True, batch=P.EQ_BATCH, checkpoint_during_training=True)
    assert torch.equal(la, lb)
    P._same_grads(ga, gb, bitwise, "rotary checkpoint")


def case_layout_passed_in(dev, dtype, bitwise=True, variants=("infonce", "dcl_multiview"), pool_last=False):
    """a layout built from CPU tokens and the implicit one: the same bits (also with an augmented text: two layouts concatenated)"""
    for variant in variants:
        _, l0, g0, _ = run(dev, dtype, variant, True, pool_last, batch=P.EQ_BATCH)
        _, l1, g1, _ = run(dev, dtype, variant, True, pool_last, layout_from="cpu", batch=P.EQ_BATCH)
        assert torch.equal(l0, l1), variant
        P._same_grads(g0, g1, bitwise, ("rotary layout", variant))


DEAD_ID = 999          # no batch below holds this id on a kept row


def case_dead_rows(dev, dtype, pool_last):
    """the token ids of the positions the layout drops are never read: with DEAD_ID written over every padded position of the batch handed to
    forward (the layout still that of the padding) no output bit moves, and DEAD_ID's and the pad id's embedding rows get exactly zero gradient"""
    cfg = _cfg_for(dtype)

    def edit(text):
        assert not bool((text == DEAD_ID).any()) and bool((text == cfg.text_pad_id).any())
        return torch.where(text == cfg.text_pad_id, torch.full_like(text, DEAD_ID), text)
    _, l0, g0, text = run(dev, dtype, "infonce", True, pool_last, layout_from="cpu", batch=P.EQ_BATCH)
    _, l1, g1, _ = run(dev, dtype, "infonce", True, pool_last, layout_from="cpu", batch=P.EQ_BATCH, text_edit=edit)
    assert torch.equal(l0, l1), "a token id on a dropped row moved the loss"
    P._same_grads(g0, g1, True, "rotary dead rows")
    same = text_layout(edit(text), pad_id=cfg.text_pad_id, mask=text != cfg.text_pad_id)
    want = text_layout(text, pad_id=cfg.text_pad_id)
    assert all(torch.equal(getattr(same, f), getattr(want, f)) for f in ("cu", "pos", "tok"))
    for g in (g0, g1):
        dE = g["text_transformer.token_emb.weight"]
        assert float(dE[[cfg.text_pad_id, DEAD_ID]].abs().max()) == 0.0, "a token only dropped rows hold received a gradient"
        assert float(dE[int(text[1, 0])].abs().max()) > 0.0


def case_embed_text(dev, dtype, pool_last=False):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype, cfg=_cfg_for(dtype))
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype).eval()
    model.pack_text_rotary = True
    model.pack_text_pool_last = pool_last
    with torch.no_grad():
        tl, _ = model(text.to(dev), image.to(dev), return_latents=True)
        assert tl.shape == (text.shape[0], cfg.dim_latent) and torch.equal(model.embed_text(text.to(dev)), tl)


def case_cached_step(dev, dtype, head="infonce", b=8):
    """one CachedContrastiveStep.step (two slices) against the one-pass step of the same packed model, cached_cases' bars"""
    cfg = _cfg_for(dtype)
    res = []
    for micro in (None, b // 2):
        model = CC.build(dev, dtype, cfg, head)
        model.pack_text_rotary = True
        text, image = CC.batch(cfg, b, dtype)
        text = P.padded_text(cfg, text)
        if micro is None:
            loss = model(text.to(dev), image.to(dev), return_loss=True)
            loss.backward()
        else:
            opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
            loss = CachedContrastiveStep(model, opt, micro_batch=micro).step(text.to(dev), image.to(dev))
        res.append((float(loss.detach()), CC.grads_of(model)))
    (l1, g1), (l2, g2) = res
    CC.compare(f"packed rotary cached {head} vs one pass", dtype, l2, g2, l1, g1)


def case_switches(dev):
    """every raise of the interface, by message"""
    base = CFG.ctor_kwargs()
    model = CLIP(**base)
    assert model.pack_text_rotary is False and model.pack_text is False and model.pack_text_causal is False
    with pytest.raises(NotImplementedError, match="text_rotary_pos_emb"):
        model.pack_text = True                                   # pack_text itself goes on refusing a rotary model
    assert model.pack_text is False
    model.pack_text_rotary = True
    assert model.pack_text_rotary is True
    for other in ("pack_text", "pack_text_causal"):              # two of the three at once
        with pytest.raises(ValueError, match="pack_text_rotary"):
            setattr(model, other, True)
        assert getattr(model, other) is False
    plain = CLIP(**O.CFG1.ctor_kwargs())
    with pytest.raises(ValueError, match="pack_text"):
        plain.pack_text_rotary = True                            # a CLS-token model with a position table
    plain.pack_text = True
    with pytest.raises(ValueError, match="pack_text"):
        plain.pack_text_rotary = True
    assert plain.pack_text_rotary is False
    with pytest.raises(ValueError, match="pack_text_causal"):
        CLIP(**dataclasses.replace(O.CFG1, text_causal_mask=True, text_eos_id=3, text_has_cls_token=False).ctor_kwargs()).pack_text_rotary = True

    class Plug(torch.nn.Module):
        def forward(self, x, mask=None):
            return torch.zeros(x.shape[0], x.shape[1] + 1, CFG.dim_text)
    with pytest.raises(ValueError, match="pack_text"):
        CLIP(**dict(base, text_encoder=Plug())).pack_text_rotary = True
    for over, name in ((dict(use_all_token_embeds=True), "use_all_token_embeds"), (dict(use_mlm=True), "use_mlm"),
                       (dict(text_has_cls_token=False), "text_has_cls_token"), (dict(text_encode_without_mask=True), "text_encode_without_mask")):
        m = CLIP(**dict(base, **over))
        with pytest.raises(NotImplementedError, match=name):
            m.pack_text_rotary = True
        assert m.pack_text_rotary is False
    from x_clip_amd import TextTransformer
    _, _, _, text, image, _, _ = P.small_setup("infonce", F32, cfg=CFG)
    for kw, name in ((dict(attn_dropout=0.1), "attn_dropout"), (dict(ff_dropout=0.1), "ff_dropout")):
        enc = TextTransformer(dim=CFG.dim_text, num_tokens=CFG.num_text_tokens, max_seq_len=CFG.text_seq_len, depth=1, heads=2, dim_head=32,
                              rotary_pos_emb=True, **kw)
        m = CLIP(**dict(base, text_encoder=enc)).train()
        with pytest.raises(NotImplementedError, match=name):
            m.pack_text_rotary = True
        m.eval()
        m.pack_text_rotary = True                                # (no dropout in eval mode) ... and checked again at the call, in train mode
        m.train()
        with pytest.raises(NotImplementedError, match=name):
            m.to(dev)(text.to(dev), image.to(dev), return_loss=True)
    model = model.to(dev).train()
    with pytest.raises(NotImplementedError, match="return_encodings"):
        model(text.to(dev), image.to(dev), return_encodings=True)
    model.pack_text_rotary = False
    with pytest.raises(ValueError, match="pack_text"):
        model(text.to(dev), image.to(dev), return_loss=True, text_layout=text_layout(text))


def case_stack_guards(dev):
    """functional.text_encode_packed: rotary beside a position table, or on a layout without CLS rows, is refused"""
    from x_clip_amd import functional as XF
    D, heads = 64, 2
    spec = XF.StackSpec(depth=0, heads=heads, dim_head=32, rotary=inv_freq(32, dev))
    E, Ptab, cls, g = (torch.zeros(s, device=dev) for s in ((10, D), (9, D), (D,), (D,)))
    tok = ragged_tokens()
    with pytest.raises(NotImplementedError, match="text_rotary_pos_emb"):
        XF.text_encode_packed(text_layout(tok).to(dev), E, Ptab, cls, [g, g], spec)
    with pytest.raises(ValueError, match="CLS row"):
        XF.text_encode_packed(text_layout(torch.where(tok == 0, 1, tok), has_cls=False).to(dev), E, None, cls, [g, g], spec)


def case_off_is_unchanged(dev, dtype, bitwise=True):
    """the attribute never touched against set to False: the same bits; and the rotary model with it off against the reference's own numbers
    (the fixture cfg1_rotary.json, at the bars of tests/test_clip_emu.py's fixture test)"""
    _, l0, g0, _ = run(dev, dtype, "infonce", None, batch=P.EQ_BATCH)
    model, l1, g1, _ = run(dev, dtype, "infonce", False, batch=P.EQ_BATCH)
    assert model.pack_text_rotary is False and torch.equal(l0, l1)
    P._same_grads(g0, g1, bitwise, "rotary off")


def case_off_matches_reference_fixture(dev):
    assert O.ClipConfig(**C.load_golden("cfg1_rotary")["config"]).text_rotary_pos_emb
    C.case_golden(dev, "cfg1_rotary")
