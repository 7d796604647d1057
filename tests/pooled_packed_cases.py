"""Shared cases of the packed text tower's pooled last layer (CLIP.pack_text_pool_last): the one-query varlen attention kernels
(csrc/kernels/attention_pool.h, the packed wrappers) and xclip_rows_add_at against fp64 / bit references, and the public interface end to end.
tests/test_pooled_packed_emu.py runs them on the CPU emulator build, tests/test_pooled_packed_gpu.py on an MI355X.

Bars: the kernels hold kernel_cases.case_attention_pool's (out 2 bf16 ulps of the scale / 2e-5, lse the fp32 bar, dq / dkv 2 ulps / 6e-5); end to end
against the oracle packed_cases.case_vs_oracle's (fp32 loss 1e-5, gradients 3e-4; bf16 3e-4, 8 % with cosine 0.999), against the packed tower with the
dense last layer clip_cases._pruned_compare's (fp32 loss 1e-6, gradients 1e-5 of the norm; bf16 2e-3 / 4 %, scalars 10 %)."""
import pytest
import torch

import cached_cases as CC
import clip_cases as C
import kernel_cases as K
import packed_cases as P
from oracle import clip_oracle as O
from x_clip_amd import CachedContrastiveStep, FusedAdamW, _lib, ops, text_layout
from x_clip_amd import functional as XF

F32, BF16 = P.F32, P.BF16
GUARD = P.GUARD
# a length on each side of every multiple of KPL in {2, 4, 8} (keys per wave-wide load: fp32 slot 128, fp32 slot 64 / bf16 slot 128, bf16 slot 64) up
# to 16: every partial last load is hit; eleven samples x 2 heads leave the last four-wave work-group partly empty (as nine do in LENS_A)
LENS_KPL = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
LENS_HOLE = (3, 9, 0, 5, 1)                        # a unit of length 0 between two others


# ---- the one-query varlen attention ---------------------------------------------------------------------------------------------------------
def pool_varlen_launch(q, kv, dout, cu, heads, slot, scale):
    """both entry points through the C ABI into NaN-poisoned buffers with GUARD rows behind row R of dkv and behind row B of out / lse / dq
    -> (out, lse, dq, dkv) without the guards, after checking that every guard element kept its poison bit for bit"""
    L = _lib.lib()
    (R, _), B, dev, dt = kv.shape, q.shape[0], q.device, q.dtype
    inner = heads * slot
    out, dq = P._poison((B + GUARD, inner), dt, dev), P._poison((B + GUARD, inner), dt, dev)
    lse = P._poison((B * heads + GUARD,), F32, dev)
    dkv = P._poison((R + GUARD, 2 * inner), dt, dev)
    guards = lambda: (out[B:], lse[B * heads:], dq[B:], dkv[R:])
    want = [P._bits(t).clone() for t in guards()]
    code, st = ops.dtype_code(q), ops._stream(q)
    _lib.check(L.xclip_attention_pool_varlen_fwd(q.data_ptr(), kv.data_ptr(), cu.data_ptr(), out.data_ptr(), lse.data_ptr(), R, B, heads, slot, scale,
                                                 code, st), "xclip_attention_pool_varlen_fwd")
    _lib.check(L.xclip_attention_pool_varlen_bwd(q.data_ptr(), kv.data_ptr(), cu.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                 dq.data_ptr(), dkv.data_ptr(), R, B, heads, slot, scale, code, st), "xclip_attention_pool_varlen_bwd")
    for name, t, w in zip(("out", "lse", "dq", "dkv"), guards(), want):
        assert torch.equal(P._bits(t), w), f"pooled varlen attention wrote behind the last row of {name}"
    got = out[:B], lse[:B * heads].view(B, heads), dq[:B], dkv[:R]
    for name, t in zip(("out", "lse", "dq", "dkv"), got):
        assert bool(torch.isfinite(t).all()), f"{name}: a row below the guards is not finite (never written?)"
    return got


def pool_varlen_data(lens, heads, slot, dim_head, dtype, dev, seed=0):
    """packed qkv rows as packed_cases.varlen_data draws them -> (qkv [R, 3 inner] for the reference, q of the samples' first rows, kv, dout [B, inner]);
    a sample of length 0 owns no row: its query is drawn on its own"""
    qkv, _ = P.varlen_data(lens, heads, slot, dim_head, dtype, dev, seed)
    g = torch.Generator().manual_seed(9300 + seed)
    inner, B = heads * slot, len(lens)
    dout = P._nonzero_randn((B, inner), g, dtype).to(dev)
    q = P._nonzero_randn((B, heads, slot), g, dtype)
    q[..., dim_head:] = 0
    q = q.view(B, inner).to(dev)
    cu = P._cu(lens, dev)
    live = torch.tensor([n > 0 for n in lens], device=dev)
    if bool(live.any()):
        q[live] = qkv[cu[:-1].long()[live], :inner]
    return qkv, q.contiguous(), qkv[:, inner:].contiguous(), dout


def pool_varlen_reference(qkv, q, dout, lens, heads, slot, scale):
    """kernel_cases.attention_ref_blocked restricted to query row 0, per group of equal-length samples -> (out, lse, dq, dkv) fp64; a sample of
    length 0 keeps zeros everywhere (the kernels' "no visible key" convention)"""
    (R, w), dev, B, inner = qkv.shape, qkv.device, len(lens), heads * slot
    out = torch.zeros(B, inner, dtype=torch.float64, device=dev)
    lse = torch.zeros(B, heads, dtype=torch.float64, device=dev)
    dq = torch.zeros(B, inner, dtype=torch.float64, device=dev)
    dkv = torch.zeros(R, 2 * inner, dtype=torch.float64, device=dev)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    for n in sorted(set(lens) - {0}):
        who = torch.tensor([s for s in range(B) if lens[s] == n], device=dev)
        rows = torch.cat([torch.arange(starts[s], starts[s] + n) for s in who.tolist()]).to(dev)
        o, l, gq = K.attention_ref_blocked(qkv[rows].view(-1, n, w), dout[who], None, heads, scale, hd=slot, query_row=0)
        assert float(gq[:, 1:, :inner].abs().max() if n > 1 else 0.0) == 0.0      # (the reference's dQ is zero off the pooled row)
        out[who], lse[who], dq[who] = o, l, gq[:, 0, :inner]
        dkv[rows] = gq[:, :, inner:].reshape(-1, 2 * inner)
    return out, lse, dq, dkv


def check_pool_varlen(got, want, dtype, tag):
    (out, lse, dq, dkv), (r_out, r_lse, r_dq, r_dkv) = got, want
    K.close(out, r_out, dtype, f"pooled varlen attn out {tag}", ulps=2.0, unit="scale")
    K.close(lse, r_lse, F32, f"pooled varlen attn lse {tag}" + (" <- bf16" if dtype == BF16 else ""))
    K.close(dq, r_dq, dtype, f"pooled varlen attn dq {tag}", mult=3.0, ulps=2.0, unit="scale")
    K.close(dkv, r_dkv, dtype, f"pooled varlen attn dkv {tag}", mult=3.0, ulps=2.0, unit="scale")


def case_pool_varlen(dev, dtype, lens, heads, slot, dim_head, seed=0):
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, dim_head, dtype, dev, seed)
    scale = dim_head ** -0.5
    got = pool_varlen_launch(q, kv, dout, P._cu(lens, dev), heads, slot, scale)
    check_pool_varlen(got, pool_varlen_reference(qkv, q, dout, lens, heads, slot, scale), dtype, f"lens {lens[:4]}.. h{heads} slot{slot}/{dim_head}")
    return got


def case_pool_varlen_empty_unit(dev, dtype, heads=2, slot=64):
    """a cu with one unit of length 0 in the middle: out = 0, lse = 0, dq = 0 for it, bit for bit; its neighbours' rows are their own results (the
    reference check) -- and the launch without the empty unit gives them the same bits"""
    lens = LENS_HOLE
    hole = lens.index(0)
    out, lse, dq, dkv = case_pool_varlen(dev, dtype, lens, heads, slot, slot, seed=2)
    for name, t in (("out", out), ("lse", lse), ("dq", dq)):
        assert float(t[hole].abs().max()) == 0.0, f"{name} of the empty unit is not zero"
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed=2)
    keep = [s for s in range(len(lens)) if s != hole]
    o2, l2, q2, k2 = pool_varlen_launch(q[keep].contiguous(), kv, dout[keep].contiguous(), P._cu([lens[s] for s in keep], dev), heads, slot, slot ** -0.5)
    assert torch.equal(o2, out[keep]) and torch.equal(l2, lse[keep]) and torch.equal(q2, dq[keep]) and torch.equal(k2, dkv)


def case_pool_varlen_equals_dense_pool(dev, dtype, B, n, heads, slot):
    """B samples of one length: ops.attention_pool_fwd / _bwd without a mask on the same data viewed as [B, n, ...], within the kernel bars"""
    lens = (n,) * B
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed=3)
    scale = slot ** -0.5
    out, lse, dq, dkv = pool_varlen_launch(q, kv, dout, P._cu(lens, dev), heads, slot, scale)
    d_out, d_lse = ops.attention_pool_fwd(q, kv.view(B, n, -1), None, heads, scale, slot)
    d_dq, d_dkv = ops.attention_pool_bwd(q, kv.view(B, n, -1), None, d_out, dout, d_lse, heads, scale, slot)
    tag = f"== dense pool B{B} n{n} slot{slot}"
    check_pool_varlen((out, lse, dq, dkv), (d_out.double(), d_lse.double(), d_dq.double(), d_dkv.view(B * n, -1).double()), dtype, tag)


EQUAL_BITS_NS = (1, 7, 9, 70)              # one key; a partial and a whole wave-wide load of bf16 slot 64 plus one key; many loads


def case_pool_varlen_equals_dense_pool_bits(dev, dtype, n, slot, B=3, heads=3):
    """B samples of one length, no mask, visible_keys = n: the packed and the dense pooled kernels walk the same keys in the same order --
    out, lse, dq and dkv bit for bit"""
    lens = (n,) * B
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed=3)
    scale = slot ** -0.5
    got = pool_varlen_launch(q, kv, dout, P._cu(lens, dev), heads, slot, scale)
    d_out, d_lse = ops.attention_pool_fwd(q, kv.view(B, n, -1), None, heads, scale, slot)
    d_dq, d_dkv = ops.attention_pool_bwd(q, kv.view(B, n, -1), None, d_out, dout, d_lse, heads, scale, slot)
    for name, a, b in zip(("out", "lse", "dq", "dkv"), got, (d_out, d_lse, d_dq, d_dkv.view(B * n, -1))):
        assert torch.equal(P._bits(a), P._bits(b)), f"{name}: packed and dense pooled differ in bits at n {n} slot {slot}"


PLAIN_ROUTES = ((F32, 64), (F32, 128), (BF16, 128))       # (dtype, slot) that xclip_attention_varlen_* sends to its plain one-wave-per-row kernels
LENS_PLAIN = LENS_KPL + (70,)                             # a one-key unit, partial loads, a whole load plus one, several loads


def case_plain_varlen_equals_pool_varlen_bits(dev, dtype, slot, lens=LENS_PLAIN, heads=3):
    """the plain varlen kernels (packed_cases.varlen_launch, every row a query) and the pooled varlen kernels (the samples' first rows as the
    queries) run ONE key sweep (attention_pool.h ap_fwd_unit / ap_bwd_unit) over the same keys in the same order: on the same packed qkv, with
    dout zero off the first rows, out / lse / dq of the first rows bit for bit.  dK / dV are not compared: the plain kernel sums them over the
    sample's queries."""
    assert (dtype, slot) in PLAIN_ROUTES
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed=4)
    scale, cu, inner = slot ** -0.5, P._cu(lens, dev), heads * slot
    first = cu[:-1].long()
    dout_rows = torch.zeros(qkv.shape[0], inner, dtype=dtype, device=dev)
    dout_rows[first] = dout
    out, lse, dqkv = P.varlen_launch(qkv, dout_rows, cu, max(lens), heads, slot, scale)
    p_out, p_lse, p_dq, _ = pool_varlen_launch(q, kv, dout, cu, heads, slot, scale)
    for name, a, b in (("out", out[first], p_out), ("lse", lse[:, first].t(), p_lse), ("dq", dqkv[first, :inner], p_dq)):
        assert torch.equal(P._bits(a), P._bits(b)), f"{name}: plain and pooled varlen differ in bits at slot {slot} {dtype}"


def case_pool_varlen_full(dev, dtype=BF16, samples=256, heads=8, slot=64, repeats=3):
    """GPU: 2048 (sample, head) units, every unit checked against the fp64 reference evaluated on the device, three launches bit-identical"""
    lens = tuple(P.LENS_A[i % len(P.LENS_A)] for i in range(samples))
    qkv, q, kv, dout = pool_varlen_data(lens, heads, slot, slot, dtype, dev, seed=5)
    scale, cu = slot ** -0.5, P._cu(lens, dev)
    got = pool_varlen_launch(q, kv, dout, cu, heads, slot, scale)
    check_pool_varlen(got, pool_varlen_reference(qkv, q, dout, lens, heads, slot, scale), dtype, f"full {samples} x {heads}")
    for i in range(repeats - 1):
        again = pool_varlen_launch(q, kv, dout, cu, heads, slot, scale)
        for a, b, name in zip(got, again, ("out", "lse", "dq", "dkv")):
            assert torch.equal(a, b), f"{name} differs between launch 0 and {i + 1}"


# ---- rows_add_at ----------------------------------------------------------------------------------------------------------------------------
def case_rows_add_at(dev, dtype, strided, rows_out=12, dim=64):
    """idx hits the first row, the last row and adjacent rows: touched rows are the fp32 sum rounded once, bit for bit; untouched rows, the guard rows
    behind the last one and (strided dst) the columns between the rows keep their bits"""
    ld = dim + (16 if strided else 0)
    idx = torch.tensor([0, 1, 2, 5, rows_out - 2, rows_out - 1], dtype=torch.int32)
    base = K.rnd((rows_out + GUARD, ld), dtype, 71).to(dev)
    src = K.rnd((idx.numel(), dim), dtype, 72).to(dev)
    before = base.clone()
    dst = base[:rows_out, :dim]
    assert dst.stride(0) == ld
    ret = ops.rows_add_at(dst, idx.to(dev), src)
    assert ret.data_ptr() == dst.data_ptr()
    want = before.clone()
    want[idx.long().to(dev), :dim] = (before[idx.long().to(dev), :dim].float() + src.float()).to(dtype)
    assert torch.equal(P._bits(base), P._bits(want)), "rows_add_at: a touched row is not the fp32 sum rounded once, or an untouched element moved"
    assert not torch.equal(P._bits(base[:rows_out]), P._bits(before[:rows_out]))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def run_pooled(dev, dtype, variant, layout_from=None, batch=None, wide=False, attr=True, **ctor):
    """packed_cases.run_model with pack_text on and pack_text_pool_last = attr (None: never touched)"""
    cfg, sd, extra, text, image, aug_t, aug_i = P.small_setup(variant, dtype, batch, wide=wide)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype, **extra, **ctor)
    model.pack_text = True
    if attr is not None:
        model.pack_text_pool_last = attr
    kw = {}
    if aug_t:
        kw.update(aug_text=[a.to(dev) for a in aug_t], aug_image=[a.to(dev) for a in aug_i])
    if layout_from is not None:
        kw["text_layout"] = text_layout(text if layout_from == "cpu" else text.to(dev), pad_id=cfg.text_pad_id)
    loss = model(text.to(dev), image.to(dev), return_loss=True, **kw)
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}


def case_vs_oracle(dev, dtype, variant):
    """packed_cases.case_vs_oracle with the pooled last layer: the same oracle, the same bars"""
    wide = dtype != F32
    key = (variant, dtype, repr(None), None)
    if key not in P._ORACLE:
        P._ORACLE[key] = P.oracle(variant, dtype, wide=wide)
    ref_loss, ref_grads = P._ORACLE[key]
    _, loss, grads = run_pooled(dev, dtype, variant, wide=wide)
    fp32 = dtype == F32
    err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    print(f"pooled packed {variant} {dtype}: loss err {err:.2e}")
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
        print(f"pooled packed {variant} {dtype} {k}: rel {rel:.2e} cos {cos:.6f}")
        assert (rel < 3e-4) if fp32 else (rel < 0.08 and cos > 0.999), (k, rel, cos)
    pad_row = grads["text_transformer.token_emb.weight"][O.CFG1.text_pad_id]
    assert float(pad_row.abs().max()) == 0.0, "the pad id's embedding row received a gradient"


def _f64(grads):
    return {k: (None if g is None else g.detach().double().cpu()) for k, g in grads.items()}


def case_vs_dense_last_layer(dev, dtype, variant="infonce"):
    """against pack_text = True with the dense last layer on the same tokens, within clip_cases._pruned_compare's bars"""
    _, l1, g1 = run_pooled(dev, dtype, variant, batch=P.EQ_BATCH)
    _, l0, g0 = P.run_model(dev, dtype, variant, True, batch=P.EQ_BATCH)
    C._pruned_compare([(float(l1), _f64(g1)), (float(l0), _f64(g0))], dtype, False)


class _Counted:
    """counts the calls of a module-level function while it is wrapped"""

    def __init__(self, mod, name):
        self.mod, self.name, self.real, self.calls = mod, name, getattr(mod, name, None), 0

    def __enter__(self):
        assert self.real is not None, f"{self.mod.__name__}.{self.name} does not exist"

        def counted(*a, **k):
            self.calls += 1
            return self.real(*a, **k)
        setattr(self.mod, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.mod, self.name, self.real)


def case_routing(dev, dtype, bitwise=True):
    """attribute on: the packed pooled body runs once per text pass (twice with checkpointing: its re-run in the backward) and the dense varlen
    attention depth - 1 times; off: never, and loss and gradients are those of a run that never touched the attribute"""
    depth = O.CFG1.text_enc_depth
    for checkpoint in (False, True):
        with _Counted(XF, "_layer_forward_pooled_packed") as body, _Counted(ops, "attention_varlen_fwd") as dense, \
                _Counted(ops, "attention_pool_varlen_fwd") as pooled:
            run_pooled(dev, dtype, "infonce", batch=P.EQ_BATCH, checkpoint_during_training=checkpoint)
        re_run = 2 if checkpoint else 1
        assert body.calls == re_run, (checkpoint, body.calls)
        assert pooled.calls == re_run and dense.calls == (depth - 1) * re_run, (checkpoint, pooled.calls, dense.calls)
    with _Counted(XF, "_layer_forward_pooled_packed") as body, _Counted(ops, "attention_varlen_fwd") as dense:
        _, l0, g0 = run_pooled(dev, dtype, "infonce", batch=P.EQ_BATCH, attr=False)
    assert body.calls == 0 and dense.calls == depth
    _, l1, g1 = P.run_model(dev, dtype, "infonce", True, batch=P.EQ_BATCH)         # the attribute never touched
    assert torch.equal(l0, l1)
    P._same_grads(g0, g1, bitwise, "pool_last off")
    # with pack_text off the attribute is ignored
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype, P.EQ_BATCH)
    res = []
    for attr in (True, None):
        model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype)
        if attr is not None:
            model.pack_text_pool_last = attr
        with _Counted(XF, "_layer_forward_pooled_packed") as body:
            loss = model(text.to(dev), image.to(dev), return_loss=True)
            loss.backward()
        assert body.calls == 0
        res.append((loss.detach(), {k: p.grad for k, p in model.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    P._same_grads(res[0][1], res[1][1], bitwise, "pack_text off")


def case_checkpoint(dev, dtype, bitwise=True):
    _, la, ga = run_pooled(dev, dtype, "infonce", batch=P.EQ_BATCH)
    _, lb, gb = run_pooled(dev, dtype, "infonce", batch=P.EQ_BATCH, checkpoint_during_training=True)
    assert torch.equal(la, lb)
    P._same_grads(ga, gb, bitwise, "checkpoint")


def case_layout_passed_in(dev, dtype, bitwise=True, variants=("infonce", "dcl_multiview")):
    """a layout built from CPU tokens, one built from device tokens and the implicit one: the same bits (also with augmented texts)"""
    for variant in variants:
        _, l0, g0 = run_pooled(dev, dtype, variant, batch=P.EQ_BATCH)
        for src in ("cpu", "dev"):
            _, l1, g1 = run_pooled(dev, dtype, variant, layout_from=src, batch=P.EQ_BATCH)
            assert torch.equal(l0, l1), (variant, src)
            P._same_grads(g0, g1, bitwise, (variant, src))


def case_embed_text(dev, dtype):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", dtype)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, dtype).eval()
    model.pack_text = True
    model.pack_text_pool_last = True
    with _Counted(XF, "_layer_forward_pooled_packed") as body, torch.no_grad():
        tl, _ = model(text.to(dev), image.to(dev), return_latents=True)
        assert torch.equal(model.embed_text(text.to(dev)), tl)
    assert body.calls == 2


def case_cached_step(dev, dtype, cfg=O.CFG1, head="infonce", b=8):
    """CachedContrastiveStep over one slice and over two slices of the same padded batch agree within cached_cases' bars"""
    res = []
    for micro in (b, b // 2):
        model = CC.build(dev, dtype, cfg, head)
        model.pack_text = True
        model.pack_text_pool_last = True
        opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
        step = CachedContrastiveStep(model, opt, micro_batch=micro)
        text, image = CC.batch(cfg, b, dtype)
        with _Counted(XF, "_layer_forward_pooled_packed") as body:
            loss = step.step(P.padded_text(cfg, text).to(dev), image.to(dev))
        assert body.calls >= b // micro
        res.append((float(loss), CC.grads_of(model)))
    (l1, g1), (l2, g2) = res
    CC.compare(f"pooled packed cached {head} two slices vs one", dtype, l2, g2, l1, g1)


def case_adamw_steps(dev):
    cfg, sd, extra, text, image, _, _ = P.small_setup("infonce", BF16)
    model = C.build_clip(cfg, {k: t.float() for k, t in sd.items()}, dev, BF16)
    model.pack_text = True
    model.pack_text_pool_last = True
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
    """GPU: the default architecture (dim 512, depth 6, n = 256) in bf16, at fill ~ 1/8 or (fill = 1) without padding: loss and per-parameter gradient
    norms against pack_text off within packed_cases.case_default_architecture's bars; the peak of allocated memory with the attribute on is below the
    one with it off (pack_text on in both) -- the last layer's tape holds B rows instead of R behind the attention"""
    from x_clip_amd import CLIP
    torch.manual_seed(5)
    model = CLIP(visual_patch_dropout=0.0).to(BF16).to(dev).train()
    g = torch.Generator().manual_seed(6)
    n = model.text_seq_len
    text = torch.randint(1, 10000, (batch, n), generator=g)
    if fill < 1:
        lens = torch.randint(1, int(2 * fill * n), (batch,), generator=g)
        text[torch.arange(n)[None] >= lens[:, None]] = 0
    text, image = text.to(dev), torch.randn(batch, 3, 256, 256, generator=g).to(BF16).to(dev)
    res = {}
    for pack, pool in ((False, False), (True, False), (True, True)):
        model.pack_text, model.pack_text_pool_last = pack, pool
        for _ in range(2):                                       # (the first pass warms the allocator and the workspaces)
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            loss = model(text, image, return_loss=True)
            loss.backward()
            torch.cuda.synchronize()
        res[pack, pool] = (float(loss.detach()), {k: float(p.grad.double().norm()) for k, p in model.named_parameters() if p.grad is not None},
                           torch.cuda.max_memory_allocated())
    (l0, g0, _), (_, _, m_dense), (l1, g1, m_pool) = res[False, False], res[True, False], res[True, True]
    print(f"default architecture b={batch} fill~{fill}: loss {l0:.6f} / {l1:.6f}; peak allocated, packed: dense last {m_dense / 2**20:.0f} -> pooled {m_pool / 2**20:.0f} MiB")
    assert abs(l0 - l1) / max(1.0, abs(l0)) < 3e-4, (l0, l1)
    for k, n0 in g0.items():
        if n0 < 1e-12:
            continue
        assert abs(n0 - g1[k]) / n0 < 0.08, (k, n0, g1[k])
    assert m_pool < m_dense, (m_dense, m_pool)
