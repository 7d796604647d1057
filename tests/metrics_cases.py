"""Shared cases of the in-batch retrieval metrics (x_clip_amd.metrics, ops.simrank*, csrc/kernels/simrank.h): the CPU suite runs them on
the wave64 emulator (tests/test_metrics_emu.py), the GPU suite on the MI355X (tests/test_metrics_gpu.py).  The reference is plain dense
torch in fp64 on the dtype-rounded inputs.

Exact cases: entries from {-3 .. 3} / 8 and d <= 128 make every dot product exact in fp32 in any summation order; the one rounding left
is the product with the scale, which IEEE fixes.  Ties are frequent by construction, so every row pins the strict comparison and the
lowest-column rule.  Realistic cases: the fp32 accumulation bound
    eps_i = d 2^-24 c |q_i| max_j |k_j| + 2^-23 |thr_i|
brackets the rank, lo_i = #{S64 > thr + eps} <= rank_i <= hi_i = #{S64 > thr - eps}; at most 10 % of the rows may have lo != hi."""
import math

import torch

from x_clip_amd import ops

NEG = -3.0e38


def poison(dev, nq, slots):
    """0x7f.. into the scratch the next call will use, and into freshly freed blocks of the sizes its outputs have"""
    ws = ops.workspace(dev, 3 * slots * nq * 4)
    ws.fill_(0x7F)
    junk = [torch.full((nq,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    junk += [torch.full((nq,), 0x7F7F7F7F, dtype=torch.int32, device=dev) for _ in range(3)]
    del junk


def run(dev, q, chunks, scale, off, log_scale=None, thr=None):
    poison(dev, q.shape[0], sum((k.shape[0] + 63) // 64 for k, _ in chunks))
    return ops.simrank_chunked(q, chunks, scale, off, log_scale=log_scale, thr=None if thr is None else thr.clone())


def dense(S, thr, off):
    """S [nq, nk] (any float type, compared as given), thr [nq] -> rank, hard_val, hard_idx (lowest column among equal maxima)"""
    nq, nk = S.shape
    cols = torch.arange(nk, device=S.device)
    neg = cols[None, :] != (torch.arange(nq, device=S.device) + off)[:, None]
    rank = ((S > thr[:, None]) & neg).sum(1)
    Sm = S.masked_fill(~neg, float("-inf"))
    hv = Sm.max(1).values
    hi = torch.where(Sm == hv[:, None], cols[None, :], nk).min(1).values
    return rank, hv, hi


def exact_inputs(nq, nk, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (nq, d), generator=g).to(torch.float32) / 8
    k = torch.randint(-3, 4, (nk, d), generator=g).to(torch.float32) / 8
    return q.to(dtype), k.to(dtype)


def device_scale(dev, dtype, scale, log_scale):
    """scale * exp(log_scale) as the kernels form it, read back through the positive of a unit vector (1 * c = c exactly).
    Deliberate: the device's expf may differ from the host's in the last bit, and the exact reference needs ITS bits -- with them, every
    logit of the reference is one IEEE multiply of an exact dot product.  The value is pinned to e^tau only loosely by the caller; what
    keeps the kernels honest independently of this read-back is the power-of-two variant, whose scale the test sets itself."""
    e = torch.zeros(1, 8, dtype=dtype, device=dev)
    e[0, 0] = 1
    return ops.simrank(e, e, scale, 0, log_scale=log_scale)[3].reshape(())


def check_exact(got, S, thr, off, tag):
    rank, hv, hi, _ = got
    r_rank, r_hv, r_hi = dense(S, thr, off)
    assert torch.equal(rank.long(), r_rank), (tag, "rank", int((rank.long() != r_rank).sum()))
    assert torch.equal(hi.long(), r_hi), (tag, "hard_idx", int((hi.long() != r_hi).sum()))
    assert torch.equal(hv, r_hv.float()), (tag, "hard_val", int((hv != r_hv.float()).sum()))


def case_exact(dev, dtype, nq, nk, d, off=0, splits=None, repeats=0, seed=3):
    """both threshold variants of one shape; `splits`: K also fed as chunks cut at these columns (bit-equal to the one-chunk call);
    `repeats`: that many further launches must return identical bits"""
    assert d <= 128
    q, k = exact_inputs(nq, nk, d, dtype, seed)
    q, k = q.to(dev), k.to(dev)
    dots = q.double() @ k.double().t()                               # exact, and exact in fp32
    assert torch.equal(dots.float().double(), dots)
    rows = torch.arange(nq, device=dev)
    has = (rows + off >= 0) & (rows + off < nk)
    pdot = torch.where(has, dots[rows, (rows + off).clamp(0, nk - 1)], torch.zeros((), dtype=torch.float64, device=dev))
    # (1) a power-of-two scale, the threshold computed here
    scale = 4.0
    S = dots.float() * scale
    thr = (pdot.float() * scale)
    got = run(dev, q, [(k, 0)], scale, off, thr=thr)
    check_exact(got, S, thr, off, (nq, nk, d, "pow2"))
    # (2) a temperature on the device: the threshold from xclip_simrank_pos and from the forward's pos, bit-equal
    tau = torch.tensor([0.7], dtype=torch.float32, device=dev)
    c32 = device_scale(dev, dtype, 1.0, tau)
    assert abs(float(c32) - math.exp(0.7)) < 1e-5
    S = dots.float() * c32
    got = run(dev, q, [(k, 0)], 1.0, off, log_scale=tau)
    thr_pos = got[3]
    _, fwd_pos = ops.simloss_fwd(q, k, 1.0, off, False, 0.0, None, log_scale=tau)
    assert torch.equal(thr_pos, fwd_pos), (nq, nk, d, "thr from simrank_pos != forward pos")
    assert torch.equal(thr_pos, pdot.float() * c32)
    check_exact(got, S, thr_pos, off, (nq, nk, d, "tau"))
    got2 = run(dev, q, [(k, 0)], 1.0, off, log_scale=tau, thr=fwd_pos)
    for a, b in zip(got, got2):
        assert torch.equal(a, b)
    if splits:
        cuts = [0, *splits, nk]
        chunks = [(k[a:b].contiguous(), a) for a, b in zip(cuts[:-1], cuts[1:])]
        for order in (chunks, chunks[::-1]):
            gc = run(dev, q, order, 1.0, off, log_scale=tau)
            for a, b in zip(got, gc):
                assert torch.equal(a, b), (nq, nk, d, "chunked != one chunk")
    for _ in range(repeats):
        again = run(dev, q, [(k, 0)], 1.0, off, log_scale=tau)
        for a, b in zip(got, again):
            assert torch.equal(a, b), (nq, nk, d, "not reproducible")


def case_nan_row(dev, nq=512, nk=768, d=64, bad=300):
    """diverged latents: a row of NaN has no logit above anything and no hardest negative -- rank 0, hard_idx -1, never a garbage
    column -- on interior tiles (columns 256 .. 767 of row 300) as on diagonal ones; every other row is untouched"""
    q, k = exact_inputs(nq, nk, d, torch.bfloat16, 5)
    q, k = q.to(dev), k.to(dev)
    clean = run(dev, q, [(k, 0)], 4.0, 0)
    q2 = q.clone()
    q2[bad] = float("nan")
    rank, hv, hi, thr = run(dev, q2, [(k, 0)], 4.0, 0)
    assert int(rank[bad]) == 0 and int(hi[bad]) == -1 and float(hv[bad]) == float(torch.tensor(NEG, dtype=torch.float32)) and bool(torch.isnan(thr[bad]))
    keep = torch.arange(nq, device=dev) != bad
    for a, b in zip(clean, (rank, hv, hi, thr)):
        assert torch.equal(a[keep], b[keep])


EXACT_GENERAL = [(5, 7, 8), (70, 130, 40)]                            # fp32 and bf16
EXACT_RING = [(128, 128, 64, 0, None), (256, 256, 64, 0, None), (512, 768, 128, 0, None), (520, 777, 64, 0, (256, 520)),
              (520, 777, 64, 200, None)]                             # bf16: (nq, nk, d, diag_off, splits)


def case_realistic(dev, dtype, nq, nk, d, off, c, seed=9):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1).to(dtype).to(dev)
    k = torch.nn.functional.normalize(torch.randn(nk, d, generator=g), dim=1).to(dtype).to(dev)
    tau = torch.tensor([math.log(c)], dtype=torch.float32, device=dev)
    rank, hv, hi, thr = run(dev, q, [(k, 0)], 1.0, off, log_scale=tau)
    c64 = math.exp(float(tau))
    q64, k64 = q.double(), k.double()
    S = c64 * (q64 @ k64.t())
    eps = d * 2.0 ** -24 * c64 * q64.norm(dim=1) * k64.norm(dim=1).max() + 2.0 ** -23 * thr.double().abs()
    rows = torch.arange(nq, device=dev)
    assert bool(((rows + off >= 0) & (rows + off < nk)).all())
    assert bool(((thr.double() - S[rows, rows + off]).abs() <= eps).all()), "positive outside the accumulation bound"
    lo, r_hv, _ = dense(S, thr.double() + eps, off)
    hi_, _, _ = dense(S, thr.double() - eps, off)
    amb = float((lo != hi_).double().mean())
    print(f"simrank realistic {tuple(q.shape)} x {nk} off {off} c {c} {dtype}: ambiguous rows {amb:.4f}, max |hard_val - ref| / eps "
          f"{float(((hv.double() - r_hv).abs() / eps).max()):.3f}")
    assert bool(((lo <= rank.long()) & (rank.long() <= hi_)).all()), int(((lo > rank.long()) | (rank.long() > hi_)).sum())
    assert bool(((hv.double() - r_hv).abs() <= eps).all())
    assert bool(((hi.long() >= 0) & (hi.long() < nk) & (hi.long() != rows + off)).all())
    assert bool((S[rows, hi.long()] >= r_hv - 2 * eps).all())
    assert amb <= 0.10, amb


REALISTIC = [(70, 130, 40, 0, 14.3), (300, 700, 128, 50, 14.3), (520, 777, 64, 0, 100.0)]


# ---- public interface --------------------------------------------------------------------------------------------------------------
def small_clip(dev, dtype, batch=12, **cfg_over):
    import dataclasses
    import clip_cases as C
    from oracle import clip_oracle as O
    cfg = dataclasses.replace(O.CFG1, **cfg_over) if cfg_over else O.CFG1
    sd = O.make_state_dict(cfg, 11, torch.float32)
    text, image, _, _ = O.make_inputs(cfg, batch, 12)
    model = C.build_clip(cfg, sd, dev, dtype)
    return model, text.to(dev), image.to(dtype).to(dev)


def check_direction(out, q, k, tau, ks, B=None, off=0):
    """one direction of contrastive_metrics against dense fp64 torch on the latents (banded as the realistic cases)"""
    nq, d = q.shape
    c64 = math.exp(float(tau))
    S = c64 * (q.double() @ k.double().t())
    rows = torch.arange(nq, device=q.device)
    pos = S[rows, rows + off]
    eps = d * 2.0 ** -24 * c64 * q.double().norm(dim=1) * k.double().norm(dim=1).max() + 2.0 ** -23 * pos.abs()
    lo, r_hv, _ = dense(S, pos + 2 * eps, off)
    hi_, _, _ = dense(S, pos - 2 * eps, off)
    rank = out["rank"].long()
    assert out["rank"].dtype == torch.int32 and out["hard_idx"].dtype == torch.int32
    assert bool(((lo <= rank) & (rank <= hi_)).all()), (lo, rank, hi_)
    assert bool(((out["margin"].double() - (pos - r_hv)).abs() <= 2 * eps).all())
    hidx = out["hard_idx"].long()
    assert bool(((hidx >= 0) & (hidx < k.shape[0]) & (hidx != rows + off)).all())
    assert bool((S[rows, hidx] >= r_hv - 2 * eps).all())
    if B is None:                                                    # single process: the scalars follow from the returned ranks, exactly
        for kk in ks:
            assert torch.equal(out[f"recall@{kk}"], ((rank < kk).sum().double() / nq).float()), kk
        assert torch.equal(out["mean_rank"], (rank.sum().double() / nq).float())


def case_public_metrics(dev, dtype):
    from x_clip_amd import contrastive_metrics
    model, text, image = small_clip(dev, dtype)
    with torch.no_grad():
        tl, il = model(text, image, return_latents=True)
    ks = (1, 3, 5)
    m = contrastive_metrics(tl, il, model.temperature, ks=ks)
    assert set(m) == {"t2i", "i2t"}
    for name in m:
        assert set(m[name]) == {"rank", "hard_idx", "margin", "mean_rank"} | {f"recall@{k}" for k in ks}
    tau = model.temperature.detach().float()
    check_direction(m["t2i"], tl, il, tau, ks)
    check_direction(m["i2t"], il, tl, tau, ks)
    with __import__("pytest").raises(ValueError, match="matched pairs"):
        contrastive_metrics(tl, il[:-1], model.temperature)


# gradients the fp32 backward accumulates with float atomics on the GPU: their summation order varies from run to run, with tracking or
# without it (tests/test_clip_gpu.py test_checkpointing_is_bit_identical holds them to the same bar)
def _atomic_grad(name):
    return "token_emb" in name or name.endswith(".g") or "pos_emb" in name or "cls_token" in name or name.endswith("bias") or name == "temperature"


def case_track_metrics_changes_nothing(dev, dtype):
    """three steps on one model: tracking off, on, off again.  Loss and gradients are the same bits -- except, in fp32 on the GPU, the
    gradients whose backward adds floats atomically: those are not reproducible between two runs WITHOUT tracking either, and are
    held to rtol 1e-4 / atol 1e-6 (the order of a handful of fp32 additions)"""
    model, text, image = small_clip(dev, dtype, batch=4)
    assert model.last_metrics is None
    loose = dev.type == "cuda" and dtype == torch.float32

    def step():
        model.zero_grad(set_to_none=True)
        loss = model(text, image, return_loss=True)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    l0, g0 = step()
    assert model.last_metrics is None
    model.track_metrics((1, 2))
    l1, g1 = step()
    m = model.last_metrics
    assert m is not None and set(m) == {"t2i", "i2t"} and "recall@2" in m["t2i"] and m["t2i"]["rank"].shape == (4,)
    assert not m["t2i"]["margin"].requires_grad
    model.track_metrics(None)
    assert model.last_metrics is None
    l2, g2 = step()
    assert model.last_metrics is None
    assert torch.equal(l0, l1) and torch.equal(l0, l2), (float(l0), float(l1), float(l2))
    assert set(g0) == set(g1) == set(g2)
    for n in g0:
        for other in (g1[n], g2[n]):
            if loose and _atomic_grad(n):
                torch.testing.assert_close(other, g0[n], rtol=1e-4, atol=1e-6)
            else:
                assert torch.equal(g0[n], other), n


def case_filip_is_not_tracked(dev, dtype, monkeypatch):
    model, text, image = small_clip(dev, dtype, batch=4, use_all_token_embeds=True)
    model.track_metrics()

    def boom(*a, **k):
        raise AssertionError("the fine-grained head launched the metrics")

    monkeypatch.setattr(ops, "simrank_chunked", boom)
    loss = model(text, image, return_loss=True)
    assert bool(torch.isfinite(loss)) and model.last_metrics is None


# ---- two ranks, ragged batches ---------------------------------------------------------------------------------------------------------
def dist_latents(dev, dtype=torch.float32, B=8, d=32):
    g = torch.Generator().manual_seed(77)
    t = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=1)
    i = torch.nn.functional.normalize(t + 0.7 * torch.randn(B, d, generator=g), dim=1)
    return t.to(dtype).to(dev), i.to(dtype).to(dev), torch.tensor(2.0, device=dev)


def worker_metrics(rank, world, port, tmp, kind="cpu"):
    import os
    import dist_cases as D
    dev = D.setup(rank, world, port, kind)
    import torch.distributed as dist
    from x_clip_amd import contrastive_metrics
    t, i, tau = dist_latents(dev)
    sizes = [5, 3]
    lo = sum(sizes[:rank])
    sl = slice(lo, lo + sizes[rank])
    m = contrastive_metrics(t[sl], i[sl], tau, ks=(1, 2, 5))
    # a rank without rows (8 + 0) still takes part in the gather and the reduction
    lo0 = 0 if rank == 0 else 8
    m0 = contrastive_metrics(t[lo0:8], i[lo0:8], tau, ks=(1, 2, 5))
    raised = False
    try:                                                             # rank 0 brings one image fewer: 8 texts, 7 images
        contrastive_metrics(t[sl], i[sl][: sizes[rank] - (1 if rank == 0 else 0)], tau)
    except ValueError:
        raised = True
    torch.save({"m": {k: {n: v.cpu() for n, v in d.items()} for k, d in m.items()}, "raised": raised, "lo": lo, "n": sizes[rank],
                "m0": {k: {n: v.cpu() for n, v in d.items()} for k, d in m0.items()}},
               os.path.join(tmp, f"rank{rank}.pt"))
    dist.destroy_process_group()


def check_two_ranks(tmp, dev):
    import os
    from x_clip_amd import contrastive_metrics
    t, i, tau = dist_latents(dev)
    whole = contrastive_metrics(t, i, tau, ks=(1, 2, 5), distributed=False)
    recs = [torch.load(os.path.join(tmp, f"rank{r}.pt")) for r in range(2)]
    for rec in recs:
        assert rec["raised"]
        for dname in ("t2i", "i2t"):
            got, want = rec["m"][dname], whole[dname]
            for n in ("mean_rank", "recall@1", "recall@2", "recall@5"):
                assert torch.equal(got[n], want[n].cpu()), (dname, n, got[n], want[n])
                assert torch.equal(got[n], recs[0]["m"][dname][n])
            for n in ("rank", "hard_idx", "margin"):
                assert torch.equal(got[n], want[n].cpu()[rec["lo"]: rec["lo"] + rec["n"]]), (dname, n)
    for r, rec in enumerate(recs):                                   # 8 + 0 rows: rank 0 holds everything, rank 1 empty vectors
        for dname in ("t2i", "i2t"):
            got, want = rec["m0"][dname], whole[dname]
            for n in ("mean_rank", "recall@1", "recall@2", "recall@5"):
                assert torch.equal(got[n], want[n].cpu()), (dname, n, "8 + 0")
            for n in ("rank", "hard_idx", "margin"):
                assert torch.equal(got[n], want[n].cpu() if r == 0 else want[n].cpu()[:0]), (dname, n, "8 + 0")
