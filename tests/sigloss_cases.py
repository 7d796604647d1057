"""Shared cases of the pairwise sigmoid (SigLIP) head (ops.sigloss_*, losses.sigmoid_loss, CLIP(sigmoid_loss=True);
csrc/kernels/sigloss.h): the CPU suite runs them on the wave64 emulator (tests/test_sigloss_emu.py), the GPU suite on the MI355X
(tests/test_sigloss_gpu.py).  The reference is dense torch in fp64 with autograd on the definition
    l = t q k^T + beta,  z = +1 at j = i + off else -1,  rowloss_i = sum_j softplus(-z l),  L = coef sum_i rowloss_i,
    G = gmul dL/dl,  dtau = sum G o (l - beta),  dbeta = sum G
evaluated on the CPU on the dtype-rounded inputs.

Bars (through kernel_cases.close): kernel level rowloss 1e-5 of its scale; the loss, dtau and dbeta 1e-5 of
themselves (at beta = +10 every sigma is ~1 and dtau = gc sum s cancels to 1/500 of its terms: the kernels sum it in split form,
csrc/kernels/sigloss.h); two launches' dtau / dbeta agree to 1e-6 of themselves.  G 1e-6 of its scale in fp32, in bf16 one bf16 ulp element-wise OR two ulps of its scale.  End to end: fp32 loss 1e-5, gradients 3e-4;
bf16 loss 3e-4, gradients 8 % with cosine 0.999.

Exact inputs: entries from {-3 .. 3} / 8 (or +-1/8 sign vectors of unit norm) with d <= 128 make every dot product exact in fp32 in
any summation order; with a host scale the logits the kernels see differ from the reference's by the roundings of one fma."""
import math

import torch

import kernel_cases as KC
from x_clip_amd import ops

F32 = torch.float32


# ---- reference ----------------------------------------------------------------------------------------------------------------------
def dense(q, k, t, beta, off, coef, gmul):
    """fp64, CPU -> rowloss [nq], loss, G [nq, nk], dtau, dbeta"""
    q64, k64 = q.detach().cpu().double(), k.detach().cpu().double()
    nq, nk = q64.shape[0], k64.shape[0]
    s = t * (q64 @ k64.t())
    l = (s + beta).requires_grad_(True)
    z = -torch.ones(nq, nk, dtype=torch.float64)
    rows = torch.arange(nq)
    ok = (rows + off >= 0) & (rows + off < nk)
    z[rows[ok], rows[ok] + off] = 1.0
    rowloss = torch.nn.functional.softplus(-z * l).sum(1)
    loss = coef * rowloss.sum()
    (G,) = torch.autograd.grad(loss, l)
    G = G * gmul
    assert bool(torch.isfinite(rowloss).all()) and bool(torch.isfinite(G).all()), "the reference itself is not finite"
    return rowloss.detach(), loss.detach(), G, (G * s).sum(), G.sum(), float((G * s).abs().sum()), float(G.abs().sum())


def close_g(G, want, dtype, name):
    if dtype == F32:
        KC.close(G, want, dtype, name, mult=0.05)                    # 1e-6 of the scale
        return
    try:
        KC.close(G, want, dtype, name, ulps=1.0, unit="elem")
    except AssertionError:
        KC.close(G, want, dtype, name + " {scale}", ulps=2.0, unit="scale")


def scalar(x):
    return x.detach().reshape(1).cpu()


def poison(dev, nq, slots):
    """NaN into the scratch the next call will use -> a NaN-filled rowloss for it to write into (G is poisoned where it is made)"""
    ws = ops.workspace(dev, slots * nq * 4)
    ws.fill_(0xFF)                                                   # (0xffffffff is a NaN)
    return torch.full((nq,), float("nan"), dtype=F32, device=dev)


def chunked(k, cuts, reverse=False):
    cuts = [0, *cuts, k.shape[0]]
    ch = [(k[a:b].contiguous(), a) for a, b in zip(cuts[:-1], cuts[1:])]
    return ch[::-1] if reverse else ch


def case_kernel(dev, dtype, q, k, off=0, scale=1.0, tau=None, beta=-2.0, coef=0.37, gmul=1.7, chunk_sets=(), repeats=0, tag=""):
    """forward (one chunk, then every chunk set: same bars), backward with and without the scale folded in, NULL accumulators"""
    q, k = q.to(dtype).to(dev), k.to(dtype).to(dev)
    nq, nk = q.shape[0], k.shape[0]
    v = ops.vec(dtype)
    ldg = (nk + v - 1) // v * v
    tau_t = None if tau is None else torch.tensor([tau], dtype=F32, device=dev)
    beta_t = torch.tensor([beta], dtype=F32, device=dev)
    gmul_t = torch.tensor([gmul], dtype=F32, device=dev)
    t64 = scale * (math.exp(float(torch.tensor(tau, dtype=F32))) if tau is not None else 1.0)
    r_row, r_loss, r_G, r_dtau, r_dbeta, s_dtau, s_dbeta = dense(q, k, t64, float(beta_t), off, coef, gmul)
    name = f"sigloss {tag} {nq}x{nk}x{q.shape[1]} off {off}"
    first = None
    for chunks in ([(k, 0)], *chunk_sets):
        rowloss = poison(dev, nq, sum((c.shape[0] + 63) // 64 for c, _ in chunks))
        loss = torch.zeros(1, dtype=F32, device=dev)
        assert ops.sigloss_chunked_fwd(q, chunks, scale, off, coef, loss, log_scale=tau_t, bias=beta_t, out=rowloss) is rowloss
        print(f"{name}: rowloss err {float((rowloss.cpu().double() - r_row).abs().max() / r_row.abs().max()):.2e} "
              f"loss err {abs(float(loss) - float(r_loss)) / abs(float(r_loss)):.2e}")
        KC.close(rowloss, r_row, F32, name + " rowloss", mult=0.5)
        KC.close(scalar(loss), scalar(r_loss), F32, name + " loss", mult=0.5)
        if first is None:
            first = (rowloss.clone(), loss.clone())
            for _ in range(repeats):                                 # the forward is deterministic
                l2 = torch.zeros(1, dtype=F32, device=dev)
                again = ops.sigloss_chunked_fwd(q, chunks, scale, off, coef, l2, log_scale=tau_t, bias=beta_t)
                assert torch.equal(again, first[0]) and torch.equal(l2, first[1]), name + ": forward not reproducible"
    G1 = None
    for times_scale in (False, True):
        G = torch.full((nq, ldg), float("nan"), dtype=dtype, device=dev)
        dtau = torch.zeros(1, dtype=F32, device=dev)
        dbeta = torch.zeros(1, dtype=F32, device=dev)
        out = ops.sigloss_grad(q, k, scale, off, coef, dtau, dbeta, log_scale=tau_t, bias=beta_t, gmul=gmul_t, times_scale=times_scale, out=G)
        assert out is G
        want = r_G * (t64 if times_scale else 1.0)
        print(f"{name} x{int(times_scale)}: dtau err {abs(float(dtau) - float(r_dtau)) / s_dtau:.2e} (of itself "
              f"{abs(float(dtau) - float(r_dtau)) / abs(float(r_dtau)):.2e}) dbeta err {abs(float(dbeta) - float(r_dbeta)) / s_dbeta:.2e} "
              f"(of itself {abs(float(dbeta) - float(r_dbeta)) / abs(float(r_dbeta)):.2e})")
        close_g(G[:, :nk], want, dtype, name + " G")
        assert bool((G[:, nk:] == 0).all()), name + ": padding columns of G are not zero"
        KC.close(scalar(dtau), scalar(r_dtau), F32, name + " dtau", mult=0.5)          # 1e-5 of itself
        KC.close(scalar(dbeta), scalar(r_dbeta), F32, name + " dbeta", mult=0.5)
        if not times_scale:
            G1 = G
            for _ in range(repeats):
                Gb = torch.full((nq, ldg), float("nan"), dtype=dtype, device=dev)
                dt2 = torch.zeros(1, dtype=F32, device=dev)
                db2 = torch.zeros(1, dtype=F32, device=dev)
                ops.sigloss_grad(q, k, scale, off, coef, dt2, db2, log_scale=tau_t, bias=beta_t, gmul=gmul_t, out=Gb)
                assert torch.equal(Gb, G), name + ": G not reproducible"
                # (float atomics, one pair per work-group)
                print(f"{name}: repeat dtau diff {abs(float(dt2) - float(dtau)) / abs(float(dtau)):.2e} dbeta diff {abs(float(db2) - float(dbeta)) / abs(float(dbeta)):.2e} of themselves")
                assert abs(float(dt2) - float(dtau)) <= 1e-6 * abs(float(dtau)) and abs(float(db2) - float(dbeta)) <= 1e-6 * abs(float(dbeta))
    # gmul = NULL (= 1) and no accumulators
    G0 = ops.sigloss_grad(q, k, scale, off, coef, None, None, log_scale=tau_t, bias=beta_t)
    close_g(G0[:, :nk], r_G / gmul, dtype, name + " G (gmul NULL)")
    assert bool((G0[:, nk:] == 0).all())
    return G1


def exact_inputs(nq, nk, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (nq, d), generator=g).to(F32) / 8
    k = torch.randint(-3, 4, (nk, d), generator=g).to(F32) / 8
    return q, k


def sign_inputs(nq, nk, d, seed, matched=()):
    """unit-norm rows of +-1 / sqrt(d) (d a power of four: exact in bf16); `matched` rows share their positive's vector"""
    assert d in (16, 64)
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(0, 2, (nq, d), generator=g).to(F32) * 2 - 1) / math.sqrt(d)
    k = (torch.randint(0, 2, (nk, d), generator=g).to(F32) * 2 - 1) / math.sqrt(d)
    return q, k, matched


GENERAL = [(5, 7, 8), (70, 130, 40)]                                  # fp32 and bf16
# bf16, the ring loop: (nq, nk, d, diag_off, chunk cut sets) -- a partial tile, a diagonal tile, the interior PLAIN path, ragged
RING = [(128, 128, 64, 0, ()), (256, 256, 64, 0, ()), (512, 768, 128, 0, ()), (520, 777, 64, 0, ((256, 520),)), (520, 777, 64, 200, ((256, 520),))]


def case_shape(dev, dtype, nq, nk, d, off=0, cuts=(), repeats=0):
    q, k = exact_inputs(nq, nk, d, 3)
    q, k = q * 0.5, k * 0.5                                          # |l| up to a few tens at exp(0.7)
    sets = []
    for c in cuts:
        sets += [chunked(k.to(dtype).to(dev), c), chunked(k.to(dtype).to(dev), c, reverse=True)]
    case_kernel(dev, dtype, q, k, off=off, tau=0.7, beta=-2.0, chunk_sets=sets, repeats=repeats, tag="shape")


# numerical regimes: (label, host scale t, beta, matched pairs)
REGIMES = [("siglip-init", 10.0, -10.0, False), ("beta+10", 10.0, 10.0, False), ("t200", 200.0, -10.0, True), ("t400", 400.0, 0.0, True)]


def case_regime(dev, dtype, label, t, beta, matched, ring):
    """The narrowest case is `beta+10` on the ring loop.  Every sigma is ~1, dtau = gc sum s cancels to 1/500 of its terms, and the
    full-tile epilogue sums G * acc, so the rounding of each G (equal logits round alike) stays in the sum: on the MI355X dtau reads
    8.0e-6 of itself with the scale folded into G and 3.6e-7 without, against the bar of 1e-5.  The edge and general kernels sum dtau
    in split form; the same split spilled 237 - 291 registers in the full-tile epilogue (csrc/kernels/sigloss.h)."""
    nq, nk, d = (256, 384, 64) if ring else (70, 130, 64)
    q, k, _ = sign_inputs(nq, nk, d, 17)
    if matched:                                                      # a few perfectly matched pairs among unrelated ones: l = t + beta
        for i in (0, 1, 2, 3, 37):
            k[i] = q[i]
    # the matched-pair regimes take their temperature through the device's exp(*log_scale), the others as the host scale
    case_kernel(dev, dtype, q, k, scale=1.0 if matched else t, tau=math.log(t) if matched else None, beta=beta, tag=label)


def log1p_inputs(nq, nk, d):
    """every negative at exactly l = -18, every positive at l = +30 with t = 64, beta = -10: dot = -1/8 and 5/8"""
    assert d > nq
    q = torch.zeros(nq, d)
    k = torch.zeros(nk, d)
    q[torch.arange(nq), torch.arange(nq)] = 1.0
    q[:, nq] = 0.5
    k[torch.arange(nq), torch.arange(nq)] = 0.75
    k[:, nq] = -0.25
    return q, k


def case_log1p(dev, dtype, nq=64, nk=4096, d=128):
    """rowloss_i = (nk - 1) log1p(e^-18) + log1p(e^-30) ~ (nk - 1) 1.5e-8: an fp32 log(1 + e) returns 0 for every term"""
    q, k = log1p_inputs(nq, nk, d)
    q, k = q.to(dtype).to(dev), k.to(dtype).to(dev)
    beta_t = torch.tensor([-10.0], dtype=F32, device=dev)
    r_row, r_loss = dense(q, k, 64.0, -10.0, 0, 1.0, 1.0)[:2]
    assert abs(float(r_row[0]) - ((nk - 1) * math.log1p(math.exp(-18.0)) + math.log1p(math.exp(-30.0)))) < 1e-12
    loss = torch.zeros(1, dtype=F32, device=dev)
    rowloss = ops.sigloss_fwd(q, k, 64.0, 0, 1.0, loss, bias=beta_t)
    err = float(((rowloss.cpu().double() - r_row) / r_row).abs().max())
    print(f"sigloss log1p {nq}x{nk}x{d} {dtype}: rowloss {float(rowloss[0]):.6e} want {float(r_row[0]):.6e} rel err {err:.2e}")
    assert err <= 1e-5, err
    assert abs(float(loss) - float(r_loss)) <= 1e-5 * float(r_loss)


def case_more_tiles_than_compute_units(dev):
    """GPU only: 4352 x 4096 = 17 x 16 tiles on 256 CUs, some work-group walks a second tile; three forward launches and G bit-identical"""
    q, k = exact_inputs(4352, 4096, 64, 3)
    case_kernel(dev, torch.bfloat16, q * 0.5, k * 0.5, tau=0.7, beta=-2.0, repeats=2, tag="272 tiles")


# ---- losses.sigmoid_loss: multiview weights ------------------------------------------------------------------------------------------
def latents(m, b, d, seed, dtype, dev):
    g = torch.Generator().manual_seed(seed)
    t = torch.nn.functional.normalize(torch.randn(m, b, d, generator=g), dim=-1)
    return t.to(dtype).to(dev)


def dense_loss(T, I, tau, beta, main_w, mv_w, off=0, B=None):
    """fp64 with autograd: T [m, b, d] rows against I [n, B, d], weights as _ContrastiveFn pairs them"""
    m, n = T.shape[0], I.shape[0]
    B = I.shape[1] if B is None else B
    loss = 0.0
    for i in range(m):
        for j in range(n):
            w = main_w if (i == 0 and j == 0) else mv_w / max(m * n - 1, 1)
            l = tau.exp() * (T[i] @ I[j].t()) + beta
            z = -torch.ones_like(l)
            rows = torch.arange(T.shape[1])
            z[rows, rows + off] = 1.0
            loss = loss + w / B * torch.nn.functional.softplus(-z * l).sum()
    return loss


def e2e_close(got, want, dtype, name):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), name
    rel = float((got - want).norm() / want.norm())
    cos = float((got * want).sum() / (got.norm() * want.norm()))
    print(f"{name}: rel {rel:.2e} cos {cos:.6f}")
    if dtype == F32:
        assert rel < 3e-4, (name, rel)
    else:
        assert rel < 0.08 and cos > 0.999, (name, rel, cos)


def case_multiview(dev, dtype, m=2, n=3, b=12, d=32):
    from x_clip_amd.losses import ContrastiveSpec, sigmoid_loss
    T = latents(m, b, d, 5, dtype, dev).requires_grad_(True)
    I = latents(n, b, d, 6, dtype, dev).requires_grad_(True)
    tau = torch.tensor(math.log(10.0), dtype=dtype, device=dev, requires_grad=True)
    beta = torch.tensor(-10.0, dtype=dtype, device=dev, requires_grad=True)
    spec = ContrastiveSpec(main_weight=0.8, multiview_weight=0.1, sigmoid=True)
    loss = sigmoid_loss(tau, beta, T, I, spec)
    (loss * 1.5).backward()
    T64, I64 = T.detach().cpu().double().requires_grad_(True), I.detach().cpu().double().requires_grad_(True)
    tau64, beta64 = tau.detach().cpu().double().requires_grad_(True), beta.detach().cpu().double().requires_grad_(True)
    ref = dense_loss(T64, I64, tau64, beta64, 0.8, 0.1)
    (ref * 1.5).backward()
    assert loss.dtype == F32
    assert abs(float(loss.detach()) - float(ref.detach())) <= (1e-5 if dtype == F32 else 3e-4) * max(1.0, abs(float(ref.detach()))), (float(loss.detach()), float(ref.detach()))
    for nme, a, r in (("dT", T, T64), ("dI", I, I64), ("dtau", tau, tau64), ("dbeta", beta, beta64)):
        e2e_close(a.grad, r.grad, dtype, f"sigmoid multiview {nme}")
    with __import__("pytest").raises(RuntimeError, match="retain_graph is not supported"):
        loss.backward()


# ---- public interface -------------------------------------------------------------------------------------------------------------------
def small_clip(dev, dtype, batch=12, ctor=None, sigmoid=True):
    import clip_cases as C
    from oracle import clip_oracle as O
    cfg = O.CFG1
    sd = O.make_state_dict(cfg, 11, F32)
    extra = dict(ctor or {})
    if sigmoid:
        sd = dict(sd, temperature=torch.tensor(math.log(10.0)), logit_bias=torch.tensor(-10.0))
        extra["sigmoid_loss"] = True
    text, image, _, _ = O.make_inputs(cfg, batch, 12)
    model = C.build_clip(cfg, sd, dev, dtype, **extra)
    return model, text.to(dev), image.to(dtype).to(dev)


def case_public(dev, dtype):
    """loss and every parameter gradient against the fp64 dense formula on the model's own latents (chained through the model's own
    tower backward); the state dict carries logit_bias; three FusedAdamW steps reduce the loss and move logit_bias"""
    from x_clip_amd import CLIP, FusedAdamW
    model, text, image = small_clip(dev, dtype)
    fresh = CLIP(**__import__("oracle.clip_oracle", fromlist=["CFG1"]).CFG1.ctor_kwargs(), sigmoid_loss=True)
    assert abs(float(fresh.temperature.detach()) - math.log(10.0)) < 1e-6 and float(fresh.logit_bias.detach()) == -10.0
    assert fresh.logit_bias.dtype == fresh.temperature.dtype and fresh.logit_bias.dim() == 0
    assert "logit_bias" in model.state_dict()
    groups = FusedAdamW.default_param_groups(model)
    assert any(p is model.logit_bias for p in groups[1]["params"]) and not any(p is model.logit_bias for p in groups[0]["params"])
    loss = model(text, image, return_loss=True)
    loss.backward()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert "temperature" in got and "logit_bias" in got
    model.zero_grad(set_to_none=True)
    tl, il = model(text, image, return_latents=True)
    ref = dense_loss(tl.double()[None].cpu(), il.double()[None].cpu(), model.temperature.double().cpu(), model.logit_bias.double().cpu(), 1.0, 0.0)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= (1e-5 if dtype == F32 else 3e-4) * max(1.0, abs(float(ref.detach()))), (float(loss.detach()), float(ref.detach()))
    for n, p in model.named_parameters():
        if p.grad is None:
            assert n not in got or float(got[n].abs().max()) == 0.0, n
            continue
        assert n in got, n
        if float(p.grad.double().norm()) < 1e-12:
            continue
        e2e_close(got[n], p.grad, dtype, f"sigmoid clip {n}")


def case_adamw_steps(dev, dtype):
    from x_clip_amd import FusedAdamW
    model, text, image = small_clip(dev, dtype)
    opt = FusedAdamW(FusedAdamW.default_param_groups(model), lr=1e-2)
    b0 = float(model.logit_bias.detach())
    losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        loss = model(text, image, return_loss=True)
        losses.append(float(loss.detach()))
        if len(losses) < 4:
            loss.backward()
            opt.step()
    assert all(math.isfinite(v) for v in losses) and losses[3] < losses[0], losses
    assert float(model.logit_bias.detach()) != b0


def case_off_is_unchanged(dev, dtype):
    """sigmoid_loss=False: state_dict keys and the loss are those of a model built without the keyword, bit for bit"""
    a, text, image = small_clip(dev, dtype, sigmoid=False)
    b, _, _ = small_clip(dev, dtype, sigmoid=False, ctor={"sigmoid_loss": False})
    assert list(a.state_dict()) == list(b.state_dict()) and "logit_bias" not in b.state_dict()
    la, lb = a(text, image, return_loss=True), b(text, image, return_loss=True)
    assert torch.equal(la, lb)
    assert b.sigmoid_loss is False and not hasattr(b, "logit_bias")


def case_rejected_combinations():
    import pytest
    from oracle import clip_oracle as O
    from x_clip_amd import CLIP
    base = O.CFG1.ctor_kwargs()
    for over, word in ((dict(decoupled_contrastive_learning=True), "decoupled_contrastive_learning"),
                       (dict(use_all_token_embeds=True), "use_all_token_embeds"),
                       (dict(extra_latent_projection=True), "extra_latent_projection"),
                       (dict(extra_latent_projection=True, sim_reg_loss_weight=0.1), "sim_reg_loss_weight")):
        with pytest.raises(AssertionError, match=word):
            CLIP(**dict(base, **over), sigmoid_loss=True)


def case_track_metrics(dev, dtype):
    model, text, image = small_clip(dev, dtype, batch=4)
    l0 = model(text, image, return_loss=True).detach().clone()
    model.track_metrics((1, 2))
    l1 = model(text, image, return_loss=True).detach().clone()
    assert model.last_metrics is not None and model.last_metrics["t2i"]["rank"].shape == (4,)
    model.track_metrics(None)
    l2 = model(text, image, return_loss=True).detach().clone()
    assert torch.equal(l0, l1) and torch.equal(l0, l2)


# ---- two ranks, ragged batches ---------------------------------------------------------------------------------------------------------
def dist_inputs(dev, B=8, d=32):
    g = torch.Generator().manual_seed(77)
    t = torch.nn.functional.normalize(torch.randn(1, B, d, generator=g), dim=-1)
    i = torch.nn.functional.normalize(t + 0.7 * torch.randn(1, B, d, generator=g), dim=-1)
    return t.to(dev), i.to(dev), torch.tensor(math.log(10.0), device=dev), torch.tensor(-10.0, device=dev)


def run_loss(t, i, tau, beta, spec):
    from x_clip_amd.losses import sigmoid_loss
    t, i = t.clone().requires_grad_(True), i.clone().requires_grad_(True)
    tau, beta = tau.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    loss = sigmoid_loss(tau, beta, t, i, spec)
    loss.backward()
    return {"loss": loss.detach().cpu(), "dT": t.grad.cpu(), "dI": i.grad.cpu(), "dtau": tau.grad.cpu(), "dbeta": beta.grad.cpu()}


def worker_sigloss(rank, world, port, tmp, kind="cpu"):
    import os
    import dist_cases as D
    dev = D.setup(rank, world, port, kind)
    import torch.distributed as dist
    from x_clip_amd.losses import ContrastiveSpec
    t, i, tau, beta = dist_inputs(dev)
    spec = ContrastiveSpec(distributed=True, sigmoid=True)
    out = {}
    for label, sizes in (("5+3", [5, 3]), ("8+0", [8, 0])):
        lo = sum(sizes[:rank])
        sl = slice(lo, lo + sizes[rank])
        out[label] = dict(run_loss(t[:, sl], i[:, sl], tau, beta, spec), lo=lo, n=sizes[rank])
    torch.save(out, os.path.join(tmp, f"rank{rank}.pt"))
    dist.destroy_process_group()


def check_two_ranks(tmp, dev):
    import os
    from x_clip_amd.losses import ContrastiveSpec
    t, i, tau, beta = dist_inputs(dev)
    whole = run_loss(t, i, tau, beta, ContrastiveSpec(sigmoid=True))
    recs = [torch.load(os.path.join(tmp, f"rank{r}.pt")) for r in range(2)]
    for label in ("5+3", "8+0"):
        for rec in (r[label] for r in recs):
            assert torch.equal(rec["loss"], recs[0][label]["loss"]), label
            torch.testing.assert_close(rec["loss"], whole["loss"], rtol=1e-5, atol=0)
            sl = slice(rec["lo"], rec["lo"] + rec["n"])
            for nme in ("dT", "dI"):
                assert rec[nme].shape == whole[nme][:, sl].shape
                if rec["n"]:
                    KC.close(rec[nme], whole[nme][:, sl], F32, f"sigloss dist {label} {nme}", scale=float(whole[nme].abs().max()))
            for nme in ("dtau", "dbeta"):
                torch.testing.assert_close(rec[nme], whole[nme], rtol=1e-5, atol=0)
