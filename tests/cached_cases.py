"""Cases for FusedAdamW.accumulate_begin / accumulate / accumulate_end (csrc/kernels/optim.h grad_accum_kernel) and for
x_clip_amd.cached.CachedContrastiveStep, shared by tests/test_cached_emu.py (CPU, wave64 emulator build of the kernel sources),
tests/test_cached_gpu.py (MI355X, libxclip_hip.so) and the two-rank worker of tests/test_cached_dist.py.

Bars.  The accumulator: fp32 summation of k terms, element-wise k * 2^-24 * sum |g| against the fp64 sum (k roundings of at most half
an fp32 ulp of a partial sum that never exceeds sum |g|: derived, not measured).  The materialised gradient: the bits of torch's own
round-to-nearest-even cast of the accumulator.  The step: DESIGN.md section 7, the bars the one-pass step is held to -- fp32 loss 1e-5
and every gradient 3e-4 relative; bf16 loss 3e-4, gradients 8 % relative and cosine 0.999 -- against the one-pass step on the same batch
and against the fp64 oracle.
"""
import dataclasses
import functools
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import clip_cases as C  # noqa: E402
import optim_cases as OC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402
from x_clip_amd import CachedContrastiveStep, FusedAdamW, ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
CHUNK = ops.OPTIM_CHUNK
SIZES = [1, 7, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
GROUP_OF = [0, 1, 0, 1, 0, 1]
# the dim-512 model of the GPU suite's oracle checks (tests/test_clip_gpu.py MID): the smallest one whose bf16 loss holds DESIGN.md's 3e-4
MID = O.ClipConfig(dim_text=512, dim_image=512, dim_latent=512, num_text_tokens=2000, text_enc_depth=2, text_seq_len=70,
                   text_heads=8, visual_enc_depth=2, visual_image_size=128, visual_patch_size=32, visual_heads=8)
HEADS = ("infonce", "dcl", "sigmoid")


def _once(fn):
    """a reference is computed once per case and shared by the tests that need it (ClipConfig is not hashable: keyed by repr)"""
    memo = {}

    @functools.wraps(fn)
    def wrapped(*args):
        key = repr(args)
        if key not in memo:
            memo[key] = fn(*args)
        return memo[key]
    return wrapped


# ---- kernel and optimizer --------------------------------------------------------------------------------------------------------------
def _mixed(dev, first, seed=1):
    """parameters of SIZES, alternating fp32 / bf16 starting with `first`, in two param groups"""
    dts = [first if i % 2 == 0 else (BF16 if first == F32 else F32) for i in range(len(SIZES))]
    g = torch.Generator().manual_seed(seed)
    params = [(torch.randn(n, generator=g) * 0.5 + 0.1).to(dt) for n, dt in zip(SIZES, dts)]
    ps, opt = OC.fused(dev, params, GROUP_OF)
    return ps, opt, dts


def _grads(dts, k, seed=2):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g))).to(dt) for n, dt in zip(SIZES, dts)]
            for _ in range(k)]


def _acc(opt, p):
    D, i = opt._where[id(p)]
    return D.view(D.acc, i)


def case_accumulate(dev, first, k):
    """k accumulate() calls; parameter 1 is absent from call 0 (for k = 1: never has a gradient), parameter 4 from call 1"""
    ps, opt, dts = _mixed(dev, first)
    grads = _grads(dts, k)
    for t in range(k):
        if t == 0:
            grads[t][1] = None
        if t == 1:
            grads[t][4] = None
    opt.accumulate_begin()
    for t in range(k):
        OC.set_grads(ps, grads[t], dev)
        opt.accumulate()
        assert all(p.grad is None for p in ps)
    opt.accumulate_end()
    for i, p in enumerate(ps):
        terms = [grads[t][i].double() for t in range(k) if grads[t][i] is not None]
        if not terms:
            assert p.grad is None, i
            assert not bool(_acc(opt, p).any()), i
            continue
        want = torch.stack(terms).sum(0)
        bound = k * 2.0 ** -24 * torch.stack(terms).abs().sum(0)
        acc = _acc(opt, p).detach().cpu()
        err = (acc.double() - want).abs()
        print(f"accumulate k={k} param[{i}] {dts[i]} n={SIZES[i]}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (i, float((err - bound).max()))
        assert p.grad is not None and p.grad.dtype == dts[i] and p.grad.shape == p.shape, i
        assert torch.equal(OC._bits(p.grad.detach().cpu()), OC._bits(acc.to(dts[i]))), i     # rounded to nearest even, once


def why_fp32_inputs(k=64, n=4099, seed=3):
    """bf16 gradients whose bf16 running sum (torch's own, on the CPU) loses more than one ulp: a large first term, then terms below half
    an ulp of the partial sums"""
    g = torch.Generator().manual_seed(seed)
    gs = [(torch.randn(n, generator=g).sign() * 256.0).to(BF16)] + [(torch.rand(n, generator=g) * 0.75 + 0.25).to(BF16) for _ in range(k - 1)]
    s64 = torch.stack([x.double() for x in gs]).sum(0)
    ulp = torch.exp2(torch.floor(torch.log2(s64.abs())) - 7)
    return gs, s64, ulp


def case_why_fp32(dev, k=64):
    gs, s64, ulp = why_fp32_inputs(k)
    run = gs[0].clone()
    for x in gs[1:]:
        run += x                                                 # what autograd's += does to a bf16 .grad
    off = ((run.double() - s64.to(BF16).double()).abs() / ulp).max()
    assert float(off) > 1.0, float(off)                         # inputs for which this does not hold prove nothing
    p = torch.nn.Parameter(torch.zeros(gs[0].numel(), dtype=BF16, device=dev))
    opt = FusedAdamW([p])
    opt.accumulate_begin()
    for x in gs:
        p.grad = x.clone().to(dev)
        opt.accumulate()
    opt.accumulate_end()
    err = ((p.grad.detach().cpu().double() - s64).abs() / ulp).max()
    print(f"k={k} bf16 gradients: torch's bf16 running sum is {float(off):.1f} ulps off, the materialised fp32 sum {float(err):.3f}")
    assert float(err) <= 1.0, float(err)


def case_nonfinite(dev, first, bad=float("inf")):
    """an inf in slice 2 of 3: the materialised gradient is not finite, step() is skipped on the device, every bit stays"""
    ps, opt, dts = _mixed(dev, first)
    grads = _grads(dts, 3, seed=4)
    for i in (2, 3):                                            # one bf16 and one fp32 gradient, vector part and tail
        grads[1][i][-1] = bad
        grads[1][i][8] = bad
    D = opt._one()

    def snapshot():
        out = [p.detach().clone() for p in ps]
        for p in ps:
            out += [v.clone() for kk, v in sorted(opt.state[p].items())]
        return out + [D.step_base.clone(), opt.step_count.clone()]

    before = snapshot()
    opt.accumulate_begin()
    for t in range(3):
        OC.set_grads(ps, grads[t], dev)
        opt.accumulate()
    opt.accumulate_end()
    for i in (2, 3):
        assert not bool(torch.isfinite(ps[i].grad[-1])) and not bool(torch.isfinite(ps[i].grad[8])), i
    opt.step()
    after = snapshot()
    assert all(torch.equal(OC._bits(a), OC._bits(b)) for a, b in zip(before, after))
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 0


def case_noop_equivalence(dev, first, steps=2):
    """the same gradients through an optimizer that never accumulates and through begin / accumulate / end around each single backward:
    the same parameter bits (fp32 gradients: a copy through the accumulator; bf16: one exact round trip) -- and the plain optimizer has
    no accumulator"""
    a, oa, dts = _mixed(dev, first)
    b, ob, _ = _mixed(dev, first)
    where = []
    for gs in _grads(dts, steps, seed=5):
        OC.set_grads(a, gs, dev)
        oa.step()
        ob.accumulate_begin()
        OC.set_grads(b, gs, dev)
        ob.accumulate()
        ob.accumulate_end()
        for q, g in zip(b, gs):
            assert torch.equal(OC._bits(q.grad.detach().cpu()), OC._bits(g)), "one pass through the fp32 sum is exact"
        where.append([q.grad.data_ptr() for q in b])
        ob.step()
        oa.zero_grad()
        ob.zero_grad()
    assert oa._one().acc is None and not oa._one().acc_grad
    assert int(oa.step_count) == int(ob.step_count) == steps
    for x, y in zip(a, b):
        assert torch.equal(OC._bits(x.detach()), OC._bits(y.detach()))
        for kk in oa.state[x]:
            assert torch.equal(OC._bits(oa.state[x][kk]), OC._bits(ob.state[y][kk])), kk
    assert set(map(str, ob.state_dict())) == set(map(str, oa.state_dict()))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} | ({"master"} if "master" in s else set()) for s in ob.state_dict()["state"].values())
    # from the second step on accumulate_end() writes to the addresses it wrote to before
    assert where[0] == where[-1]


def case_open_accumulation_raises(dev):
    p = torch.nn.Parameter(torch.zeros(9, device=dev))
    opt = FusedAdamW([p])
    with pytest.raises(RuntimeError, match="accumulate_begin"):
        opt.accumulate()
    opt.accumulate_begin()
    p.grad = torch.ones(9, device=dev)
    with pytest.raises(RuntimeError, match="between accumulate_begin"):
        opt.step()
    with pytest.raises(RuntimeError, match="not taken"):
        opt.accumulate_end()
    opt.accumulate()
    opt.accumulate_end()
    assert torch.equal(p.grad.cpu(), torch.ones(9))
    opt.step()


# ---- the step ------------------------------------------------------------------------------------------------------------------------------
def head_cfg(cfg, head):
    return dataclasses.replace(cfg, decoupled_contrastive_learning=(head == "dcl"))


def _state_dict(cfg, head, dtype, seed=11):
    sd = O.make_state_dict(cfg, seed, F32)
    if head == "sigmoid":
        sd = dict(sd, temperature=torch.tensor(math.log(10.0)), logit_bias=torch.tensor(-10.0))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def build(dev, dtype, cfg, head, patch_dropout=0.0, **extra):
    if head == "sigmoid":
        extra["sigmoid_loss"] = True
    sd = _state_dict(cfg, head, dtype)
    return C.build_clip(head_cfg(cfg, head), {k: v.float() for k, v in sd.items()}, dev, dtype, patch_dropout=patch_dropout, **extra)


def batch(cfg, b, dtype, seed=12):
    text, image, _, _ = O.make_inputs(cfg, b, seed)
    return text, image.to(dtype)


def grads_of(model):
    return {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in model.named_parameters()}


@_once
def oracle(cfg, head, dtype, b, keep_seed=None, keep_n=None):
    """fp64 loss and gradients on the dtype-rounded parameters and inputs (bf16: with the bf16 LayerNorm epsilon, as clip_cases);
    the sigmoid head is the dense fp64 formula of tests/sigloss_cases.py on the oracle's latents.  Computed once per case, shared."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in _state_dict(cfg, head, dtype).items()}
    text, image = batch(cfg, b, dtype)
    keep = None
    if keep_seed is not None:
        keep = torch.randn(b, cfg.num_patches, generator=torch.Generator().manual_seed(keep_seed)).topk(keep_n, dim=-1).indices
    with O.layer_norm_eps(1e-5 if dtype == F32 else 1e-3):
        if head != "sigmoid":
            loss, grads = C.oracle_run(head_cfg(cfg, head), sd, text, image.double(), [], [], keep)
        else:
            import sigloss_cases as S
            sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
            tl, il = O.clip_forward(sd, cfg, text, image.double(), keep_idx=keep, return_latents=True)
            loss = S.dense_loss(tl[None], il[None], sd["temperature"], sd["logit_bias"], 1.0, 0.0)
            loss.backward()
            loss, grads = loss.detach(), {k: v.grad for k, v in sd.items() if v.is_floating_point()}
    return float(loss), grads


def compare(tag, dtype, loss, grads, ref_loss, ref_grads, strict_none=True):
    """DESIGN.md section 7's bars; every parameter has a gradient where the reference has one and none where it has none"""
    fp32 = dtype == F32
    err = abs(loss - ref_loss) / max(1.0, abs(ref_loss))
    worst = (0.0, "", 1.0, "")
    fails = [] if err < (1e-5 if fp32 else 3e-4) else [("loss", loss, ref_loss)]
    for k, g in grads.items():
        rg = ref_grads.get(k)
        if rg is None or float(rg.abs().max()) == 0.0:
            assert g is None or (not strict_none and float(g.abs().max()) == 0.0), (tag, k, "has a gradient the reference has not")
            continue
        assert g is not None, (tag, k, "has no gradient")
        assert bool(torch.isfinite(g).all()), (tag, k)
        if float(rg.norm()) < 1e-12:
            continue
        rel = float((g - rg).norm() / rg.norm())
        cos = float((g * rg).sum() / (g.norm() * rg.norm())) if g.numel() > 1 else 1.0
        if rel > worst[0]:
            worst = (rel, k, worst[2], worst[3])
        if cos < worst[2]:
            worst = (worst[0], worst[1], cos, k)
        if not (rel < 3e-4 if fp32 else (rel < 0.08 and cos > 0.999)):
            fails.append((k, rel, cos))
    print(f"{tag}: loss err {err:.2e} | worst rel {worst[0]:.2e} ({worst[1]}) | lowest cos {worst[2]:.6f} ({worst[3]})")
    assert not fails, (tag, fails)


def one_pass(dev, dtype, cfg, head, b, keep=None, seeds=None, **extra):
    model = build(dev, dtype, cfg, head, **extra)
    text, image = batch(cfg, b, dtype)
    if keep is not None:
        model.visual_transformer.keep_indices_override = keep.to(torch.int32).to(dev)
    loss = model(text.to(dev), image.to(dev), return_loss=True)
    loss.backward()
    return float(loss.detach()), grads_of(model)


@_once
def one_pass_cached(dev, dtype, cfg, head, b):
    return one_pass(dev, dtype, cfg, head, b)


def cached_step(dev, dtype, cfg, head, b, micro, keep=None, track=False, freeze_image=False, verify=False, **extra):
    model = build(dev, dtype, cfg, head, **extra)
    if track:
        model.track_metrics((1, 2))
    if keep is not None:
        model.visual_transformer.keep_indices_override = keep.to(torch.int32).to(dev)
    opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
    step = CachedContrastiveStep(model, opt, micro_batch=micro)
    step.verify_replay = verify
    text, image = batch(cfg, b, dtype)
    loss = step.step(text.to(dev), image.to(dev), freeze_image_encoder=freeze_image)
    assert loss.dtype == F32 and loss.dim() == 0 and not loss.requires_grad and loss.device.type == dev.type
    return float(loss), grads_of(model), model, opt, step


def case_step(dev, dtype, cfg, head, micro, b=8):
    loss, grads, model, opt, _ = cached_step(dev, dtype, cfg, head, b, micro)
    tag = f"cached {head} {'fp32' if dtype == F32 else 'bf16'} b={b} micro={micro}"
    l1, g1 = one_pass_cached(dev, dtype, cfg, head, b)
    assert grads["temperature"] is not None and (head != "sigmoid" or grads["logit_bias"] is not None)
    compare(tag + " vs one pass", dtype, loss, grads, l1, g1)
    compare(tag + " vs oracle", dtype, loss, grads, *oracle(cfg, head, dtype, b), strict_none=False)
    for p in model.parameters():                                # .grad is the parameter's dtype, ready for step()
        assert p.grad is None or p.grad.dtype == p.dtype
    opt.step()
    assert int(opt.step_count) == 1 and int(opt.skipped_steps) == 0


def injected_keep(cfg, b, seed=13):
    n = max(1, cfg.num_patches // 2)
    return torch.randn(b, cfg.num_patches, generator=torch.Generator().manual_seed(seed)).topk(n, dim=-1).indices, seed, n


def case_replay(dev, dtype, cfg, head="infonce", micro=3, b=8):
    """patch dropout 0.5, attention / feed-forward dropout 0.1: the second pass repeats the first bit for bit (its own draws: the seeds
    and the PatchDropout set come from the restored generators), and a replay that draws afresh is caught"""
    from x_clip_amd import functional as XF
    drop = dict(patch_dropout=0.5)
    model = build(dev, dtype, cfg, head, **drop)
    for t in (model.text_transformer.transformer, model.visual_transformer.transformer):
        _set_dropout(t, 0.1)
    opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3)
    step = CachedContrastiveStep(model, opt, micro_batch=micro)
    step.verify_replay = True
    text, image = batch(cfg, b, dtype)
    torch.manual_seed(77)
    loss = step.step(text.to(dev), image.to(dev))
    assert float(step.last_replay_diff) == 0.0, float(step.last_replay_diff)
    assert math.isfinite(float(loss)) and all(p.grad is not None for p in model.visual_transformer.parameters())
    # the check has teeth: a replay that draws fresh seeds / a fresh PatchDropout set does not reproduce the latents
    opt.zero_grad()
    real = step._set_rng_state
    step._set_rng_state = lambda state, device: None
    try:
        step.step(text.to(dev), image.to(dev))
    finally:
        step._set_rng_state = real
    assert float(step.last_replay_diff) > 0.0
    del XF


def _set_dropout(transformer, p):
    """attention and feed-forward dropout of a built stack (the toy models are built by clip_cases without the keywords)"""
    assert hasattr(transformer, "attn_dropout") and hasattr(transformer, "ff_dropout"), "Transformer keeps its dropout rates as attributes"
    transformer.attn_dropout = transformer.ff_dropout = p


def case_replay_injected(dev, dtype, cfg, head="infonce", micro=3, b=8):
    """the same injected PatchDropout set in the cached and the one-pass step: gradients within the bars of the one-pass step"""
    keep, seed, n = injected_keep(cfg, b)
    loss, grads, _, _, step = cached_step(dev, dtype, cfg, head, b, micro, keep=keep, verify=True, patch_dropout=0.5)
    assert float(step.last_replay_diff) == 0.0
    l1, g1 = one_pass(dev, dtype, cfg, head, b, keep=keep, patch_dropout=0.5)
    tag = f"cached {head} injected patch dropout {'fp32' if dtype == F32 else 'bf16'} micro={micro}"
    compare(tag + " vs one pass", dtype, loss, grads, l1, g1)
    compare(tag + " vs oracle", dtype, loss, grads, *oracle(cfg, head, dtype, b, seed, n), strict_none=False)


def case_freeze_image(dev, dtype, cfg, micro=4, b=8):
    loss, grads, model, _, _ = cached_step(dev, dtype, cfg, "infonce", b, micro, freeze_image=True)
    assert all(p.grad is None for p in model.visual_transformer.parameters())
    assert model.to_visual_latent.weight.grad is not None and all(p.grad is not None for p in model.text_transformer.parameters())
    ref = build(dev, dtype, cfg, "infonce")
    text, image = batch(cfg, b, dtype)
    l1 = ref(text.to(dev), image.to(dev), return_loss=True, freeze_image_encoder=True)
    l1.backward()
    compare("cached freeze_image_encoder vs one pass", dtype, loss, grads, float(l1.detach()), grads_of(ref))


def _same_bits(a, b, dev, dtype):
    """the same loss bits and the same gradient bits -- except the fp32 gradients whose backward adds floats atomically (tests/metrics_cases.py
    _atomic_grad; on the emulator the temperature's alone): those differ in the last bit between two runs of the one-pass step too, with
    everything off, and are held to the bar the existing same-bits tests hold them to (rtol 1e-4, atol 1e-6)"""
    from metrics_cases import _atomic_grad
    (la, ga), (lb, gb) = a, b
    assert la == lb, (la, lb)
    assert set(ga) == set(gb)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is None:
            continue
        if dtype == F32 and (k == "temperature" or (dev.type == "cuda" and _atomic_grad(k))):
            torch.testing.assert_close(ga[k], gb[k], rtol=1e-4, atol=1e-6)
        else:
            assert torch.equal(ga[k], gb[k]), k


def case_track_metrics_same_bits(dev, dtype, cfg, head="infonce", micro=3, b=8):
    off = cached_step(dev, dtype, cfg, head, b, micro)
    on = cached_step(dev, dtype, cfg, head, b, micro, track=True)
    _same_bits(off[:2], on[:2], dev, dtype)
    m = on[2].last_metrics
    assert m is not None and off[2].last_metrics is None


def case_checkpoint_same_bits(dev, dtype, cfg, head="infonce", micro=3, b=8):
    off = cached_step(dev, dtype, cfg, head, b, micro)
    on = cached_step(dev, dtype, cfg, head, b, micro, checkpoint_during_training=True)
    _same_bits(off[:2], on[:2], dev, dtype)


def case_raises(dev):
    for over, name in ((dict(use_all_token_embeds=True), "use_all_token_embeds"), (dict(use_mlm=True), "use_mlm"),
                       (dict(use_visual_ssl=True), "use_visual_ssl"), (dict(extra_latent_projection=True), "extra_latent_projection"),
                       (dict(extra_latent_projection=True, sim_reg_loss_weight=0.5), "sim_reg_loss_weight")):
        cfg = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1, **over)
        model = C.build_clip(cfg, O.make_state_dict(cfg, 11, F32), dev, F32)
        opt = FusedAdamW(model.parameters())
        with pytest.raises(NotImplementedError, match=name):
            CachedContrastiveStep(model, opt, micro_batch=4)
    import inspect
    assert "aug_text" not in inspect.signature(CachedContrastiveStep.step).parameters
    assert "aug_image" not in inspect.signature(CachedContrastiveStep.step).parameters


def case_memory(dev, cfg=MID, b=256, micro=32):
    """GPU: peak allocated memory of the cached step strictly below the one-pass step's, same process, same model and batch"""
    model = build(dev, BF16, cfg, "infonce")
    text, image = batch(cfg, b, BF16)
    text, image = text.to(dev), image.to(dev)
    opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3)
    peaks = {}
    for which in ("one pass", "cached"):
        opt.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if which == "one pass":
            model(text, image, return_loss=True).backward()
        else:
            CachedContrastiveStep(model, opt, micro_batch=micro).step(text, image)
        torch.cuda.synchronize()
        peaks[which] = torch.cuda.max_memory_allocated() - base
    print(f"peak allocated above the resident state, b={b}: one pass {peaks['one pass'] / 2**20:.1f} MiB, cached (micro {micro}, "
          f"fp32 accumulator included) {peaks['cached'] / 2**20:.1f} MiB")
    assert torch.cuda.max_memory_allocated() > 0 and peaks["cached"] < peaks["one pass"], peaks


# ---- two ranks (worker of tests/test_cached_dist.py) ----------------------------------------------------------------------------------------
def worker_two_ranks(rank, world, port, head, sizes, tmp, kind="cpu"):
    import dist_cases as D
    dev = D.setup(rank, world, port, kind)
    import torch.distributed as dist
    from x_clip_amd.distributed import GradSync
    cfg = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)
    text, image = batch(cfg, sum(sizes), F32)
    lo = sum(sizes[:rank])
    text, image = text[lo: lo + sizes[rank]].to(dev), image[lo: lo + sizes[rank]].to(dev)
    out = {}
    for which in ("one pass", "cached"):
        model = build(dev, F32, cfg, head)                     # AFTER init_process_group: requires_all_gather is latched
        assert model.requires_all_gather
        sync = GradSync(model, overlap=False)
        opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3)
        if which == "one pass":
            loss = model(text, image, return_loss=True)
            loss.backward()
        else:
            greedy = GradSync(model)                            # an overlapping sync is refused
            try:
                with pytest.raises(ValueError, match="overlap=False"):
                    CachedContrastiveStep(model, opt, micro_batch=2, sync=greedy)
                with pytest.raises(ValueError, match="overlap=False"):
                    CachedContrastiveStep(model, opt, micro_batch=2)
            finally:
                greedy.remove()
            loss = CachedContrastiveStep(model, opt, micro_batch=2, sync=sync).step(text, image)
        sync.finish()
        out[which] = (float(loss.detach()), grads_of(model), dict(sync.stats))
        sync.remove()
    torch.save(out, os.path.join(tmp, f"rank{rank}.pt"))
    dist.destroy_process_group()


def check_two_ranks(tmp, head, world=2):
    outs = [torch.load(os.path.join(tmp, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    for r, o in enumerate(outs):
        compare(f"two ranks {head} rank {r}: cached vs one pass", F32, o["cached"][0], o["cached"][1], o["one pass"][0], o["one pass"][1])
        assert o["cached"][2]["in_place"] > 0, o["cached"][2]    # accumulate_end() wrote into GradSync's slices
    (la, ga, _), (lb, gb, _) = outs[0]["cached"], outs[1]["cached"]
    assert la == lb
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        assert ga[k] is None or torch.equal(ga[k], gb[k]), k
