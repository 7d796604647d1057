"""Cases for the weight EMA of x_clip_amd.optim.FusedAdamW (`ema_decay`, `ema_warmup`, `ema_weights()`; adamw_ema_kernel in
csrc/kernels/optim.h), shared by tests/test_ema_emu.py (CPU, wave64 emulator) and tests/test_ema_gpu.py (MI355X).

Reference (`reference_ema`): tests/optim_cases.py's -- clip_grad_norm_ + torch.optim.AdamW on the CPU in fp64 -- stepped one step at a time;
after each step e += (1 - d_u)(p - e) in fp64 on the fp64 parameters that had a gradient, u = steps applied so far including this one,
d_u = min(decay, (1 + u) / (10 + u)) with warm-up, decay without.  For bf16 parameters that is the EMA of the fp64 masters' trajectory, not of
rounded parameters.  Bar: optim_cases.within_bar -- 4 x what the same loop costs torch in fp32 against fp64 plus one fp32 ulp of the
largest element, per tensor.  References are computed once per (case, dtype) and shared (`_cached`); nobody writes to them.
"""
import copy

import torch

import optim_cases as OC
from optim_cases import GROUP_OF, GROUPS, HYPER, MAX_NORM, REPORT, FusedAdamW, _bits, make_grads, make_params, set_grads, within_bar

_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def decay_at(u, decay, warmup):
    return min(decay, (1.0 + u) / (10.0 + u)) if warmup else decay


def reference_ema(params, grads, dtype, decay, warmup, max_norm=MAX_NORM, group_of=GROUP_OF, groups=GROUPS, state_from=None, ema_from=None,
                  applied=0):
    """-> (parameters, ema) after the steps of `grads` (a list per step; an entry None = no gradient in that step: not averaged), all in
    `dtype`.  `applied`: steps applied before these (`state_from` / `ema_from`: the state they left)."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    opt = torch.optim.AdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], **groups[k]) for k in range(len(groups))],
                            foreach=False, **HYPER)
    if state_from is not None:
        opt.load_state_dict(copy.deepcopy(state_from))
    ema = [p.detach().clone() for p in ps] if ema_from is None else [e.detach().cpu().to(dtype).clone() for e in ema_from]
    for u, gs in enumerate(grads, start=applied + 1):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm, foreach=False)
        opt.step()
        omd = 1.0 - decay_at(u, decay, warmup)
        if dtype == torch.float32:
            omd = float(torch.tensor(omd, dtype=torch.float32))    # (the fp32 loop holds its coefficient in fp32, as the moments' are held)
        for p, e, g in zip(ps, ema, gs):
            if g is not None:
                e.add_((p.detach() - e) * omd)
    return [p.detach() for p in ps], ema


def fused(dev, params, decay, warmup, group_of=GROUP_OF, groups=GROUPS, max_norm=MAX_NORM):
    ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in params]
    kw = {} if decay is None else dict(ema_decay=decay, ema_warmup=warmup)
    opt = FusedAdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], **groups[k]) for k in range(len(groups))],
                     max_grad_norm=max_norm, **HYPER, **kw)
    return ps, opt


def _tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def _weight(opt, p):
    return opt.state[p]["master"] if p.dtype == torch.bfloat16 else p.detach()


def _ema_bits(ps, opt):
    return [opt.state[p]["ema"].detach().clone() for p in ps]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(dev, dtype, grads, decay, warmup, params=None):
    ps, opt = fused(dev, make_params(dtype) if params is None else params, decay, warmup)
    for gs in grads:
        set_grads(ps, gs, dev)
        opt.step()
    return ps, opt


# ---- 1: parity over 10 steps -------------------------------------------------------------------------------------------------------------
def case_parity(dev, dtype, decay, warmup, steps=10):
    tag = f"ema {_tag(dtype)} d={decay}{' warm-up' if warmup else ''}"
    params, grads = make_params(dtype), make_grads(dtype, steps)
    _, e64 = _cached(("parity", dtype, decay, warmup, 64), lambda: reference_ema(params, grads, torch.float64, decay, warmup))
    _, e32 = _cached(("parity", dtype, decay, warmup, 32), lambda: reference_ema(params, grads, torch.float32, decay, warmup))
    ps, opt = _run(dev, dtype, grads, decay, warmup)
    assert int(opt.step_count) == steps and int(opt.skipped_steps) == 0
    for i, p in enumerate(ps):
        e = opt.state[p]["ema"]
        assert e.dtype == torch.float32 and e.shape == p.shape
        within_bar(f"{tag} ema[{i}] {tuple(p.shape)}", e, e64[i], e32[i])
        assert not torch.equal(e.cpu(), _weight(opt, p).cpu().float()) or p.numel() == 0     # an average, not a copy of the weights


# ---- 2: the EMA does not disturb the update -----------------------------------------------------------------------------------------------
def case_update_untouched(dev, dtype, steps=10):
    grads = make_grads(dtype, steps)
    a, oa = _run(dev, dtype, grads, 0.99, True)
    b, ob = _run(dev, dtype, grads, None, True)
    for x, y in zip(a, b):
        assert _same_bits(x.detach(), y.detach())
        assert "ema" in oa.state[x] and "ema" not in ob.state[y]
        for k in ob.state[y]:
            assert _same_bits(oa.state[x][k], ob.state[y][k]), k
    assert _same_bits(oa.grad_norm, ob.grad_norm) and int(oa.step_count) == int(ob.step_count) == steps
    assert next(iter(ob._devs.values())).ema is None            # off: no array


# ---- 3: the reason for the feature -----------------------------------------------------------------------------------------------------------
def case_bf16_stall(dev, steps=200, decay=0.99):
    """the setting of optim_cases.case_bf16_stall: the fused EMA follows the fp64 EMA of the fp64 weights; an EMA kept in bf16 from the
    bf16 parameters (lerp_ each step) is more than 100 bars away (each increment is far below half a bf16 ulp: it never moves)"""
    g = torch.Generator().manual_seed(3)
    w0 = (torch.rand(1024, generator=g) * 1.5 + 0.5).to(torch.bfloat16)
    grad = torch.ones(1024, dtype=torch.bfloat16)
    groups, hyper = [dict(lr=1e-5, weight_decay=0.0)], [[grad]] * steps
    _, e64 = _cached(("stall", 64), lambda: reference_ema([w0], hyper, torch.float64, decay, False, None, [0], groups))
    _, e32 = _cached(("stall", 32), lambda: reference_ema([w0], hyper, torch.float32, decay, False, None, [0], groups))
    ps, opt = fused(dev, [w0], decay, False, [0], groups, None)
    naive = ps[0].detach().clone()                              # bf16, from the bf16 parameter
    for _ in range(steps):
        set_grads(ps, [grad], dev)
        opt.step()
        naive.lerp_(ps[0].detach(), 1.0 - decay)
    within_bar("ema bf16 stall: fused ema", opt.state[ps[0]]["ema"], e64[0], e32[0])
    bar = REPORT["ema bf16 stall: fused ema"]["bar_rel"]
    scale = float(e64[0].norm())
    naive_rel = float((naive.cpu().double() - e64[0]).norm()) / scale
    moved = float((e64[0] - w0.double()).abs().min())
    REPORT["ema bf16 stall"] = dict(fused_rel=REPORT["ema bf16 stall: fused ema"]["fused_rel"], bf16_ema_rel=naive_rel, bar_rel=bar, fp64_moved=moved)
    print(f"ema bf16 stall: fused {REPORT['ema bf16 stall']['fused_rel']:.3e} | bf16 EMA of the bf16 parameters {naive_rel:.3e} | bar {bar:.3e} "
          f"| the fp64 EMA moved >= {moved:.3e}")
    assert naive_rel > 100.0 * bar, (naive_rel, bar)


# ---- 4: a skipped step -------------------------------------------------------------------------------------------------------------------------
def case_skipped_step(dev, dtype, bad, steps=5, at=2, decay=0.9999):
    """warm-up on: the first steps run on (1 + u) / (10 + u), so a u advanced by the skipped step would show"""
    params, grads = make_params(dtype), make_grads(dtype, steps)
    seen = grads[:at] + grads[at + 1:]                          # the reference never sees the skipped step
    _, e64 = _cached(("skip", dtype, 64), lambda: reference_ema(params, seen, torch.float64, decay, True))
    _, e32 = _cached(("skip", dtype, 32), lambda: reference_ema(params, seen, torch.float32, decay, True))
    poisoned = [g.clone() for g in grads[at]]
    poisoned[5].view(-1)[70000] = bad
    ps, opt = fused(dev, params, decay, True)
    for t, gs in enumerate(grads):
        before = _ema_bits(ps, opt)
        set_grads(ps, poisoned if t == at else gs, dev)
        opt.step()
        after = _ema_bits(ps, opt)
        same = [_same_bits(a, b) for a, b in zip(before, after)]
        assert all(same) if t == at else not any(same), (t, same)
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == steps - 1
    for i, p in enumerate(ps):
        within_bar(f"ema skip({bad}) {_tag(dtype)} ema[{i}]", opt.state[p]["ema"], e64[i], e32[i])


# ---- 5: a parameter without a gradient ---------------------------------------------------------------------------------------------------------
def case_late_gradient(dev, dtype, late=3, steps=3, decay=0.9999):
    """optim_cases.case_late_gradient's layout: parameter `late` has no gradient in the first step.  u is the optimizer's applied step
    count, not the parameter's own: with warm-up the late parameter's first average uses (1 + 2) / (10 + 2)"""
    params, grads = make_params(dtype), make_grads(dtype, steps)
    grads[0][late] = None
    _, e64 = _cached(("late", dtype, 64), lambda: reference_ema(params, grads, torch.float64, decay, True))
    _, e32 = _cached(("late", dtype, 32), lambda: reference_ema(params, grads, torch.float32, decay, True))
    ps, opt = fused(dev, params, decay, True)
    start = _ema_bits(ps, opt)
    assert all(_same_bits(e.cpu(), p.float()) for e, p in zip(start, params))           # initialised to the weights: exact
    set_grads(ps, grads[0], dev)
    opt.step()
    first = _ema_bits(ps, opt)
    assert [_same_bits(a, b) for a, b in zip(start, first)] == [i == late for i in range(len(ps))]
    for gs in grads[1:]:
        set_grads(ps, gs, dev)
        opt.step()
    assert not _same_bits(first[late], opt.state[ps[late]]["ema"])
    for i, p in enumerate(ps):
        within_bar(f"ema late-gradient {_tag(dtype)} ema[{i}]", opt.state[p]["ema"], e64[i], e32[i])


# ---- 6: reproducible ---------------------------------------------------------------------------------------------------------------------------
def case_reproducible(dev, dtype, steps=3):
    grads = make_grads(dtype, steps)
    a, oa = _run(dev, dtype, grads, 0.99, True)
    b, ob = _run(dev, dtype, grads, 0.99, True)
    for x, y in zip(a, b):
        assert _same_bits(oa.state[x]["ema"], ob.state[y]["ema"])


# ---- 7: checkpoints ----------------------------------------------------------------------------------------------------------------------------
def _twin(ps, **kw):
    b = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    return b, FusedAdamW([dict(params=[p for p, gi in zip(b, GROUP_OF) if gi == k]) for k in range(len(GROUPS))], **kw)


def case_state_roundtrip(dev, dtype):
    grads = make_grads(dtype, 4)
    a, oa = _run(dev, dtype, grads[:3], 0.999, True)
    sd = oa.state_dict()
    assert sd["ema_decay"] == 0.999 and sd["ema_warmup"] is True
    views = {oa.state[p]["ema"].data_ptr() for p in a}
    assert len(sd["state"]) == len(a) and all(s["ema"].dtype == torch.float32 and s["ema"].data_ptr() not in views for s in sd["state"].values())
    b, ob = _twin(a, ema_decay=0.5, ema_warmup=False)           # other settings: the loaded ones must win
    ob.load_state_dict(sd)
    assert ob.ema_decay == 0.999 and ob.ema_warmup is True and int(ob.step_count) == 3
    for x, y in zip(a, b):
        assert _same_bits(oa.state[x]["ema"], ob.state[y]["ema"])
    for ps, o in ((a, oa), (b, ob)):
        set_grads(ps, grads[3], dev)
        o.step()
    for x, y in zip(a, b):
        assert _same_bits(x.detach(), y.detach())
        for k in oa.state[x]:
            assert _same_bits(oa.state[x][k], ob.state[y][k]), k
    c, oc = _twin(a)                                            # built without EMA: a dict's `ema` is ignored
    oc.load_state_dict(oa.state_dict())
    assert oc.ema_decay is None and all("ema" not in oc.state[p] for p in c)


def case_load_without_ema(dev, dtype):
    grads = make_grads(dtype, 3)
    a, oa = _run(dev, dtype, grads, None, True)
    sd = oa.state_dict()
    assert "ema_decay" not in sd and all("ema" not in s for s in sd["state"].values())
    b, ob = _twin(a, ema_decay=0.99, ema_warmup=False)
    for p in b:
        ob.state[p]["ema"].fill_(7.0)                           # (whatever it held)
    ob.load_state_dict(sd)
    assert ob.ema_decay == 0.99 and ob.ema_warmup is False      # the dict has none: the constructor's stay
    for x, y in zip(a, b):
        assert _same_bits(ob.state[y]["ema"], _weight(oa, x).float())


def case_load_torch_adamw(dev):
    params, grads = make_params(torch.float32), make_grads(torch.float32, 4)
    mid, _, _, _, topt = OC.reference(params, grads[:3], torch.float32)
    sd = copy.deepcopy(topt.state_dict())
    ps, opt = fused(dev, mid, 0.9999, True)                     # warm-up: the next step's u = 4 comes from the loaded step counts
    for p in ps:
        opt.state[p]["ema"].fill_(7.0)
    opt.load_state_dict(sd)
    for p, m in zip(ps, mid):
        assert _same_bits(opt.state[p]["ema"].cpu(), m)
    set_grads(ps, grads[3], dev)
    opt.step()
    _, e64 = reference_ema(mid, [grads[3]], torch.float64, 0.9999, True, state_from=sd, applied=3)
    _, e32 = reference_ema(mid, [grads[3]], torch.float32, 0.9999, True, state_from=sd, applied=3)
    for i, p in enumerate(ps):
        within_bar(f"ema after torch.optim.AdamW state ema[{i}]", opt.state[p]["ema"], e64[i], e32[i])


# ---- 8: ema_weights() ----------------------------------------------------------------------------------------------------------------------------
def case_ema_weights(dev, dtype, idle=1):
    """parameter `idle` never gets a gradient (step_base < 0): it is swapped too, its EMA is its initial value"""
    import pytest
    grads = make_grads(dtype, 4)
    for gs in grads:
        gs[idle] = None
    a, oa = _run(dev, dtype, grads[:3], 0.9, False)
    b, ob = _run(dev, dtype, grads[:3], 0.9, False)             # never enters the context
    before = [p.detach().clone() for p in a]
    ptrs = [p.data_ptr() for p in a]
    with oa.ema_weights():
        for i, p in enumerate(a):
            assert _same_bits(p.detach(), oa.state[p]["ema"].to(dtype)), i
        same = [_same_bits(p.detach(), q) for p, q in zip(a, before)]
        assert same[idle] and not same[3] and not same[5], same  # (a small bf16 tensor's rounded EMA may be its rounded master)
        with pytest.raises(RuntimeError, match="ema_weights"):
            oa.step()
        with pytest.raises(RuntimeError, match="already active"):
            with oa.ema_weights():
                pass
    assert [p.data_ptr() for p in a] == ptrs
    for p, q in zip(a, before):
        assert _same_bits(p.detach(), q)
    try:                                                        # an exception inside restores too
        with oa.ema_weights():
            raise KeyError("x")
    except KeyError:
        pass
    for p, q in zip(a, before):
        assert _same_bits(p.detach(), q)
    uploads = oa.table_uploads
    for ps, o in ((a, oa), (b, ob)):
        set_grads(ps, grads[3], dev)
        o.step()
    for x, y in zip(a, b):
        assert _same_bits(x.detach(), y.detach())
        for k in oa.state[x]:
            assert _same_bits(oa.state[x][k], ob.state[y][k]), k
    assert int(oa.step_count) == 4 and oa.table_uploads - uploads == ob.table_uploads - uploads
    plain = fused(dev, make_params(dtype), None, True)[1]
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


def case_invalid_decay(dev):
    import pytest
    p = torch.nn.Parameter(torch.zeros(4, device=dev))
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW([p], ema_decay=bad)
    assert FusedAdamW([p], ema_decay=0.0).ema_decay == 0.0


# ---- 9: end to end -------------------------------------------------------------------------------------------------------------------------------
def case_end_to_end(dev, cfg, batch=4, steps=3, max_norm=1.0, decay=0.9):
    """three fp32 training steps of the small CLIP.  The model is the source of the gradients: each step's are read back and the
    reference (fp64, and fp32 for the bar) takes the same steps on the same gradients, as in every other case here."""
    build, text, image = OC._clip_and_batch(dev, torch.float32, cfg, batch)
    model = build()
    names = [k for k, _ in model.named_parameters()]
    ps = [p for _, p in model.named_parameters()]
    groups = FusedAdamW.default_param_groups(model, 0.1)
    group_of = [0 if any(p is q for q in groups[0]["params"]) else 1 for p in ps]
    hyper = [dict(lr=1e-3, weight_decay=g["weight_decay"]) for g in groups]
    start = [p.detach().cpu().clone() for p in ps]
    opt = FusedAdamW(groups, lr=1e-3, max_grad_norm=max_norm, ema_decay=decay, ema_warmup=False)
    grads = []
    for _ in range(steps):
        model(text, image, return_loss=True).backward()
        grads.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in ps])
        opt.step()
        opt.zero_grad()
    assert int(opt.step_count) == steps
    _, e64 = reference_ema(start, grads, torch.float64, decay, False, max_norm, group_of, hyper)
    _, e32 = reference_ema(start, grads, torch.float32, decay, False, max_norm, group_of, hyper)
    averaged = 0
    for i, (k, p) in enumerate(zip(names, ps)):
        e = opt.state[p]["ema"]
        if all(gs[i] is None for gs in grads):                  # never had a gradient: the EMA is the initial value
            assert _same_bits(e.cpu(), start[i]), k
            continue
        averaged += 1
        within_bar(f"ema end to end {k}", e, e64[i], e32[i])
    assert averaged > 0
    twin = build()
    twin.load_state_dict({**model.state_dict(), **{k: opt.state[p]["ema"].detach().clone() for k, p in zip(names, ps)}}, strict=True)
    twin.eval()
    model.eval()
    outside = model.embed_text(text)
    with opt.ema_weights():
        inside = model.embed_text(text)
    want = twin.embed_text(text)
    assert _same_bits(inside, want)
    assert not _same_bits(inside, outside)                      # the averaged weights are not the trained ones
    assert _same_bits(model.embed_text(text), outside)          # and leaving the context brings the trained ones back
