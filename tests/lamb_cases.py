"""Cases for the param-group keys `trust_ratio` (LAMB) and `bounds` of x_clip_amd.optim.FusedAdamW (lamb_norm_kernel, lamb_fold_kernel,
optim_update_kernel in csrc/kernels/optim.h), shared by tests/test_lamb_emu.py (CPU, wave64 emulator) and tests/test_lamb_gpu.py (MI355X).

Reference (`reference`): a plain-torch restatement of the formula on top of torch.nn.utils.clip_grad_norm_, run on the CPU in fp64:

    g = clip_coef grad;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2        (bias corrections by the parameter's own step count t)
    trust_ratio:  u = (m / bc1) / (sqrt(v / bc2) + eps) + wd w;  r = |w| / |u| (1 if either is 0);  w -= lr r u
    otherwise:    torch.optim.AdamW's update in its operation order
    bounds:       w = min(max(w, lo), hi), lo rounded up / hi rounded down to the parameter's storage type (`storage_bound`)
    ema:          e += (1 - d_u)(w - e) on the clamped w, as tests/ema_cases.py states it

The same code run in fp32 measures what fp32 costs; every comparison is optim_cases.within_bar (4 x that cost + one fp32 ulp of the largest
element).  Without either key the reference is optim_cases.reference's torch.optim.AdamW to the last bit (`case_reference_is_adamw`).
"""
import copy
import math

import pytest
import torch

import optim_cases as OC
from ema_cases import decay_at
from optim_cases import GROUP_OF, HYPER, MAX_NORM, SHAPES, FusedAdamW, _bits, make_grads, make_params, set_grads, within_bar

BF16 = torch.bfloat16
LAMB_GROUPS = [dict(lr=1e-3, weight_decay=0.1, trust_ratio=True), dict(lr=3e-3, weight_decay=0.0)]
LN100 = math.log(100.0)
_ALL_BF16 = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16).double()
_ALL_BF16 = _ALL_BF16[torch.isfinite(_ALL_BF16)]


def storage_bound(x, dtype, up):
    """the value a weight stored as `dtype` can hold that is nearest to x on the side asked for (None: no bound on that side)"""
    if x is None:
        return -math.inf if up else math.inf
    if dtype == BF16:                                           # (by search over all bf16 values: independent of the optimizer's bit arithmetic)
        return float(_ALL_BF16[_ALL_BF16 >= x].min() if up else _ALL_BF16[_ALL_BF16 <= x].max())
    f = torch.tensor(x, dtype=torch.float64).to(torch.float32)
    if (float(f) < x and up) or (float(f) > x and not up):
        f = torch.nextafter(f, torch.tensor(math.inf if up else -math.inf, dtype=torch.float32))
    return float(f)


def reference(params, grads, dtype, groups, group_of, max_norm=MAX_NORM, ema_decay=None, ema_warmup=False, state_from=None, store=None,
              each_step=None):
    """-> dict(p, m, v, ratio, ema, norms) after the steps of `grads` (a list per step; an entry None = no gradient), all in `dtype`.
    `store`: the dtype the fused parameters are stored in (bounds are rounded to it); `state_from`: (m, v, t) lists to continue from;
    `each_step(step, p)`: called with the weights after every step."""
    b1, b2 = HYPER["betas"]
    eps = HYPER["eps"]
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    store = store or params[0].dtype
    if state_from is None:
        m, v, t = [torch.zeros_like(p.data) for p in ps], [torch.zeros_like(p.data) for p in ps], [0] * len(ps)
    else:
        m, v, t = [x.detach().cpu().to(dtype).clone() for x in state_from[0]], [x.detach().cpu().to(dtype).clone() for x in state_from[1]], list(state_from[2])
    ratio = torch.ones(len(ps), dtype=dtype)
    ema = [p.detach().clone() for p in ps]
    norms, applied = [], max(t, default=0)
    for step, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        live = [p for p in ps if p.grad is not None]
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False).detach().clone())
        else:
            norms.append(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in live])))
        applied += 1
        omd = 1.0 - decay_at(applied, ema_decay, ema_warmup) if ema_decay is not None else None
        if omd is not None and dtype == torch.float32:
            omd = float(torch.tensor(omd, dtype=torch.float32))
        with torch.no_grad():
            for i, p in enumerate(ps):
                if p.grad is None:
                    continue
                G, g, w = groups[group_of[i]], p.grad, p.data
                lr, wd = G["lr"], G["weight_decay"]
                t[i] += 1
                bc1, bc2 = 1.0 - b1 ** t[i], 1.0 - b2 ** t[i]
                if G.get("trust_ratio", False):
                    m[i].mul_(b1).add_(g, alpha=1.0 - b1)
                    v[i].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                    u = (m[i] / bc1) / ((v[i] / bc2).sqrt() + eps) + wd * w
                    wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
                    r = wn / un if float(wn) > 0.0 and float(un) > 0.0 else torch.ones((), dtype=dtype)
                    ratio[i] = r
                    w.sub_(u * (lr * r))
                else:                                           # torch.optim.AdamW (_single_tensor_adam), operation for operation
                    w.mul_(1.0 - lr * wd)
                    m[i].lerp_(g, 1.0 - b1)
                    v[i].mul_(b2).addcmul_(g, g.conj(), value=1.0 - b2)
                    w.addcdiv_(m[i], (v[i].sqrt() / math.sqrt(bc2)).add_(eps), value=-(lr / bc1))
                if G.get("bounds") is not None:
                    w.clamp_(storage_bound(G["bounds"][0], store, True), storage_bound(G["bounds"][1], store, False))
                if omd is not None:
                    ema[i].add_((w - ema[i]) * omd)
        if each_step is not None:
            each_step(step, [p.detach() for p in ps])
    return dict(p=[p.detach() for p in ps], m=m, v=v, ratio=ratio, ema=ema, norms=norms, t=t)


def fused(dev, params, groups, group_of, max_norm=MAX_NORM, **kw):
    ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in params]
    opt = FusedAdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], **groups[k]) for k in range(len(groups))],
                     max_grad_norm=max_norm, **HYPER, **kw)
    return ps, opt


def _tag(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _weight(opt, p):
    return opt.state[p]["master"] if p.dtype == BF16 else p.detach()


def _ratios(opt, ps):
    return torch.stack([opt.state[p]["trust_ratio"].detach().cpu() for p in ps])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _snapshot(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.detach().clone() for _, v in sorted(opt.state[p].items())]
    D = opt._one()
    return out + [D.ratio.clone(), D.step_base.clone(), opt.step_count.clone()]


def _check_rounded(ps, opt, where):
    for i, p in enumerate(ps):
        if p.dtype == BF16:                                     # the parameter IS the rounded master
            assert torch.equal(p.detach(), opt.state[p]["master"].to(BF16)), (where, i)


def _compare(tag, ps, opt, r64, r32, ema=False, moments=True):
    for i, p in enumerate(ps):
        within_bar(f"{tag} param[{i}] {tuple(p.shape)}", _weight(opt, p), r64["p"][i], r32["p"][i])
        if moments:
            within_bar(f"{tag} exp_avg[{i}]", opt.state[p]["exp_avg"], r64["m"][i], r32["m"][i])
            within_bar(f"{tag} exp_avg_sq[{i}]", opt.state[p]["exp_avg_sq"], r64["v"][i], r32["v"][i])
        if ema:
            within_bar(f"{tag} ema[{i}]", opt.state[p]["ema"], r64["ema"][i], r32["ema"][i])
    got = _ratios(opt, ps)
    assert got.dtype == torch.float32 and got.shape == (len(ps),) and bool(torch.isfinite(got).all())
    within_bar(f"{tag} trust ratios", got, r64["ratio"], r32["ratio"])


# ---- 0: the reference itself ---------------------------------------------------------------------------------------------------------------
def case_reference_is_adamw():
    """without the keys `reference` is clip_grad_norm_ + torch.optim.AdamW (optim_cases.reference), bit for bit, in fp64 and in fp32"""
    params, grads = make_params(torch.float32), make_grads(torch.float32, 4)
    for dtype in (torch.float64, torch.float32):
        p, m, v, n, _ = OC.reference(params, grads, dtype)
        r = reference(params, grads, dtype, OC.GROUPS, GROUP_OF)
        for i in range(len(params)):
            assert torch.equal(p[i], r["p"][i]) and torch.equal(m[i], r["m"][i]) and torch.equal(v[i], r["v"][i]), (dtype, i)
        assert all(torch.equal(a, b) for a, b in zip(n, r["norms"])) and bool((r["ratio"] == 1).all())


# ---- 1: LAMB parity ------------------------------------------------------------------------------------------------------------------------
def case_parity(dev, dtype, steps=10):
    tag = f"lamb {_tag(dtype)}"
    params, grads = make_params(dtype), make_grads(dtype, steps)
    r64 = reference(params, grads, torch.float64, LAMB_GROUPS, GROUP_OF)
    r32 = reference(params, grads, torch.float32, LAMB_GROUPS, GROUP_OF)
    ps, opt = fused(dev, params, LAMB_GROUPS, GROUP_OF)
    clipped = 0
    for t, gs in enumerate(grads):
        set_grads(ps, gs, dev)
        opt.step()
        within_bar(f"{tag} grad_norm step {t}", opt.grad_norm, r64["norms"][t], r32["norms"][t])
        clipped += int(float(r64["norms"][t]) > MAX_NORM)
        _check_rounded(ps, opt, t)
    assert 0 < clipped < steps, clipped                         # both branches of min(1, .) ran
    assert int(opt.step_count) == steps and int(opt.skipped_steps) == 0
    _compare(tag, ps, opt, r64, r32)
    got = _ratios(opt, ps)
    for i, gi in enumerate(GROUP_OF):                           # the plain group's entries were never written; LAMB's are real ratios
        assert (float(got[i]) == 1.0) == (gi == 1), (i, float(got[i]))
    st = opt.state[ps[3]]["trust_ratio"]
    assert st.dtype == torch.float32 and st.ndim == 0 and st.data_ptr() == opt._one().ratio[opt._where[id(ps[3])][1]].data_ptr()


# ---- 2: ratio edges ------------------------------------------------------------------------------------------------------------------------
def case_ratio_edges(dev, dtype, steps=3):
    """[0] zero-initialised, wd 0: |w| = 0 in the first step, r = 1.  [1] zero weight, zero gradient, wd 0.1: |u| = 0 in every step, r = 1
    and the weight stays 0.  [2] a scalar under the trust ratio: r = |w| / |u| of one element."""
    tag = f"lamb edges {_tag(dtype)}"
    shapes, group_of = [(513,), (7,), ()], [0, 1, 1]
    groups = [dict(lr=1e-2, weight_decay=0.0, trust_ratio=True), dict(lr=1e-2, weight_decay=0.1, trust_ratio=True)]
    params = make_params(dtype, 7, shapes)
    params[0].zero_()
    params[1].zero_()
    grads = make_grads(dtype, steps, 8, shapes)
    for gs in grads:
        gs[1].zero_()
    firsts = {}
    r64 = reference(params, grads, torch.float64, groups, group_of)
    r32 = reference(params, grads, torch.float32, groups, group_of)
    ps, opt = fused(dev, params, groups, group_of)
    for t, gs in enumerate(grads):
        set_grads(ps, gs, dev)
        opt.step()
        got = _ratios(opt, ps)
        firsts[t] = got
        assert float(got[1]) == 1.0 and not bool(opt.state[ps[1]]["exp_avg"].any()) and not bool(_weight(opt, ps[1]).any()), t
        for p in ps:
            assert all(bool(torch.isfinite(x).all()) for x in [p.detach(), *opt.state[p].values()]), t
    assert float(firsts[0][0]) == 1.0 and float(firsts[1][0]) != 1.0        # |w| = 0 only before the first step
    assert float(firsts[0][2]) != 1.0
    _compare(tag, ps, opt, r64, r32)


# ---- 3: bounds -----------------------------------------------------------------------------------------------------------------------------
def _bounds_setup(dtype, steps):
    """a scalar driven up for 3 steps, then down; a 513-vector with a fixed sign per element, flipped after 4 steps"""
    gen = torch.Generator().manual_seed(21)
    scalar = torch.tensor(4.5).to(dtype)
    vector = (torch.randn(513, generator=gen) * 0.5 + 0.1).to(dtype)
    sign = torch.where(torch.rand(513, generator=gen) < 0.5, -1.0, 1.0)
    grads = []
    for t in range(steps):
        mag = torch.rand(513, generator=gen) + 0.5
        grads.append([torch.tensor(-1.0 if t < 3 else 1.0).to(dtype), (mag * sign * (1.0 if t < 4 else -1.0)).to(dtype)])
    return [scalar, vector], grads


def case_bounds(dev, dtype, trust, ema_decay, steps=14):
    """both ends are values bf16 cannot hold (3.3, ln 100; -0.3, 0.7): the fp32 weight follows reference + clamp, the master and the
    bf16 parameter stay inside the bounds AS GIVEN after every step, and the EMA is the reference's EMA of the clamped weights"""
    tag = f"bounds {_tag(dtype)} {'lamb' if trust else 'adamw'}{' ema' if ema_decay else ''}"
    params, grads = _bounds_setup(dtype, steps)
    bounds = [(3.3, LN100), (-0.3, 0.7)]
    groups = [dict(lr=0.5, weight_decay=0.0, bounds=bounds[0]), dict(lr=1.0 if trust else 0.3, weight_decay=0.01, bounds=bounds[1])]
    if trust:
        groups = [dict(g, trust_ratio=True) for g in groups]
    kw = dict(ema_decay=ema_decay, ema_warmup=False) if ema_decay is not None else {}
    hit = {}

    def watch(step, ws):                                        # the reference decides whether the case exercises what it claims
        for i, (lo, hi) in enumerate(bounds):
            if bool((ws[i] == storage_bound(hi, dtype, False)).any()):
                hit.setdefault((i, "hi"), step)
            if bool((ws[i] == storage_bound(lo, dtype, True)).any()):
                hit.setdefault((i, "lo"), step)

    r64 = reference(params, grads, torch.float64, groups, [0, 1], each_step=watch, **kw)
    r32 = reference(params, grads, torch.float32, groups, [0, 1], **kw)
    assert set(hit) == {(0, "hi"), (0, "lo"), (1, "hi"), (1, "lo")} and hit[(0, "hi")] < hit[(0, "lo")], hit
    ps, opt = fused(dev, params, groups, [0, 1], **kw)
    for t, gs in enumerate(grads):
        set_grads(ps, gs, dev)
        opt.step()
        _check_rounded(ps, opt, t)
        for p, (lo, hi) in zip(ps, bounds):
            for x in (_weight(opt, p), p.detach()):
                assert lo <= float(x.double().min()) and float(x.double().max()) <= hi, (t, lo, float(x.double().min()), float(x.double().max()), hi)
    _compare(tag, ps, opt, r64, r32, ema=ema_decay is not None)


def case_one_sided_bounds(dev, dtype, steps=14):
    """(None, hi) on the scalar, (lo, None) on the vector: the open side is really open (the reference passes where the other case's bound was)"""
    tag = f"one-sided bounds {_tag(dtype)}"
    params, grads = _bounds_setup(dtype, steps)
    groups = [dict(lr=0.5, weight_decay=0.0, bounds=(None, LN100)), dict(lr=0.3, weight_decay=0.01, bounds=(-0.3, None))]
    r64 = reference(params, grads, torch.float64, groups, [0, 1])
    r32 = reference(params, grads, torch.float32, groups, [0, 1])
    assert float(r64["p"][0]) < 3.3 and float(r64["p"][1].max()) > 0.7 and float(r64["p"][1].min()) == storage_bound(-0.3, dtype, True)
    ps, opt = fused(dev, params, groups, [0, 1])
    for t, gs in enumerate(grads):
        set_grads(ps, gs, dev)
        opt.step()
        for x in (_weight(opt, ps[0]), ps[0].detach()):
            assert float(x) <= LN100, t
        for x in (_weight(opt, ps[1]), ps[1].detach()):
            assert float(x.double().min()) >= -0.3, t
    _compare(tag, ps, opt, r64, r32)


def case_invalid_bounds(dev):
    p = torch.nn.Parameter(torch.zeros(4, device=dev))
    q = torch.nn.Parameter(torch.zeros(4, dtype=BF16, device=dev))
    for bad in ((1.0, 0.5), (float("nan"), 1.0), (None, float("nan")), (1.0,), 3.0):
        with pytest.raises(ValueError, match="bounds"):
            FusedAdamW([p], bounds=bad)
        with pytest.raises(ValueError, match="bounds"):
            FusedAdamW([dict(params=[p], bounds=bad)])
    FusedAdamW([p], bounds=(1.001, 1.002))                      # fine in fp32 ...
    with pytest.raises(ValueError, match="bounds"):             # ... and empty once lo is rounded up and hi down to bf16
        FusedAdamW([q], bounds=(1.001, 1.002))
    opt = FusedAdamW([q], bounds=(None, None))
    opt.param_groups[0]["bounds"] = (2.0, 1.0)                  # read at every step, as lr is
    q.grad = torch.zeros_like(q)
    with pytest.raises(ValueError, match="bounds"):
        opt.step()


# ---- 4: off means off ----------------------------------------------------------------------------------------------------------------------
def _equal_runs(pairs):
    for (x, ox), (y, oy) in pairs:
        assert _same_bits(x.detach(), y.detach())
        for k in ox.state[x]:
            assert _same_bits(ox.state[x][k], oy.state[y][k]), k


def case_off_means_off(dev, dtype, ema_decay, steps=10):
    params, grads = make_params(dtype), make_grads(dtype, steps)
    kw = dict(ema_decay=ema_decay) if ema_decay is not None else {}
    a, oa = fused(dev, params, OC.GROUPS, GROUP_OF, **kw)                                                # built without the keys
    b, ob = fused(dev, params, [dict(g, trust_ratio=False, bounds=None) for g in OC.GROUPS], GROUP_OF, trust_ratio=False, bounds=None, **kw)
    c, oc = fused(dev, params, [dict(OC.GROUPS[0], trust_ratio=True, bounds=(-0.25, 0.75)), OC.GROUPS[1]], GROUP_OF, **kw)   # mixed
    assert all(set(g) == {"params", "lr", "betas", "eps", "weight_decay"} for g in oa.param_groups)
    for gs in grads:
        for ps, o in ((a, oa), (b, ob), (c, oc)):
            set_grads(ps, gs, dev)
            o.step()
    _equal_runs([((x, oa), (y, ob)) for x, y in zip(a, b)])
    _equal_runs([((x, oa), (z, oc)) for x, z, gi in zip(a, c, GROUP_OF) if gi == 1])                     # the un-keyed group of the mixed one
    assert not any(_same_bits(x.detach(), z.detach()) for x, z, gi in zip(a, c, GROUP_OF) if gi == 0)
    assert _same_bits(oa.grad_norm, ob.grad_norm) and _same_bits(oa.grad_norm, oc.grad_norm)
    assert oa._one().pairs is None and ob._one().pairs is None  # off: no array
    sa, sb = oa.state_dict(), ob.state_dict()
    assert all("trust_ratio" not in s for s in sa["state"].values()) and all("trust_ratio" not in s for s in sb["state"].values())


def case_default_param_groups():
    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb, self.lin, self.norm = torch.nn.Embedding(5, 8), torch.nn.Linear(8, 8), torch.nn.LayerNorm(8)
            self.temperature = torch.nn.Parameter(torch.tensor(1.0))
            self.logit_bias = torch.nn.Parameter(torch.tensor(-10.0))

    toy = Toy()
    decay, plain = [toy.lin.weight], [toy.temperature, toy.logit_bias, toy.emb.weight, toy.lin.bias, toy.norm.weight, toy.norm.bias]

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert set(g) == set(w) and all(g[k] == w[k] for k in w if k != "params"), (g, w)
            assert len(g["params"]) == len(w["params"]) and all(x is y for x, y in zip(g["params"], w["params"]))

    same(FusedAdamW.default_param_groups(toy, 0.2), [{"params": decay, "weight_decay": 0.2}, {"params": plain, "weight_decay": 0.0}])     # today's list
    same(FusedAdamW.default_param_groups(toy, 0.2, trust_ratio=True),
         [{"params": decay, "weight_decay": 0.2, "trust_ratio": True}, {"params": plain, "weight_decay": 0.0, "trust_ratio": False}])
    same(FusedAdamW.default_param_groups(toy, 0.2, trust_ratio=True, temperature_bounds=(0.0, LN100)),
         [{"params": decay, "weight_decay": 0.2, "trust_ratio": True}, {"params": plain[1:], "weight_decay": 0.0, "trust_ratio": False},
          {"params": [toy.temperature], "weight_decay": 0.0, "trust_ratio": False, "bounds": (0.0, LN100)}])
    same(FusedAdamW.default_param_groups(toy, 0.2, temperature_bounds=(0.0, None)),
         [{"params": decay, "weight_decay": 0.2}, {"params": plain[1:], "weight_decay": 0.0},
          {"params": [toy.temperature], "weight_decay": 0.0, "trust_ratio": False, "bounds": (0.0, None)}])
    with pytest.raises(ValueError, match="temperature"):
        FusedAdamW.default_param_groups(torch.nn.Linear(4, 4), 0.2, temperature_bounds=(0.0, 1.0))


# ---- 5: a skipped step ---------------------------------------------------------------------------------------------------------------------
def case_skipped_step(dev, dtype, bad):
    tag = f"lamb skip({bad}) {_tag(dtype)}"
    groups = [dict(LAMB_GROUPS[0], bounds=(-1.5, 1.5)), LAMB_GROUPS[1]]
    params, grads = make_params(dtype), make_grads(dtype, 3)
    seen = [grads[0], grads[2]]                                 # the reference never sees the skipped step
    r64 = reference(params, seen, torch.float64, groups, GROUP_OF, ema_decay=0.99)
    r32 = reference(params, seen, torch.float32, groups, GROUP_OF, ema_decay=0.99)
    poisoned = [g.clone() for g in grads[1]]
    poisoned[5].view(-1)[70000] = bad
    ps, opt = fused(dev, params, groups, GROUP_OF, ema_decay=0.99, ema_warmup=False)
    set_grads(ps, grads[0], dev)
    opt.step()
    before = _snapshot(opt, ps)
    assert float(before[-3][opt._where[id(ps[3])][1]]) != 1.0   # a stored ratio that a skipped step could have overwritten
    set_grads(ps, poisoned, dev)
    opt.step()
    after = _snapshot(opt, ps)
    assert all(_same_bits(a, b) for a, b in zip(before, after))
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 1 and not bool(torch.isfinite(opt.grad_norm))
    set_grads(ps, grads[2], dev)
    opt.step()
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 2
    _compare(tag, ps, opt, r64, r32, ema=True)


# ---- 6: reproducible -----------------------------------------------------------------------------------------------------------------------
def case_reproducible(dev, dtype, steps=3):
    grads = make_grads(dtype, steps)
    runs = []
    for _ in range(2):
        ps, opt = fused(dev, make_params(dtype), LAMB_GROUPS, GROUP_OF)
        for gs in grads:
            set_grads(ps, gs, dev)
            opt.step()
        runs.append(_snapshot(opt, ps) + [opt.grad_norm.clone()])
    assert all(_same_bits(a, b) for a, b in zip(*runs))


# ---- 7: absent / late gradient -------------------------------------------------------------------------------------------------------------
def case_absent_and_late_gradient(dev, dtype, late=3, pause=2, steps=5):
    """parameter `late` (16 chunks, LAMB) gets its first gradient in the third step: until then weight, moments and ratio (1) keep their
    bits, afterwards it runs on its own step count.  Parameter `pause` (LAMB) has no gradient in the fourth step: weight, moments and
    the ratio stored by the third keep their bits."""
    tag = f"lamb late-gradient {_tag(dtype)}"
    params, grads = make_params(dtype), make_grads(dtype, steps)
    grads[0][late] = grads[1][late] = grads[3][pause] = None
    r64 = reference(params, grads, torch.float64, LAMB_GROUPS, GROUP_OF)
    r32 = reference(params, grads, torch.float32, LAMB_GROUPS, GROUP_OF)
    assert r64["t"][late] == steps - 2 and r64["t"][pause] == steps - 1
    ps, opt = fused(dev, params, LAMB_GROUPS, GROUP_OF)

    def own(i):
        return [ps[i].detach().clone()] + [v.detach().clone() for _, v in sorted(opt.state[ps[i]].items())]

    start = own(late)
    for t, gs in enumerate(grads):
        held = own(pause) if t == 3 else None
        set_grads(ps, gs, dev)
        opt.step()
        if t < 2:
            assert all(_same_bits(a, b) for a, b in zip(start, own(late))), t
            assert float(opt.state[ps[late]]["trust_ratio"]) == 1.0
        if t == 3:
            assert all(_same_bits(a, b) for a, b in zip(held, own(pause)))
            assert float(opt.state[ps[pause]]["trust_ratio"]) != 1.0
    _compare(tag, ps, opt, r64, r32)
    counts = opt.state_dict()["state"]
    assert sorted(float(s["step"]) for s in counts.values()) == sorted(float(x) for x in r64["t"])


# ---- 8: checkpoints ------------------------------------------------------------------------------------------------------------------------
def case_state_roundtrip(dev, dtype):
    groups = [dict(LAMB_GROUPS[0], bounds=(-1.25, LN100)), LAMB_GROUPS[1]]
    params, grads = make_params(dtype), make_grads(dtype, 4)
    a, oa = fused(dev, params, groups, GROUP_OF, ema_decay=0.99)
    for gs in grads[:3]:
        set_grads(a, gs, dev)
        oa.step()
    sd = oa.state_dict()
    assert sd["param_groups"][0]["trust_ratio"] is True and tuple(sd["param_groups"][0]["bounds"]) == (-1.25, LN100)
    assert "trust_ratio" not in sd["param_groups"][1] and "bounds" not in sd["param_groups"][1]
    # (a state dict numbers the parameters group by group: the LAMB group's come first)
    assert all(("trust_ratio" in s) == (i < GROUP_OF.count(0)) for i, s in sd["state"].items())
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = FusedAdamW([dict(params=[p for p, gi in zip(b, GROUP_OF) if gi == k]) for k in range(2)], ema_decay=0.99)       # built without the keys
    ob.load_state_dict(copy.deepcopy(sd))
    assert ob.param_groups[0]["trust_ratio"] is True and ob.param_groups[0]["bounds"] == (-1.25, LN100)
    assert "trust_ratio" not in ob.param_groups[1] and "bounds" not in ob.param_groups[1]
    assert _same_bits(oa._one().ratio, ob._one().ratio)
    for ps, o in ((a, oa), (b, ob)):
        set_grads(ps, grads[3], dev)
        o.step()
    _equal_runs([((x, oa), (y, ob)) for x, y in zip(a, b)])
    assert _same_bits(oa._one().ratio, ob._one().ratio)


def case_load_torch_adamw(dev):
    """a torch.optim.AdamW dict has neither key: the constructor's stay, and the next step is LAMB + bounds on torch's moments"""
    params, grads = make_params(torch.float32), make_grads(torch.float32, 4)
    mid, m, v, _, topt = OC.reference(params, grads[:3], torch.float32)
    sd = copy.deepcopy(topt.state_dict())
    groups = [dict(lr=g["lr"], weight_decay=g["weight_decay"], trust_ratio=True, bounds=(-0.5, 0.5)) for g in OC.GROUPS]
    ps, opt = fused(dev, mid, OC.GROUPS, GROUP_OF, trust_ratio=True, bounds=(-0.5, 0.5))
    opt.load_state_dict(sd)
    assert all(g["trust_ratio"] is True and g["bounds"] == (-0.5, 0.5) for g in opt.param_groups)
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in OC.GROUPS]
    set_grads(ps, grads[3], dev)
    opt.step()
    state = (m, v, [3] * len(params))
    r64 = reference(mid, [grads[3]], torch.float64, groups, GROUP_OF, state_from=state)
    r32 = reference(mid, [grads[3]], torch.float32, groups, GROUP_OF, state_from=state)
    _compare("lamb after torch.optim.AdamW state", ps, opt, r64, r32)


# ---- 9: LAMB + EMA + accumulate ------------------------------------------------------------------------------------------------------------
def case_lamb_ema_accumulate(dev, dtype, steps=3, micro=2):
    tag = f"lamb ema accumulate {_tag(dtype)}"
    groups = [dict(LAMB_GROUPS[0], bounds=(-1.0, 1.25)), LAMB_GROUPS[1]]
    params = make_params(dtype)
    parts = [make_grads(dtype, steps, seed=30 + k) for k in range(micro)]
    # what accumulate_end() leaves in `.grad`: the fp32 sum of the passes, rounded once to the gradient's dtype
    summed = [[sum(parts[k][t][i].float() for k in range(micro)).to(dtype) for i in range(len(params))] for t in range(steps)]
    r64 = reference(params, summed, torch.float64, groups, GROUP_OF, ema_decay=0.9, ema_warmup=True)
    r32 = reference(params, summed, torch.float32, groups, GROUP_OF, ema_decay=0.9, ema_warmup=True)
    ps, opt = fused(dev, params, groups, GROUP_OF, ema_decay=0.9, ema_warmup=True)
    for t in range(steps):
        opt.accumulate_begin()
        for k in range(micro):
            set_grads(ps, parts[k][t], dev)
            opt.accumulate()
        opt.accumulate_end()
        for p, g in zip(ps, summed[t]):
            assert _same_bits(p.grad.detach().cpu(), g)
        opt.step()
        opt.zero_grad()
        _check_rounded(ps, opt, t)
    assert int(opt.step_count) == steps
    _compare(tag, ps, opt, r64, r32, ema=True)


# ---- 10: end to end ------------------------------------------------------------------------------------------------------------------------
def case_end_to_end(dev, cfg, batch=4, steps=3, max_norm=1.0, t0=5.0):
    """three fp32 training steps of the small CLIP with default_param_groups(clip, 0.2, trust_ratio=True, temperature_bounds=(0, ln 100)).
    The model is the source of the gradients: each step's are read back and the reference takes the same steps on them.  The temperature
    starts above hi: the first step (|step| <= lr = 1e-3 from 5.0) leaves it above hi and the clamp puts it AT hi, exactly.  Whether it
    is still there after the third step is the model's business, not the optimizer's: on this model and batch the loss wants a LOWER
    temperature (d loss / d temperature = +6.19 at 5.0 on the one-layer twin), so steps two and three move it ~1e-3 each below hi, in
    the reference as here.  The check is therefore: at hi after the first step; equal to the reference's (by the bar) and <= hi at the
    end; at hi at the end exactly when the reference's is."""
    build, text, image = OC._clip_and_batch(dev, torch.float32, cfg, batch)
    model = build()
    with torch.no_grad():
        model.temperature.fill_(t0)
    names = [k for k, _ in model.named_parameters()]
    ps = [p for _, p in model.named_parameters()]
    groups = FusedAdamW.default_param_groups(model, 0.2, trust_ratio=True, temperature_bounds=(0.0, LN100))
    assert len(groups) == 3 and groups[2]["params"][0] is model.temperature
    group_of = [next(k for k, g in enumerate(groups) if any(p is q for q in g["params"])) for p in ps]
    hyper = [dict({k: v for k, v in g.items() if k != "params"}, lr=1e-3) for g in groups]
    start = [p.detach().cpu().clone() for p in ps]
    opt = FusedAdamW(groups, lr=1e-3, max_grad_norm=max_norm)
    grads, temps = [], []
    for _ in range(steps):
        model(text, image, return_loss=True).backward()
        grads.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in ps])
        opt.step()
        opt.zero_grad()
        temps.append(model.temperature.detach().clone())
    assert int(opt.step_count) == steps and int(opt.skipped_steps) == 0
    r64 = reference(start, grads, torch.float64, hyper, group_of, max_norm)
    r32 = reference(start, grads, torch.float32, hyper, group_of, max_norm)
    hi = storage_bound(LN100, torch.float32, False)
    it = names.index("temperature")
    assert hi <= LN100 < t0 - 1e-3 and float(temps[0]) == hi, (hi, [float(x) for x in temps])
    print(f"lamb end to end: temperature {t0} -> {[float(x) for x in temps]} (hi {hi!r}); reference ends at {float(r64['p'][it])!r}")
    assert float(temps[-1]) <= hi and (float(temps[-1]) == hi) == (float(r64["p"][it]) == hi)
    stepped = 0
    for i, (k, p) in enumerate(zip(names, ps)):
        if all(gs[i] is None for gs in grads):                  # never had a gradient
            assert _same_bits(p.detach().cpu(), start[i]) and float(opt.state[p]["trust_ratio"]) == 1.0, k
            continue
        stepped += 1
        within_bar(f"lamb end to end {k}", p, r64["p"][i], r32["p"][i])
    assert stepped > 0
    got = _ratios(opt, ps)
    within_bar("lamb end to end trust ratios", got, r64["ratio"], r32["ratio"])
    assert any(float(got[i]) != 1.0 for i in range(len(ps)) if group_of[i] == 0)
    assert all(float(got[i]) == 1.0 for i in range(len(ps)) if group_of[i] != 0)
