"""Cases for x_clip_amd.optim.FusedAdamW, shared by tests/test_optim_emu.py (CPU, wave64 emulator build of the kernel sources) and
tests/test_optim_gpu.py (MI355X, libxclip_hip.so), and the two-rank worker of tests/test_optim_dist.py.

The reference of every check is torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW run on the CPU in fp64 on copies of the same
parameters and gradients (`reference` below).  The bar is not a constant: the same reference run in fp32 measures, per tensor, what fp32
arithmetic costs torch itself (|p32 - p64|), and the fused result must stay within 4 x that plus one fp32 ulp of the tensor's largest
element (`within_bar`).  A wrong formula (decay after the update, eps inside the root, a missing bias correction) is off by 1e-3 or more.
"""
import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from x_clip_amd.optim import FusedAdamW  # noqa: E402

# name -> measured figure(s); tests print them and the end-to-end check reads the fp32 cost check 1 measured
REPORT = {}

SHAPES = [(), (7,), (513,), (512, 2048), (1001,), (3, 70001)]        # scalar, tiny, odd, 16 chunks, not a multiple of 8, chunk-spanning + ragged
GROUP_OF = [0, 1, 0, 0, 1, 1]
GROUPS = [dict(lr=1e-3, weight_decay=0.1), dict(lr=3e-3, weight_decay=0.0)]
HYPER = dict(betas=(0.9, 0.999), eps=1e-8)
MAX_NORM = 30.0                                                      # gradient norms alternate ~1122 / ~1.12: both branches of min(1, .) run


def make_params(dtype, seed=1, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * 0.5 + 0.1).to(dtype) for s in shapes]


def make_grads(dtype, steps, seed=2, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(s, generator=g) * (1.0 if t % 2 == 0 else 1e-3)).to(dtype) for s in shapes] for t in range(steps)]


def reference(params, grads, dtype, max_norm=MAX_NORM, group_of=GROUP_OF, groups=GROUPS, state_from=None):
    """clip_grad_norm_ + torch.optim.AdamW on the CPU in `dtype` (fp64: the reference; fp32: what fp32 costs torch itself) on the VALUES of
    `params` / `grads` (lists per step; an entry None = no gradient).  -> (parameters, exp_avg, exp_avg_sq, [grad norm per step])"""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    opt = torch.optim.AdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], **groups[k]) for k in range(len(groups))],
                            foreach=False, **HYPER)
    if state_from is not None:
        # (a copy: torch keeps the `step` tensors and same-dtype moments of the dict it loads and updates them in place)
        opt.load_state_dict(copy.deepcopy(state_from))
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm, foreach=False).detach().clone())
        else:
            norms.append(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps if p.grad is not None])))
        opt.step()
    st = [opt.state.get(p, {}) for p in ps]
    return ([p.detach() for p in ps], [s.get("exp_avg") for s in st], [s.get("exp_avg_sq") for s in st], norms, opt)


def fused(dev, params, group_of=GROUP_OF, groups=GROUPS, max_norm=MAX_NORM):
    ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in params]
    opt = FusedAdamW([dict(params=[p for p, gi in zip(ps, group_of) if gi == k], **groups[k]) for k in range(len(groups))],
                     max_grad_norm=max_norm, **HYPER)
    return ps, opt


def set_grads(ps, gs, dev):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.detach().clone().to(dev)


def _bits(t):
    return t.reshape(-1).view(torch.uint8) if t.is_floating_point() else t


def ulp32(x):
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (torch.frexp(torch.tensor(x, dtype=torch.float64))[1].item() - 1 - 23)


def within_bar(name, got, ref64, ref32):
    """|got - ref64| <= 4 |ref32 - ref64| + one fp32 ulp of the largest element; records the three figures (relative to |ref64|)"""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().double(), ref32.detach().double()
    scale = max(float(ref64.norm()), 1e-300)
    err, cost = float((got - ref64).norm()), float((ref32 - ref64).norm())
    bar = 4.0 * cost + ulp32(ref64.abs().max())
    REPORT[name] = dict(fused_rel=err / scale, torch_fp32_rel=cost / scale, bar_rel=bar / scale)
    print(f"{name:44s} fused {err / scale:9.3e} | torch fp32 {cost / scale:9.3e} | bar {bar / scale:9.3e}")
    assert err <= bar, (name, err / scale, cost / scale, bar / scale)
    return cost / scale


def fp32_cost():
    """largest per-tensor relative figure of torch's own fp32 run against fp64 on check 1's case (CPU only): the end-to-end bar"""
    if "fp32_cost" not in REPORT:
        params, grads = make_params(torch.float32), make_grads(torch.float32, 10)
        p64 = reference(params, grads, torch.float64)[0]
        p32 = reference(params, grads, torch.float32)[0]
        REPORT["fp32_cost"] = max(float((a.double() - b).norm() / b.norm()) for a, b in zip(p32, p64))
    return REPORT["fp32_cost"]


# ---- 1 / 2a / 2b -------------------------------------------------------------------------------------------------------------------
def case_parity(dev, dtype, steps=10):
    tag = "bf16" if dtype == torch.bfloat16 else "fp32"
    params, grads = make_params(dtype), make_grads(dtype, steps)
    p64, m64, v64, n64, _ = reference(params, grads, torch.float64)
    p32, m32, v32, n32, _ = reference(params, grads, torch.float32)
    ps, opt = fused(dev, params)
    clipped = 0
    for t, gs in enumerate(grads):
        set_grads(ps, gs, dev)
        opt.step()
        within_bar(f"optim {tag} grad_norm step {t}", opt.grad_norm, n64[t], n32[t])
        clipped += int(float(n64[t]) > MAX_NORM)
        if dtype == torch.bfloat16:
            for i, p in enumerate(ps):                          # 2b: the parameter IS the rounded master, after every step
                assert torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16)), (t, i)
    assert 0 < clipped < steps, clipped                         # both branches of min(1, .) ran
    assert int(opt.step_count) == steps and int(opt.skipped_steps) == 0
    worst = 0.0
    for i, p in enumerate(ps):
        w = opt.state[p]["master"] if dtype == torch.bfloat16 else p
        worst = max(worst, within_bar(f"optim {tag} param[{i}] {tuple(p.shape)}", w, p64[i], p32[i]))
        within_bar(f"optim {tag} exp_avg[{i}]", opt.state[p]["exp_avg"], m64[i], m32[i])
        within_bar(f"optim {tag} exp_avg_sq[{i}]", opt.state[p]["exp_avg_sq"], v64[i], v32[i])
    if dtype == torch.float32:
        REPORT["fp32_cost"] = worst


# ---- 2c: the stall that motivates the feature ----------------------------------------------------------------------------------------
def case_bf16_stall(dev, steps=200):
    g = torch.Generator().manual_seed(3)
    w0 = (torch.rand(1024, generator=g) * 1.5 + 0.5).to(torch.bfloat16)
    grad = torch.ones(1024, dtype=torch.bfloat16)
    groups, hyper = [dict(lr=1e-5, weight_decay=0.0)], [[grad]] * steps
    plain = torch.nn.Parameter(w0.clone())                      # torch.optim.AdamW on the bf16 tensor itself
    o = torch.optim.AdamW([plain], lr=1e-5, weight_decay=0.0, foreach=False, **HYPER)
    for _ in range(steps):
        plain.grad = grad.clone()
        o.step()
    stalled = float((plain.detach().double() - w0.double()).abs().max())
    p64 = reference([w0], hyper, torch.float64, None, [0], groups)[0][0]
    p32 = reference([w0], hyper, torch.float32, None, [0], groups)[0][0]
    moved = float((p64 - w0.double()).abs().min())
    ps, opt = fused(dev, [w0], [0], groups, None)
    for _ in range(steps):
        set_grads(ps, [grad], dev)
        opt.step()
    within_bar("optim bf16 stall: master", opt.state[ps[0]]["master"], p64, p32)
    got = ps[0].detach().cpu().double()
    half_ulp = torch.exp2(torch.floor(torch.log2(p64.abs())) - 7) / 2
    slack = 4.0 * (p32.double() - p64).abs().max() + ulp32(p64.abs().max())
    excess = float(((got - p64).abs() - half_ulp).max())
    REPORT["optim bf16 stall"] = dict(plain_bf16_adamw_moved=stalled, fp64_moved=moved, fused_excess_over_half_ulp=excess)
    print(f"bf16 stall: plain bf16 AdamW moved {stalled:.3e}, fp64 moved >= {moved:.3e}, fused - half ulp {excess:.3e}")
    assert stalled <= 0.1 * moved and moved > 1.5e-3, (stalled, moved)
    assert excess <= float(slack), (excess, float(slack))


# ---- 3: skip on non-finite -------------------------------------------------------------------------------------------------------------
def case_skip_nonfinite(dev, dtype, bad):
    shapes, group_of = [(), (513,), (300, 300)], [1, 0, 0]
    params = make_params(dtype, 5, shapes)
    g_bad, g_ok = make_grads(dtype, 2, 6, shapes)
    g_bad[2].view(-1)[70000] = bad
    ps, opt = fused(dev, params, group_of)

    def snapshot():
        out = [p.detach().clone() for p in ps]
        for p in ps:
            out += [v.clone() for k, v in sorted(opt.state[p].items())]
        return out + [next(iter(opt._devs.values())).step_base.clone(), opt.step_count.clone()]

    before = snapshot()
    set_grads(ps, g_bad, dev)
    opt.step()
    after = snapshot()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, after))
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 0
    assert not bool(torch.isfinite(opt.grad_norm))
    set_grads(ps, g_ok, dev)
    opt.step()
    assert int(opt.skipped_steps) == 1 and int(opt.step_count) == 1
    p64 = reference(params, [g_ok], torch.float64, MAX_NORM, group_of)[0]      # the reference's FIRST step: bias corrections from t = 1
    p32 = reference(params, [g_ok], torch.float32, MAX_NORM, group_of)[0]
    for i, p in enumerate(ps):
        within_bar(f"optim skip({bad}) {dtype} next step param[{i}]", opt.state[p]["master"] if dtype == torch.bfloat16 else p, p64[i], p32[i])


# ---- 4: reproducible, layout-free, late gradients -------------------------------------------------------------------------------------------
def _run(dev, dtype, steps, flat=False, late=None):
    params, grads = make_params(dtype), make_grads(dtype, steps)
    ps, opt = fused(dev, params)
    buf, offs = None, []
    if flat:                                                    # GradSync's layout: one flat buffer, 128-byte aligned slices
        step = 128 // params[0].element_size()
        off = 0
        for p in ps:
            offs.append(off)
            off += (p.numel() + step - 1) // step * step
        buf = torch.zeros(off, dtype=dtype, device=dev)
    for t, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(ps, gs)):
            if late is not None and i == late and t == 0:
                p.grad = None
            elif flat:
                p.grad = buf[offs[i]: offs[i] + p.numel()].view(p.shape)
                p.grad.copy_(g)
            else:
                p.grad = g.clone().to(dev)
        opt.step()
    return ps, opt


def case_reproducible(dev, dtype):
    a, oa = _run(dev, dtype, 3)
    b, ob = _run(dev, dtype, 3)
    c, oc = _run(dev, dtype, 3, flat=True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
        for k in oa.state[x]:
            assert torch.equal(oa.state[x][k], ob.state[y][k]) and torch.equal(oa.state[x][k], oc.state[z][k]), k
    assert torch.equal(oa.grad_norm, ob.grad_norm) and torch.equal(oa.grad_norm, oc.grad_norm)
    assert oc.table_uploads == 1                                # persistent slices: one upload, then none


def case_late_gradient(dev, dtype, late=3):
    params, grads = make_params(dtype), make_grads(dtype, 3)
    grads[0][late] = None
    ps, opt = _run(dev, dtype, 1, late=late)
    assert torch.equal(ps[late].detach().cpu(), params[late])   # untouched while it has no gradient
    assert not bool(opt.state[ps[late]]["exp_avg"].any())
    ps, opt = _run(dev, dtype, 3, late=late)
    assert opt.table_uploads >= 2
    p64 = reference(params, grads, torch.float64)[0]
    p32 = reference(params, grads, torch.float32)[0]
    for i, p in enumerate(ps):                                  # the late parameter's own step count starts at 1 in step 2 (torch semantics)
        within_bar(f"optim late-gradient {dtype} param[{i}]", opt.state[p]["master"] if dtype == torch.bfloat16 else p, p64[i], p32[i])
    steps = opt.state_dict()["state"]
    assert sorted(float(s["step"]) for s in steps.values()) == [2.0] + [3.0] * (len(ps) - 1)


# ---- 5: state round trip ---------------------------------------------------------------------------------------------------------------------
def case_state_roundtrip(dev, dtype):
    params, grads = make_params(dtype), make_grads(dtype, 4)
    a, oa = fused(dev, params)
    for gs in grads[:3]:
        set_grads(a, gs, dev)
        oa.step()
    set_grads(a, [torch.full_like(g, float("inf")) for g in grads[0]], dev)
    oa.step()                                                   # a skipped step: the counter travels with the checkpoint
    calls = []
    oa.register_state_dict_pre_hook(lambda o: calls.append("pre"))
    oa.register_state_dict_post_hook(lambda o, d: calls.append("post"))
    sd = oa.state_dict()
    assert calls == ["pre", "post"]
    assert all(v.dtype == torch.float32 for s in sd["state"].values() for v in s.values())
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = FusedAdamW([dict(params=[p for p, gi in zip(b, GROUP_OF) if gi == k]) for k in range(len(GROUPS))])
    ob.register_load_state_dict_pre_hook(lambda o, d: calls.append("load-pre"))
    ob.register_load_state_dict_post_hook(lambda o: calls.append("load-post"))
    ob.load_state_dict(sd)
    assert calls[2:] == ["load-pre", "load-post"]
    assert int(oa.skipped_steps) == 1 and int(ob.skipped_steps) == 1 and int(ob.step_count) == 3
    assert ob.max_grad_norm == MAX_NORM and [g["lr"] for g in ob.param_groups] == [g["lr"] for g in GROUPS]
    for ps, o in ((a, oa), (b, ob)):
        set_grads(ps, grads[3], dev)
        o.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        for k in oa.state[x]:
            assert torch.equal(oa.state[x][k], ob.state[y][k]), k


def case_load_torch_adamw(dev):
    params, grads = make_params(torch.float32), make_grads(torch.float32, 4)
    mid, _, _, _, topt = reference(params, grads[:3], torch.float32)
    sd = copy.deepcopy(topt.state_dict())
    ps, opt = fused(dev, mid)
    opt.load_state_dict(sd)
    set_grads(ps, grads[3], dev)
    opt.step()
    p64 = reference(mid, [grads[3]], torch.float64, state_from=sd)[0]
    p32 = reference(mid, [grads[3]], torch.float32, state_from=sd)[0]
    assert sorted(float(s["step"]) for s in sd["state"].values()) == [3.0] * len(params)         # nobody stepped the loaded dict itself
    for i, p in enumerate(ps):
        within_bar(f"optim after torch.optim.AdamW state param[{i}]", p, p64[i], p32[i])
    # of torch's group keys (foreach, fused, capturable, ...) only the four that mean something here are taken
    assert all(set(g) == {"params", "lr", "betas", "eps", "weight_decay"} for g in opt.param_groups), [sorted(g) for g in opt.param_groups]


# ---- 6: end to end ---------------------------------------------------------------------------------------------------------------------------
def _clip_and_batch(dev, dtype, cfg, batch):
    import clip_cases as C
    from oracle import clip_oracle as O
    sd = O.make_state_dict(cfg, 11, torch.float32)
    text, image, _, _ = O.make_inputs(cfg, batch, 12)
    return (lambda: C.build_clip(cfg, sd, dev, dtype)), text.to(dev), image.to(dtype).to(dev)


def case_end_to_end_fp32(dev, cfg, batch=4, steps=3, max_norm=1.0):
    build, text, image = _clip_and_batch(dev, torch.float32, cfg, batch)
    ours, theirs = build(), build()
    opt = FusedAdamW(FusedAdamW.default_param_groups(ours, 0.1), lr=1e-3, max_grad_norm=max_norm)
    ref = torch.optim.AdamW(FusedAdamW.default_param_groups(theirs, 0.1), lr=1e-3, foreach=False)
    for _ in range(steps):                                      # no host synchronisation between the launches of these steps
        ours(text, image, return_loss=True).backward()
        opt.step()
        opt.zero_grad()
    for _ in range(steps):
        theirs(text, image, return_loss=True).backward()
        torch.nn.utils.clip_grad_norm_(theirs.parameters(), max_norm)
        ref.step()
        ref.zero_grad()
    bar = 4.0 * fp32_cost()
    worst = (0.0, "")
    for (k, p), q in zip(ours.named_parameters(), theirs.parameters()):
        if not ref.state.get(q) and not opt.state[p]["exp_avg"].any():       # never had a gradient, in either run
            assert torch.equal(p, q), k
            continue
        worst = max(worst, (float((p.detach().double() - q.detach().double()).norm() / q.detach().double().norm()), k))
    REPORT["optim end to end fp32"] = dict(worst_rel=worst[0], param=worst[1], bar=bar)
    print(f"end to end fp32: worst {worst[0]:.3e} ({worst[1]}) | bar {bar:.3e} = 4 x torch's fp32 cost {fp32_cost():.3e}")
    assert int(opt.step_count) == steps
    assert worst[0] <= bar, (worst, bar)


def case_end_to_end_bf16(dev, cfg, batch=4, steps=20):
    build, text, image = _clip_and_batch(dev, torch.bfloat16, cfg, batch)
    model = build()
    opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0)
    losses = []
    for _ in range(steps):
        loss = model(text, image, return_loss=True)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach())
    losses = [float(x) for x in losses]
    REPORT["optim end to end bf16"] = dict(first=losses[0], last=losses[-1])
    print(f"end to end bf16: loss {losses[0]:.4f} -> {losses[-1]:.4f} over {steps} steps")
    assert losses[-1] < losses[0], losses
    stepped = 0
    for p in model.parameters():
        assert torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16))
        stepped += int(bool(opt.state[p]["exp_avg"].any()))
    assert stepped > 0 and int(opt.step_count) + int(opt.skipped_steps) == steps


# ---- 7: two ranks (worker of tests/test_optim_dist.py; helpers of tests/dist_cases.py) -----------------------------------------------------------
def worker_two_ranks(rank, world, port, cfg_kwargs, batch, tmp, kind="cpu"):
    import dist_cases as D
    dev = D.setup(rank, world, port, kind)
    import torch.distributed as dist
    from x_clip_amd import CLIP
    from x_clip_amd.distributed import GradSync
    from oracle import clip_oracle as O
    cfg = O.ClipConfig(**cfg_kwargs)
    sd = O.make_state_dict(cfg, 5, torch.float32)
    text, image, _, _ = O.make_inputs(cfg, batch * world, 6)
    sl = slice(rank * batch, (rank + 1) * batch)                # different data per rank
    out = {}
    for with_opt in (False, True):
        model = CLIP(**cfg.ctor_kwargs(), visual_patch_dropout=0.0)
        model.load_state_dict(sd)
        model = model.to(dev).train()
        model.assume_equal_batch = True
        sync = GradSync(model)
        opt = FusedAdamW(FusedAdamW.default_param_groups(model, 0.1), lr=1e-3, max_grad_norm=1.0) if with_opt else None
        in_place, uploads, norms = [], [], []
        for _ in range(2):
            model(text[sl].to(dev), image[sl].float().to(dev), return_loss=True).backward()
            sync.finish()
            in_place.append(sync.stats["in_place"])
            if opt is not None:
                opt.step()
                uploads.append(opt.table_uploads)
                norms.append(opt.grad_norm.detach().cpu().clone())
                opt.zero_grad()
            else:
                model.zero_grad(set_to_none=True)
        out[with_opt] = dict(in_place=in_place, uploads=uploads, norms=norms,
                             params={k: p.detach().cpu().clone() for k, p in model.named_parameters()})
        sync.remove()
    if kind != "cpu":
        torch.cuda.synchronize()
    torch.save(out, os.path.join(tmp, f"rank{rank}.pt"))
    dist.destroy_process_group()


def check_two_ranks(tmp, world=2):
    outs = [torch.load(os.path.join(tmp, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    a, b = outs[0][True], outs[1][True]
    moved = 0
    for k in a["params"]:
        assert torch.equal(a["params"][k], b["params"][k]), k                   # the same bits on both ranks, no collective in the optimizer
        moved += int(not torch.equal(a["params"][k], outs[0][False]["params"][k]))
    assert moved > 0
    for x, y in zip(a["norms"], b["norms"]):
        assert torch.equal(x, y) and bool(torch.isfinite(x)) and float(x) > 0
    for o in outs:
        assert o[True]["in_place"][1] == o[False]["in_place"][1] > 0, (o[True]["in_place"], o[False]["in_place"])
        assert o[True]["uploads"] == [1, 1], o[True]["uploads"]                    # from step 2 on no chunk-table upload
