"""Time one optimizer step on the default model's parameter set (MI355X): FusedAdamW (clip + AdamW, fp32 masters for bf16) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (foreach, and fused=True where this torch build has it), bf16 and fp32 parameters,
random gradients.  HIP events around each step, the variants alternated inside every repeat, median / best of N repeats after warm-up; the
shader clock is sampled right behind the timed steps (xclip_clock_sample) and the LayerNorm-forward streaming figure of the same
session is printed beside the fused step's achieved bytes / s.  The fused step is timed with two chunk sizes (elements per work-group: the
product's 64 Ki and 16 Ki) alternated in the same rounds, and its three phases -- norm pass, the one-work-group prepare kernel, update pass -- are
timed on their own (the phases of a step are dependent launches: their sum is the step without the gaps between them).  The weight EMA
(FusedAdamW(ema_decay=...)) is timed in the same rounds: its update pass (adamw_ema_kernel, 36 B per parameter) bracketed by two runs of
the EMA-off pass (28 B; the ratio is taken against the mean of the two and printed beside the byte ratio 36 / 28 with 10 % margin), the
whole step with EMA, and the two-pass alternative: the EMA-off step followed by torch._foreach_lerp_ on fp32 copies from the fp32
masters (bf16) / parameters (fp32).
usage: python tools/probe_optim.py [repeats]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from x_clip_amd import CLIP, FusedAdamW, _lib, ops

MAX_NORM = 1.0
EMA_DECAY = 0.9999
EMA_EXPECTED = 36.0 / 28.0 * 1.1   # the EMA update pass over the EMA-off pass: its byte ratio, 10 % margin for a ninth address stream
ALT_CHUNK = 16384           # the second chunk size the fused step is timed with (the product's: ops.OPTIM_CHUNK)


def clock_mhz(dev):
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().xclip_clock_sample(out.data_ptr(), 2000, torch.cuda.current_stream(dev).cuda_stream), "xclip_clock_sample")
    c, t = out.tolist()
    return c / max(t, 1) * 100.0


def ln_ceiling(dev):
    rows, dim = 2 * 2048 * 289, 1024
    x = torch.randn(rows, dim, device=dev, dtype=torch.bfloat16)
    g = torch.ones(dim, device=dev, dtype=torch.bfloat16)
    ts = []
    for i in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.layernorm_fwd(x, g, None, False)
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return rows * dim * 2 * 2 / ts[len(ts) // 2] / 1e6          # TB/s


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda")
    shapes = [tuple(p.shape) for p in CLIP().parameters()]
    n = sum(torch.Size(s).numel() for s in shapes)
    print(f"default CLIP: {len(shapes)} parameters, {n / 1e6:.1f} M elements; torch {torch.__version__}; {_lib.lib().xclip_build_info().decode()}")
    print(f"LayerNorm forward 1.18 M x 1024 bf16 (this session's streaming figure): {ln_ceiling(dev):.2f} TB/s; shader clock {clock_mhz(dev):.0f} MHz")
    for dtype, bytes_per in ((torch.bfloat16, 30), (torch.float32, 32)):
        g = torch.Generator(device=dev).manual_seed(1)
        variants = {}

        def make():
            ps = [torch.nn.Parameter((torch.randn(s, device=dev, generator=g) * 0.02).to(dtype)) for s in shapes]
            for p in ps:
                p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-2).to(dtype)
            return ps

        ps = make()
        fo = FusedAdamW(ps, lr=1e-4, max_grad_norm=MAX_NORM)
        variants["FusedAdamW (clip + AdamW" + (", fp32 masters)" if dtype == torch.bfloat16 else ")")] = fo.step
        product_chunk = ops.OPTIM_CHUNK
        ops.OPTIM_CHUNK = ALT_CHUNK                              # (the kernels take any chunk length; the table is built on the host)
        ps_c = make()
        fc = FusedAdamW(ps_c, lr=1e-4, max_grad_norm=MAX_NORM)
        fc.step()                                                # builds its table with the other chunk size
        ops.OPTIM_CHUNK = product_chunk
        variants[f"Fused, {ALT_CHUNK}-element chunks"] = fc.step
        D = fo._one()
        fo.step()
        half = {0: torch.float32, 1: torch.bfloat16}

        def norm_pass():
            for c0, cn, gc in D.norm_segments:
                ops.gradnorm_partial(D.table, c0, cn, half[gc], D.partials)

        def update_pass():
            for c0, cn, gi, pc, gc in D.segments:
                grp = fo.param_groups[gi]
                ops.adamw_step(D.table, c0, cn, half[pc], half[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base, grp["lr"],
                               grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"])

        variants["  phase: norm pass alone"] = norm_pass
        variants["  phase: prepare kernel alone"] = lambda: ops.optim_prepare(D.partials, D.n_chunks, MAX_NORM, D.block, D.step_base, D.absent, D.n_absent)
        variants["  phase: update pass alone"] = update_pass
        ps_e = make()
        fe = FusedAdamW(ps_e, lr=1e-4, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY)
        fe.step()
        E = fe._one()

        def update_pass_ema():
            for c0, cn, gi, pc, gc in E.segments:
                grp = fe.param_groups[gi]
                ops.adamw_ema_step(E.table, c0, cn, half[pc], half[gc], E.exp_avg, E.exp_avg_sq, E.master, E.block, E.step_base, grp["lr"],
                                   grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], E.ema, fe.ema_decay, fe.ema_warmup)

        variants["  phase: update pass alone, EMA on"] = update_pass_ema
        variants["  phase: update pass alone (EMA off) again"] = update_pass     # (the order inside a round matters: EMA on is bracketed)
        variants["Fused with EMA (ema_decay)"] = fe.step
        weights = [fo.state[p]["master"] if dtype == torch.bfloat16 else p.detach() for p in ps]
        lerp_ema = [w.clone() for w in weights]                  # the two-pass alternative's fp32 EMA, one tensor per parameter
        variants["  _foreach_lerp_ on the fp32 weights alone"] = lambda: torch._foreach_lerp_(lerp_ema, weights, 1.0 - EMA_DECAY)
        variants["Fused (EMA off) + _foreach_lerp_"] = lambda: (fo.step(), torch._foreach_lerp_(lerp_ema, weights, 1.0 - EMA_DECAY))
        ps_f = make()
        to = torch.optim.AdamW(ps_f, lr=1e-4, foreach=True)
        variants["clip_grad_norm_ + AdamW(foreach)"] = lambda ps_f=ps_f, to=to: (torch.nn.utils.clip_grad_norm_(ps_f, MAX_NORM), to.step())
        try:
            ps_u = make()
            tu = torch.optim.AdamW(ps_u, lr=1e-4, fused=True)
            tu.step()
            variants["clip_grad_norm_ + AdamW(fused=True)"] = lambda ps_u=ps_u, tu=tu: (torch.nn.utils.clip_grad_norm_(ps_u, MAX_NORM), tu.step())
        except Exception as e:                                   # noqa: BLE001 -- report what this build says
            print(f"  AdamW(fused=True) not available for {dtype}: {type(e).__name__}: {str(e)[:120]}")
        times = {k: [] for k in variants}
        for r in range(repeats + 3):                              # 3 warm-up rounds; the variants alternate inside every round
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if r >= 3:
                    times[k].append(a.elapsed_time(b) * 1e3)
        mhz = clock_mhz(dev)
        print(f"{'bf16' if dtype == torch.bfloat16 else 'fp32'} parameters and gradients, {repeats} repeats, shader clock behind the runs {mhz:.0f} MHz "
              f"(uploads of the fused chunk table: {fo.table_uploads})")
        for k, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            extra = f"   {n * bytes_per / med / 1e6:5.2f} TB/s of {bytes_per} B / parameter" if k.startswith("Fused") else ""
            if "norm pass" in k:
                extra = f"   {n * (bytes_per - 28) / med / 1e6:5.2f} TB/s of {bytes_per - 28} B / parameter"
            if "EMA on" in k:
                extra = f"   {n * 36 / med / 1e6:5.2f} TB/s of 36 B / parameter"
            elif "update pass" in k:
                extra = f"   {n * (bytes_per - (2 if dtype == torch.bfloat16 else 4)) / med / 1e6:5.2f} TB/s of {bytes_per - (2 if dtype == torch.bfloat16 else 4)} B / parameter"
            print(f"  {k:44s} median {med:8.1f} us   best {ts[0]:8.1f} us{extra}")
        med = {k: sorted(ts)[len(ts) // 2] for k, ts in times.items()}
        off = 0.5 * (med["  phase: update pass alone"] + med["  phase: update pass alone (EMA off) again"])
        ratio = med["  phase: update pass alone, EMA on"] / off
        print(f"  EMA update pass / EMA-off update pass (mean of the two around it): {ratio:.3f} (expected <= {EMA_EXPECTED:.3f}: {'met' if ratio <= EMA_EXPECTED else 'NOT met'}); "
              f"step with EMA / step + _foreach_lerp_: {med['Fused with EMA (ema_decay)'] / med['Fused (EMA off) + _foreach_lerp_']:.3f}")
        print(f"  work-groups per step: {D.n_chunks} with {product_chunk}-element chunks, {fc._one().n_chunks} with {ALT_CHUNK}")
        del ps, ps_f, ps_c, ps_e, fo, fc, fe, to, variants, D, E, weights, lerp_ema
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
