"""Time `FusedAdamW.step()` with and without the layer-wise trust ratio (LAMB) on the default model's parameter set (MI355X): 58.5 M bf16
parameters and gradients (fp32 too), random values, `default_param_groups(clip, 0.2)` against `default_param_groups(clip, 0.2,
trust_ratio=True, temperature_bounds=(0, ln 100))`.  HIP events around each step on an otherwise empty stream, AdamW and LAMB alternating
inside every round of one session, medians with min ... max after three warm-up rounds.  The LAMB step's own launches are timed alone as
well: the norm pass (lamb_norm_kernel: reads g, m, v, w = 14 B per bf16 parameter), the fold (lamb_fold_kernel) and the update pass
(optim_update_kernel, 28 B) of the trust-ratio group.  Expectation from the byte counts: the LAMB step costs the AdamW step plus what its
extra pass reads, i.e. about (30 + 14) / 30 of it for the weight-matrix group.
usage: python tools/probe_lamb.py [repeats]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from x_clip_amd import CLIP, FusedAdamW, _lib, ops

MAX_NORM = 1.0


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda")
    print(f"torch {torch.__version__}; {_lib.lib().xclip_build_info().decode()}")
    for dtype in (torch.bfloat16, torch.float32):
        gen = torch.Generator(device=dev).manual_seed(1)

        def make():
            model = CLIP().to(dev).to(dtype)
            with torch.no_grad():
                for p in model.parameters():
                    if p.ndim >= 2:
                        p.copy_((torch.randn(p.shape, device=dev, generator=gen) * 0.02).to(dtype))
            for p in model.parameters():
                p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 1e-2).to(dtype)
            return model

        ma, ml = make(), make()
        n = sum(p.numel() for p in ma.parameters())
        oa = FusedAdamW(FusedAdamW.default_param_groups(ma, 0.2), lr=1e-4, max_grad_norm=MAX_NORM)
        groups = FusedAdamW.default_param_groups(ml, 0.2, trust_ratio=True, temperature_bounds=(0.0, math.log(100.0)))
        n_trust = sum(p.numel() for p in groups[0]["params"])
        ol = FusedAdamW(groups, lr=1e-4, max_grad_norm=MAX_NORM)
        oa.step()
        ol.step()
        D = ol._one()
        half = {0: torch.float32, 1: torch.bfloat16}
        trust = [(c0, cn, ol.param_groups[gi], pc, gc) for c0, cn, gi, pc, gc in D.segments if ol.param_groups[gi].get("trust_ratio", False)]

        def norm_pass():
            for c0, cn, grp, pc, gc in trust:
                ops.lamb_norm(D.table, c0, cn, half[pc], half[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base, grp["betas"][0],
                              grp["betas"][1], grp["eps"], grp["weight_decay"], D.pairs)

        def fold():
            for c0, cn, grp, pc, gc in trust:
                ops.lamb_fold(D.table, c0, cn, D.pairs, D.block, D.ratio)

        def update_pass():
            for c0, cn, grp, pc, gc in trust:
                ops.optim_update(D.table, c0, cn, half[pc], half[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base, grp["lr"],
                                 grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], D.ratio, -math.inf, math.inf)

        variants = {"AdamW step": oa.step, "LAMB step (trust ratio + bounded temperature)": ol.step, "  LAMB norm pass alone": norm_pass,
                    "  LAMB fold alone": fold, "  LAMB update pass alone": update_pass, "AdamW step again": oa.step}
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
        el = dtype.itemsize
        print(f"{'bf16' if dtype == torch.bfloat16 else 'fp32'}: {n / 1e6:.1f} M parameters, {n_trust / 1e6:.1f} M of them under the trust ratio, "
              f"{len(trust)} trust-ratio segment(s), {D.n_chunks} chunks; {repeats} repeats; steps skipped: {int(oa.skipped_steps)} / {int(ol.skipped_steps)}")
        med = {}
        for k, ts in times.items():
            ts.sort()
            med[k] = ts[len(ts) // 2]
            extra = ""
            if "norm pass" in k:
                extra = f"   {n_trust * (el + 12) / med[k] / 1e6:5.2f} TB/s of {el + 12} B / parameter"
            if "update pass" in k:
                extra = f"   {n_trust * (24 + 2 * el) / med[k] / 1e6:5.2f} TB/s of {24 + 2 * el} B / parameter"
            print(f"  {k:48s} median {med[k]:8.1f} us   min {ts[0]:8.1f} ... max {ts[-1]:8.1f} us{extra}")
        base = 0.5 * (med["AdamW step"] + med["AdamW step again"])
        expected = 1.0 + (el + 12) * n_trust / ((24 + 3 * el) * n)
        print(f"  LAMB step / AdamW step (mean of the two around it): {med['LAMB step (trust ratio + bounded temperature)'] / base:.3f}; "
              f"byte ratio {expected:.3f}")
        del ma, ml, oa, ol, D, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
