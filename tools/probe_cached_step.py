"""What the cached contrastive step (x_clip_amd.cached.CachedContrastiveStep) costs and buys on the default bf16 model (MI355X):

  * step time (forward + backward + FusedAdamW.step, HIP events, median of the timed steps) and peak reserved memory of the one-pass
    step at b = 1024 and of the cached step at b = 1024 / micro 256 -- expected ratio about 4/3 (one extra forward, forward = one third);
  * the largest b in {1024, 2048, 4096, 8192} the one-pass step fits at, against the cached step at b = 8192 / micro 1024;
  * the accumulate kernel alone over the model's parameters (grad_accum_kernel: 10 B per bf16 gradient element to add, 6 B to
    materialise) beside the adamw_kernel update pass over the same chunk table (28 B) in the same process.

Every measurement is a child process of its own under its own `timeout`, chained with `&&`: a measurement that faults, hangs or is killed
ends the run, nothing is started on the GPU behind it.  A one-pass step that does not fit (torch.OutOfMemoryError, a clean error) ends its
chain with exit status 3 and the run goes on with the next group.
usage: python tools/probe_cached_step.py [timed steps per measurement]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NO_FIT = 3


def batch(b, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(b)
    text = torch.randint(1, 10000, (b, 256), generator=g, device=dev)
    image = torch.randn(b, 3, 256, 256, generator=g, device=dev, dtype=torch.bfloat16)
    return text, image


def model_and_opt(dev):
    import torch
    from x_clip_amd import CLIP, FusedAdamW
    torch.manual_seed(0)
    clip = CLIP(visual_patch_dropout=0.5).to(torch.bfloat16).to(dev).train()
    return clip, FusedAdamW(FusedAdamW.default_param_groups(clip, 0.2), lr=1e-5, max_grad_norm=1.0)


def child_step(kind, b, micro, steps):
    import torch
    from x_clip_amd import CachedContrastiveStep
    dev = torch.device("cuda")
    clip, opt = model_and_opt(dev)
    text, image = batch(b, dev)
    cached = CachedContrastiveStep(clip, opt, micro_batch=micro) if kind == "cached" else None
    times = []
    try:
        for i in range(steps + 2):                               # two warm-up steps
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if cached is None:
                clip(text, image, return_loss=True).backward()
            else:
                cached.step(text, image)
            opt.step()
            opt.zero_grad()
            e.record()
            torch.cuda.synchronize()
            if i >= 2:
                times.append(a.elapsed_time(e))
    except torch.OutOfMemoryError:
        print(json.dumps(dict(kind=kind, b=b, micro=micro, fits=False)), flush=True)
        sys.exit(NO_FIT)
    times.sort()
    print(json.dumps(dict(kind=kind, b=b, micro=micro, fits=True, step_ms=round(times[len(times) // 2], 2), best_ms=round(times[0], 2),
                          peak_reserved_gb=round(torch.cuda.max_memory_reserved() / 2 ** 30, 2),
                          peak_allocated_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), table_uploads=opt.table_uploads,
                          steps=len(times))), flush=True)


def child_kernel(repeats):
    import torch
    from x_clip_amd import ops
    dev = torch.device("cuda")
    clip, opt = model_and_opt(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    n = 0
    for p in clip.parameters():
        p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-2).to(p.dtype)
        n += p.numel()
    opt.step()                                                   # builds the chunk table these gradients are walked through
    D = opt._one()
    opt.accumulate_begin()
    half = {0: torch.float32, 1: torch.bfloat16}

    def accumulate(materialise):
        for c0, cn, gc in D.norm_segments:
            ops.grad_accumulate(D.table, c0, cn, half[gc], D.acc, materialise)

    def update_pass():
        for c0, cn, gi, pc, gc in D.segments:
            grp = opt.param_groups[gi]
            ops.adamw_step(D.table, c0, cn, half[pc], half[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base, grp["lr"],
                           grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"])

    variants = {"accumulate (add), 10 B": (lambda: accumulate(False), 10), "adamw update pass, 28 B": (update_pass, 28),
                "accumulate (materialise), 6 B": (lambda: accumulate(True), 6)}
    times = {k: [] for k in variants}
    for r in range(repeats + 3):                                 # the variants alternate inside every round
        for k, (fn, _) in variants.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= 3:
                times[k].append(a.elapsed_time(e) * 1e3)
    out = dict(kind="kernel", parameters_m=round(n / 1e6, 1), chunks=D.n_chunks)
    for k, (_, nbytes) in variants.items():
        ts = sorted(times[k])
        out[k] = dict(median_us=round(ts[len(ts) // 2], 1), best_us=round(ts[0], 1), tb_per_s=round(n * nbytes / ts[len(ts) // 2] / 1e6, 2))
    print(json.dumps(out), flush=True)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    me = os.path.abspath(__file__)

    def one(limit, *args):
        return f"timeout -k 10 {limit} {sys.executable} {me} --child {' '.join(str(a) for a in args)}"

    groups = [
        " && ".join([one(240, "one_pass", 1024, 0, steps), one(240, "cached", 1024, 256, steps)]),
        " && ".join([one(240, "one_pass", 2048, 0, 2), one(300, "one_pass", 4096, 0, 2), one(300, "one_pass", 8192, 0, 2)]),
        " && ".join([one(420, "cached", 8192, 1024, 2), one(240, "kernel", 0, 0, 20)]),
    ]
    rows = []
    for cmd in groups:
        proc = subprocess.run(["bash", "-c", cmd], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(proc.stdout)
        sys.stdout.flush()
        rows += [json.loads(l) for l in proc.stdout.splitlines() if l.startswith("{")]
        if proc.returncode not in (0, NO_FIT):
            print(f"# a measurement ended with exit status {proc.returncode}: nothing more is started", flush=True)
            sys.exit(proc.returncode)
    by = {(r["kind"], r.get("b"), r.get("micro")): r for r in rows}
    a, c = by.get(("one_pass", 1024, 0)), by.get(("cached", 1024, 256))
    if a and c:
        print(f"# b = 1024: cached / one-pass step time {c['step_ms'] / a['step_ms']:.3f} (expected about 1.333), "
              f"peak reserved {c['peak_reserved_gb']} GB against {a['peak_reserved_gb']} GB")
    fit = [r["b"] for r in rows if r["kind"] == "one_pass" and r.get("fits")]
    print(f"# one-pass step fits up to b = {max(fit) if fit else None} of (1024, 2048, 4096, 8192)")
    k = by.get(("kernel", None, None))
    if k:
        print(f"# accumulate (add) / adamw update pass: {k['accumulate (add), 10 B']['median_us'] / k['adamw update pass, 28 B']['median_us']:.3f} "
              f"in time, {10 / 28:.3f} in bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        kind, b, micro, steps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
        if kind == "kernel":
            child_kernel(steps)
        else:
            child_step(kind, b, micro, steps)
    else:
        main()
