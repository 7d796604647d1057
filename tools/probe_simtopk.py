"""The fused similarity top-k against its yardsticks, on the same operands in one session with HIP events: (a) each of its four launches
-- slot maxima (`simrank_partial`), `simtopk_select`, `simtopk_mask`, `simtopk_finish` -- and the whole `ops.simtopk` call; (b) the LSE
forward (`simloss_partial`, and with its combine), which the two sweeps should sit beside; (c) what a user does without it:
`torch.matmul` + `torch.topk` (the temperature applied to the k returned values), with its peak memory next to the fused path's workspace.  Shapes: 4096 x 32768 x 512 and 1024 x 1024 x 512,
bf16, k = 10.  Every figure is the median of 21 rounds x 10 launches, the candidates alternating inside a round, after a warm-up of
every candidate.  Appends to profiles/<prefix>_simtopk_probe.log (`--log PATH` for another file)."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from x_clip_amd import _lib, ops  # noqa: E402

ROUNDS, ITERS = 21, 10


def log_path():
    if "--log" in sys.argv:
        return sys.argv[sys.argv.index("--log") + 1]
    prof = os.path.join(ROOT, "profiles")
    mine = sorted(glob.glob(os.path.join(prof, "r*_simtopk_probe.log")))
    if mine:
        return mine[-1]
    rounds = [int(m.group(1)) for f in os.listdir(prof) for m in [re.match(r"r(\d+)_", f)] if m]
    return os.path.join(prof, f"r{max(rounds, default=0) + 1:02d}_simtopk_probe.log")


def timed(fn, iters=ITERS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    k = 10
    lines = [f"# tools/probe_simtopk.py on {torch.cuda.get_device_name(0)}: us per launch, median of {ROUNDS} rounds x {ITERS} launches "
             f"[min .. max], candidates alternating inside a round; bf16, k = {k}"]
    for nq, nk, d in [(4096, 32768, 512), (1024, 1024, 512)]:
        g = torch.Generator(device=dev).manual_seed(1)
        Q = torch.nn.functional.normalize(torch.randn(nq, d, device=dev, generator=g), dim=-1).bfloat16()
        K = torch.nn.functional.normalize(torch.randn(nk, d, device=dev, generator=g), dim=-1).bfloat16()
        tau = torch.tensor([2.66], device=dev)
        slots = (nk + 63) // 64
        ws = torch.empty(5 * slots * nq, dtype=torch.int32, device=dev)
        pos, lse = torch.zeros(nq, device=dev), torch.empty(nq, device=dev)
        never = torch.full((nq,), float("inf"), device=dev)
        thr = torch.empty(nq, device=dev)
        values = torch.empty(nq, k, device=dev)
        indices = torch.empty(nq, k, dtype=torch.int32, device=dev)
        q, kk, tp, w = Q.data_ptr(), K.data_ptr(), tau.data_ptr(), ws.data_ptr()

        def lse_partial():
            _lib.check(L.xclip_simloss_partial(q, kk, nq, nk, d, 1.0, tp, 0, 0, w, 0, slots, pos.data_ptr(), 1, st), "simloss_partial")

        def lse_fwd():
            lse_partial()
            _lib.check(L.xclip_simloss_combine(w, nq, slots, pos.data_ptr(), lse.data_ptr(), 0, 0.0, st), "simloss_combine")

        def slot_max():
            _lib.check(L.xclip_simrank_partial(q, kk, nq, nk, d, 1.0, tp, -(1 << 30), 0, never.data_ptr(), w, 0, slots, 1, st), "simrank_partial")

        def select():
            _lib.check(L.xclip_simtopk_select(w, nq, slots, k, thr.data_ptr(), st), "simtopk_select")

        def mask():
            _lib.check(L.xclip_simtopk_mask(q, kk, nq, nk, d, 1.0, tp, thr.data_ptr(), w, 0, slots, 1, st), "simtopk_mask")

        def finish():                                               # (from an empty list every time: the same work per launch)
            values.fill_(-3.0e38)
            indices.fill_(-1)
            _lib.check(L.xclip_simtopk_finish(q, kk, nq, nk, d, 1.0, tp, 0, w, 0, slots, k, values.data_ptr(), indices.data_ptr(), 1, st),
                       "simtopk_finish")

        def fills():                                                # what `finish` above spends outside the kernel
            values.fill_(-3.0e38)
            indices.fill_(-1)

        def fused():
            return ops.simtopk(Q, K, k, 1.0, log_scale=tau)

        def dense():
            # (exp(tau) > 0 is monotone: the selection needs no scaled copy of the logits, the scale goes on the k values)
            v, i = torch.topk(torch.matmul(Q, K.t()), k, dim=1)
            return v.float() * tau.exp(), i

        # the four launches in their order once, so that each later one finds what it consumes
        slot_max()
        select()
        mask()
        finish()
        torch.cuda.synchronize()
        cand = sum((((ws[(3 * slots) * nq:].view(2 * slots, nq) >> b) & 1).sum(0) for b in range(32)))
        fv, fi = fused()
        assert torch.equal(fv, values) and torch.equal(fi, indices)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        dv, di = dense()
        torch.cuda.synchronize()
        dense_peak = torch.cuda.max_memory_allocated(dev) - base
        del dv, di
        # (the check: against torch.topk on the fp32 logits of the same bf16 latents -- the bf16 logits of the line above tie in thousands)
        d32 = torch.topk(torch.matmul(Q.float(), K.float().t()) * tau.exp(), k, dim=1)
        agree = float((d32.indices == fi).all(1).float().mean())
        worst = float((d32.values - fv).abs().max())
        del d32

        order = [("slot maxima (simrank_partial)", slot_max), ("simtopk_select", select), ("simtopk_mask", mask), ("simtopk_finish + 2 fills", finish),
                 ("the 2 fills alone", fills), ("ops.simtopk, whole call", fused), ("LSE forward partial (sim_fwd)", lse_partial),
                 ("LSE forward partial + combine", lse_fwd), ("torch.matmul + torch.topk", dense)]
        # (slot maxima directly in front of select in every round: the LSE candidates share the workspace and overwrite the hmax table;
        #  the mask words, which finish reads, lie beyond what they touch)
        for _, fn in order:
            timed(fn, 3)
        t = {name: [] for name, _ in order}
        for _ in range(ROUNDS):
            for name, fn in order:
                t[name].append(timed(fn))
        med = {}
        fl = 2.0 * nq * nk * d
        lines.append(f"{nq} x {nk} x {d}:")
        for name, _ in order:
            v = sorted(t[name])
            med[name] = v[len(v) // 2]
            lines.append(f"   {name:34s} {med[name]:9.1f} us [{v[0]:.1f} .. {v[-1]:.1f}]")
        ref = med["LSE forward partial (sim_fwd)"]
        four = med["slot maxima (simrank_partial)"] + med["simtopk_select"] + med["simtopk_mask"] + med["simtopk_finish + 2 fills"] - med["the 2 fills alone"]
        lines.append(f"   sweeps against the LSE forward partial: slot maxima {med['slot maxima (simrank_partial)'] / ref:.3f} x, mask "
                     f"{med['simtopk_mask'] / ref:.3f} x ({fl / med['simtopk_mask'] / 1e6:.1f} TF/s);  four launches {four:.1f} us, whole call "
                     f"{med['ops.simtopk, whole call']:.1f} us against torch.matmul + torch.topk {med['torch.matmul + torch.topk']:.1f} us = "
                     f"{med['ops.simtopk, whole call'] / med['torch.matmul + torch.topk']:.3f} x")
        lines.append(f"   memory: fused workspace {5 * slots * nq * 4 / 2 ** 20:.1f} MiB (+ {nq * (2 * k + 2) * 4 / 2 ** 10:.0f} KiB results and thresholds); "
                     f"torch.matmul + torch.topk peak {dense_peak / 2 ** 20:.1f} MiB")
        lines.append(f"   (check: candidates per row mean {float(cand.float().mean()):.1f}, max {int(cand.max())}; rows whose index list equals "
                     f"torch.topk's on the fp32 logits: {agree:.4f}, max |value difference| {worst:.2e})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    path = log_path()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
