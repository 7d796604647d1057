"""Packed text tower against the pruned dense one, BASELINE configs[1] (default CLIP, bf16, b = 1024, forward + backward, optimizer not included).

    python tools/probe_packed_text.py [--batch 1024] [--rounds 6] > profiles/rNN_packed_text_probe.log

Token lengths are drawn with a fixed seed, uniform in [1, 2 f n], so that the fill R / (b (n + 1)) is about f = 1/16, 1/4 and 1 of n = 256 (f = 1:
no padding at all).  At each fill the step is timed in three modes -- `pack_text` off (the pruned dense path), on, and on with
`pack_text_pool_last` -- ALTERNATING in one session (off, on, pool, off, on, pool, ...: drift of the clocks hits all alike); reported: the median
step of each, the ratios to off, the peak of reserved memory of each mode (measured in a pass of its own after emptying the cache), and per layer
on the layout of that fill the varlen attention forward / backward and the one-query varlen attention forward / backward (8 heads); at fill 1 also
the dense one-query kernels (attn_pool_*) on the same rows viewed as [b, n + 1], for comparison.

    python tools/probe_packed_text.py --row-multiple 256 > profiles/rNN_packed_bucket_probe.log

adds two modes to the alternation -- `on_m` and `pool_m`: the same with a layout whose row count is rounded up to the multiple
(text_layout(row_multiple=)) -- and a second line per fill (`bucket`): the two row counts, every mode's median step with its min .. max, the
ratios of the bucketed modes to their unbucketed twins, the losses of one step per mode behind the same seed (the patch dropout then keeps the
same patches; equal bits where the row count was a multiple already), and from that step of every packed mode (probed, ops.KernelProbe) the milliseconds per kernel family, with the GEMMs whose M or K is the row count -- the text tower's
large products -- counted apart."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x_clip_amd import CLIP, ops, text_layout  # noqa: E402

MODES = ("off", "on", "pool")


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-multiple", type=int, default=None, help="also time the packed modes on a layout bucketed to this multiple")
    args = ap.parse_args()
    modes = MODES + (("on_m", "pool_m") if args.row_multiple else ())
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CLIP().to(torch.bfloat16).to(dev).train()
    n, b = model.text_seq_len, args.batch
    g = torch.Generator().manual_seed(1)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)
    med = lambda fn: statistics.median(timed(fn, dev) for _ in range(10))
    print(f"# default CLIP bf16, b = {b}, n = {n}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; times in ms (median)")
    print("# off = pack_text off (pruned dense tower); on = pack_text; pool = pack_text + pack_text_pool_last")
    print("# fill_target fill R max_len | step_off step_on step_pool on/off pool/off pool/on | reserved_off_GiB reserved_on_GiB reserved_pool_GiB | "
          "varlen_attn_fwd varlen_attn_bwd pool_varlen_fwd pool_varlen_bwd (one layer, 8 heads) | attn_pool_fwd attn_pool_bwd (dense, fill 1 only)")
    for f in (1 / 16, 1 / 4, 1.0):
        text = torch.randint(1, 10000, (b, n), generator=g)
        if f < 1.0:
            lens = torch.randint(1, int(2 * f * n) + 1, (b,), generator=g)
            text[torch.arange(n)[None] >= lens[:, None]] = 0
        lay = text_layout(text, pad_id=0)
        lay_m = text_layout(text, pad_id=0, row_multiple=args.row_multiple) if args.row_multiple else None
        text = text.to(dev)
        losses = {}

        def step(mode):
            model.pack_text, model.pack_text_pool_last = mode != "off", mode.startswith("pool")
            model.zero_grad(set_to_none=True)
            loss = model(text, image, return_loss=True, **(dict(text_layout=lay_m if mode.endswith("_m") else lay) if mode != "off" else {}))
            loss.backward()
            losses[mode] = loss.detach()

        times = {m: [] for m in modes}
        for r in range(args.warmup + args.rounds):
            for mode in modes:
                t = timed(lambda: step(mode), dev)
                if r >= args.warmup:
                    times[mode].append(t)
        reserved = {}
        for mode in MODES:
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            step(mode)
            torch.cuda.synchronize(dev)
            reserved[mode] = torch.cuda.max_memory_reserved(dev) / 2 ** 30
        model.zero_grad(set_to_none=True)
        layd = lay.to(dev)
        qkv = torch.randn(lay.R, 3 * 8 * 64, device=dev).to(torch.bfloat16)
        do = torch.randn(lay.R, 8 * 64, device=dev).to(torch.bfloat16)
        out, lse = ops.attention_varlen_fwd(qkv, layd.cu, lay.max_len, 8, 0.125)
        tf = med(lambda: ops.attention_varlen_fwd(qkv, layd.cu, lay.max_len, 8, 0.125))
        tb = med(lambda: ops.attention_varlen_bwd(qkv, layd.cu, lay.max_len, out, do, lse, 8, 0.125))
        del out, lse
        q, kv, doc = qkv[:b, :512].contiguous(), qkv[:, 512:].contiguous(), do[:b].contiguous()
        oc, lsec = ops.attention_pool_varlen_fwd(q, kv, layd.cu, 8, 0.125)
        pf = med(lambda: ops.attention_pool_varlen_fwd(q, kv, layd.cu, 8, 0.125))
        pb = med(lambda: ops.attention_pool_varlen_bwd(q, kv, layd.cu, oc, doc, lsec, 8, 0.125))
        dense = "- -"
        if lay.R == b * (n + 1):
            kvd = kv.view(b, n + 1, 1024)
            df = med(lambda: ops.attention_pool_fwd(q, kvd, None, 8, 0.125))
            db = med(lambda: ops.attention_pool_bwd(q, kvd, None, oc, doc, lsec, 8, 0.125))
            dense = f"{df:.3f} {db:.3f}"
        off, on, pool = (statistics.median(times[m]) for m in MODES)
        print(f"{f:.4f} {lay.R / (b * (n + 1)):.4f} {lay.R} {lay.max_len} | {off:.2f} {on:.2f} {pool:.2f} {on / off:.3f} {pool / off:.3f} {pool / on:.3f} | "
              f"{reserved['off']:.2f} {reserved['on']:.2f} {reserved['pool']:.2f} | {tf:.3f} {tb:.3f} {pf:.3f} {pb:.3f} | {dense}", flush=True)
        del qkv, do, q, kv, doc, oc, lsec
        if lay_m is not None:
            spread = lambda m: f"{statistics.median(times[m]):.2f} ({min(times[m]):.2f} .. {max(times[m]):.2f})"
            ratio = lambda a, b_: statistics.median(times[a]) / statistics.median(times[b_])
            fam = {}
            torch.manual_seed(7)
            step("off")
            for mode in modes[1:]:                              # (the same seed in front of each: the vision tower's patch dropout draws the same patches)
                rows = (lay_m if mode.endswith("_m") else lay).R
                torch.manual_seed(7)
                with ops.KernelProbe() as probe:
                    step(mode)
                torch.cuda.synchronize(dev)
                ms = {}
                for family, _, e0, e1, _, key in probe.records:
                    text_gemm = family == "gemm" and key is not None and rows in (key[0], key[2])
                    name = "gemm_text_rows" if text_gemm else family
                    ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
                fam[mode] = " ".join(f"{k}={v:.2f}" for k, v in sorted(ms.items()))
            loss_bits = {m: float(losses[m]) for m in modes}
            first = {m: losses[m] for m in ("on", "pool")}      # the control of the bit comparison: the same mode, seed and layout once more
            for m in first:
                torch.manual_seed(7)
                step(m)
            again = " ".join(f"{m}=={m} again: {bool(torch.equal(first[m], losses[m]))}" for m in first)
            print(f"bucket {f:.4f} R {lay.R} (R % 8 = {lay.R % 8}) -> {lay_m.R} | " + " | ".join(f"{m} {spread(m)}" for m in modes) +
                  f" | on_m/on {ratio('on_m', 'on'):.3f} pool_m/pool {ratio('pool_m', 'pool'):.3f} on_m/off {ratio('on_m', 'off'):.3f} "
                  f"pool_m/off {ratio('pool_m', 'off'):.3f} | loss " + " ".join(f"{m}={v:.6f}" for m, v in loss_bits.items()) +
                  f" on_m==on bits: {bool(torch.equal(losses['on_m'], first['on']))} pool_m==pool bits: {bool(torch.equal(losses['pool_m'], first['pool']))} (control: {again})", flush=True)
            for mode in modes[1:]:
                print(f"bucket {f:.4f} families (ms, one probed step, both towers) {mode}: {fam[mode]}", flush=True)


if __name__ == "__main__":
    main()
