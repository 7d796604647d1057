"""Packed text tower against the pruned dense one, BASELINE configs[1] (default CLIP, bf16, b = 1024, forward + backward, optimizer not included).

    python tools/probe_packed_text.py [--batch 1024] [--rounds 6] > profiles/rNN_packed_text_probe.log

Token lengths are drawn with a fixed seed, uniform in [1, 2 f n], so that the fill R / (b (n + 1)) is about f = 1/16, 1/4 and 1 of n = 256 (f = 1:
no padding at all).  At each fill the step is timed with `pack_text` off (today's pruned path) and on, ALTERNATING in one session (off, on, off,
on, ...: drift of the clocks hits both alike); reported: the median step of each, their ratio, the peak of reserved memory of each mode (measured in
a pass of its own after emptying the cache), and the varlen attention forward / backward alone on the layout of that fill."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x_clip_amd import CLIP, ops, text_layout  # noqa: E402


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CLIP().to(torch.bfloat16).to(dev).train()
    n, b = model.text_seq_len, args.batch
    g = torch.Generator().manual_seed(1)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)
    print(f"# default CLIP bf16, b = {b}, n = {n}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; times in ms (median)")
    print("# fill_target fill R max_len | step_off step_on on/off | reserved_off_GiB reserved_on_GiB | varlen_attn_fwd varlen_attn_bwd (one layer, 8 heads)")
    for f in (1 / 16, 1 / 4, 1.0):
        text = torch.randint(1, 10000, (b, n), generator=g)
        if f < 1.0:
            lens = torch.randint(1, int(2 * f * n) + 1, (b,), generator=g)
            text[torch.arange(n)[None] >= lens[:, None]] = 0
        lay = text_layout(text, pad_id=0)
        text = text.to(dev)

        def step(pack):
            model.pack_text = pack
            model.zero_grad(set_to_none=True)
            model(text, image, return_loss=True, **(dict(text_layout=lay) if pack else {})).backward()

        times = {False: [], True: []}
        for r in range(args.warmup + args.rounds):
            for pack in (False, True):
                t = timed(lambda: step(pack), dev)
                if r >= args.warmup:
                    times[pack].append(t)
        reserved = {}
        for pack in (False, True):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            step(pack)
            torch.cuda.synchronize(dev)
            reserved[pack] = torch.cuda.max_memory_reserved(dev) / 2 ** 30
        layd = lay.to(dev)
        qkv = torch.randn(lay.R, 3 * 8 * 64, device=dev).to(torch.bfloat16)
        do = torch.randn(lay.R, 8 * 64, device=dev).to(torch.bfloat16)
        out, lse = ops.attention_varlen_fwd(qkv, layd.cu, lay.max_len, 8, 0.125)
        tf = statistics.median(timed(lambda: ops.attention_varlen_fwd(qkv, layd.cu, lay.max_len, 8, 0.125), dev) for _ in range(10))
        tb = statistics.median(timed(lambda: ops.attention_varlen_bwd(qkv, layd.cu, lay.max_len, out, do, lse, 8, 0.125), dev) for _ in range(10))
        off, on = statistics.median(times[False]), statistics.median(times[True])
        print(f"{f:.4f} {lay.R / (b * (n + 1)):.4f} {lay.R} {lay.max_len} | {off:.2f} {on:.2f} {on / off:.3f} | {reserved[False]:.2f} {reserved[True]:.2f} | "
              f"{tf:.3f} {tb:.3f}", flush=True)
        del qkv, do, out, lse


if __name__ == "__main__":
    main()
