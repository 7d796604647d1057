"""Packed ROTARY text tower (CLIP.pack_text_rotary) against the dense rotary one: the sibling of tools/probe_packed_text_causal.py.

    python tools/probe_packed_text_rotary.py [--batch 1024] [--rounds 6] > profiles/rNN_packed_rotary_probe.log

The default CLIP architecture with text_rotary_pos_emb=True (n = 256), bf16, forward + backward, optimizer not included; token lengths drawn with
a fixed seed, uniform in [1, 2 f n], for fills f = 1/16, 1/4 and 1.  At each fill the step is timed in three modes -- attribute off (the dense
rotary tower, pooled last layer as by default), on, and on with `pack_text_pool_last` -- ALTERNATING in one session (drift hits all alike);
reported: the median step of each and its spread (min .. max), the ratios to off, the peak of reserved memory of each mode (a pass of its own
after emptying the cache), and xclip_rotary_pos beside xclip_rotary on equal rows: the R kept rows of that fill, [R, 1536] (median, min .. max
of 20 launches each, alternating).  At fill 1 that array is the [263,168, 1536] qkv activation of the dense tower."""
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


def spread(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f}..{max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, n = args.batch, 256
    g = torch.Generator().manual_seed(1)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)
    print(f"# default CLIP with text_rotary_pos_emb=True, bf16, b = {b}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; times in ms: median (min..max)")
    print("# off = pack_text_rotary off (dense rotary tower); on = pack_text_rotary; pool = pack_text_rotary + pack_text_pool_last")
    print("# n fill_target fill R max_len | step_off step_on step_pool on/off pool/off | reserved_off_GiB reserved_on_GiB reserved_pool_GiB | "
          "xclip_rotary xclip_rotary_pos pos/dense (in place on [R, 1536], forward)")
    torch.manual_seed(0)
    model = CLIP(text_rotary_pos_emb=True, text_seq_len=n).to(torch.bfloat16).to(dev).train()
    freq = model.text_transformer.rotary_pos_emb.frequencies(dev)
    for f in (1 / 16, 1 / 4, 1.0):
        lens = torch.randint(1, int(2 * f * n) + 1, (b,), generator=g) if f < 1.0 else torch.full((b,), n)
        text = torch.randint(1, 10000, (b, n), generator=g)
        text[torch.arange(n)[None] >= lens[:, None]] = 0
        lay = text_layout(text, pad_id=0)
        text = text.to(dev)

        def step(mode):
            model.pack_text_rotary, model.pack_text_pool_last = mode != "off", mode == "pool"
            model.zero_grad(set_to_none=True)
            model(text, image, return_loss=True, **(dict(text_layout=lay) if mode != "off" else {})).backward()

        times = {m: [] for m in MODES}
        for r in range(args.warmup + args.rounds):
            for mode in MODES:
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
        torch.cuda.empty_cache()
        layd = lay.to(dev)
        qkv = torch.randn(lay.R, 3 * 8 * 64, device=dev).to(torch.bfloat16)
        kern = {"dense": [], "pos": []}
        for r in range(22):                                      # (alternating; the first two launches of each warm up)
            td = timed(lambda: ops.rotary_(qkv, n + 1, freq), dev)
            tp = timed(lambda: ops.rotary_pos_(qkv, layd.pos, freq), dev)
            if r >= 2:
                kern["dense"].append(td)
                kern["pos"].append(tp)
        off, on, pool = (statistics.median(times[m]) for m in MODES)
        print(f"{n} {f:.4f} {lay.R / (b * (n + 1)):.4f} {lay.R} {lay.max_len} | {spread(times['off'])} {spread(times['on'])} {spread(times['pool'])} "
              f"{on / off:.3f} {pool / off:.3f} | {reserved['off']:.2f} {reserved['on']:.2f} {reserved['pool']:.2f} | "
              f"{spread(kern['dense'])} {spread(kern['pos'])} {statistics.median(kern['pos']) / statistics.median(kern['dense']):.3f}", flush=True)
        del qkv


if __name__ == "__main__":
    main()
