"""Packed CAUSAL text tower (CLIP.pack_text_causal) against the dense causal one: the sibling of tools/probe_packed_text.py.

    python tools/probe_packed_text_causal.py [--batch 1024] [--rounds 6] > profiles/rNN_packed_text_causal_probe.log

Configuration A: the default CLIP architecture with text_causal_mask=True (n = 256), bf16, forward + backward, optimizer not included; token
lengths (EOS included) drawn with a fixed seed, uniform in [1, 2 f n], for fills f = 1/16, 1/4 and 1 (f = 1: the EOS is every sample's last token).
Configuration B: a context of 77 tokens with lengths uniform in 8 .. 32.  At each row the step is timed in three modes -- attribute off (the dense
causal path), on, and on with `pack_text_pool_last` -- ALTERNATING in one session (drift hits all alike); reported: the median step of each,
the ratios to off, the peak of reserved memory of each mode (a pass of its own after emptying the cache), and for one layer on that layout (8
heads) the causal varlen attention forward / backward beside the non-causal varlen kernels on the same layout."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x_clip_amd import CLIP, ops, text_layout  # noqa: E402

MODES = ("off", "on", "pool")
EOS = 2


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def tokens(b, n, lens, g):
    """lens[s] tokens ending in the EOS, padding behind it"""
    text = torch.randint(3, 10000, (b, n), generator=g)
    at = torch.arange(n)[None]
    text[at >= lens[:, None]] = 0
    text[at == lens[:, None] - 1] = EOS
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b = args.batch
    g = torch.Generator().manual_seed(1)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)
    med = lambda fn: statistics.median(timed(fn, dev) for _ in range(10))
    print(f"# default CLIP with text_causal_mask=True, bf16, b = {b}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; times in ms (median)")
    print("# off = pack_text_causal off (dense causal tower); on = pack_text_causal; pool = pack_text_causal + pack_text_pool_last")
    print("# config n fill_target fill R max_len | step_off step_on step_pool on/off pool/off | reserved_off_GiB reserved_on_GiB reserved_pool_GiB | "
          "causal_varlen_fwd causal_varlen_bwd varlen_fwd varlen_bwd (one layer, 8 heads)")
    rows = [("A", 256, f) for f in (1 / 16, 1 / 4, 1.0)] + [("B", 77, None)]
    model, model_n = None, None
    for config, n, f in rows:
        if model_n != n:
            del model
            torch.manual_seed(0)
            model = CLIP(text_causal_mask=True, text_eos_id=EOS, text_seq_len=n).to(torch.bfloat16).to(dev).train()
            model_n = n
        if f is None:
            lens = torch.randint(8, 33, (b,), generator=g)
        elif f < 1.0:
            lens = torch.randint(1, int(2 * f * n) + 1, (b,), generator=g)
        else:
            lens = torch.full((b,), n)
        text = tokens(b, n, lens, g)
        lay = text_layout(text, pad_id=0, has_cls=False, eos_id=EOS)
        text = text.to(dev)

        def step(mode):
            model.pack_text_causal, model.pack_text_pool_last = mode != "off", mode == "pool"
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
        layd = lay.to(dev)
        qkv = torch.randn(lay.R, 3 * 8 * 64, device=dev).to(torch.bfloat16)
        do = torch.randn(lay.R, 8 * 64, device=dev).to(torch.bfloat16)
        kernel = []
        for fwd, bwd in ((ops.attention_varlen_causal_fwd, ops.attention_varlen_causal_bwd), (ops.attention_varlen_fwd, ops.attention_varlen_bwd)):
            out, lse = fwd(qkv, layd.cu, lay.max_len, 8, 0.125)
            kernel += [med(lambda: fwd(qkv, layd.cu, lay.max_len, 8, 0.125)), med(lambda: bwd(qkv, layd.cu, lay.max_len, out, do, lse, 8, 0.125))]
        off, on, pool = (statistics.median(times[m]) for m in MODES)
        print(f"{config} {n} {'-' if f is None else format(f, '.4f')} {lay.R / (b * n):.4f} {lay.R} {lay.max_len} | {off:.2f} {on:.2f} {pool:.2f} "
              f"{on / off:.3f} {pool / off:.3f} | {reserved['off']:.2f} {reserved['on']:.2f} {reserved['pool']:.2f} | "
              + " ".join(f"{t:.3f}" for t in kernel), flush=True)
        del qkv, do, out, lse


if __name__ == "__main__":
    main()
