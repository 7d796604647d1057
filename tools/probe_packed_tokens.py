"""Packed text tower for the heads that read token rows (CLIP.pack_text_tokens) against the dense tower, forward + backward, bf16.

    python tools/probe_packed_tokens.py [--batch 512] [--rounds 6] > profiles/rNN_packed_tokens_probe.log

Two models: BASELINE configs[3] (FILIP: use_all_token_embeds, image 224 / patch 16, n = 77, b = 512) and the default model with use_mlm (n = 256,
a vocabulary of 4096 -- the widest row the bf16 MLM head's bias gradient takes; its batch is --mlm-batch).  Token lengths are drawn with a fixed seed, uniform in [1, 2 f n], so that the fill R / (b (n + 1)) is about f = 1/16,
1/4 and 1 (f = 1: no padding).  At each fill the step is timed with the attribute off, on, and on with row_multiple = 256, ALTERNATING in one
session (off, on, on_m, off, ...); reported: each mode's median step with min .. max, the ratios to off, and the peak of reserved memory of each
mode (a pass of its own after emptying the cache).  The layouts are built from the CPU tokens.

Then the two kernels at [R, 512] of each FILIP fill (pos0 = 1, n_out = 77) against the formulation they replace -- ops.gather_rows over
cat([x, zero row]) with an index map, as _PackedTextEncodeFn.backward scatters dy -- and a plain device copy of the same bytes (the floor)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x_clip_amd import CLIP, ops, text_layout  # noqa: E402

MODES = ("off", "on", "on_m")


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def tokens(b, n, f, g, vocab):
    text = torch.randint(3, vocab, (b, n), generator=g)
    if f < 1.0:
        lens = torch.randint(1, int(2 * f * n) + 1, (b,), generator=g)
        text[torch.arange(n)[None] >= lens[:, None]] = 0
    return text


def probe_model(name, model, b, image, args, dev, g, vocab=10000):
    n = model.text_seq_len
    print(f"# {name}: bf16, b = {b}, n = {n}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; ms, median (min .. max)")
    print("# fill_target fill kept R_m max_len | step_off | step_on | step_on_m | on/off on_m/off | reserved GiB off on on_m")
    layouts = []
    for f in (1 / 16, 1 / 4, 1.0):
        text = tokens(b, n, f, g, vocab)
        lay, lay_m = text_layout(text, pad_id=0), text_layout(text, pad_id=0, row_multiple=256)
        layouts.append(lay)
        text = text.to(dev)

        def step(mode):
            model.pack_text_tokens = mode != "off"
            model.zero_grad(set_to_none=True)
            kw = {} if mode == "off" else dict(text_layout=lay_m if mode == "on_m" else lay)
            model(text, image, return_loss=True, **kw).backward()

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
        med = {m: statistics.median(times[m]) for m in MODES}
        spread = lambda m: f"{med[m]:.2f} ({min(times[m]):.2f} .. {max(times[m]):.2f})"
        print(f"{f:.4f} {lay.kept / (b * (n + 1)):.4f} {lay.kept} {lay_m.R} {lay.max_len} | " + " | ".join(spread(m) for m in MODES) +
              f" | {med['on'] / med['off']:.3f} {med['on_m'] / med['off']:.3f} | " + " ".join(f"{reserved[m]:.2f}" for m in MODES), flush=True)
    return layouts


def probe_kernels(layouts, n, dev, D=512, reps=20):
    print(f"# kernels at [R, {D}] bf16, pos0 = 1, n_out = {n}: {reps} launches each, alternating; ms median (min .. max); GB/s = bytes moved / median")
    print("# R dense_rows | unpack_rows | gather_rows(cat([x, 0]), map) | copy of the same bytes || pack_rows | gather_rows(dense, map) + zero rows | copy")
    for lay in layouts:
        layd = lay.to(dev)
        b = lay.batch
        x = torch.randn(lay.R, D, device=dev).to(torch.bfloat16)
        y = torch.randn(b, n, D, device=dev).to(torch.bfloat16)
        row_of = layd.row_of()[:, 1:].reshape(-1)
        to_dense = torch.where(row_of < 0, torch.full_like(row_of, lay.R), row_of).contiguous()              # dropped positions -> the appended zero row
        flat = (layd._flat() - torch.searchsorted(layd.cu[1:], torch.arange(lay.kept, dtype=torch.int32, device=dev), right=True) - 1).to(torch.int32)
        to_packed = torch.where(layd.pos[:lay.kept] > 0, flat, torch.full_like(flat, b * n)).contiguous()      # CLS rows -> the appended zero row
        nbytes = (lay.kept - b + b * n) * D * 2                                                               # rows read + rows written, once each
        half = torch.empty(nbytes // 4, device=dev, dtype=torch.bfloat16)
        src = torch.randn(nbytes // 4, device=dev).to(torch.bfloat16)
        fns = {
            "unpack": lambda: ops.unpack_rows(x, layd.cu, layd.pos, 1, n),
            "unpack_gather": lambda: ops.gather_rows(torch.cat([x, x.new_zeros(1, D)], dim=0), to_dense),
            "pack": lambda: ops.pack_rows(y, layd.cu, layd.pos, 1),
            "pack_gather": lambda: ops.gather_rows(torch.cat([y.view(b * n, D), y.new_zeros(1, D)], dim=0), to_packed),
            "copy": lambda: half.copy_(src),
        }
        got = ops.unpack_rows(x, layd.cu, layd.pos, 1, n).view(b * n, D)
        assert torch.equal(got, fns["unpack_gather"]()), "the two unpack formulations differ"
        assert torch.equal(ops.pack_rows(y, layd.cu, layd.pos, 1)[:lay.kept], fns["pack_gather"]()), "the two pack formulations differ"
        times = {k: [] for k in fns}
        for r in range(reps + 3):
            for k, fn in fns.items():
                t = timed(fn, dev)
                if r >= 3:
                    times[k].append(t)
        s = lambda k: f"{statistics.median(times[k]):.4f} ({min(times[k]):.4f} .. {max(times[k]):.4f}) {nbytes / statistics.median(times[k]) / 1e6:.0f} GB/s"
        print(f"{lay.R} {b * n} | {s('unpack')} | {s('unpack_gather')} | {s('copy')} || {s('pack')} | {s('pack_gather')} | {s('copy')}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--mlm-batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    filip = CLIP(use_all_token_embeds=True, visual_image_size=224, visual_patch_size=16, text_seq_len=77).to(torch.bfloat16).to(dev).train()
    image = torch.randn(args.batch, 3, 224, 224, generator=g).to(torch.bfloat16).to(dev)
    layouts = probe_model("configs[3] FILIP (image 224 / patch 16)", filip, args.batch, image, args, dev, g)
    probe_kernels(layouts, 77, dev)
    del filip, image
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    mlm = CLIP(use_mlm=True, num_text_tokens=4096).to(torch.bfloat16).to(dev).train()
    image = torch.randn(args.mlm_batch, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)
    # (a vocabulary of 4096: the bf16 MLM head's bias gradient is a column sum over rows of at most 4096 elements, xclip_rows_scatter_add)
    probe_model("default CLIP with use_mlm, num_text_tokens = 4096", mlm, args.mlm_batch, image, args, dev, g, vocab=4096)


if __name__ == "__main__":
    main()
