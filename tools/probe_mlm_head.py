"""The fused MLM vocabulary head (CLIP.fuse_mlm_head; csrc/kernels/vocabce.h) against the unfused head, forward + backward, bf16.

    python tools/probe_mlm_head.py [--batch 1024] [--rounds 6] > profiles/rNN_mlm_head_probe.log

The default architecture with use_mlm at vocabularies of 4096, 10,000 and 49,408, the masking drawn by the model (15 %).  At each vocabulary
the step is timed with the attribute off and on, ALTERNATING in one session (off, on, off, ...); reported: each arm's median step with
min .. max, the ratio, and the peak of reserved memory of each arm (a pass of its own after emptying the cache).  The off arm is the
unfused formulation -- logits by ops.gemm, cross_entropy_fwd / _bwd_, the bias gradient by rows_scatter_add (above 4096 columns that call
runs the wide column sum).

Then the head's own launches at nm = 0.15 b n rows of D = 512: vocab_ce_fwd, vocab_ce_bwd (G), colsum(G) against gemm + bias,
cross_entropy_fwd, cross_entropy_bwd_ and the column-sum-only rows_scatter_add."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from x_clip_amd import CLIP, ops  # noqa: E402

ARMS = ("off", "on")


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def spread(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def probe_model(vocab, args, dev, g):
    torch.manual_seed(0)
    model = CLIP(use_mlm=True, num_text_tokens=vocab).to(torch.bfloat16).to(dev).train()
    b, n = args.batch, model.text_seq_len
    text = torch.randint(3, vocab, (b, n), generator=g).to(dev)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(dev)

    def step(arm):
        model.fuse_mlm_head = arm == "on"
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)                                         # the same masking in both arms
        model(text, image, return_loss=True).backward()

    times = {a: [] for a in ARMS}
    for r in range(args.warmup + args.rounds):
        for arm in ARMS:
            t = timed(lambda: step(arm), dev)
            if r >= args.warmup:
                times[arm].append(t)
    reserved = {}
    for arm in ARMS:
        model.zero_grad(set_to_none=True)
        ops._workspaces.clear()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        step(arm)
        torch.cuda.synchronize(dev)
        reserved[arm] = torch.cuda.max_memory_reserved(dev) / 2 ** 30
    med = {a: statistics.median(times[a]) for a in ARMS}
    print(f"{vocab} | {spread(times['off'])} | {spread(times['on'])} | {med['on'] / med['off']:.3f} | {reserved['off']:.2f} {reserved['on']:.2f}", flush=True)
    del model
    ops._workspaces.clear()
    torch.cuda.empty_cache()


def probe_launches(vocab, nm, dev, g, D=512, reps=10):
    x = (torch.randn(nm, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    W = (torch.randn(vocab, D, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    bias = (torch.randn(vocab, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, vocab, (nm,), generator=g).to(dev)
    gmul = torch.ones(1, device=dev)
    acc = torch.zeros(1, device=dev)
    db = torch.zeros(vocab, device=dev)
    lse = ops.vocab_ce_fwd(x, W, bias, labels, acc)
    G = ops.vocab_ce_bwd(x, W, bias, labels, lse, gmul)
    logits = ops.gemm(x, W, nm, vocab, D, bias=bias)
    lse_u = ops.cross_entropy_fwd(logits, vocab, labels, acc)
    print(f"# vocab {vocab}: max |lse fused - lse unfused| = {float((lse - lse_u).abs().max()):.3e}")
    fns = {
        "vocab_ce_fwd": lambda: ops.vocab_ce_fwd(x, W, bias, labels, acc, out=lse),
        "vocab_ce_bwd": lambda: ops.vocab_ce_bwd(x, W, bias, labels, lse, gmul, out=G),
        "colsum": lambda: ops.colsum(G, db),
        "gemm": lambda: ops.gemm(x, W, nm, vocab, D, bias=bias, out=logits),
        "ce_fwd": lambda: ops.cross_entropy_fwd(logits, vocab, labels, acc),
        "ce_bwd": lambda: ops.cross_entropy_bwd_(logits, vocab, labels, lse_u, gmul),     # (in place: later rounds read gradients, the same traffic)
        "rows_scatter_add": lambda: ops.rows_scatter_add(logits, None, None, db),
    }
    times = {k: [] for k in fns}
    for r in range(reps + 3):
        for k, fn in fns.items():
            t = timed(fn, dev)
            if r >= 3:
                times[k].append(t)
    fused = sum(statistics.median(times[k]) for k in ("vocab_ce_fwd", "vocab_ce_bwd", "colsum"))
    unfused = sum(statistics.median(times[k]) for k in ("gemm", "ce_fwd", "ce_bwd", "rows_scatter_add"))
    print(f"{vocab} {nm} | " + " | ".join(spread(times[k]) for k in fns) + f" | {fused:.3f} {unfused:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vocabs", type=int, nargs="+", default=[4096, 10000, 49408])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    print(f"# default CLIP with use_mlm: bf16, b = {args.batch}, n = 256; {args.rounds} alternating rounds after {args.warmup} warm-up rounds; ms, median (min .. max)")
    print("# vocab | step fuse_mlm_head off | step on | on/off | reserved GiB off on")
    for vocab in args.vocabs:
        probe_model(vocab, args, dev, g)
    nm = int(0.15 * args.batch * 256)
    print(f"# the head's launches at nm = {nm}, D = 512, bf16: 10 launches each, alternating; ms median (min .. max)")
    print("# vocab nm | vocab_ce_fwd | vocab_ce_bwd (G) | colsum(G) | gemm + bias | ce_fwd | ce_bwd | rows_scatter_add | sum fused, sum unfused")
    for vocab in args.vocabs:
        probe_launches(vocab, nm, dev, g)


if __name__ == "__main__":
    main()
