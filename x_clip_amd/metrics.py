"""In-batch retrieval metrics of a contrastive step -- recall@k, mean rank of the positive, margin to the hardest negative -- computed
WITHOUT the b x B logits matrix: a third epilogue on the head's similarity tile loop (csrc/kernels/simrank.h) counts, per row, the
negatives that beat the positive and keeps the hardest one; what is left for torch are reductions over [b]-long vectors.

    m = contrastive_metrics(text_latents, image_latents, clip.temperature)
    m["t2i"]["recall@1"], m["i2t"]["mean_rank"], m["t2i"]["margin"] ...

or, inside training, `clip.track_metrics()` and `clip.last_metrics` after every forward(..., return_loss=True).  Single-process calls read
nothing back to the host; the multi-rank form reads the per-rank batch sizes once per call unless told they are equal.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import distributed as xdist
from . import ops
from .losses import _waiter

Tensor = torch.Tensor


def _direction(q: Tensor, chunks, off: int, tau32: Optional[Tensor], ks: Sequence[int], waiter):
    rank, hard_val, hard_idx, pos = ops.simrank_chunked(q, chunks, 1.0, off, log_scale=tau32, before_chunk=waiter)
    out = {"rank": rank, "hard_idx": hard_idx, "margin": pos - hard_val}
    # [1 + len(ks)] sums over the local rows: sum of ranks, then the hits per k
    sums = torch.stack([rank.sum(dtype=torch.float64)] + [(rank < k).sum().to(torch.float64) for k in ks])
    return out, sums


@torch.no_grad()
def contrastive_metrics(text_latents: Tensor, image_latents: Tensor, temperature: Optional[Tensor] = None, ks: Sequence[int] = (1, 5, 10),
                        group=None, *, distributed: Optional[bool] = None, assume_equal_batch: bool = False) -> dict:
    """text_latents [b, d], image_latents [b', d] (the l2-normalised latents of matched pairs, row i of one with row i of the other);
    temperature: the model's LOG-temperature parameter (CLIP.temperature; None = logits are plain cosines).
    -> {"t2i": {...}, "i2t": {...}}, each direction with
         rank [b] int32 (0 = the positive beats every negative), hard_idx [b] int32 (global column of the hardest negative),
         margin [b] fp32 (positive - hardest negative), recall@k (fp32 scalars, one per k in ks), mean_rank (fp32 scalar).
    The results are device tensors and no result is read back.  With an initialised process group (`group`, or the default one) every
    rank contributes its rows: the other side's latents are all-gathered (ragged batches allowed, a rank may hold no rows) and consumed
    chunk by chunk as they arrive, recall@k and mean_rank are all-reduced -- global, the same on every rank -- while the per-row vectors
    describe the local rows.  The ragged form costs ONE host read per call: the per-rank batch sizes (both sides in one exchange), as
    the loss's own gather does; `assume_equal_batch=True` (every rank holds as many texts and images as this one: what
    CLIP.assume_equal_batch promises, and what CLIP.track_metrics passes on) skips it.
    `distributed` (keyword only, beyond the reference-shaped signature): None = whether a process group with more than one rank is up;
    False forces the single-process form on the local rows (a `group` given with it is an error); CLIP.forward passes the flag it
    latched at construction, as it does for the loss."""
    assert text_latents.dim() == 2 and image_latents.dim() == 2 and text_latents.shape[1] == image_latents.shape[1]
    assert text_latents.dtype == image_latents.dtype
    ks = tuple(int(k) for k in ks)
    T, I = ops._c(text_latents.detach()), ops._c(image_latents.detach())
    dev = T.device
    tau32 = None if temperature is None else temperature.detach().reshape(1).float().contiguous()
    if distributed is None:
        distributed = xdist.is_distributed() if group is None else xdist.dist.get_world_size(group) > 1
    elif not distributed and group is not None:
        raise ValueError("contrastive_metrics: distributed=False scores the local rows alone -- it takes no process group")
    bt, bi = T.shape[0], I.shape[0]
    if distributed:
        rk = xdist.dist.get_rank(group)
        if assume_equal_batch:
            world = xdist.dist.get_world_size(group)
            tsizes, isizes = [bt] * world, [bi] * world
        else:
            # both counts in one exchange (one tiny collective, one host read), as distributed.exchange_sizes does for one
            world = xdist.dist.get_world_size(group)
            mine = torch.tensor([bt, bi], dtype=torch.int64, device=dev)
            counts = torch.empty(world, 2, dtype=torch.int64, device=dev)
            xdist._gather_into(counts, mine, group, async_op=False)
            counts = counts.tolist()
            tsizes, isizes = [int(c[0]) for c in counts], [int(c[1]) for c in counts]
        Bt, Bi = sum(tsizes), sum(isizes)
        if Bt != Bi:
            raise ValueError(f"contrastive_metrics: {Bt} texts and {Bi} images over all ranks -- in-batch retrieval needs matched pairs")
        gt, gi = xdist.GatheredViews([T], tsizes, group, tag="metrics_gather"), xdist.GatheredViews([I], isizes, group, tag="metrics_gather")
        toff, ioff = sum(tsizes[:rk]), sum(isizes[:rk])
        t2i, s1 = _direction(T, gi.chunks(0), toff, tau32, ks, _waiter(gi))
        i2t, s2 = _direction(I, gt.chunks(0), ioff, tau32, ks, _waiter(gt))
        gi.wait()
        gt.wait()
        sums = xdist.all_reduce_scalars(torch.stack([s1, s2]), group)
        B = Bt
    else:
        if bt != bi:
            raise ValueError(f"contrastive_metrics: {bt} texts and {bi} images -- in-batch retrieval needs matched pairs")
        t2i, s1 = _direction(T, [(I, 0)], 0, tau32, ks, None)
        i2t, s2 = _direction(I, [(T, 0)], 0, tau32, ks, None)
        sums = torch.stack([s1, s2])
        B = bt
    sums = (sums / B).float()
    for d, out in enumerate((t2i, i2t)):
        out["mean_rank"] = sums[d, 0]
        for j, k in enumerate(ks):
            out[f"recall@{k}"] = sums[d, 1 + j]
    return {"t2i": t2i, "i2t": i2t}
