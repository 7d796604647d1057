"""What one does with a trained CLIP: retrieval over a gallery and zero-shot classification -- the k best gallery columns of every
query WITHOUT the nq x ng logits matrix (csrc/kernels/simtopk.h: two sweeps of the head's similarity tile loop and a threshold, no
sort), on latents that come from ONE tower (CLIP.embed_text / CLIP.embed_image).

    protos = zero_shot_classifier(clip, class_prompts)                       # [C, P, seq] token ids -> [C, dim_latent]
    values, indices = similarity_topk(clip.embed_image(x), protos, 5, clip.temperature)     # zero-shot top-5

    gallery = clip.embed_image(images)                                       # or a list of (chunk, first column)
    values, indices = similarity_topk(clip.embed_text(queries), gallery, 10, clip.temperature)

Nothing is read back to the host.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from . import ops

Tensor = torch.Tensor


@torch.no_grad()
def similarity_topk(queries: Tensor, gallery: Union[Tensor, Sequence[Tuple[Tensor, int]]], k: int,
                    temperature: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """queries [nq, d]; gallery [ng, d] or a list of (chunk [ng_c, d], first global column), in any order; 1 <= k <= 32;
    temperature: the model's LOG-temperature parameter (CLIP.temperature; None = logits are plain cosines), as in contrastive_metrics.
    -> values [nq, k] fp32 (the logits exp(temperature) <q_i, g_j>, row-wise non-increasing), indices [nq, k] int32 (global gallery
    columns, the lowest column first among equal values).  A row with fewer than k scorable columns -- a gallery smaller than k, NaN
    latents -- is padded with index -1 / value -3e38.  The same call returns the same bits every time.  How the gallery is cut into
    chunks does not change the result where the logits are exact in fp32; on real latents it can change it only among near-ties inside
    the fp32 accumulation error (which columns are re-scored is decided by the tile loop's logit against a threshold that follows the
    cuts, the ranking by the re-scored logit).  Scratch: 5 4-byte words per (query, 64 gallery columns); the logits are never stored.
    The cost beyond the two sweeps grows with the number of candidates at or above a row's threshold: k to a few k on real latents, the
    whole row when every logit is equal.
    A gallery sharded over ranks: every rank calls this on its shard, as a (chunk, first global column) list, and the [nq, W * k]
    results are merged by a sort -- nothing is built in for it."""
    k = int(k)
    if not 1 <= k <= ops.SIMTOPK_MAX_K:
        raise ValueError(f"similarity_topk: k must lie in 1 .. {ops.SIMTOPK_MAX_K}, got {k}")
    chunks = [(gallery, 0)] if isinstance(gallery, Tensor) else [(c, int(col0)) for c, col0 in gallery]
    if queries.dim() != 2:
        raise ValueError(f"similarity_topk: queries must be [nq, d], got {tuple(queries.shape)}")
    for c, col0 in chunks:
        if c.dim() != 2 or c.shape[1] != queries.shape[1]:
            raise ValueError(f"similarity_topk: gallery chunk at column {col0} is {tuple(c.shape)}, queries are {tuple(queries.shape)}: "
                             "both must be [rows, d] with the same d")
        if c.dtype != queries.dtype:
            raise TypeError(f"similarity_topk: gallery chunk at column {col0} is {c.dtype}, queries are {queries.dtype}")
    tau32 = None if temperature is None else temperature.detach().reshape(1).float().contiguous()
    return ops.simtopk_chunked(ops._c(queries.detach()), [(ops._c(c.detach()), col0) for c, col0 in chunks], k, 1.0, log_scale=tau32)


@torch.no_grad()
def zero_shot_classifier(clip, class_prompts: Tensor, batch: int = 256) -> Tensor:
    """class_prompts [C, P, seq] token ids (P prompt templates per class) -> the class prototypes [C, dim_latent]: the mean over the P
    l2-normalised text latents of a class, normalised again.  The text tower runs on slices of at most `batch` prompts (rounded down to
    whole classes), so C * P need not fit in one batch."""
    if class_prompts.dim() != 3:
        raise ValueError(f"zero_shot_classifier: class_prompts must be [classes, prompts per class, seq] token ids, got {tuple(class_prompts.shape)}")
    C, P, seq = class_prompts.shape
    per = max(1, int(batch) // P)                                    # classes per slice
    protos = []
    for c0 in range(0, C, per):
        ids = class_prompts[c0: c0 + per]
        lat = clip.embed_text(ids.reshape(-1, seq))                  # [c * P, d]
        protos.append(ops.l2norm_fwd(ops.token_mean_fwd(lat.view(ids.shape[0], P, -1)))[0])
    return protos[0] if len(protos) == 1 else torch.cat(protos, dim=0)
