"""Full-batch contrastive gradients with the activation memory of one micro-batch (gradient caching: Gao et al. 2021, "Scaling Deep
Contrastive Learning Batch Size under Memory Limited Setup"; open_clip's --accum-freq).

    cached = CachedContrastiveStep(clip, opt, micro_batch=256, sync=None)
    loss = cached.step(text, image)            # backward included
    if sync is not None: sync.finish()
    opt.step(); opt.zero_grad()

Plain gradient accumulation does not help a contrastive loss: each micro-batch would see its own negatives only.  Here the towers run
twice over the batch, slice by slice, and the head once over all of it:

  1. every slice is encoded WITHOUT a graph up to its l2-normalised latents (rows are independent in both towers);
  2. the head (InfoNCE, DCL or the pairwise sigmoid loss; its own all-gather under a process group) runs once on the [b, dim_latent]
     latents as leaves: its backward gives d loss / d latents and the gradients of `temperature` / `logit_bias`;
  3. every slice is encoded again WITH a graph and its rows of d loss / d latents are pushed through it;
  4. the slices' parameter gradients are summed in fp32 by the optimizer (`FusedAdamW.accumulate`) and rounded once into `.grad`.

Loss and gradients are those of `clip(text, image, return_loss=True).backward()`; the activations alive at any time are one slice's.
"""
from __future__ import annotations

from typing import Optional

import torch

from .clip import CLIP
from .optim import FusedAdamW

_UNSUPPORTED = ("use_all_token_embeds", "use_mlm", "use_visual_ssl", "extra_latent_projection")


class CachedContrastiveStep:
    """One training step of `clip` at batch size b with the activation memory of `micro_batch` rows.  `step()` leaves the full-batch
    gradients in `.grad` (every parameter that the one-pass step gives a gradient, and no other) and returns the detached loss, a device
    scalar; nothing is read back to the host.  `clip(...)` itself is not called: the step runs CLIP's own tower, latent and head
    helpers, so what it computes is what `forward` computes.

    * Why the sum is fp32: `.grad` of a bf16 model is bf16, and autograd's `+=` over k slices rounds to an 8-bit mantissa k times.
      The slices' gradients are added into the optimizer's flat fp32 accumulator (4 bytes per parameter) and rounded once.
    * Why the second pass repeats the first exactly: dropout keep-masks are functions of a seed drawn from torch's CPU generator and
      PatchDropout draws from the device generator; the state of both is saved in front of every slice of the first pass and restored
      in front of the same slice of the second.  `verify_replay = True` checks it: `last_replay_diff` (device scalar) is the largest
      absolute difference between a slice's replayed latents and its cached rows, exactly 0 when the replay is faithful.  Off (the
      default) it costs nothing.
    * `micro_batch >= b` is one slice.  The last slice may be shorter.  `clip.text_micro_batches` / `image_micro_batches` apply inside
      a slice as they do inside `forward`.
    * With a process group `sync` must be a `GradSync(clip, overlap=False)`: a bucket completed from a hook would be all-reduced
      before `accumulate_end()` has written the sum into it.  The all-reduce is therefore exposed: the default model's buckets (117 MB
      in bf16) take about 1 ms on the ring against a step of seconds at the batch sizes this class is for.
      Ragged per-rank batches follow the heads' rules (`clip.assume_equal_batch`).
    * Not supported (raises NotImplementedError at construction): `use_all_token_embeds` (FILIP), `use_mlm`, `use_visual_ssl`,
      `extra_latent_projection`, `sim_reg_loss_weight > 0`; `step` takes no `aug_text` / `aug_image` (no multiview loss)."""

    def __init__(self, clip: CLIP, opt: FusedAdamW, micro_batch: int = 256, sync=None):
        bad = [k for k in _UNSUPPORTED if getattr(clip, k)]
        if clip.sim_reg_loss_weight > 0:
            bad.append("sim_reg_loss_weight")
        if bad:
            raise NotImplementedError(f"x_clip_amd CachedContrastiveStep: not defined for a CLIP built with {', '.join(bad)} -- the cached "
                                      "step covers the CLS heads (InfoNCE, DCL, sigmoid) without side losses")
        if int(micro_batch) < 1:
            raise ValueError(f"invalid micro_batch: {micro_batch}")
        if sync is not None or clip.requires_all_gather:
            from .distributed import GradSync
            if not isinstance(sync, GradSync) or sync.overlap:
                raise ValueError("x_clip_amd CachedContrastiveStep: with a process group (or any `sync`) pass sync=GradSync(clip, overlap=False): a "
                                 "bucket all-reduced from a backward hook would go out before accumulate_end() has written the summed gradient")
        self.clip, self.opt, self.micro_batch, self.sync = clip, opt, int(micro_batch), sync
        self.verify_replay = False
        self.last_replay_diff: Optional[torch.Tensor] = None

    @staticmethod
    def _rng_state(device):
        return torch.get_rng_state(), (torch.cuda.get_rng_state(device) if device.type == "cuda" else None)

    @staticmethod
    def _set_rng_state(state, device):
        torch.set_rng_state(state[0])
        if state[1] is not None:
            torch.cuda.set_rng_state(state[1], device)

    def step(self, text, image, freeze_image_encoder: bool = False, freeze_text_encoder: bool = False) -> torch.Tensor:
        clip, opt = self.clip, self.opt
        assert clip.training, 'loss cannot be used if not training'
        b, device = text.shape[0], text.device
        assert image.shape[0] == b
        bounds = [(lo, min(lo + self.micro_batch, b)) for lo in range(0, b, self.micro_batch)]
        vt = clip.visual_transformer
        keep_all = getattr(vt, "keep_indices_override", None)   # an injected PatchDropout draw is per image: slice it too

        def latents(lo, hi):
            if keep_all is not None:
                vt.keep_indices_override = keep_all[lo:hi]
            try:
                return clip._cls_latents(text[lo:hi], image[lo:hi], freeze_image_encoder, freeze_text_encoder)
            finally:
                if keep_all is not None:
                    vt.keep_indices_override = keep_all

        # 1. the latents of the whole batch, no graph
        opt.accumulate_begin()
        states, t_parts, i_parts = [], [], []
        with torch.no_grad():
            for lo, hi in bounds:
                states.append(self._rng_state(device))
                tl, il = latents(lo, hi)
                t_parts.append(tl)
                i_parts.append(il)
        text_latents = (t_parts[0] if len(bounds) == 1 else torch.cat(t_parts, dim=0)).detach().requires_grad_(True)
        image_latents = (i_parts[0] if len(bounds) == 1 else torch.cat(i_parts, dim=0)).detach().requires_grad_(True)
        del t_parts, i_parts

        # 2. the head, once: d loss / d latents and the gradients of the head's own scalars
        loss = clip._cls_head(text_latents[None], image_latents[None], None, None, clip._contrastive_spec())
        loss.backward()
        scalars = [p for p in (clip.temperature, getattr(clip, "logit_bias", None)) if p is not None and p.grad is not None]
        stash = [p.grad for p in scalars]
        for p in scalars:
            p.grad = None
        d_text, d_image = text_latents.grad, image_latents.grad

        # 3. every slice again, with a graph; its parameter gradients go into the optimizer's fp32 sum
        diff = torch.zeros((), dtype=torch.float32, device=device) if self.verify_replay else None
        for (lo, hi), state in zip(bounds, states):
            self._set_rng_state(state, device)
            tl, il = latents(lo, hi)
            if diff is not None:
                with torch.no_grad():
                    diff = torch.maximum(diff, torch.maximum((tl.detach().float() - text_latents.detach()[lo:hi].float()).abs().max(),
                                                             (il.detach().float() - image_latents.detach()[lo:hi].float()).abs().max()))
            torch.autograd.backward([tl, il], [d_text[lo:hi], d_image[lo:hi]])
            del tl, il
            opt.accumulate()
        if diff is not None:
            self.last_replay_diff = diff

        # 4. the sum, rounded once, becomes .grad
        opt.accumulate_end()
        for p, g in zip(scalars, stash):
            p.grad = g
        return loss.detach()
