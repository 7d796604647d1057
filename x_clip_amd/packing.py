"""The packed form of a padded text batch: only the rows the key-padding mask keeps, laid end to end.

`CLIP.forward` hides padded keys from attention (`text_mask = text != text_pad_id`, reference x_clip.py:614) and, under the CLS head, reads
row 0 of every sample alone (x_clip.py:708).  A padded row is then never a key, everything else in the tower is row-wise, and nothing reads
its output: it can influence nothing and its gradient is exactly zero.  `text_layout` describes the batch without those rows; the text tower
(`CLIP.pack_text`) embeds, attends and back-propagates on the `R` kept rows only.

    layout = text_layout(tokens, pad_id=0)            # tokens on the CPU (a loader's pinned buffer): no device read
    loss = clip(text, image, return_loss=True, text_layout=layout)

Built from CPU tokens the layout costs no device synchronisation: `R` and `max_len` are counted on the host and the index tensors are copied
to the device asynchronously by `.to(device)`.  Built from DEVICE tokens -- the implicit path when `pack_text` is on and no layout is passed --
it reads `R` and `max_len` back ONCE per call (one small device-to-host copy, the same kind of read the ragged multi-rank gather of
x_clip_amd.distributed makes for the per-rank batch sizes): the packed arrays cannot be allocated without their row count.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

Tensor = torch.Tensor


@dataclass(frozen=True)
class TextLayout:
    cu: Tensor          # int32 [B + 1]: sample s owns packed rows cu[s] .. cu[s+1]
    pos: Tensor         # int32 [R]: position of the row inside its sample; 0 = the CLS row when the encoder has one
    tok: Tensor         # int64 [R]: the row's token id (0 on CLS rows, where it is ignored)
    R: int
    max_len: int
    batch: int
    n: int              # tokens per sample of the padded batch this was built from
    has_cls: bool

    def to(self, device, non_blocking: bool = True) -> "TextLayout":
        if self.cu.device == torch.device(device):
            return self
        mv = lambda t: (t.pin_memory() if (t.device.type == "cpu" and torch.device(device).type == "cuda") else t).to(device, non_blocking=non_blocking)
        return TextLayout(mv(self.cu), mv(self.pos), mv(self.tok), self.R, self.max_len, self.batch, self.n, self.has_cls)

    def keys(self, vocab: int, npos: int):
        """(token key, position key) int64 [R] of the embedding gradient's segmented sums: the row's id / table position, and an id one past the
        table (dropped by xclip_scatter_add_sorted) on the CLS rows"""
        if not self.has_cls:
            return self.tok, self.pos.to(torch.int64)
        is_cls = self.pos == 0
        return (torch.where(is_cls, torch.full_like(self.tok, vocab), self.tok),
                torch.where(is_cls, torch.full_like(self.tok, npos), self.pos.to(torch.int64) - 1))


def cat_layouts(layouts) -> TextLayout:
    """the layout of several padded batches stacked along the batch dimension (the text batch and its augmented views, x_clip.py:629-639)"""
    layouts = list(layouts)
    first = layouts[0]
    if len(layouts) == 1:
        return first
    if any(l.n != first.n or l.has_cls != first.has_cls for l in layouts):
        raise ValueError("cat_layouts: layouts of batches with the same sequence length and CLS convention")
    layouts = [l.to(first.cu.device) for l in layouts]
    cus, off = [first.cu], first.R
    for l in layouts[1:]:
        cus.append(l.cu[1:] + off)
        off += l.R
    return TextLayout(torch.cat(cus), torch.cat([l.pos for l in layouts]), torch.cat([l.tok for l in layouts]), off,
                      max(l.max_len for l in layouts), sum(l.batch for l in layouts), first.n, first.has_cls)


def text_layout(tokens: Tensor, pad_id: int = 0, mask: Optional[Tensor] = None, has_cls: bool = True) -> TextLayout:
    """tokens int64 [B, n] (+ an explicit bool key mask [B, n] instead of `tokens != pad_id`) -> the packed layout.  The CLS row of every sample
    is always kept (`F.pad(mask, (1, 0), True)`, x_clip.py:334); a pad id in mid-sequence is simply a dropped row -- exactly what the dense
    masked attention computes.  The tensors live where `tokens` lives."""
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise TypeError("text_layout: int64 tokens [batch, n]")
    B, n = tokens.shape
    keep = (tokens != pad_id) if mask is None else mask.to(torch.bool)
    if tuple(keep.shape) != (B, n):
        raise ValueError(f"text_layout: mask {tuple(keep.shape)} does not match tokens {(B, n)}")
    if has_cls:
        keep = torch.cat([keep.new_ones(B, 1), keep], dim=1)
        tokens = torch.cat([tokens.new_zeros(B, 1), tokens], dim=1)
    elif B > 0 and not bool(keep.any(dim=1).all()):
        raise ValueError("text_layout: without a CLS row every sample needs at least one kept token")
    lens = keep.sum(dim=1, dtype=torch.int32)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=tokens.device)
    torch.cumsum(lens, 0, out=cu[1:])
    if B == 0:
        R = max_len = 0
    else:
        R, max_len = (int(v) for v in torch.stack([cu[-1], lens.max()]).tolist())      # (device tokens: the one read of this call)
    # kept (sample, position) pairs in row order.  On a device `nonzero` would read its result's size back (a second synchronisation):
    # a stable sort that moves the kept entries to the front, cut at the R already known
    if tokens.device.type == "cpu":
        flat = keep.reshape(-1).nonzero(as_tuple=False).reshape(-1)
    else:
        flat = torch.sort((~keep).reshape(-1).to(torch.uint8), stable=True).indices[:R]
    npos = keep.shape[1]
    pos = (flat % npos).to(torch.int32)
    tok = tokens.reshape(-1)[flat].contiguous()
    return TextLayout(cu.contiguous(), pos.contiguous(), tok, R, max_len, B, n, bool(has_cls))
