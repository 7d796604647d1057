"""The packed form of a padded text batch: only the rows the key-padding mask keeps, laid end to end.

`CLIP.forward` hides padded keys from attention (`text_mask = text != text_pad_id`, reference x_clip.py:614) and, under the CLS head, reads
row 0 of every sample alone (x_clip.py:708).  A padded row is then never a key, everything else in the tower is row-wise, and nothing reads
its output: it can influence nothing and its gradient is exactly zero.  `text_layout` describes the batch without those rows; the text tower
(`CLIP.pack_text`) embeds, attends and back-propagates on the `R` kept rows only.

    layout = text_layout(tokens, pad_id=0)            # tokens on the CPU (a loader's pinned buffer): no device read
    loss = clip(text, image, return_loss=True, text_layout=layout)

The causal encoder (`CLIP.pack_text_causal`: no CLS row, a causal mask, read at the first EOS token) takes `text_layout(tokens, pad_id,
has_cls=False, eos_id=...)`: under the causal mask a row behind the first EOS is a key of no row that is read either, so the layout ends every
sample at that token and the pooled row is the sample's last, cu[s+1] - 1 (`TextLayout.ends_at_eos`).

The rotary encoder (`CLIP.pack_text_rotary`) takes the plain layout: `pos` is the position every kept row had in its padded sample, which is
what its q, k and v are rotated by (xclip_rotary_pos) -- a pad dropped in mid-sequence leaves the positions behind it unchanged.

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
    R: int              # rows of every packed array: `kept`, rounded up to a multiple of `row_multiple` when there is one
    max_len: int
    batch: int
    n: int              # tokens per sample of the padded batch this was built from
    has_cls: bool
    ends_at_eos: bool = False    # every sample's kept rows end at its first EOS token: the pooled row of sample s is cu[s+1] - 1
    kept: int = -1               # the rows a sample owns, cu[batch]; rows [kept, R) are filler (pos = 0, tok = 0, no owner).  -1: R
    row_multiple: Optional[int] = None      # what R was rounded up to (cat_layouts pads its result to the largest of its inputs')

    def __post_init__(self):
        if self.kept < 0:
            object.__setattr__(self, "kept", self.R)

    def to(self, device, non_blocking: bool = True) -> "TextLayout":
        if self.cu.device == torch.device(device):
            return self
        mv = lambda t: (t.pin_memory() if (t.device.type == "cpu" and torch.device(device).type == "cuda") else t).to(device, non_blocking=non_blocking)
        return TextLayout(mv(self.cu), mv(self.pos), mv(self.tok), self.R, self.max_len, self.batch, self.n, self.has_cls, self.ends_at_eos,
                          self.kept, self.row_multiple)

    def keys(self, vocab: int, npos: int):
        """(token key, position key) int64 [R] of the embedding gradient's segmented sums: the row's id / table position, and an id one past the
        table (dropped by xclip_scatter_add_sorted) on the CLS rows -- and on filler rows, whose pos is 0 too.  Without a CLS row (the causal
        encoder) filler rows carry the keys (0, 0): their gradient rows are exactly zero, so row 0 of both tables receives zeros"""
        if not self.has_cls:
            return self.tok, self.pos.to(torch.int64)
        is_cls = self.pos == 0
        return (torch.where(is_cls, torch.full_like(self.tok, vocab), self.tok),
                torch.where(is_cls, torch.full_like(self.tok, npos), self.pos.to(torch.int64) - 1))

    def _flat(self) -> Tensor:
        """int64 [kept]: sample * (n + has_cls) + pos of every owned row -- its place in the dense [B, n + has_cls] order.  Index arithmetic on
        cu and pos alone: nothing is read back from the device"""
        rows = torch.arange(self.kept, dtype=self.cu.dtype, device=self.cu.device)
        sample = torch.searchsorted(self.cu[1:], rows, right=True)          # the largest s with cu[s] <= r
        return sample * (self.n + int(self.has_cls)) + self.pos[:self.kept].to(torch.int64)

    def with_tokens(self, tokens: Tensor) -> "TextLayout":
        """the same layout with `tok` gathered from another int64 [B, n] id tensor whose kept pattern is this one's (the MLM pass: the masked ids
        sit exactly where the original ones do, a masked position is never a pad).  cu, pos and every count are shared; no device read"""
        if tokens.dtype != torch.int64 or tuple(tokens.shape) != (self.batch, self.n):
            raise TypeError(f"with_tokens: int64 tokens [{self.batch}, {self.n}], got {tokens.dtype} {tuple(tokens.shape)}")
        tokens = tokens.to(self.cu.device)
        if self.has_cls:
            tokens = torch.cat([tokens.new_zeros(self.batch, 1), tokens], dim=1)
        tok = tokens.reshape(-1)[self._flat()]
        if self.R > self.kept:
            tok = torch.cat([tok, tok.new_zeros(self.R - self.kept)])
        return TextLayout(self.cu, self.pos, tok.contiguous(), self.R, self.max_len, self.batch, self.n, self.has_cls, self.ends_at_eos,
                          self.kept, self.row_multiple)

    def row_of(self) -> Tensor:
        """int32 [B, n + has_cls]: the packed row of every dense position, -1 where the position is dropped.  No device read"""
        npos = self.n + int(self.has_cls)
        out = torch.full((self.batch * npos,), -1, dtype=torch.int32, device=self.cu.device)
        out[self._flat()] = torch.arange(self.kept, dtype=torch.int32, device=self.cu.device)
        return out.view(self.batch, npos)


def cat_layouts(layouts) -> TextLayout:
    """the layout of several padded batches stacked along the batch dimension (the text batch and its augmented views, x_clip.py:629-639)"""
    layouts = list(layouts)
    first = layouts[0]
    if len(layouts) == 1:
        return first
    if any(l.n != first.n or l.has_cls != first.has_cls or l.ends_at_eos != first.ends_at_eos for l in layouts):
        raise ValueError("cat_layouts: layouts of batches with the same sequence length, CLS convention and ends_at_eos")
    layouts = [l.to(first.cu.device) for l in layouts]
    # the KEPT rows of every input end to end (filler never sits between two samples), padded once behind the last sample
    cus, off = [first.cu], first.kept
    for l in layouts[1:]:
        cus.append(l.cu[1:] + off)
        off += l.kept
    multiple = max((l.row_multiple for l in layouts if l.row_multiple is not None), default=None)
    R = _round_up(off, multiple)
    pos, tok = [l.pos[:l.kept] for l in layouts], [l.tok[:l.kept] for l in layouts]
    if R > off:
        pos.append(first.pos.new_zeros(R - off))
        tok.append(first.tok.new_zeros(R - off))
    return TextLayout(torch.cat(cus), torch.cat(pos), torch.cat(tok), R, max(l.max_len for l in layouts), sum(l.batch for l in layouts),
                      first.n, first.has_cls, first.ends_at_eos, off, multiple)


def _check_row_multiple(row_multiple, who: str) -> Optional[int]:
    """None, or a positive int (bool is not one): anything else is a ValueError"""
    if row_multiple is None:
        return None
    if isinstance(row_multiple, bool) or not isinstance(row_multiple, int) or row_multiple < 1:
        raise ValueError(f"{who}: row_multiple is None or a positive int (256 recommended), not {row_multiple!r}")
    return row_multiple


def _round_up(rows: int, multiple: Optional[int]) -> int:
    return rows if multiple is None else -(-rows // multiple) * multiple


def text_layout(tokens: Tensor, pad_id: int = 0, mask: Optional[Tensor] = None, has_cls: bool = True, eos_id: Optional[int] = None,
                row_multiple: Optional[int] = None) -> TextLayout:
    """tokens int64 [B, n] (+ an explicit bool key mask [B, n] instead of `tokens != pad_id`) -> the packed layout.  The CLS row of every sample
    is always kept (`F.pad(mask, (1, 0), True)`, x_clip.py:334); a pad id in mid-sequence is simply a dropped row -- exactly what the dense
    masked attention computes.  The tensors live where `tokens` lives.

    `eos_id` (the causal encoder, which has no CLS row and is read at its first EOS token, `eos_to_front` x_clip.py:675): a row is kept iff
    the mask keeps it AND it lies at or before the sample's FIRST `eos_id` token.  Under the causal mask a row behind that token is a key of
    no row that is read, so it is as dead as a padded one; and every sample's rows now END at its EOS (`ends_at_eos`), so the pooled row is
    cu[s+1] - 1.  ValueError for a sample without the token (the assertion of `functional.eos_to_front`) or whose mask hides its first one.

    `row_multiple` (a positive int, 256 recommended; default None = off): the row count `R` of the packed arrays is the kept row count rounded
    up to this multiple, so that the tower's GEMMs -- every forward and input-gradient product has M = R, every weight gradient contracts over
    K = R -- get a shape their fast kernels take (256 = the 256 x 256 tile's M; it also satisfies M % 8 and K % 64).  The surplus rows
    [kept, R) are FILLER: pos = 0, tok = 0 (valid table indices in every encoder form), owned by no sample (`cu` is unchanged, cu[B] = kept).
    The attention kernels write zeros there; everything else is row-wise, so filler activations are finite and filler gradients exactly 0,
    and every weight gradient's filler term is finite x 0.  `R` is computed on the host from the one read this call makes anyway."""
    row_multiple = _check_row_multiple(row_multiple, "text_layout")
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise TypeError("text_layout: int64 tokens [batch, n]")
    B, n = tokens.shape
    keep = (tokens != pad_id) if mask is None else mask.to(torch.bool)
    if tuple(keep.shape) != (B, n):
        raise ValueError(f"text_layout: mask {tuple(keep.shape)} does not match tokens {(B, n)}")
    eos_ok = None
    if eos_id is not None:
        if has_cls:
            raise ValueError("text_layout: eos_id describes the causal encoder, which has no CLS row (has_cls=False)")
        is_eos = tokens == eos_id
        upto = is_eos.to(torch.int32).cumsum(dim=1)
        first = is_eos & (upto == 1)                            # the first EOS of each sample
        keep = keep & ((upto == 0) | first)
        eos_ok = (first & keep).any(dim=1).all() if B > 0 else None     # every sample has a first EOS and the mask keeps it
    elif has_cls:
        keep = torch.cat([keep.new_ones(B, 1), keep], dim=1)
        tokens = torch.cat([tokens.new_zeros(B, 1), tokens], dim=1)
    elif B > 0 and not bool(keep.any(dim=1).all()):
        raise ValueError("text_layout: without a CLS row every sample needs at least one kept token")
    lens = keep.sum(dim=1, dtype=torch.int32)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=tokens.device)
    torch.cumsum(lens, 0, out=cu[1:])
    if B == 0:
        kept = max_len = 0
    elif eos_ok is None:
        kept, max_len = (int(v) for v in torch.stack([cu[-1], lens.max()]).tolist())      # (device tokens: the one read of this call)
    else:                                                       # (the EOS check rides in the same read)
        kept, max_len, ok = (int(v) for v in torch.stack([cu[-1], lens.max(), eos_ok.to(torch.int32)]).tolist())
        if not ok:
            raise ValueError(f"text_layout: every sample needs an eos_id ({eos_id}) token that the mask keeps "
                             "(a sample has none, or its first one is masked / a pad)")
    # kept (sample, position) pairs in row order.  On a device `nonzero` would read its result's size back (a second synchronisation):
    # a stable sort that moves the kept entries to the front, cut at the row count already known
    if tokens.device.type == "cpu":
        flat = keep.reshape(-1).nonzero(as_tuple=False).reshape(-1)
    else:
        flat = torch.sort((~keep).reshape(-1).to(torch.uint8), stable=True).indices[:kept]
    npos = keep.shape[1]
    pos = (flat % npos).to(torch.int32)
    tok = tokens.reshape(-1)[flat]
    R = _round_up(kept, row_multiple)
    if R > kept:                                                # filler rows behind the last sample
        pos = torch.cat([pos, pos.new_zeros(R - kept)])
        tok = torch.cat([tok, tok.new_zeros(R - kept)])
    return TextLayout(cu.contiguous(), pos.contiguous(), tok.contiguous(), R, max_len, B, n, bool(has_cls), eos_id is not None, kept, row_multiple)
