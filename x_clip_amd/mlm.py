"""Masked-language-model side loss of the text tower: the host mirror of reference x_clip/mlm.py (`MLM`, mlm.py:36-109).

The random token masking (mlm.py:70-94) is index bookkeeping on an int64 [b, n] tensor and stays in torch; everything that
touches activations runs in the gfx950 kernels: the shared TextTransformer encodes the masked sequence, ONLY the masked
positions are gathered and projected onto the vocabulary (xclip_gather_rows + xclip_gemm with the `to_logits` bias row --
F.cross_entropy(..., ignore_index=pad) ignores every other position, so their logits are never formed), and the softmax
cross-entropy and its gradient are xclip_cross_entropy_fwd / _bwd.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops

Tensor = torch.Tensor


class _MlmHeadFn(torch.autograd.Function):
    """emb [b, n + 1, D] (token 0 = CLS), flat row indices of the masked positions, their labels -> mean cross-entropy (fp32).
    emb [R, D] (the packed tower, CLIP.pack_text_tokens): the indices are packed rows (TextLayout.row_of) and the backward scatters into
    [R, D] -- no dense [b (n + 1), D] array on that path"""

    @staticmethod
    def forward(ctx, emb: Tensor, rows: Tensor, labels: Tensor, W: Tensor, bias: Tensor):
        emb = ops._c(emb)
        shape, D = tuple(emb.shape), emb.shape[-1]
        V = W.shape[0]
        dt, dev = emb.dtype, emb.device
        v = ops.vec(dt)
        Vp = (V + v - 1) // v * v                              # GEMM N: whole 16-byte chunks; the padding columns are ignored
        Wc, bc = ops._c(W), ops._c(bias)
        if Vp != V:
            Wp = torch.zeros(Vp, D, dtype=dt, device=dev)
            Wp[:V].copy_(Wc)
            bp = torch.zeros(Vp, dtype=dt, device=dev)
            bp[:V].copy_(bc)
        else:
            Wp, bp = Wc, bc
        nm = rows.numel()
        x = ops.gather_rows(emb.view(-1, D), rows)             # [nm, D]
        logits = ops.gemm(x, Wp, nm, Vp, D, bias=bp)           # to_logits                                   mlm.py:100
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        lse = ops.cross_entropy_fwd(logits, V, labels, acc)    # F.cross_entropy over the non-ignored rows   mlm.py:103-107
        ctx.save_for_backward(x, Wp, logits, lse, labels, rows)
        ctx.meta = (shape, D, V, Vp, dt, W.dtype, bias.dtype)
        return (acc / nm).reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        x, Wp, logits, lse, labels, rows = ctx.saved_tensors
        shape, D, V, Vp, dt, wdt, bdt = ctx.meta
        nm = rows.numel()
        dev = x.device
        g = dloss.detach().float().reshape(1).contiguous()
        dlog = ops.cross_entropy_bwd_(logits, V, labels, lse, g)            # [nm, Vp], in place
        demb = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dlog, Wp, nm, D, Vp, b_kmajor=True)
            table = torch.zeros(math.prod(shape[:-1]), D, dtype=torch.float32, device=dev)
            ops.rows_scatter_add(dx, rows, table, None)
            demb = ops.cast_from_f32(table, dt).view(shape)
        if ctx.needs_input_grad[3]:
            dW = ops.gemm(dlog, x, Vp, D, nm, a_kmajor=True, b_kmajor=True)[:V].to(wdt)
        if ctx.needs_input_grad[4]:
            acc = torch.zeros(Vp, dtype=torch.float32, device=dev)
            ops.rows_scatter_add(dlog, None, None, acc)
            db = acc[:V].to(bdt)
        return demb, None, None, dW, db


class _MlmFusedHeadFn(torch.autograd.Function):
    """_MlmHeadFn without the logits matrix (MLM.fused_head; csrc/kernels/vocabce.h): the same arguments, dense or packed.  The forward
    reduces z = x W^T + bias to lse and the label logit on the contrastive head's tile loop; the backward recomputes z and writes
    G = dloss / nm (softmax - onehot) once.  W is used as it is (no padded copy); nothing with nm * V elements is saved."""

    @staticmethod
    def forward(ctx, emb: Tensor, rows: Tensor, labels: Tensor, W: Tensor, bias: Tensor):
        emb = ops._c(emb)
        shape, D = tuple(emb.shape), emb.shape[-1]
        dt, dev = emb.dtype, emb.device
        nm = rows.numel()
        x = ops.gather_rows(emb.view(-1, D), rows)             # [nm, D]
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        lse = ops.vocab_ce_fwd(x, ops._c(W).to(dt), ops._c(bias).to(dt), labels, acc)    # to_logits + F.cross_entropy    mlm.py:100-107
        ctx.save_for_backward(x, W, bias, lse, labels, rows)
        ctx.meta = (shape, D, dt)
        return (acc / nm).reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        x, W, bias, lse, labels, rows = ctx.saved_tensors
        shape, D, dt = ctx.meta
        nm, V = rows.numel(), W.shape[0]
        dev = x.device
        g = dloss.detach().float().reshape(1).contiguous()
        Wc = ops._c(W).to(dt)
        G = ops.vocab_ce_bwd(x, Wc, ops._c(bias).to(dt), labels, lse, g)     # [nm, Vp], padding columns zero
        Vp = G.shape[1]
        demb = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(G, Wc if Vp == V else _pad_rows(Wc, Vp), nm, D, Vp, b_kmajor=True)
            table = torch.zeros(math.prod(shape[:-1]), D, dtype=torch.float32, device=dev)
            ops.rows_scatter_add(dx, rows, table, None)
            demb = ops.cast_from_f32(table, dt).view(shape)
        if ctx.needs_input_grad[3]:
            dW = ops.gemm(G, x, Vp, D, nm, a_kmajor=True, b_kmajor=True)[:V].to(W.dtype)
        if ctx.needs_input_grad[4]:
            acc = torch.zeros(Vp, dtype=torch.float32, device=dev)
            ops.colsum(G, acc)
            db = acc[:V].to(bias.dtype)
        return demb, None, None, dW, db


def _pad_rows(W: Tensor, Vp: int) -> Tensor:
    """W with zero rows up to Vp, for dx = G W over a vocabulary that is no whole number of 16-byte chunks: the GEMM's K runs over G's
    padding columns too (the one padded copy the fused head still makes, in the backward only; 10,000 and 49,408 need none)"""
    Wp = torch.zeros(Vp, W.shape[1], dtype=W.dtype, device=W.device)
    Wp[:W.shape[0]].copy_(W)
    return Wp


def _any_of(t: Tensor, ids) -> Tensor:
    hit = torch.zeros_like(t, dtype=torch.bool)
    for i in ids:
        hit |= t == i
    return hit


def _subset_with_prob(candidates: Tensor, prob: float) -> Tensor:
    """picks, per row, a random subset of the True positions of `candidates` [b, n]: the mlm.py:22-34 procedure (uniform scores,
    top-k over the row, slot k dropped when the running count of candidates over the first k + 1 sequence positions exceeds
    ceil(prob * #candidates)), one torch.rand((b, n)) draw"""
    b, n = candidates.shape
    dev = candidates.device
    k = math.ceil(prob * n)
    quota = (candidates.sum(dim=-1, keepdim=True) * prob).ceil()
    excess = (candidates.cumsum(dim=-1) > quota)[:, :k]
    scores = torch.rand((b, n), device=dev).masked_fill(~candidates, -1e9)
    picked = scores.topk(k, dim=-1).indices + 1                # slot 0 of the scatter target collects the dropped picks
    picked = picked.masked_fill(excess, 0)
    out = torch.zeros((b, n + 1), device=dev)
    out.scatter_(-1, picked, 1)
    return out[:, 1:].bool()


class MLM(nn.Module):
    """reference MLM (mlm.py:36-109): `transformer` is the CLIP text tower itself (shared parameters), `to_logits` the vocabulary
    head.  forward(seq int64 [b, n], mask=...) -> scalar loss."""

    def __init__(self, transformer, *, dim, num_tokens, mask_prob=0.15, replace_prob=0.9, random_token_prob=0., mask_token_id=2,
                 pad_token_id=0, mask_ignore_token_ids=[]):
        super().__init__()
        self.transformer = transformer
        self.mask_prob = mask_prob
        self.replace_prob = replace_prob
        self.num_tokens = num_tokens
        self.random_token_prob = random_token_prob
        self.pad_token_id = pad_token_id
        self.mask_token_id = mask_token_id
        self.mask_ignore_token_ids = set([*mask_ignore_token_ids, pad_token_id])
        self.to_logits = nn.Linear(dim, num_tokens)
        self.masked_override: Optional[Tuple[Tensor, Tensor]] = None   # parity harness: (masked_seq, labels) instead of the random draw
        self.fused_head = False                                        # the vocabulary head without its logits matrix (_MlmFusedHeadFn; CLIP.fuse_mlm_head)

    def draw(self, seq: Tensor) -> Tuple[Tensor, Tensor]:
        """(masked_seq, labels): mlm.py:70-94 -- special / pad tokens are never chosen; labels hold the original id at the chosen
        positions and the pad id elsewhere; a chosen position shows the [mask] id with probability replace_prob (or, with
        random_token_prob > 0, a random non-special token)"""
        chosen = _subset_with_prob(~_any_of(seq, self.mask_ignore_token_ids), self.mask_prob)
        labels = seq.masked_fill(~chosen, self.pad_token_id)
        masked = seq.clone().detach()
        if self.random_token_prob > 0:
            assert self.num_tokens is not None, 'num_tokens keyword must be supplied when instantiating MLM if using random token replacement'
            swap = torch.zeros_like(seq).float().uniform_(0, 1) < self.random_token_prob
            rnd = torch.randint(0, self.num_tokens, seq.shape, device=seq.device)
            swap &= ~_any_of(rnd, self.mask_ignore_token_ids)
            masked = torch.where(swap, rnd, masked)
            chosen = chosen & ~swap
        show_mask = torch.zeros_like(seq).float().uniform_(0, 1) < self.replace_prob
        masked = masked.masked_fill(chosen & show_mask, self.mask_token_id)
        return masked, labels

    def forward(self, seq, layout=None, **kwargs):
        """layout (not a reference keyword; packing.TextLayout of `seq` under its key mask, CLIP.pack_text_tokens): the tower runs on the kept rows
        of the MASKED ids (layout.with_tokens: a masked position is never a pad, so the kept pattern is the same) and returns them [R, dim];
        the head gathers the chosen positions by packed row (layout.row_of)"""
        masked, labels = self.masked_override if self.masked_override is not None else self.draw(seq)
        masked, labels = masked.to(seq.device), labels.to(seq.device)
        b, n = labels.shape
        chosen = labels != self.pad_token_id                                  # rows that F.cross_entropy does not ignore
        if layout is not None:
            layout = layout.to(seq.device)
            emb = self.transformer(masked, layout=layout.with_tokens(masked), rows=True, **kwargs)     # [R, dim]
            assert emb.dim() == 2 and emb.shape[0] == layout.R and layout.has_cls, 'the packed MLM pass returns the kept rows of a CLS-token encoder'
            row_of = layout.row_of()[:, 1:]                                   # logits[:, 1:]: skip the CLS position
            chosen = chosen & (row_of >= 0)                                   # (a position an explicit key mask drops has no row to read)
        else:
            emb = self.transformer(masked, **kwargs)                          # [b, n + 1, dim], CLS first      mlm.py:97
            assert emb.dim() == 3 and emb.shape[1] == n + 1, 'the MLM head expects the text encoder to prepend one CLS token'
        pos = chosen.nonzero()
        if pos.shape[0] == 0:
            return torch.full((), float('nan'), dtype=torch.float32, device=seq.device)   # mean over nothing, like the reference
        if layout is not None:
            rows = row_of[pos[:, 0], pos[:, 1]].contiguous()
        else:
            rows = (pos[:, 0] * (n + 1) + 1 + pos[:, 1]).to(torch.int32).contiguous()      # logits[:, 1:]: skip the CLS position
        picked = labels[pos[:, 0], pos[:, 1]].contiguous()
        head = _MlmFusedHeadFn if self.fused_head else _MlmHeadFn
        return head.apply(emb, rows, picked, self.to_logits.weight, self.to_logits.bias)
