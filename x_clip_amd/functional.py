"""Autograd boundary of the MI355X path: every differentiable piece of `CLIP.forward` (reference x_clip/x_clip.py:597-875)
is one `torch.autograd.Function` whose forward AND backward are explicit sequences of C-ABI kernel launches
(x_clip_amd.ops -> libxclip_hip.so).  torch provides tensors, streams and the autograd graph between these nodes;
no arithmetic of the hot path is left to ATen and there is no CPU fallback.

Nodes
  text_encode     TextTransformer.forward   (x_clip.py:317-338)  tokens -> [b, n+1, D]
  vision_encode   VisionTransformer.forward (x_clip.py:372-390)  image  -> [b, 1+n_keep, D]
  transformer     Transformer.forward       (x_clip.py:274-291)  the block stack on its own
  linear / l2norm / select_row              the latent projections, F.normalize, enc[:, 0]  (x_clip.py:708-715)

The block stack keeps the residual stream in the model dtype and saves, per layer, exactly the tensors its backward
reads (pre-norm outputs, packed QKV, attention output + log-sum-exp, FF1 output, LayerNorm statistics); with
`checkpoint=True` (reference `checkpoint_during_training`, x_clip.py:69-79,280-286) it keeps only the two residual
inputs of a layer and re-runs that layer's forward inside the backward.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import ops

Tensor = torch.Tensor

# Weight-gradient GEMMs are off the critical path of the backward (only the optimiser consumes them), so they are issued on a
# side HIP stream -- one per (device, issuing stream) -- where they run beside the HBM-bound LayerNorm / attention backward
# kernels of the main chain.  Their operands (a layer's activations and gradients, gigabytes each) are NOT handed to the
# caching allocator with record_stream(): its event-deferred frees come back at timing-dependent moments, the pool fragments,
# and the step keeps calling hipMalloc (measured: ~100 device mallocs in 8 steps, 44 -> 140 GB reserved, occasional 3x slower
# steps).  Instead the operands are kept referenced until the main stream has been ordered behind the side stream's work on
# them, one layer late: `layer_done()` records an event after a layer's weight gradients and makes the main stream wait for the
# PREVIOUS layer's event before dropping that layer's operands.  Same overlap, deterministic allocation pattern.
OVERLAP_WGRAD = True
_wgrad_streams = {}

# Optional destination for parameter gradients (x_clip_amd.distributed.GradSync registers itself): an object whose
# `claim(weight, shape, dtype)` returns the buffer the gradient of the parameter stored at `weight` should be written into -- a slice of
# a persistent flat all-reduce bucket -- or None.  The backward then produces that gradient in place instead of into a fresh tensor.
# Several sinks may be registered (one GradSync per model): each is asked in turn, the first that knows the weight answers.
_grad_sinks: list = []


def add_grad_sink(sink) -> None:
    if sink not in _grad_sinks:
        _grad_sinks.append(sink)


def remove_grad_sink(sink) -> None:
    if sink in _grad_sinks:
        _grad_sinks.remove(sink)


def grad_sinks():
    return tuple(_grad_sinks)


def _grad_out(weight: Optional[Tensor], shape, dtype, device) -> Tensor:
    if weight is not None:
        for sink in _grad_sinks:
            out = sink.claim(weight, shape, dtype)
            if out is not None:
                return out
    return torch.empty(*shape, dtype=dtype, device=device)


class _SideGemm:
    def __init__(self, device):
        self.main = self.side = None
        if OVERLAP_WGRAD and device.type == "cuda":
            self.main = torch.cuda.current_stream(device)
            key = (device, self.main.cuda_stream)
            self.side = _wgrad_streams.get(key)
            if self.side is None:
                self.side = _wgrad_streams[key] = torch.cuda.Stream(device=device)
        self.keep = []                                           # operands of the current layer's side-stream GEMMs
        self.pending = []                                        # [(event, operands)] of finished layers, oldest first

    def wgrad(self, dy: Tensor, x: Tensor, N1: int, N2: int, M: int, w: Optional[Tensor] = None) -> Tensor:
        """dW [N1, N2] = dy^T x (contraction over the M token rows), issued on the side stream; `w`: the weight it is the gradient of"""
        return self.wgrad_into(dy, x, N1, N2, M, _grad_out(w, (N1, N2), dy.dtype, dy.device))   # main-stream memory (or a bucket slice): consumed after join()

    def wgrad_into(self, dy: Tensor, x: Tensor, N1: int, N2: int, M: int, out: Tensor) -> Tensor:
        """the same product written into a given [N1, N2] view (a row block of a weight gradient assembled from two products)"""
        if self.side is None:
            return ops.gemm(dy, x, N1, N2, M, a_kmajor=True, b_kmajor=True, out=out)
        self.side.wait_stream(self.main)                     # dy was just produced on the main stream
        with torch.cuda.stream(self.side):
            ops.gemm(dy, x, N1, N2, M, a_kmajor=True, b_kmajor=True, out=out)
        self.keep.append((dy, x))
        return out

    def layer_done(self):
        if self.side is None:
            return
        ev = torch.cuda.Event()
        ev.record(self.side)
        self.pending.append((ev, self.keep))
        self.keep = []
        while len(self.pending) > 1:                             # the side stream may lag one layer behind
            ev0, _ = self.pending.pop(0)
            self.main.wait_event(ev0)                            # everything the main stream does from here on is behind those GEMMs

    def join(self):
        if self.side is not None:
            self.main.wait_stream(self.side)
        self.keep, self.pending = [], []


def _draw_seed() -> int:
    """a fresh 62-bit seed from torch's default CPU generator (host side: no device sync)"""
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())


# One layer's parameters in their flat order (clip.Transformer.stack_params): attn_norm.g, to_qkv.w, to_out.0.w, to_out.1.g, ff_norm.g, net.0.w, net.2.g, net.4.w
LayerWeights = NamedTuple("LayerWeights", [(f, Tensor) for f in "g_attn w_qkv w_out g_out g_ff w_ff1 g_inner w_ff2".split()])
LAYER_PARAMS = len(LayerWeights._fields)
IS_GAIN = tuple(f.startswith("g_") for f in LayerWeights._fields)       # LayerNorm gains (_GainGrads); the others are GEMM weights (_SideGemm.wgrad)
# What a layer's backward reads (m*, r*: LayerNorm statistics; qkv / o: the packed rotated qkv and the attention output, or the one-query
# pooled layer's (q, kv) and pooled output; p: to_out.0's output; x1: the stream between the blocks; a: what net.4 saw)
LayerTape = NamedTuple("LayerTape", [(f, object) for f in "x h m1 r1 qkv o lse p m2 r2 x1 h2 m3 r3 u a m4 r4".split()])


def layer_weights(flat: Sequence, l: int):
    """(layer l's entries by name, their offset) of the flat params norm_in.g, depth x LayerWeights, norm_out.g -- or of a list aligned with them"""
    base = 1 + LAYER_PARAMS * l
    return LayerWeights._make(flat[base: base + LAYER_PARAMS]), base


def head_slot(dim_head: int) -> int:        # features per head slot in the packed qkv / attention output: 64, or 128 for heads wider than 64
    return 64 if dim_head <= 64 else 128


@dataclass(frozen=True)
class StackSpec:
    depth: int
    heads: int
    dim_head: int = 64
    checkpoint: bool = False
    rotary: Optional[Tensor] = None         # rotary embedding on q, k, v: the inv_freq buffer (min(dim_head, 32) / 2 fp32), x_clip.py:155-176,221-223,311
    causal: bool = False                    # causal attention (the autoregressive text encoder), x_clip.py:231-234
    attn_dropout: float = 0.0               # dropout on the softmax probabilities (x_clip.py:212,241); 0 outside training
    ff_dropout: float = 0.0                 # dropout between the inner LayerNorm and the second Linear (x_clip.py:193-194)

    def __post_init__(self):
        # the attention kernels hold head slots of 64 features (the head-resident kernels) or 128 (wide heads: two 64-wide halves
        # through the tiled kernels).  A head narrower than its slot runs with its extra q / k / v columns zero
        # (clip.Transformer.stack_params pads to_qkv / to_out with zero rows / columns: q.k and the softmax are unchanged, the
        # padded output columns are zero and meet zero weights); only the scale dim_head^-0.5 is the head's own.
        if not 1 <= self.dim_head <= 128:
            raise NotImplementedError("x_clip_amd attention kernels hold heads of up to 128 dimensions (the reference default is 64)")
        if not (0.0 <= self.attn_dropout < 1.0 and 0.0 <= self.ff_dropout < 1.0):
            raise ValueError("dropout probabilities must lie in [0, 1)")

    @property
    def head_slot(self) -> int:
        return head_slot(self.dim_head)

    @property
    def inner(self) -> int:                 # width of the packed attention output
        return self.heads * self.head_slot

    @property
    def scale(self) -> float:
        return self.dim_head ** -0.5


class _GainGrads:
    """All LayerNorm gain gradients of one backward share a flat fp32 accumulator (the LN backward kernels add into it with atomics) and are
    converted to the parameter dtype by one cast launch at the end.  `views`: the accumulators, aligned with the parameter list (None elsewhere)"""

    def __init__(self, params: Sequence[Tensor], is_gain: Sequence[bool]):
        self.at = [i for i, g in enumerate(is_gain) if g]
        self.sizes = [params[i].numel() for i in self.at]
        self.dtype = params[0].dtype
        self.flat = torch.zeros(sum(self.sizes), dtype=torch.float32, device=params[0].device)
        self.views = self._put(self.flat, [None] * len(params))

    def _put(self, flat: Tensor, out: list) -> list:
        for i, v in zip(self.at, flat.split(self.sizes)):
            out[i] = v
        return out

    def finish(self, grads: list) -> None:                      # the finished gain gradients into their places in `grads`
        self._put(self.flat if self.dtype == torch.float32 else ops.cast_from_f32(self.flat, self.dtype), grads)


# ---- one pre-norm residual block pair (x_clip.py:285-289): the attention block and the feed-forward block -----------------------------
# c: what a pass shares; seed: the layer's dropout seed (+ 1: the feed-forward block's); need / dg: the layer's `need` flags / gain accumulators
# layout (packing.TextLayout, or None): the rows are the kept rows of a padded batch laid end to end -- M = layout.R instead of B n; the
# attention takes the samples' row ranges from layout.cu (attention_varlen.h), everything row-wise runs on the R rows unchanged.
# Filler rows (layout.kept <= r < layout.R, text_layout(row_multiple=)) are ordinary rows to everything but the attention, which writes
# zeros there.  The invariant that keeps them out of every result: their activations are FINITE (the embedding of (tok 0, pos 0), then row-wise
# operations on finite input, attention output 0) and their gradients EXACTLY 0 (dy enters at pooled rows only, dqkv / dkv filler is 0, and the
# row-wise backwards map a zero row to a zero row) -- so the filler term of every weight gradient is finite x 0.
# A packed pass WITH a mask (stack_forward `dense_attention`): the mask is the dense key mask [batch, layout.n + 1] of the layout, and the
# attention alone runs through the DENSE kernels on the rows put back by position (_attn_dense_on_packed) -- the route of the heads that read
# token rows wherever the varlen entry points would take their plain form, whose summation order is not the dense kernels'.
_Pass = NamedTuple("_Pass", [("spec", StackSpec), ("B", int), ("n", int), ("mask", Optional[Tensor]), ("layout", object)])
_Pass.__new__.__defaults__ = (None,)
VARLEN_RESIDENT_MAX_LEN = 288          # csrc/kernels/attention3.h A3_MAX_N, as csrc/xclip_attn.hip attn_varlen_resident reads it


def varlen_is_head_resident(dtype, head_slot: int, max_len: int) -> bool:
    """does the varlen attention of a packed pass run attention3.h's head-resident bodies -- the dense bf16 kernels' own, bit for bit on the
    kept rows under a key mask -- or its plain form (csrc/xclip_attn.hip attn_varlen_resident)?"""
    return dtype == torch.bfloat16 and head_slot == 64 and max_len <= VARLEN_RESIDENT_MAX_LEN


def _attn_dense_on_packed(c: _Pass, qkv: Tensor, o: Optional[Tensor] = None, do: Optional[Tensor] = None, lse: Optional[Tensor] = None):
    """the dense masked attention on packed rows: qkv [R, 3 inner] (and, backward, o / do [R, inner]) go back to their (sample, position) places
    (xclip_unpack_rows: +0 where the layout keeps no row -- a key the mask hides, whose value is never read into a sum, and a query nobody
    reads), the dense kernels run under the layout's key mask, and the result's kept rows are packed again (xclip_pack_rows: +0 on filler rows,
    what the varlen kernels write there).  The dense arrays are transients of this call; the tape keeps packed rows and the dense lse.
    forward -> (o [R, inner], lse [batch, heads, n + 1]); backward -> dqkv [R, 3 inner]"""
    spec, lay = c.spec, c.layout
    n1 = lay.n + 1
    qd = ops.unpack_rows(qkv, lay.cu, lay.pos, 0, n1)
    if do is None:
        od, lse = ops.attention_fwd(qd, c.mask, spec.heads, spec.scale, False, spec.head_slot)
        return ops.pack_rows(od, lay.cu, lay.pos, 0), lse
    dqd = ops.attention_bwd(qd, c.mask, ops.unpack_rows(o, lay.cu, lay.pos, 0, n1), ops.unpack_rows(do, lay.cu, lay.pos, 0, n1), lse,
                            spec.heads, spec.scale, False, spec.head_slot)
    return ops.pack_rows(dqd, lay.cu, lay.pos, 0)


def _attn_forward(h: Tensor, W: LayerWeights, c: _Pass, seed: int):
    """the dense attention behind the PreNorm output h [B n, D] -> (packed qkv as the kernels read it, attention output, log-sum-exp)"""
    M, D = h.shape
    spec, inner = c.spec, c.spec.inner
    qkv = ops.gemm(h, W.w_qkv, M, 3 * inner, D)                                        # to_qkv            :216
    if c.layout is not None:                                   # samples of different lengths, end to end: no mask, no dropout (text_encode_packed)
        if spec.rotary is not None:                            # q, k, v rotated by the position the row had in its sample, not by its packed index  :221-223
            ops.rotary_pos_(qkv, c.layout.pos, spec.rotary, head_dim=spec.head_slot)
        if c.mask is not None:                                 # (the dense kernels on the rows put back by position: see _Pass)
            o, lse = _attn_dense_on_packed(c, qkv)
            return qkv, o, lse
        fwd = ops.attention_varlen_causal_fwd if spec.causal else ops.attention_varlen_fwd      # (causal: key j <= query i by packed row)
        o, lse = fwd(qkv, c.layout.cu, c.layout.max_len, spec.heads, spec.scale, spec.head_slot)
        return qkv, o, lse
    if spec.rotary is not None:
        ops.rotary_(qkv, c.n, spec.rotary, head_dim=spec.head_slot)                    # q, k, v rotated   :221-223
    o, lse = ops.attention_fwd(qkv.view(c.B, c.n, 3 * inner), c.mask, spec.heads, spec.scale, spec.causal, spec.head_slot, spec.attn_dropout, seed)   # :217-244
    return qkv, o, lse


def _ffn_forward(p: Tensor, x: Tensor, W: LayerWeights, c: _Pass, seed: int):
    """to_out.0's output p and the residual stream x, on whatever rows they hold -> (the layer output, the tape's fields from m2 on)"""
    M, D = x.shape
    x1, m2, r2, h2, m3, r3 = ops.layernorm_chain_fwd(p, W.g_out, x, W.g_ff)            # to_out.1 + skip :245,288 and PreNorm :126, one pass
    u = ops.gemm(h2, W.w_ff1, M, W.w_ff1.shape[0], D)                                  # net.0             :191
    a, m4, r4 = ops.layernorm_fwd(u, W.g_inner, geglu=True)                            # GEGLU + net.2     :192-193
    if c.spec.ff_dropout > 0.0:
        ops.dropout(a, c.spec.ff_dropout, seed + 1, out=a)                             # net.3 Dropout     :194 (in place: `a` is only read by net.4)
    x2 = ops.gemm(a, W.w_ff2, M, D, a.shape[1], residual=x1)                           # net.4 + skip      :195,289
    return x2, dict(m2=m2, r2=r2, x1=x1, h2=h2, m3=m3, r3=r3, u=u, a=a, m4=m4, r4=r4)


def _layer_forward(x: Tensor, W: LayerWeights, c: _Pass, seed: int):
    M, D = x.shape
    h, m1, r1 = ops.layernorm_fwd(x, W.g_attn)                                         # PreNorm           :126
    qkv, o, lse = _attn_forward(h, W, c, seed)
    p = ops.gemm(o.view(M, c.spec.inner), W.w_out, M, D, c.spec.inner)                 # to_out.0          :245
    x2, ff = _ffn_forward(p, x, W, c, seed)
    return x2, LayerTape(x=x, h=h, m1=m1, r1=r1, qkv=qkv, o=o, lse=lse, p=p, **ff)


def _ffn_backward(dx2: Tensor, t: LayerTape, W: LayerWeights, need: LayerWeights, dg: LayerWeights, c: _Pass, sg: _SideGemm, seed: int, x2=None, rowc=None):
    """dx2: gradient w.r.t. the layer output, on the rows the feed-forward block ran on -> (gradient w.r.t. x1 through the skip and the
    PreNorm, gradient w.r.t. to_out.0's output p, dWff1, dWff2).  x2 / rowc: see _layer_backward; without them the two-kernel form"""
    M, D = dx2.shape
    F2, Fh, p_ff = W.w_ff1.shape[0], W.w_ff1.shape[0] // 2, c.spec.ff_dropout
    if (x2 is not None or rowc is not None) and p_ff == 0.0 and ops.ffn_dgrad_geglu_ok(M, Fh, D, dx2.dtype):
        # net.4's input gradient and net.2's (GEGLU-LayerNorm) backward in one kernel: d a never reaches memory (csrc/kernels/gemm9.h)
        du, _ = ops.ffn_dgrad_geglu(dx2, W.w_ff2, t.u, W.g_inner, t.m4, t.r4, x2, t.x1, dg=dg.g_inner, rowc=rowc)
        d_ff2 = sg.wgrad(dx2, t.a, D, Fh, M, W.w_ff2) if need.w_ff2 else None
    else:
        da = ops.gemm(dx2, W.w_ff2, M, Fh, D, b_kmajor=True)
        d_ff2 = sg.wgrad(dx2, t.a, D, Fh, M, W.w_ff2) if need.w_ff2 else None     # (`a` is the dropped activation: what net.4 saw)
        if p_ff > 0.0:
            ops.dropout(da, p_ff, seed + 1, out=da)                                         # the same mask on the gradient
        du, _ = ops.layernorm_bwd(da, t.u, W.g_inner, t.m4, t.r4, geglu=True, dg=dg.g_inner)
        del da
    dh2 = ops.gemm(du, W.w_ff1, M, D, F2, b_kmajor=True)
    d_ff1 = sg.wgrad(du, t.h2, F2, D, M, W.w_ff1) if need.w_ff1 else None
    del du
    # PreNorm backward + skip, then to_out's LayerNorm backward (the attention block), one pass over the rows
    dx1, dp = ops.layernorm_chain_bwd(dh2, t.x1, W.g_ff, t.m3, t.r3, dx2, t.p, W.g_out, t.m2, t.r2, dg.g_ff, dg.g_out)
    del dh2
    return dx1, dp, d_ff1, d_ff2


def _attn_backward(do: Tensor, t: LayerTape, c: _Pass, seed: int) -> Tensor:
    """the dense attention: gradient w.r.t. its output [M, inner] -> gradient w.r.t. the packed rotated qkv [M, 3 inner]"""
    spec, B, n, inner = c.spec, c.B, c.n, c.spec.inner
    if c.layout is not None and c.mask is not None:
        return _attn_dense_on_packed(c, t.qkv, t.o, do, t.lse)
    if c.layout is not None:
        bwd = ops.attention_varlen_causal_bwd if spec.causal else ops.attention_varlen_bwd
        return bwd(t.qkv, c.layout.cu, c.layout.max_len, t.o, do, t.lse, spec.heads, spec.scale, spec.head_slot)
    dqkv = ops.attention_bwd(t.qkv.view(B, n, 3 * inner), c.mask, t.o, do.view(B, n, inner), t.lse, spec.heads, spec.scale, spec.causal, spec.head_slot, spec.attn_dropout, seed)
    return dqkv.view(B * n, 3 * inner)


def _qkv_backward(dqkv: Tensor, t: LayerTape, W: LayerWeights, need: LayerWeights, c: _Pass, sg: _SideGemm):
    """gradient w.r.t. the packed rotated qkv (rotated back in place) -> (gradient w.r.t. the PreNorm output h, dWqkv)"""
    (M, D), N = t.h.shape, dqkv.shape[1]
    if c.spec.rotary is not None and c.layout is not None:
        ops.rotary_pos_(dqkv, c.layout.pos, c.spec.rotary, inverse=True, head_dim=c.spec.head_slot)
    elif c.spec.rotary is not None:
        ops.rotary_(dqkv, c.n, c.spec.rotary, inverse=True, head_dim=c.spec.head_slot)      # the saved qkv is the rotated one; R^T maps its gradient back
    dh = ops.gemm(dqkv, W.w_qkv, M, D, N, b_kmajor=True)
    return dh, sg.wgrad(dqkv, t.h, N, D, M, W.w_qkv) if need.w_qkv else None


def _layer_backward(dx2: Tensor, t: LayerTape, W: LayerWeights, need: LayerWeights, dg: LayerWeights, c: _Pass, sg: _SideGemm, seed: int,
                    x2: Tensor, stats=(None, None)):
    """dx2: gradient w.r.t. the layer output [M, D] -> (gradient w.r.t. the layer input, the weight gradients by field name).
    x2 = the layer's output (the next layer's saved input): with it the feed-forward block's first two backward steps run as one kernel; stats = (rowc, below): that kernel's
    per-row constants when the pass that produced dx2 already wrote them (ops.layernorm_bwd(ffn_stats=...)), and ops.ffn_stats_request for the layer BELOW, whose dx2 this one writes"""
    M, D = dx2.shape
    rowc, below = stats
    dx1, dp, d_ff1, d_ff2 = _ffn_backward(dx2, t, W, need, dg, c, sg, seed, x2, rowc)
    do = ops.gemm(dp, W.w_out, M, c.spec.inner, D, b_kmajor=True)
    d_out = sg.wgrad(dp, t.o.view(M, c.spec.inner), D, c.spec.inner, M, W.w_out) if need.w_out else None
    del dp
    dqkv = _attn_backward(do, t, c, seed)
    del do
    dh, d_qkv = _qkv_backward(dqkv, t, W, need, c, sg)
    del dqkv
    dx, _ = ops.layernorm_bwd(dh, t.x, W.g_attn, t.m1, t.r1, dres=dx1, dg=dg.g_attn, ffn_stats=below)
    return dx, dict(w_qkv=d_qkv, w_out=d_out, w_ff1=d_ff1, w_ff2=d_ff2)


# ---- the LAST layer when only one token row per sample leaves the stack (the CLS row: x_clip.py:708 `enc_text[:, 0]`) -----------------
# Everything behind the attention is row-wise (to_out + its LayerNorm + skip, the feed-forward block, norm_out), so the rows nobody reads
# are dead in the forward, and in the backward their gradient is exactly zero: the loss reaches the layer through the pooled row alone.
# The pooled variants run that part on B rows instead of B n (the last text layer of the default CLIP: 1,024 rows instead of 263,168 --
# four large GEMMs and five row-kernel passes in the forward, five GEMMs and their weight gradients in the backward); the attention itself,
# to_qkv and the first LayerNorm stay dense (every key / value row feeds the pooled query).  The same function of the same inputs: exact in
# fp32; in bf16 the pooled rows' gradients are rounded at other points than in the dense layer (the LayerNorm backward's dx and the skip
# gradient are added as two bf16 tensors where the dense kernel fuses them in fp32; dh is the sum of two rounded products where the dense layer
# takes one contraction over 3 inner), so toggling `prune_unused_rows` moves results by bf16 ulps -- the tests hold pooled against dense to the
# bars of the dense layer against the oracle, not to bit equality.  No dropout here (can_pool): the shared blocks get the seed 0.
def _pool_view(t2d: Tensor, B: int, n: int, row: int) -> Tensor:
    """rows b n + row of a contiguous [B n, W] tensor as a [B, W] view (row stride n W)"""
    Wd = t2d.shape[1]
    return t2d.view(B, n * Wd)[:, row * Wd:(row + 1) * Wd]


def _add_to_pooled_rows(full: Tensor, add: Tensor, B: int, n: int, row: int) -> None:
    """full[b n + row] += add[b]: the pooled rows copied out, added, copied back"""
    rows = _pool_view(full, B, n, row)
    t = torch.empty(B, full.shape[1], dtype=full.dtype, device=full.device)
    ops.copy_rows(rows, t)
    ops.copy_rows(ops.add_rows(t, add), rows)


def _layer_forward_pooled(x: Tensor, W: LayerWeights, c: _Pass, row: int):
    if c.layout is not None:
        return _layer_forward_pooled_packed(x, W, c)
    spec, B, n, inner = c.spec, c.B, c.n, c.spec.inner
    M, D = x.shape
    h, m1, r1 = ops.layernorm_fwd(x, W.g_attn)
    xc = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ops.copy_rows(_pool_view(x, B, n, row), xc)                                        # the skip connection's pooled rows
    if spec.rotary is None or row == 0:
        # one query per head: to_qkv's first third on the pooled rows, the other two on every row, attention_pool.h (causal: the pooled row sees the keys
        # up to itself).  Rotary: keys and values are rotated at their positions; the query at position 0 by the angle 0 -- the identity (x_clip.py:155-176)
        q = ops.gemm(_pool_view(h, B, n, row), W.w_qkv[:inner], B, inner, D)
        kv = ops.gemm(h, W.w_qkv[inner:], M, 2 * inner, D)
        if spec.rotary is not None:
            ops.rotary_(kv, n, spec.rotary, head_dim=spec.head_slot)
        oc, lse = ops.attention_pool_fwd(q, kv.view(B, n, 2 * inner), c.mask, spec.heads, spec.scale, spec.head_slot, row + 1 if spec.causal else None)
        qkv, o = (q, kv), oc                                                           # (the tape's qkv / o fields: the pooled forms)
    else:                                                      # (the rotary kernel walks whole packed qkv rows: the dense attention, then its pooled rows)
        qkv, o, lse = _attn_forward(h, W, c, 0)
        oc = _pool_view(o.view(M, inner), B, n, row)
    p = ops.gemm(oc, W.w_out, B, D, inner)                                             # from here on: B rows
    x2, ff = _ffn_forward(p, xc, W, c, 0)
    return x2, LayerTape(x=x, h=h, m1=m1, r1=r1, qkv=qkv, o=o, lse=lse, p=p, **ff)


def _layer_backward_pooled(dx2: Tensor, t: LayerTape, W: LayerWeights, need: LayerWeights, dg: LayerWeights, c: _Pass, sg: _SideGemm, row: int):
    """dx2 [B, D]: gradient w.r.t. the pooled rows of the layer output -> (gradient w.r.t. the layer input [B n, D], weight gradients)"""
    if c.layout is not None:
        return _layer_backward_pooled_packed(dx2, t, W, need, dg, c, sg)
    spec, B, n, inner = c.spec, c.B, c.n, c.spec.inner
    M, D = t.x.shape
    dx1, dp, d_ff1, d_ff2 = _ffn_backward(dx2, t, W, need, dg, c, sg, 0)
    if spec.rotary is None or row == 0:
        q, kv = t.qkv
        d_out = sg.wgrad(dp, t.o, D, inner, B, W.w_out) if need.w_out else None
        doc = ops.gemm(dp, W.w_out, B, inner, D, b_kmajor=True)
        dq, dkv = ops.attention_pool_bwd(q, kv.view(B, n, 2 * inner), c.mask, t.o, doc, t.lse, spec.heads, spec.scale, spec.head_slot, row + 1 if spec.causal else None)
        if spec.rotary is not None:
            ops.rotary_(dkv.view(M, 2 * inner), n, spec.rotary, inverse=True, head_dim=spec.head_slot)    # the saved kv is the rotated one; R^T maps its gradient back
        # d h = dkv W_kv on every row, + dq W_q on the pooled rows
        dh = ops.gemm(dkv.view(M, 2 * inner), W.w_qkv[inner:], M, D, 2 * inner, b_kmajor=True)
        _add_to_pooled_rows(dh, ops.gemm(dq, W.w_qkv[:inner], B, D, inner, b_kmajor=True), B, n, row)
        d_qkv = None
        if need.w_qkv:                                         # both parts of the weight gradient into ONE tensor (a bucket slice, if claimed)
            d_qkv = _grad_out(W.w_qkv, (3 * inner, D), dp.dtype, dp.device)
            sg.wgrad_into(dq, _pool_view(t.h, B, n, row), inner, D, B, d_qkv[:inner])
            sg.wgrad_into(dkv.view(M, 2 * inner), t.h, 2 * inner, D, M, d_qkv[inner:])
        del dkv
    else:
        d_out = sg.wgrad(dp, _pool_view(t.o.view(M, inner), B, n, row), D, inner, B, W.w_out) if need.w_out else None
        # the attention sees a gradient on the pooled query rows only (dK / dV of every row come from those queries)
        do = torch.zeros(M, inner, dtype=dp.dtype, device=dp.device)
        ops.gemm(dp, W.w_out, B, inner, D, b_kmajor=True, out=_pool_view(do, B, n, row))
        dqkv = _attn_backward(do, t, c, 0)
        del do
        dh, d_qkv = _qkv_backward(dqkv, t, W, need, c, sg)
        del dqkv
    dx, _ = ops.layernorm_bwd(dh, t.x, W.g_attn, t.m1, t.r1, dg=dg.g_attn)
    _add_to_pooled_rows(dx, dx1, B, n, row)                    # the skip connection carries a gradient on the pooled rows only
    return dx, dict(w_qkv=d_qkv, w_out=d_out, w_ff1=d_ff1, w_ff2=d_ff2)


# ---- the same for a packed batch (c.layout): the pooled row is the FIRST row of every sample, row cu[s] of the [R, D] arrays ----------------
# -- or, for a layout that ends every sample at its first EOS token (the causal encoder, layout.ends_at_eos), its LAST row cu[s+1] - 1.  Under the
# causal mask that row sees every row of its sample, which is what the one-query varlen attention computes: the kernels are the same, only
# the rows the query / skip connection are gathered from (and their gradients added to) differ.
def pooled_rows(layout) -> Tensor:
    """int32 [batch]: the packed row the text head reads of every sample"""
    return layout.cu[1:] - 1 if layout.ends_at_eos else layout.cu[:-1]


# The rows of a sample are not a fixed stride apart, so the strided views above become gathers (xclip_gather_rows by cu[:-1]) and the two
# "add into the pooled rows" become xclip_rows_add_at; the one-query attention reads each sample's own keys through cu
# (attention_pool.h, the packed wrappers).  Same algebra and the same rounding points as the dense pooled layer above.
def _layer_forward_pooled_packed(x: Tensor, W: LayerWeights, c: _Pass):
    spec, lay, inner = c.spec, c.layout, c.spec.inner
    (R, D), B, first = x.shape, c.layout.batch, pooled_rows(c.layout)
    h, m1, r1 = ops.layernorm_fwd(x, W.g_attn)                                         # PreNorm, every kept row   :126
    xc = ops.gather_rows(x, first)                                                     # the skip connection's pooled rows
    hc = ops.gather_rows(h, first)
    q = ops.gemm(hc, W.w_qkv[:inner], B, inner, D)                                     # to_qkv: the query third on B rows,
    kv = ops.gemm(h, W.w_qkv[inner:], R, 2 * inner, D)                                 # keys | values on all R      :216
    if spec.rotary is not None:
        # keys and values rotated at their positions; the query is the CLS row, position 0: the angle 0, sincosf(0) = (0, 1) exactly -- the
        # identity, as in the dense pooled layer at row == 0
        assert lay.has_cls and not lay.ends_at_eos, "rotary in the packed tower: the pooled row is the CLS row at position 0"
        ops.rotary_pos_(kv, lay.pos, spec.rotary, head_dim=spec.head_slot)
    oc, lse = ops.attention_pool_varlen_fwd(q, kv, lay.cu, spec.heads, spec.scale, spec.head_slot)
    p = ops.gemm(oc, W.w_out, B, D, inner)                                             # from here on: B rows
    x2, ff = _ffn_forward(p, xc, W, c, 0)
    return x2, LayerTape(x=x, h=h, m1=m1, r1=r1, qkv=(q, kv, hc), o=oc, lse=lse, p=p, **ff)


def _layer_backward_pooled_packed(dx2: Tensor, t: LayerTape, W: LayerWeights, need: LayerWeights, dg: LayerWeights, c: _Pass, sg: _SideGemm):
    """dx2 [B, D]: gradient w.r.t. the CLS rows of the layer output -> (gradient w.r.t. the layer input [R, D], weight gradients)"""
    spec, lay, inner = c.spec, c.layout, c.spec.inner
    (R, D), B, first = t.x.shape, c.layout.batch, pooled_rows(c.layout)
    dx1, dp, d_ff1, d_ff2 = _ffn_backward(dx2, t, W, need, dg, c, sg, 0)
    q, kv, hc = t.qkv
    d_out = sg.wgrad(dp, t.o, D, inner, B, W.w_out) if need.w_out else None
    doc = ops.gemm(dp, W.w_out, B, inner, D, b_kmajor=True)
    dq, dkv = ops.attention_pool_varlen_bwd(q, kv, lay.cu, t.o, doc, t.lse, spec.heads, spec.scale, spec.head_slot)
    if spec.rotary is not None:
        assert lay.has_cls and not lay.ends_at_eos, "rotary in the packed tower: the pooled row is the CLS row at position 0"
        ops.rotary_pos_(dkv, lay.pos, spec.rotary, inverse=True, head_dim=spec.head_slot)    # the saved kv is the rotated one; R^T maps its gradient back
    # d h = dkv W_kv on every row, + dq W_q on the CLS rows
    dh = ops.gemm(dkv, W.w_qkv[inner:], R, D, 2 * inner, b_kmajor=True)
    ops.rows_add_at(dh, first, ops.gemm(dq, W.w_qkv[:inner], B, D, inner, b_kmajor=True))
    d_qkv = None
    if need.w_qkv:                                             # both parts of the weight gradient into ONE tensor (a bucket slice, if claimed)
        d_qkv = _grad_out(W.w_qkv, (3 * inner, D), dp.dtype, dp.device)
        sg.wgrad_into(dq, hc, inner, D, B, d_qkv[:inner])
        sg.wgrad_into(dkv, t.h, 2 * inner, D, R, d_qkv[inner:])
    del dkv
    dx, _ = ops.layernorm_bwd(dh, t.x, W.g_attn, t.m1, t.r1, dg=dg.g_attn)
    ops.rows_add_at(dx, first, dx1)                            # the skip connection carries a gradient on the CLS rows only
    return dx, dict(w_qkv=d_qkv, w_out=d_out, w_ff1=d_ff1, w_ff2=d_ff2)


# ---- the whole stack: norm_in -> depth x (attention, feed-forward) -> norm_out ------------------------------------------
def can_pool(spec: StackSpec) -> bool:
    """may the last layer run on one row per sample (`pool_row`)?  Dropout masks are indexed by the element's position in the dense
    activation (the oracle rebuilds them from it), so a stack with dropout keeps the dense last layer"""
    return spec.depth >= 1 and spec.attn_dropout == 0.0 and spec.ff_dropout == 0.0


def _packed_key_mask(layout, pool_row, spec: StackSpec) -> Tensor:
    """bool [batch, n + 1]: the positions a layout keeps -- the key mask the dense tower runs the same batch under (index arithmetic only)"""
    assert layout is not None and layout.has_cls and not spec.causal and pool_row is None, "dense_attention: a CLS-token layout, every row wanted"
    return (layout.row_of() >= 0).contiguous()


def stack_forward(x0: Tensor, B: int, n: int, spec: StackSpec, params: Sequence[Tensor], mask: Optional[Tensor],
                  out: Optional[Tensor] = None, out_group: int = 0, keep_tape: bool = True, pool_row: Optional[int] = None, layout=None,
                  dense_attention: bool = False):
    """x0 [B*n, D] -> norm_out(...) [B*n, D] (or written into `out`, see ops.layernorm_fwd) and the backward tape.
    pool_row = r: only token row r of every sample is wanted -> [B, D] (the last layer's row-wise part runs on those rows alone).
    layout (packing.TextLayout): x0 is [R, D], the kept rows end to end (_Pass); every layer runs on all R rows -- with pool_row = 0 (the first
    row of every sample, its CLS row) the last layer's row-wise part runs on those B rows (_layer_forward_pooled_packed) -> [B, D].
    dense_attention (with a layout that has CLS rows, no pooled layer): every layer's attention runs through the dense kernels on the rows put
    back by position (_attn_dense_on_packed); pass the same flag to stack_backward"""
    assert len(params) == 2 + LAYER_PARAMS * spec.depth
    assert pool_row is None or (can_pool(spec) and out is None and 0 <= pool_row < n)
    assert layout is None or (pool_row in (None, 0) and mask is None and out is None and x0.shape[0] == layout.R)
    assert layout is None or spec.causal == layout.ends_at_eos, "a causal stack takes a layout that ends at the EOS row, and only it"
    mask = _packed_key_mask(layout, pool_row, spec) if dense_attention else mask
    x, m_in, r_in = ops.layernorm_fwd(x0, params[0])
    # dropout: one 64-bit seed per pass from torch's CPU generator (no device sync; torch.manual_seed makes it reproducible); layer l
    # uses seed + 2 l (attention) and seed + 2 l + 1 (feed-forward); the backward and a checkpointed re-run regenerate the same masks
    seed0 = _draw_seed() if (spec.attn_dropout > 0.0 or spec.ff_dropout > 0.0) else 0
    layers, c = [], _Pass(spec, B, n, mask, layout)
    for l in range(spec.depth):
        W, _ = layer_weights(params, l)
        if pool_row is not None and l == spec.depth - 1:
            x, lt = _layer_forward_pooled(x, W, c, pool_row)
        else:
            x, lt = _layer_forward(x, W, c, seed0 + 2 * l)
        if keep_tape:
            layers.append(lt.x if spec.checkpoint else lt)       # checkpointing: the layer's input alone
    y, m_out, r_out = ops.layernorm_fwd(x, params[-1], out=out, out_group=out_group)
    return y, (x0, m_in, r_in, layers, x, m_out, r_out, seed0, pool_row) if keep_tape else None


def stack_backward(dy: Tensor, tape, B: int, n: int, spec: StackSpec, params: Sequence[Tensor], mask: Optional[Tensor], need: Sequence[bool],
                   layout=None, dense_attention: bool = False):
    """dy [B*n, D] contiguous ([B, D] for a pooled forward; [R, D] with the forward's `layout`) -> (dx0, grads aligned with `params` (None where not needed))"""
    x0, m_in, r_in, layers, x_last, m_out, r_out, seed0, pool_row = tape
    mask = _packed_key_mask(layout, pool_row, spec) if dense_attention else mask
    gg = _GainGrads(params, (True,) + spec.depth * IS_GAIN + (True,))
    grads: List[Optional[Tensor]] = [None] * len(params)
    sg, c = _SideGemm(dy.device), _Pass(spec, B, n, mask, layout)
    def stats_for(l: int):
        """the row constants of layer l's fused feed-forward backward can be written by the kernel that produces its output gradient -- the LayerNorm
        backward of the layer above it, or of norm_out -- whose input row is layer l's output.  Not with recompute (layer l's tape does not exist yet at that
        point), dropout, a pooled layer (l itself, or the one above it: its kernel's dx is completed on the pooled rows afterwards) or shapes the fused kernel does not take"""
        lt = layers[l] if 0 <= l < spec.depth else None
        if not isinstance(lt, LayerTape) or spec.ff_dropout != 0.0 or (pool_row is not None and l >= spec.depth - 2):
            return None
        Wl, _ = layer_weights(params, l)
        return ops.ffn_stats_request(Wl.w_ff2, Wl.g_inner, lt.x1, lt.m4, lt.r4)

    st = stats_for(spec.depth - 1) if pool_row is None else None
    dx, _ = ops.layernorm_bwd(dy, x_last, params[-1], m_out, r_out, dg=gg.views[-1], ffn_stats=st)
    x_out = x_last if pool_row is None else None             # the output of the layer being walked (= the saved input of the one above it)
    for l in reversed(range(spec.depth)):
        W, base = layer_weights(params, l)
        lt, seed = layers[l], seed0 + 2 * l
        pooled = pool_row is not None and l == spec.depth - 1
        if not isinstance(lt, LayerTape):        # checkpointed: re-run the layer forward from its saved input
            _, lt = _layer_forward_pooled(lt, W, c, pool_row) if pooled else _layer_forward(lt, W, c, seed)
        (need_l, _), (dg, _) = layer_weights(need, l), layer_weights(gg.views, l)
        below = stats_for(l - 1)                 # (None for the layer under a pooled one)
        if pooled:
            dx, dws = _layer_backward_pooled(dx, lt, W, need_l, dg, c, sg, pool_row)
        else:
            dx, dws = _layer_backward(dx, lt, W, need_l, dg, c, sg, seed, x_out, (None if st is None else st[5], below))
        st = below
        x_out, layers[l] = lt.x, None            # release this layer's activations
        sg.layer_done()
        for f, d in dws.items():
            grads[base + LayerWeights._fields.index(f)] = d
    dx0, _ = ops.layernorm_bwd(dx, x0, params[0], m_in, r_in, dg=gg.views[0])
    sg.join()
    gg.finish(grads)
    return dx0, [g if nd else None for g, nd in zip(grads, need)]


def _contig_grad(d: Optional[Tensor], like_shape, dtype, device) -> Tensor:
    if d is None:
        return torch.zeros(like_shape, dtype=dtype, device=device)
    return d if d.is_contiguous() else d.contiguous()


def _take_tape(ctx):
    """the activation tape of a node, exactly once: it is released while the backward walks it (gigabytes per layer), so a second
    backward through the same graph (retain_graph=True, two losses sharing a tower) cannot be served -- say so instead of failing
    on a None deep inside"""
    tape = ctx.tape
    if tape is None:
        raise RuntimeError("x_clip_amd: this encoder pass was already back-propagated and its activations were released during that "
                           "backward; run the forward again (or sum the losses before calling backward once) -- retain_graph is not supported")
    ctx.tape = None
    return tape


class _TransformerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec: StackSpec, mask: Optional[Tensor], grad_mode: bool, x: Tensor, *params: Tensor):
        B, n, D = x.shape
        # (ctx.needs_input_grad reflects the parameters' requires_grad even under torch.no_grad(): without the caller's grad mode
        #  an inference pass or a frozen tower would build and hold the whole training tape until forward returned)
        keep = grad_mode and any(ctx.needs_input_grad)
        x2 = ops._c(x).view(B * n, D)
        y, tape = stack_forward(x2, B, n, spec, params, mask, keep_tape=keep)
        ctx.save_for_backward(*params)                       # autograd's version counters then catch in-place edits before backward
        ctx.spec, ctx.mask, ctx.tape, ctx.shape = spec, mask, tape, (B, n, D)
        return y.view(B, n, D)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, n, D = ctx.shape
        params = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]
        dy = _contig_grad(dy, (B, n, D), params[0].dtype, params[0].device).view(B * n, D)
        dx, grads = stack_backward(dy, _take_tape(ctx), B, n, ctx.spec, params, ctx.mask, need)
        return (None, None, None, dx.view(B, n, D) if ctx.needs_input_grad[3] else None, *grads)


def transformer(x: Tensor, params: Sequence[Tensor], spec: StackSpec, mask: Optional[Tensor] = None) -> Tensor:
    """Transformer.forward (x_clip.py:274-291) on [b, n, D]; mask: bool [b, n] key-padding mask or None."""
    return _TransformerFn.apply(spec, mask, torch.is_grad_enabled(), x, *params)


# ---- text encoder ---------------------------------------------------------------------------------------------------------
class _TextEncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec: StackSpec, tokens: Tensor, mask: Optional[Tensor], grad_mode: bool, pool_row: Optional[int], E: Tensor,
                P: Optional[Tensor], cls: Optional[Tensor], *stack: Tensor):
        B, n = tokens.shape
        npos = n + (1 if cls is not None else 0)
        D = E.shape[1]
        keep = grad_mode and any(ctx.needs_input_grad)
        ctx_pos_rows = P.shape[0] if P is not None else 0              # rows of the full table (its gradient keeps that shape)
        if P is not None and P.shape[0] != n:
            P = P[:n]                                                   # abs_pos_emb(arange(n))      x_clip.py:323
        x0 = ops.text_embed_fwd(tokens, E, P, cls)                      # token_emb + pos, cls concat  :320-331
        kmask = None
        if mask is not None:                                            # F.pad(mask, (1, 0), True)    :334
            kmask = mask if cls is None else torch.cat([mask.new_ones(B, 1), mask], dim=1)
            kmask = kmask.contiguous()
        y, tape = stack_forward(x0.view(B * npos, D), B, npos, spec, stack, kmask, keep_tape=keep, pool_row=pool_row)
        ctx.save_for_backward(*stack)
        ctx.spec, ctx.kmask, ctx.tape = spec, kmask, tape
        ctx.tokens, ctx.meta = tokens, (B, n, npos, D, E.shape[0], P is not None, cls is not None, E.dtype)
        ctx.pos_rows, ctx.pool_row = ctx_pos_rows, pool_row
        return y.view(B, npos, D) if pool_row is None else y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, n, npos, D, vocab, has_pos, has_cls, dtype = ctx.meta
        need = ctx.needs_input_grad[2:]                                  # (indices below: without the grad_mode and pool_row slots)
        if ctx.pool_row is None:
            dy = _contig_grad(dy, (B, npos, D), dtype, ctx.tokens.device).view(B * npos, D)
        else:
            dy = _contig_grad(dy, (B, D), dtype, ctx.tokens.device)
        dx0, sgrads = stack_backward(dy, _take_tape(ctx), B, npos, ctx.spec, ctx.saved_tensors, ctx.kmask, need[6:])
        dE = dP = dcls = None
        if need[3] or need[4] or need[5]:
            st = ops.sort_ids(ctx.tokens.reshape(-1), vocab) if need[3] else None    # ids ascending + their positions (sort.h)
            aE, aP, acls = ops.text_embed_bwd(dx0.view(B, npos, D), ctx.tokens, vocab, has_pos, has_cls, sorted_tokens=st)
            dE = ops.cast_from_f32(aE, dtype) if need[3] else None
            dP = ops.cast_from_f32(aP, dtype) if (need[4] and has_pos) else None
            if dP is not None and dP.shape[0] != ctx.pos_rows:           # text shorter than max_seq_len: the unused positions get zero
                full = torch.zeros(ctx.pos_rows, D, dtype=dP.dtype, device=dP.device)
                full[:dP.shape[0]].copy_(dP)
                dP = full
            dcls = ops.cast_from_f32(acls, dtype) if (need[5] and has_cls) else None
        return (None, None, None, None, None, dE, dP, dcls, *sgrads)


def text_encode(tokens: Tensor, mask: Optional[Tensor], E: Tensor, P: Optional[Tensor], cls: Optional[Tensor],
                stack: Sequence[Tensor], spec: StackSpec, pool_row: Optional[int] = None) -> Tensor:
    """TextTransformer.forward (x_clip.py:317-338): int64 tokens [b, n] (+ bool key mask [b, n]) -> [b, n+1, D];
    pool_row = r (the caller reads `[:, r]` and nothing else): -> [b, D], that row of every sample (stack_forward)."""
    if tokens.dtype != torch.int64:
        raise TypeError(f"text tokens must be int64, got {tokens.dtype}")
    if P is not None and tokens.shape[1] > P.shape[0]:
        raise IndexError(f"text length {tokens.shape[1]} exceeds max_seq_len {P.shape[0]}")
    if mask is not None and mask.dtype != torch.bool:
        mask = mask.bool()
    if pool_row is not None and not can_pool(spec):                   # (dropout: dense last layer, then the row)
        return select_row(_TextEncodeFn.apply(spec, tokens, mask, torch.is_grad_enabled(), None, E, P, cls, *stack), pool_row)
    return _TextEncodeFn.apply(spec, tokens, mask, torch.is_grad_enabled(), pool_row, E, P, cls, *stack)


class _PackedTextEncodeFn(torch.autograd.Function):
    """the text encoder on the kept rows alone (packing.TextLayout) -> the CLS row of every sample [b, D].  Padded rows are never embedded,
    normalised, multiplied or attended from, forward or backward; no [b (n + 1), D] array is allocated on this path.
    pool_last: the stack is asked for the CLS rows (stack_forward `pool_row = 0`): its last layer runs everything behind the attention on them alone
    pool_last = None (text_encode_packed(rows=True)): the stack's whole [R, D] output is the result, for the heads that read token rows (the
    fine-grained head, the MLM head, return_encodings); dy [R, D] enters stack_backward as it is"""

    @staticmethod
    def forward(ctx, spec: StackSpec, layout, grad_mode: bool, pool_last: Optional[bool], E: Tensor, P: Optional[Tensor], cls: Tensor, *stack: Tensor):
        keep = grad_mode and any(ctx.needs_input_grad)
        x0 = ops.text_embed_packed_fwd(layout.tok, layout.pos, E, P, cls)                # token_emb + pos, the cls rows   :320-331
        # every row wanted (rows=True): where the varlen attention would take its plain form (fp32, 128-wide slots, a sample beyond the
        # head-resident limit) the attention runs through the dense kernels instead, so that the kept rows are the dense tower's bit for bit
        dense_attn = pool_last is None and not varlen_is_head_resident(E.dtype, spec.head_slot, layout.max_len)
        y, tape = stack_forward(x0, layout.batch, layout.max_len, spec, stack, None, keep_tape=keep, pool_row=0 if pool_last else None, layout=layout,
                                dense_attention=dense_attn)
        ctx.save_for_backward(*stack)
        ctx.spec, ctx.layout, ctx.tape, ctx.pool_last, ctx.dense_attn = spec, layout, tape, pool_last, dense_attn
        ctx.meta = (E.shape[0], E.shape[1], 0 if P is None else P.shape[0], E.dtype)
        if pool_last is None:
            return y                                                                     # every kept row (and the filler rows behind them)
        return y if pool_last else ops.gather_rows(y, pooled_rows(layout))               # enc_text[:, 0] (causal: of eos_to_front)  :708

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        vocab, D, npos, dtype = ctx.meta
        lay = ctx.layout
        need = ctx.needs_input_grad[4:]
        dyr = _contig_grad(dy, (lay.R if ctx.pool_last is None else lay.batch, D), dtype, lay.cu.device)
        if ctx.pool_last is False:
            # dy into the CLS rows of a zeroed [R, D]: as a gather, row r takes dy[s] where r = cu[s] and the appended zero row elsewhere
            src = torch.full((lay.R,), lay.batch, dtype=torch.int32, device=dyr.device)
            src[pooled_rows(lay).long()] = torch.arange(lay.batch, dtype=torch.int32, device=dyr.device)
            dyr = ops.gather_rows(torch.cat([dyr, dyr.new_zeros(1, D)], dim=0), src)
        dx0, sgrads = stack_backward(dyr, _take_tape(ctx), lay.batch, lay.max_len, ctx.spec, ctx.saved_tensors, None, need[3:], layout=lay,
                                     dense_attention=ctx.dense_attn)
        dE = dP = dcls = None
        if need[0] or need[1] or need[2]:
            tok_key, pos_key = lay.keys(vocab, npos)
            aE, aP, acls = ops.text_embed_packed_bwd(dx0, tok_key, pos_key, lay.cu, vocab, npos, lay.has_cls, need_E=need[0], need_P=need[1])
            dE = ops.cast_from_f32(aE, dtype) if need[0] else None
            dP = ops.cast_from_f32(aP, dtype) if (need[1] and aP is not None) else None
            dcls = ops.cast_from_f32(acls, dtype) if (need[2] and acls is not None) else None
        return (None, None, None, None, dE, dP, dcls, *sgrads)


def text_encode_packed(layout, E: Tensor, P: Optional[Tensor], cls: Optional[Tensor], stack: Sequence[Tensor], spec: StackSpec,
                       pool_last: bool = False, rows: bool = False) -> Tensor:
    """TextTransformer.forward (x_clip.py:317-338) followed by `[:, 0]` (x_clip.py:708) for a packed batch -> [b, D]: the same function of
    the same tokens as text_encode(..., mask, pool_row=0), computed on the kept rows only.  Every layer runs on all R rows; with pool_last the
    last one runs its attention as one query per (sample, head) and everything behind it on the b CLS rows (the packed twin of the dense
    path's pooled last layer, with its rounding points: see _layer_forward_pooled).
    rows = True (CLIP.pack_text_tokens): -> [R, D], the stack's output on every packed row -- row r is what the dense tower computes at
    (sample of r, layout.pos[r]); unpack_rows puts them back by position.  Never pools the last layer"""
    # the causal encoder: no CLS row, a causal mask, read at the first EOS token -- on a layout that ends every sample there (text_layout(eos_id=))
    eos = cls is None and spec.causal and layout.ends_at_eos and not layout.has_cls
    if cls is None and not eos:
        raise NotImplementedError("pack_text: the packed text tower returns the CLS row (text_has_cls_token=True)")
    # rotary (CLIP.pack_text_rotary): the rows are rotated by layout.pos (xclip_rotary_pos); a rotary encoder has a CLS row and no position table
    if (spec.rotary is not None and (eos or P is not None)) or (spec.causal and not eos) or spec.attn_dropout > 0.0 or spec.ff_dropout > 0.0:
        raise NotImplementedError("pack_text: no rotary embedding (text_rotary_pos_emb) beside a position table or the causal encoder, no causal mask "
                                  "(text_causal_mask) without an EOS layout and no dropout in the packed text tower")
    if not eos and (not layout.has_cls or layout.ends_at_eos or layout.kept < layout.batch):
        raise ValueError("pack_text: the layout must keep a CLS row per sample (text_layout(..., has_cls=True))")
    if eos and layout.kept < layout.batch:
        raise ValueError("pack_text_causal: the layout must keep every sample's EOS row")
    if P is not None and layout.n > P.shape[0]:
        raise IndexError(f"text length {layout.n} exceeds max_seq_len {P.shape[0]}")
    if layout.cu.device != E.device:
        layout = layout.to(E.device)
    if rows:
        if eos:
            raise NotImplementedError("pack_text: rows=True (every token row) is defined for the CLS-token encoder, not the causal one")
        return _PackedTextEncodeFn.apply(spec, layout, torch.is_grad_enabled(), None, E, P, cls, *stack)
    return _PackedTextEncodeFn.apply(spec, layout, torch.is_grad_enabled(), bool(pool_last) and can_pool(spec), E, P, cls, *stack)


class _UnpackRowsFn(torch.autograd.Function):
    """packed [R, D] -> dense [b, n_out, D] by (sample, position) (xclip_unpack_rows); the backward is the transpose, xclip_pack_rows"""

    @staticmethod
    def forward(ctx, x: Tensor, layout, pos0: int, n_out: int):
        ctx.layout, ctx.pos0 = layout, pos0
        return ops.unpack_rows(x, layout.cu, layout.pos, pos0, n_out)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.pack_rows(dy, ctx.layout.cu, ctx.layout.pos, ctx.pos0), None, None, None


class _PackRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, layout, pos0: int):
        ctx.layout, ctx.pos0, ctx.n_out = layout, pos0, x.shape[1]
        return ops.pack_rows(x, layout.cu, layout.pos, pos0)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return ops.unpack_rows(dy, ctx.layout.cu, ctx.layout.pos, ctx.pos0, ctx.n_out), None, None


def _rows_layout(x: Tensor, layout, rows_dim: int):
    if layout.cu.device != x.device:
        layout = layout.to(x.device)
    if x.dim() != rows_dim or (rows_dim == 2 and x.shape[0] != layout.R) or (rows_dim == 3 and x.shape[0] != layout.batch):
        raise ValueError(f"packed rows are [R = {layout.R}, D], dense rows [batch = {layout.batch}, n_out, D]; got {tuple(x.shape)}")
    return layout


def unpack_rows(x: Tensor, layout, pos0: int, n_out: int) -> Tensor:
    """x [R, D] on the rows of `layout` (packing.TextLayout) -> [batch, n_out, D]: out[s, p - pos0] = the row of sample s at position p, +0
    where the layout keeps none.  pos0 = 1, n_out = n: `enc_text[:, 1:]` (x_clip.py:704); pos0 = 0, n_out = n + 1: the whole encoding"""
    return _UnpackRowsFn.apply(x, _rows_layout(x, layout, 2), int(pos0), int(n_out))


def pack_rows(x: Tensor, layout, pos0: int) -> Tensor:
    """x [batch, n_out, D] -> [R, D]: out[r] = x[sample of r, layout.pos[r] - pos0], +0 on the rows in front of pos0 and on filler rows --
    unpack_rows' transpose"""
    return _PackRowsFn.apply(x, _rows_layout(x, layout, 3), int(pos0))


# ---- vision encoder -----------------------------------------------------------------------------------------------------------
class _VisionEncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec: StackSpec, patch: int, image: Tensor, keep_idx: Optional[Tensor], grad_mode: bool, w_tok: Tensor,
                b_tok: Tensor, pos: Tensor, w_cls: Tensor, *stack: Tensor):
        B, C, H, Wd = image.shape
        D = w_tok.shape[0]
        npatch = (H // patch) * (Wd // patch)
        keep = grad_mode and any(ctx.needs_input_grad)
        if keep_idx is not None:                                        # PatchDropout keep-set        x_clip.py:140-151
            nk = keep_idx.shape[1]
            rowidx = keep_idx.reshape(-1)
        else:
            nk = npatch
            rowidx = torch.arange(npatch, dtype=torch.int32, device=image.device).repeat(B)
        patches = ops.patchify(image, patch, keep_idx)                  # Rearrange (p1 p2 c)          :357
        Kp = patches.shape[1]
        if w_tok.shape[1] != Kp:                                        # K padded to the 16-byte chunk (e.g. 588 -> 592)
            w_pad = w_tok.new_zeros(D, Kp)
            ops.copy_rows(w_tok, w_pad[:, : w_tok.shape[1]]) if w_tok.shape[1] % ops.vec(w_tok.dtype) == 0 else \
                w_pad[:, : w_tok.shape[1]].copy_(w_tok)
        else:
            w_pad = w_tok
        # Linear(patch_dim, dim) + bias + pos_emb[patch]                :358,382-383 (dropout after the add == gather of both)
        tok = ops.gemm(patches, w_pad, B * nk, D, Kp, bias=b_tok, addrows=pos, rowidx=rowidx)
        enc = torch.empty(B, 1 + nk, D, dtype=tok.dtype, device=tok.device)
        y, tape = stack_forward(tok, B, nk, spec, stack, None, out=enc.view(B * (1 + nk), D), out_group=nk, keep_tape=keep)
        pooled = ops.token_mean_fwd(enc[:, 1:])                         # Reduce('b n d -> b d', 'mean') :367
        ops.gemm(pooled, w_cls, B, D, D, out=enc[:, 0])                 # to_cls_tokens Linear + concat  :368,389-390
        ctx.save_for_backward(w_cls, *stack)
        ctx.spec, ctx.tape = spec, tape
        ctx.saved = (patches if keep else None, rowidx, pooled, w_pad)
        ctx.meta = (B, nk, D, npatch, Kp, w_tok.shape[1], w_tok.dtype)
        return enc

    @staticmethod
    @once_differentiable
    def backward(ctx, denc):
        B, nk, D, npatch, Kp, Kw, dtype = ctx.meta
        patches, rowidx, pooled, w_pad = ctx.saved
        w_cls, *stack = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]                                  # (indices below: without the grad_mode slot)
        denc = _contig_grad(denc, (B, 1 + nk, D), dtype, pooled.device)
        dcls = denc[:, 0]                                               # [B, D], row stride (1+nk) D
        dpooled = ops.gemm(dcls, w_cls, B, D, D, b_kmajor=True)
        dw_cls = ops.gemm(dcls, pooled, D, D, B, a_kmajor=True, b_kmajor=True) if need[7] else None
        dy = ops.token_mean_bwd(dpooled, nk, add=denc[:, 1:])           # mean-pool backward + direct token gradients
        dtok, sgrads = stack_backward(dy.view(B * nk, D), _take_tape(ctx), B, nk, ctx.spec, stack, None, need[8:])
        dw_tok = db = dpos = None
        if need[4]:
            dw_tok = ops.gemm(dtok, patches, D, Kp, B * nk, a_kmajor=True, b_kmajor=True)
            if Kp != Kw:
                dw_tok = dw_tok[:, :Kw].contiguous()
        if need[5] or need[6]:
            acc_b = torch.zeros(D, dtype=torch.float32, device=dtok.device) if need[5] else None
            acc_p = torch.zeros(npatch, D, dtype=torch.float32, device=dtok.device) if need[6] else None
            if need[5]:
                ops.rows_scatter_add(dtok, None, None, acc_b)           # bias gradient = column sum
            if need[6]:
                ops.scatter_add_sorted(dtok, *ops.sort_ids(rowidx.to(torch.int64).reshape(-1), npatch), acc_p)
            db = ops.cast_from_f32(acc_b, dtype) if need[5] else None
            dpos = ops.cast_from_f32(acc_p, dtype) if need[6] else None
        return (None, None, None, None, None, dw_tok, db, dpos, dw_cls, *sgrads)


def vision_encode(image: Tensor, keep_idx: Optional[Tensor], patch: int, w_tok: Tensor, b_tok: Tensor, pos: Tensor,
                  w_cls: Tensor, stack: Sequence[Tensor], spec: StackSpec) -> Tensor:
    """VisionTransformer.forward (x_clip.py:372-390): image [b, c, H, W] -> [b, 1 + n_keep, D].  keep_idx: int32
    [b, n_keep] kept patch indices (the PatchDropout draw) or None to keep all patches.  The image itself receives no
    gradient."""
    if image.dtype != w_tok.dtype:
        raise TypeError(f"image dtype {image.dtype} must match the model dtype {w_tok.dtype}")
    if keep_idx is not None and keep_idx.dtype != torch.int32:
        keep_idx = keep_idx.to(torch.int32)
    return _VisionEncodeFn.apply(spec, patch, image, None if keep_idx is None else keep_idx.contiguous(), torch.is_grad_enabled(),
                                 w_tok, b_tok, pos, w_cls, *stack)


# ---- small differentiable pieces of the head -------------------------------------------------------------------------------
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor):
        lead = x.shape[:-1]
        K = x.shape[-1]
        x2 = x if (x.dim() == 2 and x.stride(1) == 1) else ops._c(x).view(-1, K)
        M, N = x2.shape[0], w.shape[0]
        y = ops.gemm(x2, w, M, N, K)
        ctx.save_for_backward(x2, w)
        ctx.lead = lead
        return y.view(*lead, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        M, K = x2.shape
        N = w.shape[0]
        dy2 = ops._c(dy).view(M, N)
        dx = ops.gemm(dy2, w, M, K, N, b_kmajor=True).view(*ctx.lead, K) if ctx.needs_input_grad[0] else None
        dw = ops.gemm(dy2, x2, N, K, M, a_kmajor=True, b_kmajor=True, out=_grad_out(w, (N, K), dy2.dtype, dy2.device)) if ctx.needs_input_grad[1] else None
        return dx, dw


def linear(x: Tensor, w: Tensor) -> Tensor:
    """bias-free nn.Linear (to_text_latent / to_visual_latent, x_clip.py:556,570,713-714)"""
    return _LinearFn.apply(x, w)


class _DownsampleFn(torch.autograd.Function):
    """`downsample_image_embeds` projection (x_clip.py:560-568): depthwise 4 x 4 / stride 2 / pad 1 convolution over the square token
    grid, then the 1 x 1 convolution with bias = a GEMM with a bias row.  tokens [b, n, C] -> [b, n / 4, L]."""

    @staticmethod
    def forward(ctx, x: Tensor, w_dw: Tensor, w_pw: Tensor, b_pw: Tensor):
        x = ops._c(x)
        b, n, C = x.shape
        L = w_pw.shape[0]
        wd = ops._c(w_dw).view(C, 16)
        wp = ops._c(w_pw).view(L, C)
        y = ops.dwconv4s2_fwd(x, wd)                                           # [b, n/4, C]
        M = y.shape[0] * y.shape[1]
        z = ops.gemm(y.view(M, C), wp, M, L, C, bias=ops._c(b_pw))
        ctx.save_for_backward(x, wd, y, wp)
        ctx.meta = (b, n, C, L, w_dw.shape, w_pw.shape, b_pw.dtype)
        return z.view(b, y.shape[1], L)

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        x, wd, y, wp = ctx.saved_tensors
        b, n, C, L, dw_shape, pw_shape, bdt = ctx.meta
        M = y.shape[0] * y.shape[1]
        dz2 = ops._c(dz).view(M, L)
        dy = ops.gemm(dz2, wp, M, C, L, b_kmajor=True)                         # [M, C]
        d_pw = ops.gemm(dz2, y.view(M, C), L, C, M, a_kmajor=True, b_kmajor=True).view(pw_shape) if ctx.needs_input_grad[2] else None
        d_b = None
        if ctx.needs_input_grad[3]:
            acc = torch.zeros(L, dtype=torch.float32, device=dz.device)
            ops.rows_scatter_add(dz2, None, None, acc)                         # column sums
            d_b = acc.to(bdt)
        dwa = torch.zeros(C * 16, dtype=torch.float32, device=dz.device)
        dx = ops.dwconv4s2_bwd(dy.view(b, M // b, C), x, wd, dwa)
        d_dw = dwa.to(wd.dtype).view(dw_shape) if ctx.needs_input_grad[1] else None
        return (dx if ctx.needs_input_grad[0] else None), d_dw, d_pw, d_b


def downsample_latents(tokens: Tensor, w_dw: Tensor, w_pw: Tensor, b_pw: Tensor) -> Tensor:
    return _DownsampleFn.apply(tokens, w_dw, w_pw, b_pw)


class _L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        y, rn = ops.l2norm_fwd(x)
        ctx.save_for_backward(y, rn)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        y, rn = ctx.saved_tensors
        return ops.l2norm_bwd(ops._c(dy), y, rn)


def l2norm(x: Tensor) -> Tensor:
    """F.normalize(dim=-1) (x_clip.py:54-55,715)"""
    return _L2NormFn.apply(x)


class _PairSimilarityFn(torch.autograd.Function):
    """einsum('b d, b d -> b'): the similarity of matched pairs, the reference's inference return (x_clip.py:744-746)"""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        ctx.save_for_backward(a, b)
        return ops.rowdot(a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        a, b = ctx.saved_tensors
        ds = ds.unsqueeze(-1)
        return (ds * b if ctx.needs_input_grad[0] else None), (ds * a if ctx.needs_input_grad[1] else None)


def pair_similarity(a: Tensor, b: Tensor) -> Tensor:
    return _PairSimilarityFn.apply(a, b)


def _pad_dim(x: Tensor, dim: int, mult: int) -> Tensor:
    n = x.shape[dim]
    if n % mult == 0:
        return x.contiguous()
    shape = list(x.shape)
    shape[dim] = (n + mult - 1) // mult * mult
    out = x.new_zeros(shape)
    out.narrow(dim, 0, n).copy_(x)
    return out


class _TokenSimilarityFn(torch.autograd.Function):
    """einsum('b t d, b i d -> b t i'): every text token against every image token of the MATCHED pair -- the reference's fine-grained
    inference return (x_clip.py:742-743).  One batched launch forward, one per gradient (xclip_gemm_batched)."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        B, t, d = a.shape
        i = b.shape[1]
        v = ops.vec(a.dtype)
        assert d % v == 0, "latent width must be a multiple of the 16-byte chunk"
        a, bp = a.contiguous(), _pad_dim(b, 1, v)               # (the product's N is a whole number of chunks: zero rows behind the image tokens)
        ctx.save_for_backward(a, b.contiguous())
        return ops.bmm(a, bp, t, bp.shape[1], d)[:, :, :i]

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        a, b = ctx.saved_tensors
        B, t, d = a.shape
        i = b.shape[1]
        dsp = _pad_dim(ds, 2, ops.vec(a.dtype))                 # [B, t, ip], zero columns behind i
        da = ops.bmm(dsp, b, t, d, i, False, True) if ctx.needs_input_grad[0] else None          # dS b
        db = ops.bmm(dsp, a, i, d, t, True, True) if ctx.needs_input_grad[1] else None           # dS^T a
        return da, db


def token_similarity(a: Tensor, b: Tensor) -> Tensor:
    return _TokenSimilarityFn.apply(a, b)


class _SelectRowFn(torch.autograd.Function):
    """enc[:, index] as a contiguous [b, D] tensor (x_clip.py:708-709); the backward scatters into a zeroed buffer."""

    @staticmethod
    def forward(ctx, enc: Tensor, index: int):
        B, n, D = enc.shape
        out = torch.empty(B, D, dtype=enc.dtype, device=enc.device)
        ops.copy_rows(enc[:, index], out)
        ctx.meta = (B, n, D, index)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        B, n, D, index = ctx.meta
        denc = torch.zeros(B, n, D, dtype=dout.dtype, device=dout.device)
        ops.copy_rows(ops._c(dout), denc[:, index])
        return denc, None


def select_row(enc: Tensor, index: int = 0) -> Tensor:
    return _SelectRowFn.apply(enc, index)


class _PermuteRowsFn(torch.autograd.Function):
    """out[r] = x[idx[r]] for a PERMUTATION idx of the rows of x [rows, D]; the backward gathers with the inverse permutation"""

    @staticmethod
    def forward(ctx, x: Tensor, idx: Tensor, inv: Tensor):
        ctx.save_for_backward(inv)
        return ops.gather_rows(x, idx)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (inv,) = ctx.saved_tensors
        return ops.gather_rows(ops._c(dout), inv), None, None


def eos_to_front(enc: Tensor, tokens: Tensor, eos_id: int) -> Tensor:
    """the causal text encoder's pooling (x_clip.py:670-685): per sample, the encoding at the FIRST eos token moves to position 0
    and the other positions follow in their original order.  The index bookkeeping is integer work on the [b, n] token tensor;
    the rows move through xclip_gather_rows."""
    B, n, D = enc.shape
    is_eos = tokens == eos_id
    assert torch.all(torch.any(is_eos, dim=-1)), f'some of the text rows does not have the eos id {eos_id}'
    e = is_eos.float().argmax(dim=-1, keepdim=True)                           # first eos per row                  x_clip.py:675
    j = torch.arange(n, device=tokens.device)[None]
    src = torch.where(j == 0, e, torch.where(j <= e, j - 1, j))               # out position j <- source position
    base = torch.arange(B, device=tokens.device)[:, None] * n
    idx = (src + base).reshape(-1)
    inv = torch.empty_like(idx)
    inv[idx] = torch.arange(B * n, device=tokens.device)
    out = _PermuteRowsFn.apply(ops._c(enc).view(B * n, D), idx.to(torch.int32).contiguous(), inv.to(torch.int32).contiguous())
    return out.view(B, n, D)
