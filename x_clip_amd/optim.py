"""The step after `loss.backward()`: clip-by-global-norm + AdamW as three kinds of kernel launches over ALL parameters (csrc/kernels/optim.h),
with fp32 master weights for bf16 parameters kept inside the optimizer.

    opt = FusedAdamW(FusedAdamW.default_param_groups(model, weight_decay=0.2), lr=5e-4, max_grad_norm=1.0)
    loss.backward(); sync.finish(); opt.step(); opt.zero_grad()

Why: `torch.optim.AdamW` on a `.bfloat16()` model keeps both moments in bf16 and adds lr * update to an 8-bit mantissa -- at CLIP's
learning rates most updates are below half an ulp of the weight and are rounded away.  Here the model keeps exactly the bf16 tensors it
has (forward and backward are untouched); the optimizer owns an fp32 copy, updates that, and writes each parameter as its rounded value.
Python does bookkeeping only: every number is computed by the HIP kernels, nothing is read back to the host during a step.
`ema_decay=...` keeps an fp32 moving average of those unrounded weights in the same pass; `with opt.ema_weights():` evaluates on it.
Param-group keys `trust_ratio` (LAMB's layer-wise step) and `bounds` (a clamp of the fp32 weight, e.g. CLIP's temperature) act on the masters.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from itertools import chain
from typing import Optional

import numpy as np
import torch

from . import ops

_ALIGN_ELEMS = 32                                               # state slices are 128-byte aligned (as GradSync's)
# csrc/kernels/optim.h OptChunk
_TABLE_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("state_off", "<i8"), ("n", "<i4"), ("dtypes", "<i4"), ("param", "<i4"),
                         ("first", "<i4"), ("reserved", "<i4", (2,))])
assert _TABLE_DTYPE.itemsize == ops.OPTIM_CHUNK_BYTES
_CODE = {torch.float32: 0, torch.bfloat16: 1}
_STAGING = 4                                                    # pinned staging buffers per device (see _DeviceState)
_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "trust_ratio", "bounds")       # what a param group means here
_BLK_NORM, _BLK_CLIP, _BLK_BAD, _BLK_STEP, _BLK_SKIPPED = 0, 1, 2, 3, 4


def _round_bound(x: float, dtype, up: bool) -> float:
    """the value of `dtype` (fp32 / bf16) nearest to x on the side asked for (up: >= x, else <= x): a bound the stored weight can hold"""
    f = np.float32(x)
    if float(f) != x and (float(f) < x) == up:
        f = np.nextafter(f, np.float32(np.inf if up else -np.inf))
    if dtype == torch.bfloat16 and np.isfinite(f):
        bits = int(f.view(np.uint32))
        if bits & 0xffff:                                       # truncation rounds towards zero: one step away from it where that is asked for
            bits = (bits & 0xffff0000) + (0x10000 if up == (f > 0) else 0)
            f = np.uint32(bits).view(np.float32)
    return float(f)


def _group_bounds(group, dtype):
    """(lo, hi) a group's `bounds` mean for weights stored as `dtype`: floats the kernels take, -inf / +inf where there is none"""
    bounds = group.get("bounds")
    if bounds is None:
        return -math.inf, math.inf
    try:
        lo, hi = bounds
        lo, hi = -math.inf if lo is None else float(lo), math.inf if hi is None else float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"invalid bounds: {bounds!r} (None or a pair (lo, hi), either end None)") from None
    if math.isnan(lo) or math.isnan(hi) or lo > hi or lo == math.inf or hi == -math.inf:
        raise ValueError(f"invalid bounds: {bounds!r} (lo > hi)")
    rlo, rhi = _round_bound(lo, dtype, True), _round_bound(hi, dtype, False)
    if rlo > rhi:
        raise ValueError(f"invalid bounds: {bounds!r} holds no {dtype} value (lo > hi after rounding lo up to {rlo!r} and hi down to {rhi!r})")
    return rlo, rhi


class _DeviceState:
    """flat state, chunk table and state block of the parameters that live on one device"""

    def __init__(self, device, params, ema=False):
        self.device = device
        # bf16 parameters first: the master array covers only them
        self.params = [pg for pg in params if pg[0].dtype == torch.bfloat16] + [pg for pg in params if pg[0].dtype != torch.bfloat16]
        self.offset, off, master_len = [], 0, 0
        for p, _ in self.params:
            self.offset.append(off)
            off += (p.numel() + _ALIGN_ELEMS - 1) // _ALIGN_ELEMS * _ALIGN_ELEMS
            if p.dtype == torch.bfloat16:
                master_len = off
        self.exp_avg = torch.zeros(max(off, 1), dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(max(off, 1), dtype=torch.float32, device=device)
        self.master = torch.zeros(master_len, dtype=torch.float32, device=device) if master_len else None
        self.ema = torch.zeros(max(off, 1), dtype=torch.float32, device=device) if ema else None      # (every parameter, fp32 ones too)
        self.block = torch.zeros(ops.OPTIM_BLOCK_WORDS, dtype=torch.int32, device=device)
        self.step_base = torch.full((max(len(self.params), 1),), -1, dtype=torch.int32, device=device)
        self.ratio = torch.ones(max(len(self.params), 1), dtype=torch.float32, device=device)   # trust ratio of the last applied step
        self.pairs = None                                       # (sum w^2, sum u^2) per chunk: allocated by the first `trust_ratio` step
        self.max_chunks = sum((p.numel() + ops.OPTIM_CHUNK - 1) // ops.OPTIM_CHUNK for p, _ in self.params)
        table_bytes = max(self.max_chunks, 1) * ops.OPTIM_CHUNK_BYTES
        # one buffer = the chunk table followed by the list of parameters without a gradient: one copy per rebuild
        self.upload = torch.zeros(table_bytes + 4 * max(len(self.params), 1), dtype=torch.uint8, device=device)
        self.table = self.upload[:table_bytes]
        self.absent = self.upload[table_bytes:].view(torch.int32)
        # a ring of pinned staging buffers, each with the event behind its last asynchronous copy: a rebuild waits on the host only if
        # the copy issued _STAGING rebuilds ago has not left its buffer yet (the host that far ahead of the device)
        self.staging = [torch.zeros(self.upload.numel(), dtype=torch.uint8, pin_memory=device.type == "cuda") for _ in range(_STAGING)]
        self.staged = [None] * _STAGING
        self.rebuilds = 0
        self.partials = torch.zeros(max(self.max_chunks, 1), dtype=torch.float32, device=device)
        self.signature = None
        self.n_chunks = self.n_absent = 0
        self.segments = []                                      # (first chunk, chunks, param group, parameter dtype, gradient dtype)
        self.norm_segments = []                                 # (first chunk, chunks, gradient dtype)
        self.acc = None                                         # accumulate_begin(): flat fp32 sum of gradients, laid out as exp_avg
        self.acc_grad = {}                                      # parameter index -> the `.grad` tensor accumulate_end() wrote last time

    def view(self, flat, i):
        p = self.params[i][0]
        return flat[self.offset[i]: self.offset[i] + p.numel()].view(p.shape)


class FusedAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay, `torch.optim.AdamW`'s formula and operation order) with optional clipping by the global gradient
    norm (`torch.nn.utils.clip_grad_norm_`'s formula), fused into HIP kernels that walk every parameter through a chunk table in device
    memory.  float32 and bfloat16 parameters; gradients float32 or bfloat16, wherever autograd or `GradSync.claim` put them.

    * bf16 parameters get an fp32 MASTER copy (initialised from the parameter: exact); the update is applied to the master and the parameter
      is written as its round-to-nearest-even bf16.  The moments are fp32 for every parameter.  fp32 parameters have no master.
    * `max_grad_norm`: gradients are scaled by min(1, max_grad_norm / (norm + 1e-6)) inside the update (`.grad` itself is NOT modified).
      The norm pass always runs: a non-finite norm (an inf / nan gradient anywhere) SKIPS the step on the device -- parameters, moments,
      masters and step counts stay bit-identical, `skipped_steps` goes up by one.
    * no host synchronisation: the norm, the clip factor, the skip decision and the step counts live in device memory.  `grad_norm`,
      `skipped_steps` and `step_count` are device tensors (views of that state); reading them is the caller's choice to pay for a sync.
    * hyper-parameters are kernel arguments read from `param_groups` at every step: LR schedulers work, nothing is uploaded for them.
    * the chunk table is rebuilt and uploaded (pinned staging buffer, asynchronous copy) only when a parameter's or gradient's address, or
      the set of parameters that have a gradient, differs from the previous step (`table_uploads` counts).  With `GradSync` the gradients
      are persistent slices: from the second step on nothing is uploaded.  Plain autograd with `zero_grad(set_to_none=True)` may hand
      out fresh gradient addresses every step: then every step rebuilds (host time) and uploads, through a ring of 4 pinned staging
      buffers -- the host waits only if it runs more than 4 rebuilt steps ahead of the device: that bounds the queue, it does not drain it.
    * parameters whose `.grad` is None are left alone and their own step count does not advance (torch semantics).
    * `ema_decay` (None: off -- no array, the launches and bits of an optimizer without the keyword): an exponential moving average of the
      weights, fp32, 4 bytes per parameter, updated INSIDE the update pass: ema += (1 - d)(w - ema) on the fp32 master (bf16 parameters) or
      the parameter (fp32) right after its update.  It is kept here because only the optimizer has what it needs: the unrounded weights (at
      d = 0.999 an EMA of the bf16 parameters moves by less than half an ulp per step and stalls), the skip decision (a skipped step leaves
      the EMA bit-identical) and the applied step count u behind `ema_warmup` (d = min(ema_decay, (1 + u) / (10 + u)), timm's ramp).
      Initialised to the weights (exact); parameters without a gradient are not averaged.  `state[p]["ema"]` is a view of the flat array;
      `with opt.ema_weights():` evaluates or checkpoints the model on the averaged weights.
    * param-group key `trust_ratio` (False; also a constructor default): LAMB as timm / apex state it -- the same moments, the update
      u = (m / bc1) / (sqrt(v / bc2) + eps) + weight_decay w (decay INSIDE the update), and w -= lr r u with r = |w| / |u| over the whole
      tensor (1 when either norm is 0), in fp32 on the master.  Two more launches per group: u's and w's sums of squares per chunk, and a
      fold by parameter into a flat device array; `state[p]["trust_ratio"]` is a view of its entry (the r of the last applied step, 1
      for parameters outside such a group).  Nothing is read back; a skipped step leaves the array alone.
    * param-group key `bounds` (None; (lo, hi), either end None; also a constructor default): lo <= w <= hi on the fp32 weight right
      after its update, before the EMA sees it and before the bf16 parameter is rounded from it.  It is here because a user's
      `p.data.clamp_()` on a bf16 model reaches only the rounded copy, which the next step overwrites from the unclamped master.  For
      a bf16 parameter lo is rounded up and hi down to bf16 once, so the parameter stays inside as well; lo > hi: ValueError.
      Both keys are read at every step as `lr` is, travel in `state_dict()` and are absent from the groups of an optimizer that does
      not use them.  A group with neither launches exactly the kernels it launched before they existed.
    * `accumulate_begin()` / `accumulate()` / `accumulate_end()` sum the gradients of several backward passes in a flat fp32 array
      (4 bytes per parameter, allocated at the first `accumulate_begin()`) and round the sum once into `.grad`; `step()` itself is
      unchanged and raises while a sum is open.  `x_clip_amd.cached.CachedContrastiveStep` is built on them.

    Streams: `step()` runs on the current stream.  The backward's side streams join the current stream before `backward()` returns; with
    `GradSync` call `sync.finish()` FIRST (it orders the current stream behind the all-reduces).  Distributed training needs nothing else:
    after `finish()` every rank holds the same averaged gradients, so the norm, the clip factor and the skip decision are identical on
    every rank without a collective.  All parameters of one norm live on one device: with parameters on several devices each device
    clips by (and skips on) the norm of its own parameters.

    `zero_grad()` (set_to_none=True, torch's default) is what `GradSync` wants: its weight-gradient kernels write straight into the
    persistent slice only while `.grad` is None, and the re-created `.grad` has the same address, so the table stays valid."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None, ema_warmup: bool = True,
                 trust_ratio: bool = False, bounds=None):
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"invalid eps: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"invalid weight_decay: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"invalid ema_decay: {ema_decay}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema_swapped = False                               # inside `with ema_weights():`
        self._accumulating = False                              # between accumulate_begin() and accumulate_end()
        self._accumulated = {}                                  # id(param) -> param: what accumulate() has taken a gradient from
        self._devs = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        # (off = the key is absent: the groups, and with them state_dict(), of an optimizer that uses neither are what they were)
        if trust_ratio:
            defaults["trust_ratio"] = True
        if bounds is not None:
            _group_bounds({"bounds": bounds}, torch.float32)    # (raises ValueError)
            defaults["bounds"] = tuple(bounds)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for dtype in {p.dtype for p in group["params"]} & set(_CODE):
                _group_bounds(group, dtype)                     # (raises ValueError)
        self.max_grad_norm = max_grad_norm
        self.table_uploads = 0                                  # chunk-table uploads so far (tests: none from the second GradSync step on)
        self._build()

    # ---- state ----
    def add_param_group(self, param_group):
        if self._devs is not None:
            raise NotImplementedError("x_clip_amd FusedAdamW: parameter groups are fixed at construction (the flat state is laid out once)")
        super().add_param_group(param_group)

    def _build(self):
        by_dev = {}
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.dtype not in _CODE:
                    raise TypeError(f"x_clip_amd FusedAdamW supports float32 and bfloat16 parameters, got {p.dtype}")
                if not p.is_contiguous():
                    raise RuntimeError("x_clip_amd FusedAdamW: parameters must be contiguous")
                ops._dev_check(p)
                if p.numel():
                    by_dev.setdefault(p.device, []).append((p, gi))
        self._devs = {dev: _DeviceState(dev, ps, self.ema_decay is not None) for dev, ps in by_dev.items()}
        self._where = {}                                        # id(param) -> (device state, index)
        with torch.no_grad():
            for D in self._devs.values():
                for i, (p, _) in enumerate(D.params):
                    self._where[id(p)] = (D, i)
                    st = self.state[p]
                    st["exp_avg"], st["exp_avg_sq"] = D.view(D.exp_avg, i), D.view(D.exp_avg_sq, i)
                    if p.dtype == torch.bfloat16:
                        st["master"] = D.view(D.master, i)
                        st["master"].copy_(p)                   # bf16 -> fp32: exact
                    if D.ema is not None:
                        st["ema"] = D.view(D.ema, i)
                        st["ema"].copy_(p)                      # (= the master of a bf16 parameter)
                    st["trust_ratio"] = D.ratio[i]              # (a view: written on the device by a `trust_ratio` group's steps, else 1)

    def _one(self) -> _DeviceState:
        if len(self._devs) != 1:
            raise RuntimeError("x_clip_amd FusedAdamW: grad_norm / skipped_steps / step_count are per device; this optimizer holds "
                               f"parameters on {len(self._devs)} devices")
        return next(iter(self._devs.values()))

    @property
    def grad_norm(self) -> torch.Tensor:
        """device scalar (fp32): the global gradient norm the last step() saw (before clipping; inf / nan when that step was skipped)"""
        return self._one().block[_BLK_NORM: _BLK_NORM + 1].view(torch.float32)[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """device scalar (int32): steps skipped because a gradient was not finite"""
        return self._one().block[_BLK_SKIPPED]

    @property
    def step_count(self) -> torch.Tensor:
        """device scalar (int32): steps applied (skipped ones not counted)"""
        return self._one().block[_BLK_STEP]

    # ---- the chunk table ----
    def _rebuild(self, D: _DeviceState, grads):
        recs, absent = [], []
        for i, ((p, gi), g) in enumerate(zip(D.params, grads)):
            if g is None:
                absent.append(i)
                continue
            if g.device != p.device:
                raise RuntimeError(f"x_clip_amd FusedAdamW: a gradient lives on {g.device}, its parameter on {p.device}")
            if g.is_sparse or g.dtype not in _CODE or g.shape != p.shape or not g.is_contiguous():
                raise RuntimeError("x_clip_amd FusedAdamW: gradients must be dense, contiguous, float32 or bfloat16 and of the parameter's shape "
                                   f"(got {g.dtype}, {tuple(g.shape)}, contiguous={g.is_contiguous()})")
            pc, gc = _CODE[p.dtype], _CODE[g.dtype]
            pe, ge, pp, gp = p.element_size(), g.element_size(), p.data_ptr(), g.data_ptr()
            for k, lo in enumerate(range(0, p.numel(), ops.OPTIM_CHUNK)):
                n = min(ops.OPTIM_CHUNK, p.numel() - lo)
                recs.append(((gi, pc, gc), (pp + lo * pe, gp + lo * ge, D.offset[i] + lo, n, pc | (gc << 8), i, int(k == 0), (0, 0))))
        recs.sort(key=lambda r: r[0])                           # (stable: parameters keep their order inside a segment)
        assert len(recs) <= D.max_chunks
        D.segments, D.norm_segments = [], []
        for c, (key, _) in enumerate(recs):
            if D.segments and tuple(D.segments[-1][2:]) == key:
                D.segments[-1][1] += 1
            else:
                D.segments.append([c, 1, *key])
            if D.norm_segments and D.norm_segments[-1][2] == key[2]:
                D.norm_segments[-1][1] += 1
            else:
                D.norm_segments.append([c, 1, key[2]])
        D.n_chunks, D.n_absent = len(recs), len(absent)
        slot = D.rebuilds % _STAGING
        D.rebuilds += 1
        if D.staged[slot] is not None:
            D.staged[slot].synchronize()                        # (the copy issued _STAGING rebuilds ago has left this buffer: normally long done)
        host = D.staging[slot].numpy()
        tb = D.table.numel()
        if recs:
            host[: len(recs) * ops.OPTIM_CHUNK_BYTES] = np.array([r[1] for r in recs], dtype=_TABLE_DTYPE).view(np.uint8)
        if absent:
            host[tb: tb + 4 * len(absent)] = np.array(absent, dtype=np.int32).view(np.uint8)
        D.upload.copy_(D.staging[slot], non_blocking=True)
        if D.device.type == "cuda":
            D.staged[slot] = torch.cuda.current_stream(D.device).record_event()
        self.table_uploads += 1

    def _sync_table(self, D: _DeviceState):
        """the chunk table describes the gradients the parameters hold right now (rebuilt and uploaded only when it does not)"""
        grads = [p.grad for p, _ in D.params]
        # (address, dtype AND layout: a strided or reshaped gradient swapped in at the same address must reach _rebuild's checks)
        signature = tuple((p.data_ptr(), None if g is None else (g.data_ptr(), g.dtype, g.shape == p.shape and g.is_contiguous()))
                          for (p, _), g in zip(D.params, grads))
        if signature != D.signature:
            self._rebuild(D, grads)
            D.signature = signature

    @torch.no_grad()
    def step(self, closure=None):
        if self._ema_swapped:
            raise RuntimeError("x_clip_amd FusedAdamW: step() inside `with ema_weights():` -- the parameters hold the averaged weights")
        if self._accumulating:
            raise RuntimeError("x_clip_amd FusedAdamW: step() between accumulate_begin() and accumulate_end() -- `.grad` holds one backward "
                               "pass, not the sum")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dt = {0: torch.float32, 1: torch.bfloat16}
        for D in self._devs.values():
            self._sync_table(D)
            if D.n_chunks == 0:
                continue
            ctx = torch.cuda.device(D.device) if D.device.type == "cuda" else _null()
            with ctx:
                for c0, n, gc in D.norm_segments:
                    ops.gradnorm_partial(D.table, c0, n, dt[gc], D.partials)
                ops.optim_prepare(D.partials, D.n_chunks, self.max_grad_norm, D.block, D.step_base, D.absent, D.n_absent)
                for c0, n, gi, pc, gc in D.segments:
                    g = self.param_groups[gi]
                    trust, (lo, hi) = bool(g.get("trust_ratio", False)), _group_bounds(g, dt[pc])
                    if trust or lo != -math.inf or hi != math.inf:
                        if trust:
                            if D.pairs is None:
                                D.pairs = torch.zeros(2 * max(D.max_chunks, 1), dtype=torch.float32, device=D.device)
                            ops.lamb_norm(D.table, c0, n, dt[pc], dt[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base,
                                          g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], D.pairs)
                            ops.lamb_fold(D.table, c0, n, D.pairs, D.block, D.ratio)
                        ops.optim_update(D.table, c0, n, dt[pc], dt[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base,
                                         g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], D.ratio if trust else None,
                                         lo, hi, D.ema, self.ema_decay or 0.0, self.ema_warmup)
                    elif D.ema is None:
                        ops.adamw_step(D.table, c0, n, dt[pc], dt[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base,
                                       g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
                    else:
                        ops.adamw_ema_step(D.table, c0, n, dt[pc], dt[gc], D.exp_avg, D.exp_avg_sq, D.master, D.block, D.step_base,
                                           g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], D.ema, self.ema_decay,
                                           self.ema_warmup)
        return loss

    # ---- gradients of several backward passes ----
    @torch.no_grad()
    def accumulate_begin(self):
        """Open a sum of gradients over several backward passes (x_clip_amd.cached.CachedContrastiveStep; plain gradient accumulation):

            opt.accumulate_begin()
            for micro in batch: loss(micro).backward(); opt.accumulate()
            opt.accumulate_end();  sync.finish();  opt.step();  opt.zero_grad()

        The sum lives in a flat fp32 array laid out as `exp_avg` (4 bytes per parameter, allocated at the first call, zeroed at every
        call): autograd's own `+=` into the `.grad` of a bf16 model rounds to an 8-bit mantissa after every pass.  Not part of
        `state_dict()`: it is empty between steps.  An optimizer that never calls this allocates and launches nothing for it."""
        if self._accumulating:
            raise RuntimeError("x_clip_amd FusedAdamW: accumulate_begin() twice without accumulate_end()")
        for D in self._devs.values():
            if D.acc is None:
                D.acc = torch.zeros_like(D.exp_avg)
            else:
                D.acc.zero_()
        self._accumulated = {}
        self._accumulating = True

    def _accumulate_launch(self, D: _DeviceState, materialise: bool):
        self._sync_table(D)
        if D.n_chunks == 0:
            return
        dt = {0: torch.float32, 1: torch.bfloat16}
        with (torch.cuda.device(D.device) if D.device.type == "cuda" else _null()):
            for c0, n, gc in D.norm_segments:
                ops.grad_accumulate(D.table, c0, n, dt[gc], D.acc, materialise)

    @torch.no_grad()
    def accumulate(self):
        """After a backward pass: every parameter's `.grad` (fp32 or bf16, wherever autograd or `GradSync.claim` put it) is added into
        its slice of the fp32 sum -- one launch per gradient dtype over the same chunk table `step()` walks -- and `.grad` is set to
        None, so that the next backward writes a fresh gradient (a `GradSync` slice is handed back to the sink and claimed again).
        Runs on the current stream; nothing is read back.  Parameters without a gradient in this pass are left alone."""
        if not self._accumulating:
            raise RuntimeError("x_clip_amd FusedAdamW: accumulate() outside accumulate_begin() ... accumulate_end()")
        from . import functional as XF
        sinks = [s for s in XF.grad_sinks() if hasattr(s, "release")]
        for D in self._devs.values():
            self._accumulate_launch(D, False)
            for p, _ in D.params:
                if p.grad is not None:
                    self._accumulated[id(p)] = p
                    p.grad = None
                    for sink in sinks:
                        sink.release(p)

    @torch.no_grad()
    def accumulate_end(self):
        """Close the sum: every parameter accumulate() took a gradient from gets a `.grad` of its own dtype holding the fp32 sum rounded
        to nearest even ONCE -- in its `GradSync` slice where the sink hands one out, otherwise in a tensor this optimizer keeps (from
        the second step on the addresses, and with them the chunk table, are stable).  Afterwards `sync.finish()`, clipping, the skip
        decision (a non-finite gradient in any pass is a non-finite sum) and `step()` run unchanged on `.grad`."""
        if not self._accumulating:
            raise RuntimeError("x_clip_amd FusedAdamW: accumulate_end() without accumulate_begin()")
        from . import functional as XF
        for D in self._devs.values():
            pending = [i for i, (p, _) in enumerate(D.params) if p.grad is not None]
            if pending:
                raise RuntimeError(f"x_clip_amd FusedAdamW: accumulate_end(): {len(pending)} parameter(s) hold a gradient that accumulate() has "
                                   "not taken -- call accumulate() after the last backward pass")
            for i, (p, _) in enumerate(D.params):
                if id(p) not in self._accumulated:
                    continue
                out = None
                for sink in XF.grad_sinks():
                    out = sink.claim(p, p.shape, p.dtype)
                    if out is not None:
                        break
                if out is None:
                    out = D.acc_grad.get(i)
                    if out is None or out.dtype != p.dtype or out.device != p.device:
                        out = D.acc_grad[i] = torch.empty_like(p, memory_format=torch.contiguous_format)
                p.grad = out
            self._accumulate_launch(D, True)
        self._accumulated = {}
        self._accumulating = False

    # ---- the averaged weights ----
    @contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): clip.eval(); ...; torch.save(clip.state_dict(), path)`: inside, every parameter holds its EMA (bf16
        parameters its round-to-nearest-even bf16; parameters never stepped hold their initial value, which is their EMA); on exit bf16
        parameters are rewritten from their masters (exact: a parameter always is its rounded master) and fp32 parameters from a stash
        taken on entry, so training goes on with the bits it had.  Plain copies on the current stream, in place: addresses do not change and
        the chunk table stays valid.  `step()` inside raises."""
        if self.ema_decay is None:
            raise RuntimeError("x_clip_amd FusedAdamW: ema_weights() needs an optimizer built with ema_decay")
        if self._ema_swapped:
            raise RuntimeError("x_clip_amd FusedAdamW: ema_weights() is already active")
        stash = []
        with torch.no_grad():
            for D in self._devs.values():
                for i, (p, _) in enumerate(D.params):
                    if p.dtype != torch.bfloat16:
                        stash.append((p, p.detach().clone()))
                    p.copy_(D.view(D.ema, i))
        self._ema_swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                for D in self._devs.values():
                    for i, (p, _) in enumerate(D.params):
                        if p.dtype == torch.bfloat16:
                            p.copy_(D.view(D.master, i))
                for p, saved in stash:
                    p.copy_(saved)
            self._ema_swapped = False

    # ---- checkpoints ----
    def state_dict(self):
        """`torch.optim.AdamW`'s layout (`step`, `exp_avg`, `exp_avg_sq` per parameter that has been stepped, fp32) plus `master` for bf16
        parameters, `ema` with `ema_decay` and, beside torch's two keys, `max_grad_norm`, `skipped_steps` (per device) and -- with `ema_decay`
        only: a dict of an optimizer without it is what it was -- `ema_decay` / `ema_warmup`.  Param groups carry `trust_ratio` / `bounds`
        where they have them, and the parameters of a `trust_ratio` group their last `trust_ratio`.  Copies (not views of the flat state);
        reads the step counts back: a checkpoint is a synchronisation point.  `register_state_dict_pre_hook` / `_post_hook` hooks run."""
        for hook in self._optimizer_state_dict_pre_hooks.values():
            hook(self)
        packed, index = [], {}
        for group in self.param_groups:
            g = {k: v for k, v in group.items() if k != "params"}
            g["params"] = []
            for p in group["params"]:
                index[id(p)] = len(index)
                g["params"].append(index[id(p)])
            packed.append(g)
        state = {}
        for D in self._devs.values():
            total = int(D.block[_BLK_STEP])
            base = D.step_base.tolist()
            for i, (p, _) in enumerate(D.params):
                if base[i] < 0:
                    continue                                    # never stepped: no state, as in torch
                st = {"step": torch.tensor(float(total - base[i])), "exp_avg": D.view(D.exp_avg, i).clone(),
                      "exp_avg_sq": D.view(D.exp_avg_sq, i).clone()}
                if p.dtype == torch.bfloat16:
                    st["master"] = D.view(D.master, i).clone()
                if D.ema is not None:
                    st["ema"] = D.view(D.ema, i).clone()
                if self.param_groups[D.params[i][1]].get("trust_ratio", False):
                    st["trust_ratio"] = D.ratio[i].clone()
                state[index[id(p)]] = st
        out = {"state": state, "param_groups": packed, "max_grad_norm": self.max_grad_norm,
               "skipped_steps": {str(D.device): int(D.block[_BLK_SKIPPED]) for D in self._devs.values()}}
        if self.ema_decay is not None:
            out["ema_decay"], out["ema_warmup"] = self.ema_decay, self.ema_warmup
        for hook in self._optimizer_state_dict_post_hooks.values():
            res = hook(self, out)
            out = out if res is None else res
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """accepts state_dict() of this class and of `torch.optim.AdamW` (no `master`: the masters are initialised from the parameters).
        Not the base class's: that one casts floating-point state to the PARAMETER's dtype, which would round the fp32 moments and masters
        of bf16 parameters to bf16.  Of a saved param group only lr / betas / eps / weight_decay and -- where the dict has them: a
        `torch.optim.AdamW` dict or an older one leaves this optimizer's -- trust_ratio / bounds are taken (torch's foreach, fused,
        capturable ... mean nothing here; amsgrad / maximize are refused); `skipped_steps` is restored when present.  With `ema_decay`:
        `ema` is restored where the dict has it and is otherwise the loaded master / parameter (a `torch.optim.AdamW` dict, a dict saved
        without EMA, a parameter never stepped); `ema_decay` / `ema_warmup` are taken from a dict that has them.  Without: a dict's EMA
        entries are ignored.
        `register_load_state_dict_pre_hook` / `_post_hook` hooks run."""
        for hook in self._optimizer_load_state_dict_pre_hooks.values():
            res = hook(self, state_dict)
            state_dict = state_dict if res is None else res
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        ids = dict(zip(chain.from_iterable(s["params"] for s in saved), chain.from_iterable(g["params"] for g in self.param_groups)))
        if any(s.get("amsgrad") or s.get("maximize") for s in saved):
            raise ValueError("x_clip_amd FusedAdamW has no amsgrad / maximize variant")
        for s, g in zip(saved, self.param_groups):
            g.update({k: s[k] for k in _GROUP_KEYS if k in s})
            if g.get("bounds") is not None:
                g["bounds"] = tuple(g["bounds"])
            for dtype in {p.dtype for p in g["params"]} & set(_CODE):
                _group_bounds(g, dtype)                         # (raises ValueError)
        if "max_grad_norm" in state_dict:
            self.max_grad_norm = state_dict["max_grad_norm"]
        if self.ema_decay is not None and state_dict.get("ema_decay") is not None:
            if not 0.0 <= state_dict["ema_decay"] < 1.0:
                raise ValueError(f"invalid ema_decay in the loaded state dict: {state_dict['ema_decay']}")
            self.ema_decay, self.ema_warmup = float(state_dict["ema_decay"]), bool(state_dict.get("ema_warmup", self.ema_warmup))
        loaded = {id(ids[k]): v for k, v in state_dict["state"].items()}
        for D in self._devs.values():
            steps = [int(float(loaded[id(p)]["step"])) if id(p) in loaded else None for p, _ in D.params]
            total = max([s for s in steps if s is not None], default=0)
            for i, (p, _) in enumerate(D.params):
                st = loaded.get(id(p))
                m, v = D.view(D.exp_avg, i), D.view(D.exp_avg_sq, i)
                if st is None:
                    m.zero_()
                    v.zero_()
                else:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                if p.dtype == torch.bfloat16:
                    D.view(D.master, i).copy_(st["master"] if st is not None and "master" in st else p)
                if D.ema is not None:
                    weight = D.view(D.master, i) if p.dtype == torch.bfloat16 else p
                    D.view(D.ema, i).copy_(st["ema"] if st is not None and "ema" in st else weight)
                D.ratio[i] = float(st["trust_ratio"]) if st is not None and "trust_ratio" in st else 1.0
            D.step_base.copy_(torch.tensor([-1 if s is None else total - s for s in steps] or [-1], dtype=torch.int32))
            D.block[_BLK_STEP] = total
            D.block[_BLK_SKIPPED] = int(state_dict.get("skipped_steps", {}).get(str(D.device), 0))
            D.signature = None
        for hook in self._optimizer_load_state_dict_post_hooks.values():
            hook(self)

    # ---- helpers ----
    @staticmethod
    def default_param_groups(model: torch.nn.Module, weight_decay: float = 1e-2, trust_ratio: bool = False, temperature_bounds=None):
        """two groups: weight matrices with `weight_decay`; everything with ndim < 2 (LayerNorm gains, biases, cls token, temperature,
        logit_bias) and the embedding tables without.  `trust_ratio=True`: the weight-matrix group carries it (LAMB), the other does not
        -- the usual exclusion.  `temperature_bounds=(lo, hi)`: `model.temperature` moves into a third group: no decay, no trust ratio,
        those bounds (CLIP's `logit_scale.clamp_(0, ln 100)`, applied to the fp32 master).  With the defaults: the two groups as ever."""
        tables = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Embedding)}
        temperature = None
        if temperature_bounds is not None:
            temperature = getattr(model, "temperature", None)
            if not isinstance(temperature, torch.nn.Parameter) or not temperature.requires_grad:
                raise ValueError("temperature_bounds: the model has no trainable parameter `temperature`")
        decay, plain = [], []
        for p in model.parameters():
            if p.requires_grad and p is not temperature:
                (plain if p.ndim < 2 or id(p) in tables else decay).append(p)
        groups = [{"params": decay, "weight_decay": weight_decay}, {"params": plain, "weight_decay": 0.0}]
        if trust_ratio:
            groups[0]["trust_ratio"] = True
            groups[1]["trust_ratio"] = False                    # (explicit: an optimizer built with trust_ratio=True leaves these alone too)
        if temperature is not None:
            groups.append({"params": [temperature], "weight_decay": 0.0, "trust_ratio": False, "bounds": tuple(temperature_bounds)})
        return groups


class _null:
    def __enter__(self): return None
    def __exit__(self, *exc): return False
