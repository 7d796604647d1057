"""xclip_gemm on ROW-STRIDED operands and outputs, shared by tests/test_gemm_strided_emu.py (CPU, wave64 emulator build of the kernel sources)
and tests/test_gemm_strided_gpu.py (MI355X, libxclip_hip.so).

xclip_gemm takes five independent leading dimensions (lda, ldb, ldc, ldr, ld_add) and the model uses them: the pooled-row view whose rows
are n D apart, the output written into enc[:, 0], S[:, :cols], the k-major P[:, : yc ni], weight slices W[inner:].  tests/kernel_cases.py
hands the library contiguous tensors only, so a kernel family that used N for ldc in one epilogue, stored a whole 16-byte line into the gap
behind a ragged row, or read the chunk behind a row's last element would pass it.  Here every operand is a view into a larger buffer:

  * row stride = natural width (the columns rounded up to the 16-byte chunk) + a gap; the five gaps of a table case differ, so that no two
    leading dimensions can be swapped unnoticed;
  * the view starts 2 chunks behind a margin of one whole view extent at the case's LARGEST leading dimension, and the same margin lies
    behind it: a kernel that takes the wrong one of the case's leading dimensions stays inside the allocation and fails an assertion;
  * input buffers are NaN outside the view -- except what include/xclip.h's pad contract asks for: columns [K, K rounded up) of a NORMAL
    operand hold zeros.  A k-major operand has NaN behind its row K - 1 and behind its M (or N) columns;
  * the output buffer holds a fixed finite bit pattern (in place: the residual buffer does, outside the residual view).

After the launch: (a) the view against the fp64 product, kernel_cases.close with case_gemm's arguments (element-wise 1 bf16 ulp / 2e-5 of the
scale); (b) the view bit-equal to the same call on tight copies of every operand into a fresh tight output, on the same route -- the plan
reads no leading dimension beyond the limits the route query sees, so anything but equal bits is an addressing bug; (c) every element of the
output buffer outside the view still holds the pattern; (d) every input buffer bit-identical to its copy from before the call.

Which family a table case lands in is asserted through xclip_gemm_route with the case's real lda / ldb, its terms and the workspace
ops.gemm offers.  The query tells routes, not the loops inside route 1: which of them a shape takes follows from launch_gemm2
(xclip_api.hip) and is stated per table below."""
import torch

import kernel_cases as K
from x_clip_amd import _lib, ops

PATTERN = 0x4B4B                      # bf16 0x4B4B = 1.33e7, fp32 0x4B4B4B4B = 1.33e7: finite, and nothing a product of unit Gaussians reaches
TERMS_ALL = ("bias", "addrows", "residual")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pattern(dtype):
    return PATTERN if dtype == torch.bfloat16 else (PATTERN << 16) | PATTERN


class Strided:
    """a [rows, cols] view, row stride ld, into a flat buffer on `dev`: margin (rows x max_ld elements) | 2 chunks | the view | margin.
    nan: the buffer is NaN (an input) or the bit pattern (an output) outside the view.  before: rows of a contiguous weight in front of the
    view instead of the margin (W[before:]: the offset is a whole number of rows)"""

    def __init__(self, dev, dtype, rows, cols, ld, max_ld, nan, before=None):
        v = ops.vec(dtype)
        assert ld % v == 0 and ld >= K._roundup(cols, v) and max_ld >= ld
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.off = rows * max_ld + 2 * v if before is None else before * ld
        self.buf = torch.empty(self.off + rows * ld + rows * max_ld, dtype=dtype, device=dev)
        if nan:
            self.buf.fill_(float("nan"))
        else:
            _bits(self.buf).fill_(_pattern(dtype))

    def view(self, cols=None, col0=0):
        return torch.as_strided(self.buf, (self.rows, self.cols if cols is None else cols), (self.ld, 1), self.off + col0)

    def put(self, data, zero_to=None):
        self.view().copy_(data)
        if zero_to is not None and zero_to > self.cols:
            self.view(zero_to - self.cols, self.cols).zero_()
        return self

    def tight(self):
        """the same operand at its natural leading dimension in an allocation of its own (the padding columns zero)"""
        t = torch.zeros(self.rows, K._roundup(self.cols, ops.vec(self.dtype)), dtype=self.dtype, device=self.buf.device)
        t[:, : self.cols].copy_(self.view())
        return t[:, : self.cols]

    def untouched_outside_view(self):
        """an output buffer: every element outside the view still holds the pattern"""
        b = self.buf.clone()
        _bits(torch.as_strided(b, (self.rows, self.cols), (self.ld, 1), self.off)).fill_(_pattern(self.dtype))
        return bool((_bits(b) == _pattern(self.dtype)).all())


def _route(a_k, b_k, M, N, K_, lda, ldb, terms, dtype):
    """xclip_gemm_route for the product as ops.gemm would launch it (its workspace offer: the plan's bytes unless a bias / gathered rows are there)"""
    L = _lib.lib()
    code = ops._DTYPES[dtype]
    rows_or_bias = "bias" in terms or "addrows" in terms
    wbytes = 0 if (rows_or_bias or (ops.BATCH_INVARIANT_GEMM and not a_k)) else int(L.xclip_gemm_workspace_bytes(M, N, K_, code))
    return int(L.xclip_gemm_route(int(a_k), int(b_k), M, N, K_, lda, ldb, int(rows_or_bias), int("residual" in terms), wbytes, code))


def _ref_device(dev, M, N, K_):
    """the fp64 product on the CPU; from 2^27 multiply-adds on, on the device the kernel runs on (a case stays within seconds)"""
    return dev if (torch.device(dev).type == "cuda" and M * N * K_ >= (1 << 27)) else torch.device("cpu")


def _blocked_fp32_check(name, got, A, B, alpha, res, rows=16384):
    """tests/test_kernels_gpu.py test_gemm_full_size_every_element_and_repeatable's reference and bar: an fp32-accumulated product of the same
    bf16 operands in row blocks on the device, every element, none off by more than 2 bf16 ulps of its block's scale"""
    worst = 0.0
    for r0 in range(0, got.shape[0], rows):
        ref = alpha * (A[r0: r0 + rows].float() @ B.float())
        if res is not None:
            ref = ref + res[r0: r0 + rows].float()
        scale = float(ref.abs().max())
        worst = max(worst, float((got[r0: r0 + rows].float() - ref.to(torch.bfloat16).float()).abs().max()) / (scale * 2.0 ** -8))
    K._record(name, torch.bfloat16, worst, 2.0, "bf16 ulp of the row block's scale")
    assert bool(torch.isfinite(got.float()).all()) and worst <= 2.0, (name, worst)


def case_gemm_strided(dev, dtype, layout, M, N, K_, *, gaps, terms=(), alpha=1.0, in_place=False, expect_route=None, small_limit=None,
                      distinct=True, b_rows_before=None, blocked_ref=False, contiguous_twin=True):
    """gaps = (lda, ldb, ldc, ldr, ld_add) gaps in elements; terms: any of 'bias', 'addrows', 'residual'; in_place: the output view IS the
    residual view (ldc = ldr = N + gaps[3]); expect_route: what xclip_gemm_route must say (None: only returned); small_limit: the
    xclip_gemm_small_limit for the case (0: the 256 x 256 kernels take what gemm_small.h would); b_rows_before: B is W[b_rows_before:] of a
    contiguous weight; blocked_ref: check (a) against the device's fp32 row blocks (the full-size test's bar) instead of fp64.  -> the route"""
    v = ops.vec(dtype)
    a_k, b_k = layout == "tn", layout in ("nn", "tn")
    terms = tuple(terms)
    assert set(terms) <= set(TERMS_ALL) and (not in_place or "residual" in terms)
    ga, gb, gc, gr, gadd = gaps
    assert all(g % v == 0 and g >= 0 for g in gaps) and (not distinct or len(set(gaps)) == 5), gaps
    Kp = K._roundup(K_, v)
    a_rows, a_cols = (K_, M) if a_k else (M, K_)
    b_rows, b_cols = (K_, N) if b_k else (N, K_)
    lda, ldb = K._roundup(a_cols, v) + ga, K._roundup(b_cols, v) + gb
    ldr, ld_add = N + gr, N + gadd
    ldc = ldr if in_place else N + gc
    max_ld = max(lda, ldb, ldc, ldr if "residual" in terms else 0, ld_add if "addrows" in terms else 0)
    name = f"gemm strided {layout} {M}x{N}x{K_}" + ("" if not terms else " in place" if in_place else " + residual" if terms == ("residual",) else " + terms")

    # asymmetric operands, case_gemm's seeds: a transposed / mirrored output cannot pass
    A = Strided(dev, dtype, a_rows, a_cols, lda, max_ld, True).put(K.rnd((a_rows, a_cols), dtype, 17).to(dev), None if a_k else Kp)
    B = Strided(dev, dtype, b_rows, b_cols, ldb, max_ld, True, before=b_rows_before).put(K.rnd((b_rows, b_cols), dtype, 18).to(dev), None if b_k else Kp)
    bias = Strided(dev, dtype, 1, N, N, max_ld, True).put(K.rnd((1, N), dtype, 19).to(dev)) if "bias" in terms else None
    R = Strided(dev, dtype, M, N, ldr, max_ld, not in_place).put(K.rnd((M, N), dtype, 20).to(dev)) if "residual" in terms else None
    rows5 = Strided(dev, dtype, 5, N, ld_add, max_ld, True).put(K.rnd((5, N), dtype, 21).to(dev)) if "addrows" in terms else None
    rowidx = (torch.arange(M) * 3 % 5).to(torch.int32).to(dev) if "addrows" in terms else None
    C = R if in_place else Strided(dev, dtype, M, N, ldc, max_ld, False)
    inputs = [t for t in (A, B, bias, rows5, None if in_place else R) if t is not None]
    before = [_bits(t.buf).clone() for t in inputs]
    res_before = None if R is None else R.view().clone()

    def run(a, b, out, res, add, bs):
        return ops.gemm(a, b, M, N, K_, a_k, b_k, alpha, None if bs is None else bs.view(N), res, add, rowidx, out=out)

    was = None if small_limit is None else ops.gemm_small_limit(small_limit)
    try:
        route = _route(a_k, b_k, M, N, K_, lda, ldb, terms, dtype)
        assert expect_route is None or route == expect_route, (name, "route", route, "expected", expect_route)
        twin = None
        if contiguous_twin:
            tA, tB = A.tight(), B.tight()
            assert _route(a_k, b_k, M, N, K_, tA.stride(0), tB.stride(0), terms, dtype) == route, name
            twin = run(tA, tB, None, None if R is None else res_before.clone(), None if rows5 is None else rows5.tight(),
                       None if bias is None else bias.tight())
        got = run(A.view(), B.view(), C.view(), None if R is None else R.view(), None if rows5 is None else rows5.view(),
                  None if bias is None else bias.view())
        assert got.data_ptr() == C.view().data_ptr()
    finally:
        if was is not None:
            ops.gemm_small_limit(was)

    # (d) no input was written, (c) nothing outside the output view was
    for t, b0 in zip(inputs, before):
        assert torch.equal(_bits(t.buf), b0), (name, "an input buffer changed")
    assert C.untouched_outside_view(), (name, "a store outside the output view")
    # (b) the same bits as the contiguous call
    if twin is not None:
        assert twin.is_contiguous() and torch.equal(_bits(C.view().contiguous()), _bits(twin)), (name, "differs from the call on contiguous operands")
    # (a) the product
    if blocked_ref:
        assert dtype == torch.bfloat16
        _blocked_fp32_check(name, C.view(), A.view().t() if a_k else A.view(), B.view() if b_k else B.view().t(), alpha, res_before)
        return route
    rdev = _ref_device(dev, M, N, K_)
    a64, b64 = A.view().to(rdev, torch.float64), B.view().to(rdev, torch.float64)
    r = alpha * ((a64.t() if a_k else a64) @ (b64 if b_k else b64.t()))
    scale = float(r.abs().max())
    if bias is not None:
        r = r + bias.view().to(rdev, torch.float64)
    if rows5 is not None:
        r = r + rows5.view().to(rdev, torch.float64)[rowidx.long().to(rdev)]
    if R is not None:
        r = r + res_before.to(rdev, torch.float64)
    K.close(C.view(), r, dtype, name, scale=max(scale, float(r.abs().max())))
    return route


# ---- the case table: (layout, M, N, K, kwargs), per route.  bf16 unless a dtype is given ------------------------------------------------
_G = dict(gaps=(24, 8, 40, 16, 56))               # five different gaps, each a multiple of the bf16 and the fp32 chunk


def _c(layout, M, N, K_, **kw):
    return (layout, M, N, K_, dict(_G, **kw))


# route 0, gemm_small.h: its descriptor extents are built from 63 ld + 64
SMALL = {
    **{f"{lay} 128x64x192 the ring wraps": _c(lay, 128, 64, 192, expect_route=0) for lay in ("nt", "nn", "tn")},
    **{f"{lay} 64x192x512": _c(lay, 64, 192, 512, expect_route=0) for lay in ("nt", "nn", "tn")},
    "nt 64x128x256 pooled-row A (rows 5 K + 8 apart)": _c("nt", 64, 128, 256, gaps=(4 * 256 + 8, 8, 40, 16, 56), expect_route=0),
    "nn 128x64x192 ldc = 3 N (enc[:, 0])": _c("nn", 128, 64, 192, gaps=(24, 8, 2 * 64, 16, 56), expect_route=0),
    "nt 128x128x256 + residual": _c("nt", 128, 128, 256, terms=("residual",), alpha=0.5, expect_route=0),
    "nn 128x128x256 in place": _c("nn", 128, 128, 256, terms=("residual",), alpha=0.5, in_place=True, expect_route=0),
    "tn 64x128x128 in place": _c("tn", 64, 128, 128, terms=("residual",), alpha=0.5, in_place=True, expect_route=0),
}

# route 1 under xclip_gemm_small_limit(0).  The loop inside the route follows from launch_gemm2: NT / NN -> the ring loop (gemm4.h gemm5_kernel)
# in its PLAIN / RES / TERMS epilogue, or its SLAB epilogue on a (tile, slice) grid + launch_splitk_reduce when the plan splits K (a plain
# product of fewer than 129 tiles and K >= 512); TN -> the two-stage loop (gemm4_kernel), split-K on a 1-D placed grid (g2_where) + reduce
BIG = {
    **{f"{lay} 264x136x128 ring PLAIN, ragged tiles": _c(lay, 264, 136, 128, expect_route=1, small_limit=0) for lay in ("nt", "nn")},
    "nt 512x512x128 ring PLAIN, interior tiles": _c("nt", 512, 512, 128, expect_route=1, small_limit=0),
    "nt 512x512x128 ring RES in place": _c("nt", 512, 512, 128, terms=("residual",), in_place=True, expect_route=1, small_limit=0),
    "nn 264x136x64 ring RES, ragged tiles": _c("nn", 264, 136, 64, terms=("residual",), alpha=0.5, expect_route=1, small_limit=0),
    "nt 264x136x64 ring TERMS": _c("nt", 264, 136, 64, terms=TERMS_ALL, alpha=0.5, expect_route=1, small_limit=0),
    "nt 776x264x64 ring TERMS, persistent": _c("nt", 776, 264, 64, terms=TERMS_ALL, alpha=0.5, expect_route=1, small_limit=0),
    "nt 264x4096x64 ring PLAIN, banded order": _c("nt", 264, 4096, 64, expect_route=1, small_limit=0),
    # 8 / 16 interior tiles and >= G8_MIN_KSTEPS K steps, but gemm2_splits cuts K in 2 / 4 for so few tiles (g8_takes: splits == 1): the ring
    # loop's SLAB epilogue on the 2-D grid + the reduction
    "nt 1024x512x512 ring SLAB x 2 + reduce": _c("nt", 1024, 512, 512, expect_route=1, small_limit=0),
    "nn 1024x512x512 ring SLAB x 2 + reduce": _c("nn", 1024, 512, 512, expect_route=1, small_limit=0),
    "nn 2048x512x1024 ring SLAB x 4 + reduce": _c("nn", 2048, 512, 1024, expect_route=1, small_limit=0),
    "tn 520x264x192 two-stage PLAIN": _c("tn", 520, 264, 192, expect_route=1, small_limit=0),
    "tn 512x256x1024 two-stage SLAB, placed grid + reduce": _c("tn", 512, 256, 1024, expect_route=1, small_limit=0),
    "tn 128x136x1024 two-stage SLAB, ragged tile": _c("tn", 128, 136, 1024, expect_route=1, small_limit=0),
}

# route 1, the products g8_takes gives to gemm8.h's hand-scheduled body on the MI355X (the emulator has no twin of an asm unit and runs
# them on the ring loop): plain, alpha 1, interior tiles, >= G8_MIN_KSTEPS K steps, ONE K slice -- which gemm2_splits leaves to outputs of
# more than 128 tiles -- and a grid that is a multiple of 8: 17 x 8 = 136 tiles (one each), 17 x 16 = 272 tiles on 256 work-groups (16 of
# them walk a second tile: the held line stores under the next tile's MFMAs; banded order).  The route query cannot tell the two loops apart
GEMM8 = {
    "nt 4352x2048x512": _c("nt", 4352, 2048, 512, expect_route=1),
    "nn 4352x2048x512": _c("nn", 4352, 2048, 512, expect_route=1),
    "nn 4352x4096x512 272 tiles": _c("nn", 4352, 4096, 512, expect_route=1),
}

# route 3, gemm.h
GENERIC = {
    **{f"fp32 {lay} 136x72x96": _c(lay, 136, 72, 96, dtype=torch.float32, expect_route=3) for lay in ("nt", "nn", "tn")},
    **{f"{lay} 136x72x100 the pad contract": _c(lay, 136, 72, 100, expect_route=3) for lay in ("nt", "nn", "tn")},
    **{f"{lay} 133x136x64 M = 133": _c(lay, 133, 136, 64, expect_route=3) for lay in ("nt", "tn")},
    "nn 136x72x96 N = 72": _c("nn", 136, 72, 96, expect_route=3),
    "nt 40x136x64 all terms": _c("nt", 40, 136, 64, terms=TERMS_ALL, alpha=0.5, expect_route=3),
    "fp32 nt 40x136x64 all terms": _c("nt", 40, 136, 64, dtype=torch.float32, terms=TERMS_ALL, alpha=0.5, expect_route=3),
    "tn 64x64x1536 split-K + reduce": _c("tn", 64, 64, 1536, expect_route=3, small_limit=0),
    "fp32 tn 64x64x1536 split-K + reduce": _c("tn", 64, 64, 1536, dtype=torch.float32, expect_route=3),
    "nt 136x72x96 B = W[64:]": _c("nt", 136, 72, 96, gaps=(24, 0, 40, 16, 56), b_rows_before=64, expect_route=3),
}

# route 2, the row tail cut (xclip_gemm computes A + main_rows lda 2, C + main_rows ldc 2, residual + main_rows ldr 2 by hand).  On the
# MI355X: 130 row tiles x 2 = 260 tiles on 256 CUs = one round + 4 tail tiles; on the emulator told it has 4 CUs (XCLIP_EMU_CUS=4, its own
# interpreter): 5 row tiles x 2 = 2 rounds + 2 tiles
TAIL_GPU = {
    f"{lay} 33280x512x1024{' in place' if res else ''}": _c(lay, 33280, 512, 1024, expect_route=2, blocked_ref=True,
                                                            **(dict(terms=("residual",), alpha=0.5, in_place=True) if res else {}))
    for lay in ("nt", "nn") for res in (False, True)
}
# (small_limit=0: at 24 / 32 K steps and 2 - 3 GFLOP gemm_small.h would take these shapes whole -- route 0, nothing cut)
TAIL_EMU = [_c("nt", 1280, 512, 1536, expect_route=2, small_limit=0),
            _c("nn", 1280, 512, 2048, terms=("residual",), alpha=0.5, in_place=True, expect_route=2, small_limit=0),
            _c("nt", 1280, 512, 2048, terms=("residual",), alpha=0.5, expect_route=2, small_limit=0)]


def run_case(dev, case):
    layout, M, N, K_, kw = case
    kw = dict(kw)
    return case_gemm_strided(dev, kw.pop("dtype", torch.bfloat16), layout, M, N, K_, **kw)


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------------
# Route 0 is rare under case_gemm_fuzz's draws of M and N (both must be multiples of 64, no bias, at most 32 K steps: 2 - 3 of 48 cases on
# average), so the seed is the first one (of 1, 2, ...) whose 48-case list takes each of the routes 0, 1 and 3 at least 6 times -- a
# property of the host's plan alone (fuzz_routes), chosen before any kernel ran the list
FUZZ_SEED = 204
EMU_CAPS = dict(max_m8=40, max_tiles=2, max_ksteps=8, max_ksteps_tn=24)      # the emulator's sizes: M, N <= 512, K <= 512 (TN: 1536)


def fuzz_cases(cases, seed, max_m8=200, max_tiles=6, max_ksteps=40, max_ksteps_tn=300):
    """the sweep's case list (host only: shapes, layouts, terms, gaps): layout, M and N as kernel_cases.case_gemm_fuzz draws them (multiples
    of 8 from 128 up, one in four a whole number of 256-tiles), K a multiple of 64 (TN: a long contraction) with one case in five ragged,
    terms none / residual / all three, alpha, each of the five gaps from {0, chunk, 3 chunks, the natural width}.  The emulator passes smaller caps"""
    g = torch.Generator().manual_seed(seed)
    v = ops.vec(torch.bfloat16)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    out = []
    for _ in range(cases):
        lay = ["nt", "nn", "tn"][ri(0, 2)]
        M = 8 * ri(16, max_m8) if ri(0, 3) else 256 * ri(1, max_tiles)
        N = 8 * ri(16, max_m8) if ri(0, 3) else 256 * ri(1, max_tiles)
        K_ = 64 * ri(1, max_ksteps) if lay != "tn" else 64 * ri(4, max_ksteps_tn)
        if ri(0, 4) == 0:
            K_ -= ri(1, 63)
        terms = [(), (), ("residual",), TERMS_ALL][ri(0, 3)]
        alpha = [1.0, 0.5, 0.125][ri(0, 2)]
        a_cols, b_cols = (M if lay == "tn" else K_), (K_ if lay == "nt" else N)
        nat = [K._roundup(a_cols, v), K._roundup(b_cols, v), N, N, N]
        gaps = tuple([0, v, 3 * v, nat[i]][ri(0, 3)] for i in range(5))
        out.append((lay, M, N, K_, dict(gaps=gaps, terms=terms, alpha=alpha, in_place=bool(terms) and ri(0, 2) == 0, distinct=False, contiguous_twin=False)))
    return out


def fuzz_routes(cases, seed, **caps):
    """route -> how many cases of the list take it (host query only)"""
    counts = {}
    for lay, M, N, K_, kw in fuzz_cases(cases, seed, **caps):
        v = ops.vec(torch.bfloat16)
        lda = K._roundup(M if lay == "tn" else K_, v) + kw["gaps"][0]
        ldb = K._roundup(K_ if lay == "nt" else N, v) + kw["gaps"][1]
        r = _route(lay == "tn", lay in ("nn", "tn"), M, N, K_, lda, ldb, kw["terms"], torch.bfloat16)
        counts[r] = counts.get(r, 0) + 1
    return counts


def case_gemm_strided_fuzz(dev, cases, seed, **caps):
    """every case of fuzz_cases through checks (a), (c) and (d); none is dropped.  -> route -> count.
    With FUZZ_SEED the 48 cases of the MI355X list take: see tests/test_gemm_strided_gpu.py"""
    counts = {}
    for case in fuzz_cases(cases, seed, **caps):
        r = run_case(dev, case)
        counts[r] = counts.get(r, 0) + 1
    assert sum(counts.values()) == cases
    return counts
