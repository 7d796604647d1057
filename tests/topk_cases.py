"""Shared cases of the fused similarity top-k (x_clip_amd.retrieval, ops.simtopk*, csrc/kernels/simtopk.h): the CPU suite runs them on
the wave64 emulator (tests/test_topk_emu.py), the GPU suite on the MI355X (tests/test_topk_gpu.py).  The reference is plain dense
torch in fp64 on the dtype-rounded inputs, ordered by a STABLE sort of (-value, column): torch.topk promises no order among ties.

Exact cases: entries from {-3 .. 3} / 8 and d <= 128 make every dot product exact in fp32 in any summation order; the one rounding left
is the product with the scale, which IEEE fixes (metrics_cases).  Ties are frequent by construction, so every row pins the
lowest-column-first rule; values and indices must equal the reference bit for bit.
Realistic cases: normalised Gaussian latents inside the project's fp32 accumulation bound
    eps_i = d 2^-24 c |q_i| max_j |k_j| + 2^-23 max_j |S_ij|
(the second term with the row's largest logit: a top-k value is any of the row's logits, not its positive).  Every row is band-checked;
a row is DETERMINATE when all k gaps between neighbours among its first k + 1 fp64 logits exceed 2 eps -- then no admissible rounding can
swap two of them and the index list must equal the reference's.  At most 10 % of the rows may be indeterminate: a condition on the
inputs (the reference alone: 0 - 3.3 % at k = 10, none at k = 1, for these shapes and seed 9)."""
import math

import pytest
import torch

import metrics_cases as MC
from x_clip_amd import ops

NEG32 = float(torch.tensor(-3.0e38, dtype=torch.float32))
KS = (1, 3, 10, 32)


def poison(dev, nq, slots, k):
    """0x7f.. into the scratch the next call will use, and into freshly freed blocks of the sizes its outputs and temporaries have"""
    ws = ops.workspace(dev, 5 * slots * nq * 4)
    if ws is not None:
        ws.fill_(0x7F)
    junk = [torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev), torch.full((nq, k), 0x7F7F7F7F, dtype=torch.int32, device=dev)]
    junk += [torch.full((nq,), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    del junk


def run(dev, q, chunks, k, scale, log_scale=None):
    """-> values, indices, candidates (the set bits of every row's masks)"""
    poison(dev, q.shape[0], sum((c.shape[0] + 63) // 64 for c, _ in chunks), k)
    return ops.simtopk_chunked(q, chunks, k, scale, log_scale=log_scale, debug=True)


def dense_order(S):
    """S [nq, ng] (compared as given) -> every row's columns by (value descending, column ascending)"""
    return torch.sort(-S, dim=1, stable=True).indices


def dense_topk(S, order, k):
    """-> values [nq, k] (S's dtype), indices [nq, k] int64, padded with NEG32 / -1 beyond the gallery"""
    nq, ng = S.shape
    idx = order[:, :k]
    val = torch.gather(S, 1, idx)
    if ng < k:
        idx = torch.cat([idx, torch.full((nq, k - ng), -1, dtype=idx.dtype, device=S.device)], 1)
        val = torch.cat([val, torch.full((nq, k - ng), NEG32, dtype=S.dtype, device=S.device)], 1)
    return val, idx


def check_exact(got, S, order, k, tag):
    val, idx, cand = got
    r_val, r_idx = dense_topk(S, order, k)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (S.shape[0], k)
    assert bool((cand.long() >= min(k, S.shape[1])).all()), (tag, "a row's masks hold fewer than min(k, ng) candidates", int(cand.min()))
    assert torch.equal(idx.long(), r_idx), (tag, "indices", int((idx.long() != r_idx).sum()))
    assert torch.equal(val, r_val.float()), (tag, "values", int((val != r_val.float()).sum()))


def case_exact(dev, dtype, nq, ng, d, ks=KS, splits=None, repeats=0, seed=3):
    """both scale variants of one shape at every k; `splits`: the gallery also fed as chunks cut at these columns, forwards and
    backwards (bit-equal to the one-chunk call); `repeats`: that many further launches must return identical bits"""
    assert d <= 128
    q, g = MC.exact_inputs(nq, ng, d, dtype, seed)
    q, g = q.to(dev), g.to(dev)
    dots = q.double() @ g.double().t()                               # exact, and exact in fp32
    assert torch.equal(dots.float().double(), dots)
    tau = torch.tensor([0.7], dtype=torch.float32, device=dev)
    c32 = MC.device_scale(dev, dtype, 1.0, tau)                      # the device's own exp(tau) bits (metrics_cases.device_scale)
    assert abs(float(c32) - math.exp(0.7)) < 1e-5
    one = None
    for scale, ls, S in ((4.0, None, dots.float() * 4.0), (1.0, tau, dots.float() * c32)):
        order = dense_order(S)
        for k in ks:
            one = run(dev, q, [(g, 0)], k, scale, ls)
            check_exact(one, S, order, k, (nq, ng, d, k, "pow2" if ls is None else "tau"))
    k = ks[-1]                                                       # (`one`: the tau variant at the last k)
    if splits:
        cuts = [0, *splits, ng]
        chunks = [(g[a:b].contiguous(), a) for a, b in zip(cuts[:-1], cuts[1:])]
        for kk in ks:
            whole = one if kk == k else run(dev, q, [(g, 0)], kk, 1.0, tau)
            for lst in (chunks, chunks[::-1]):
                gc = run(dev, q, lst, kk, 1.0, tau)
                assert bool((gc[2].long() >= min(kk, ng)).all())
                for a, b in zip(whole[:2], gc[:2]):                  # (the candidate counts follow the slots, i.e. the cuts)
                    assert torch.equal(a, b), (nq, ng, d, kk, "chunked != one chunk")
    for _ in range(repeats):
        again = run(dev, q, [(g, 0)], k, 1.0, tau)
        for a, b in zip(one, again):
            assert torch.equal(a, b), (nq, ng, d, "not reproducible")


def case_all_equal_gallery(dev, dtype, nq=256, ng=512, d=64, k=10):
    """every gallery row the same: all logits of a row are equal, every column is a candidate (the finish kernel's worst case: the
    whole row) and the lowest-column rule alone decides -- indices 0 .. k - 1 in every row"""
    q, g = MC.exact_inputs(nq, 1, d, dtype, 4)
    q, g = q.to(dev), g.expand(ng, d).contiguous().to(dev)
    val, idx, cand = run(dev, q, [(g, 0)], k, 4.0)
    assert bool((cand == ng).all())
    assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device=dev).expand(nq, k))
    ref = ((q.double() @ g[0].double()).float() * 4.0)[:, None].expand(nq, k)
    assert torch.equal(val, ref)


def case_nan_row(dev, nq=512, ng=768, d=64, bad=300, k=10):
    """diverged latents: a row of NaN has no scorable column -- all -1 / SIM_NEG, never a garbage column -- and every other row is untouched"""
    q, g = MC.exact_inputs(nq, ng, d, torch.bfloat16, 5)
    q, g = q.to(dev), g.to(dev)
    clean = run(dev, q, [(g, 0)], k, 4.0)
    q2 = q.clone()
    q2[bad] = float("nan")
    val, idx, cand = run(dev, q2, [(g, 0)], k, 4.0)
    assert bool((idx[bad] == -1).all()) and bool((val[bad] == NEG32).all()) and int(cand[bad]) == 0
    keep = torch.arange(nq, device=dev) != bad
    for a, b in zip(clean, (val, idx, cand)):
        assert torch.equal(a[keep], b[keep])


def case_empty(dev, dtype, monkeypatch):
    """no gallery, or no queries: the neutral result, and nothing is launched"""
    from x_clip_amd import _lib

    def boom(*a, **k):
        raise AssertionError("an empty problem reached the library")

    monkeypatch.setattr(_lib, "lib", boom)
    q = torch.zeros(5, 8, dtype=dtype, device=dev)
    for chunks in ([(q[:0], 0)], [], [(q[:0], 0), (q[:0], 0)]):
        val, idx = ops.simtopk_chunked(q, chunks, 3, 1.0)
        assert val.shape == idx.shape == (5, 3) and bool((idx == -1).all()) and bool((val == NEG32).all())
    val, idx = ops.simtopk(q[:0], q, 3, 1.0)
    assert val.shape == idx.shape == (0, 3) and val.dtype == torch.float32 and idx.dtype == torch.int32


EXACT_GENERAL = [(5, 7, 8), (70, 130, 40)]                            # fp32 and bf16; (5, 7, 8): k > ng pins the padding
EXACT_RING = [(128, 128, 64, None), (256, 256, 64, None), (512, 768, 128, None), (520, 777, 64, (256, 520))]   # bf16: (nq, ng, d, splits)


# ---- realistic latents ---------------------------------------------------------------------------------------------------------------
def check_band(val, idx, S, eps, k, tag):
    """every row of (val, idx) against the fp64 logits S inside the accumulation band eps [nq]; -> the fraction of indeterminate rows
    (the determinate ones must carry the reference's index list)"""
    nq, ng = S.shape
    assert k <= ng
    order = dense_order(S)
    r_val, r_idx = dense_topk(S, order, k + 1 if ng > k else k)
    e = eps[:, None]
    idx = idx.long()
    v = val.double()
    assert bool(((idx >= 0) & (idx < ng)).all()), (tag, "index out of range")
    assert bool((v[:, 1:] <= v[:, :-1]).all()), (tag, "values increase")
    srt = idx.sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), (tag, "a column twice")
    err_rank = ((v - r_val[:, :k]).abs() / e).max()
    err_own = ((v - torch.gather(S, 1, idx)).abs() / e).max()
    print(f"simtopk {tag}: max |value - r-th fp64 logit| / eps {float(err_rank):.3f}, max |value - S64[index]| / eps {float(err_own):.3f}")
    assert float(err_rank) <= 1.0, (tag, float(err_rank))
    assert float(err_own) <= 1.0, (tag, float(err_own))
    vk = r_val[:, k - 1: k]
    must = S > vk + 2 * e                                            # every such column is returned
    got = torch.zeros_like(must)
    got.scatter_(1, idx, True)
    assert bool((got | ~must).all()), (tag, "a column above v_k + 2 eps is missing", int((must & ~got).sum()))
    assert bool((torch.gather(S, 1, idx) >= vk - 2 * e).all()), (tag, "a returned column lies below v_k - 2 eps")
    gaps = r_val[:, :-1] - r_val[:, 1:]                              # k gaps among the first k + 1 (k - 1 when the gallery ends at k)
    det = (gaps > 2 * e).all(1)
    assert torch.equal(idx[det], r_idx[:, :k][det]), (tag, "a determinate row differs from the reference", int((idx[det] != r_idx[:, :k][det]).any(1).sum()))
    return 1.0 - float(det.double().mean())


def band_eps(q, g, S, c64):
    d = q.shape[1]
    return d * 2.0 ** -24 * c64 * q.double().norm(dim=1) * g.double().norm(dim=1).max() + 2.0 ** -23 * S.abs().max(1).values


def case_realistic(dev, dtype, nq, ng, d, c, ks=(1, 10), seed=9):
    gen = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=gen), dim=1).to(dtype).to(dev)
    g = torch.nn.functional.normalize(torch.randn(ng, d, generator=gen), dim=1).to(dtype).to(dev)
    tau = torch.tensor([math.log(c)], dtype=torch.float32, device=dev)
    c64 = math.exp(float(tau))
    S = c64 * (q.double() @ g.double().t())
    eps = band_eps(q, g, S, c64)
    for k in ks:
        val, idx, cand = run(dev, q, [(g, 0)], k, 1.0, tau)
        assert bool((cand.long() >= k).all())
        tag = f"realistic {nq} x {ng} x {d} c {c} k {k} {dtype}"
        amb = check_band(val, idx, S, eps, k, tag)
        print(f"simtopk {tag}: indeterminate rows {amb:.4f}, candidates per row mean {float(cand.double().mean()):.1f} max {int(cand.max())}")
        assert amb <= 0.10, amb


REALISTIC = [(70, 130, 40, 14.3), (300, 700, 128, 14.3), (520, 777, 64, 100.0), (384, 4160, 64, 14.3)]


# ---- public interface --------------------------------------------------------------------------------------------------------------
def case_embed_matches_forward(dev, dtype):
    """eval(): the one-tower entry points are the two halves of forward(..., return_latents=True), bit for bit; similarity_topk on those
    latents inside the band, both directions"""
    from x_clip_amd import similarity_topk
    model, text, image = MC.small_clip(dev, dtype)
    model.eval()
    with torch.no_grad():
        tl, il = model(text, image, return_latents=True)
    et, ei = model.embed_text(text), model.embed_image(image)
    assert not et.requires_grad and not ei.requires_grad
    assert torch.equal(et, tl) and torch.equal(ei, il)
    tau = model.temperature.detach().float()
    c64 = math.exp(float(tau))
    for a, b, name in ((et, ei, "t2i"), (ei, et, "i2t")):
        S = c64 * (a.double() @ b.double().t())
        for k in (1, 5):
            val, idx = similarity_topk(a, b, k, model.temperature)
            assert val.shape == idx.shape == (a.shape[0], k) and val.dtype == torch.float32 and idx.dtype == torch.int32
            check_band(val, idx, S, band_eps(a, b, S, c64), k, f"public {name} k {k} {dtype}")
    # a gallery given as chunks, in any order: the same band (bit-equality across cuts is promised for exact logits only: case_exact)
    S = c64 * (et.double() @ ei.double().t())
    val, idx = similarity_topk(et, [(ei[7:], 7), (ei[:7], 0)], 5, model.temperature)
    check_band(val, idx, S, band_eps(et, ei, S, c64), 5, f"public t2i k 5 {dtype}, gallery in two chunks, reversed")
    with pytest.raises(ValueError, match="same d"):
        similarity_topk(et, ei[:, :-8], 5, model.temperature)
    with pytest.raises(ValueError, match=r"queries must be \[nq, d\]"):
        similarity_topk(et[0], ei, 5, model.temperature)
    with pytest.raises(TypeError, match="queries are"):
        similarity_topk(et, ei.to(torch.bfloat16 if dtype == torch.float32 else torch.float32), 5, model.temperature)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k must lie in 1 .. 32"):
            similarity_topk(et, ei, bad, model.temperature)


def proto_bar(ref, dtype):
    """DESIGN.md section 7, per-kernel bars: fp32 1e-5; bf16 2 ulps of the output scale (below the 1e-2 a unit-scale output would allow)"""
    if dtype == torch.float32:
        return 1e-5
    return min(1e-2, 2 * 2.0 ** (math.floor(math.log2(float(ref.abs().max()))) - 7))


def case_zero_shot(dev, dtype, C=5, P=3):
    from x_clip_amd import similarity_topk, zero_shot_classifier
    model, text, image = MC.small_clip(dev, dtype, batch=C * P)
    model.eval()
    prompts = text.view(C, P, -1)

    def ref_of(lat):
        return torch.nn.functional.normalize(lat.double().view(-1, P, lat.shape[-1]).mean(1), dim=1)

    protos = zero_shot_classifier(model, prompts)
    assert protos.shape == (C, model.to_text_latent.weight.shape[0]) and protos.dtype == dtype and not protos.requires_grad
    ref = ref_of(model.embed_text(text))
    err = float((protos.double() - ref).abs().max())
    print(f"zero_shot_classifier {dtype}: max |prototype - fp64| {err:.3e} (bar {proto_bar(ref, dtype):.3e})")
    assert err <= proto_bar(ref, dtype), err
    # in slices of two classes: against the latents of the same slices
    sliced = zero_shot_classifier(model, prompts, batch=2 * P)
    ref2 = torch.cat([ref_of(model.embed_text(prompts[c: c + 2].reshape(-1, prompts.shape[-1]))) for c in range(0, C, 2)])
    assert float((sliced.double() - ref2).abs().max()) <= proto_bar(ref2, dtype)
    # zero-shot top-1
    x = model.embed_image(image)
    val, idx = similarity_topk(x, protos, 1, model.temperature)
    c64 = math.exp(float(model.temperature.detach().float()))
    S = c64 * (x.double() @ protos.double().t())
    check_band(val, idx, S, band_eps(x, protos, S, c64), 1, f"zero-shot top-1 {dtype}")


def case_fine_grained_head_raises(dev, dtype):
    model, text, image = MC.small_clip(dev, dtype, batch=4, use_all_token_embeds=True)
    with pytest.raises(NotImplementedError, match="no single latent"):
        model.embed_text(text)
    with pytest.raises(NotImplementedError, match="no single latent"):
        model.embed_image(image)
