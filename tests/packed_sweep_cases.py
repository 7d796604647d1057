"""Cases that walk the packed text tower's kernels through every launch they can be given: every size of the varlen attention launch, every
branch of the packed embedding, cat_layouts, and one end-to-end step at a mid-range launch size.  Built on tests/packed_cases.py (its launch,
fp64 reference and bars, unchanged); tests/test_packed_sweep_gpu.py runs them on an MI355X, tests/test_packed_sweep_emu.py a thinned subset
on the CPU emulator build.  Everything the two test files parametrise from lives here."""
import os
import re

import pytest
import torch

import kernel_cases as K
from packed_cases import (BF16, F32, GUARD, LENS_A, LENS_B, _bits, _poison, case_varlen_attention, case_vs_oracle, embed_tokens)
from x_clip_amd import _lib, ops, text_layout


# ---- every launch size of the varlen kernels ----------------------------------------------------------------------------------------------
# The head-resident launch is sized by max_len (waves, LDS carve), and a unit of n <= max_len rows runs inside it: surplus waves, a tail merge
# over more partials than the unit alone would have, a single-tail seed in a wave that owns no query block.  max_len is whatever the longest
# sample of a batch happens to be, so the lists below walk it through every wave count and both sides of every cooperative-tail dip.
#
# A Python twin of the launch geometry in x_clip_amd/csrc/kernels/attention3.h (A3_MAX_N, A3_TAIL_MAX, a3_coop_tail, a3_waves, a3_single_tail,
# A3_BWD_WAVES, a3_bwd_waves), which attention_varlen.h sizes its launches with: the lists are held to what they claim to cover
# (sweep_coverage), and the constants to the header's (case_geometry_twin).
A3_MAX_N, A3_TAIL_MAX, A3_BWD_WAVES = 288, 2, 4


def a3_coop_tail(n):
    return (n & 31) != 0 and (n & 31) <= A3_TAIL_MAX and n >= 64


def a3_waves(n):
    return n // 32 if a3_coop_tail(n) else (n + 31) // 32


def a3_single_tail(n):
    return a3_coop_tail(n) and (n & 31) == 1


def a3_bwd_waves(n):
    return min(a3_waves(n), A3_BWD_WAVES)


def _csrc(*parts):
    import x_clip_amd
    return os.path.join(os.path.dirname(os.path.abspath(x_clip_amd.__file__)), "csrc", *parts)


def case_geometry_twin():
    """host only: the twin's constants are the header's, and the expressions it copies still stand there"""
    src = open(_csrc("kernels", "attention3.h")).read()
    for name, val in (("A3_MAX_N", A3_MAX_N), ("A3_TAIL_MAX", A3_TAIL_MAX), ("A3_BWD_WAVES", A3_BWD_WAVES)):
        m = re.search(rf"constexpr int {name} = (\d+);", src)
        assert m and int(m.group(1)) == val, name
    for line in ("bool a3_coop_tail(int n) { return (n & 31) != 0 && (n & 31) <= A3_TAIL_MAX && n >= 64; }",
                 "int a3_waves(int n) { return a3_coop_tail(n) ? n / 32 : (n + 31) / 32; }",
                 "int a3_bwd_waves(int n) { const int b = a3_waves(n); return b < A3_BWD_WAVES ? b : A3_BWD_WAVES; }"):
        assert line in src, line
    assert "return a3_coop_tail(n) && (n & 31) == 1" in src


SWEEP_MAX_LENS = (1, 17, 32, 33, 63, 64, 65, 66, 67, 95, 96, 97, 98, 128, 129, 131, 160, 161, 192, 193, 194, 224, 225, 256, 258, 259, 287)
FIXED_MAX_LENS = (max(LENS_A), max(LENS_B))                  # 257 and 288: test_varlen_attention of both files
SWEEP_EMU = (33, 65, 66, 97, 129, 193)                        # the emulator's share of the list


def sweep_coverage():
    """what the list is for: every forward wave count 1 .. 9, and 32 q, 32 q + 1 (single tail), 32 q + 2 (two-row tail), 32 q + 3 (an
    ordinary tail: one wave more) around the dips of the second and of the last tile -- together with the fixed cases' 257 and 288"""
    every = SWEEP_MAX_LENS + FIXED_MAX_LENS
    assert all(1 <= n <= A3_MAX_N for n in every)
    assert {a3_waves(n) for n in every} == set(range(1, a3_waves(A3_MAX_N) + 1)) == set(range(1, 10))
    assert {a3_bwd_waves(n) for n in SWEEP_MAX_LENS} == set(range(1, A3_BWD_WAVES + 1))
    for q in (2, 8):
        side = [32 * q + r for r in range(4)]
        assert all(n in every for n in side), side
        assert [a3_waves(n) for n in side] == [q, q, q, q + 1] and [a3_single_tail(n) for n in side] == [False, True, False, False]
        assert [a3_coop_tail(n) for n in side] == [False, True, True, False]
    assert set(SWEEP_EMU) <= set(SWEEP_MAX_LENS)


def sweep_lens(max_len):
    """one sample of max_len rows and, where strictly shorter: 1, 2, 31, 32, 33, the largest 32 q + 1 / + 2 / + 3 (q >= 2: a single tail, a
    two-row tail, the first length past the dip), the largest multiple of 32 and max_len - 1 -- in a seeded order, so that the long sample is
    not always the first or the last work-group"""
    cand = [1, 2, 31, 32, 33]
    for r in (1, 2, 3):
        q = (max_len - 1 - r) // 32
        if q >= 2:
            cand.append(32 * q + r)
    cand += [(max_len - 1) // 32 * 32, max_len - 1]
    lens = [max_len] + [n for n in dict.fromkeys(cand) if 1 <= n < max_len]
    order = torch.randperm(len(lens), generator=torch.Generator().manual_seed(4200 + max_len)).tolist()
    return tuple(lens[i] for i in order)


def sweep_dim_head(max_len):
    """a narrow head (zero columns behind dim_head 24) on a third of the list"""
    return 24 if SWEEP_MAX_LENS.index(max_len) % 3 == 1 else 64


def case_varlen_launch_size(dev, max_len, heads=3):
    """bf16, slot 64: the head-resident launch sized for max_len over units of every kind of length below it.  3 heads: batch * heads is no
    multiple of 8, so xcd_remap's uneven split is in every launch"""
    lens, dh = sweep_lens(max_len), sweep_dim_head(max_len)
    assert max(lens) == max_len and sum(lens) <= 1750
    print(f"max_len {max_len}: fwd waves {a3_waves(max_len)}, bwd waves {a3_bwd_waves(max_len)}, dim_head {dh}, lens {lens}")
    case_varlen_attention(dev, BF16, lens, heads, 64, dh, seed=max_len, tag=f"launch sizes 1..{A3_MAX_N - 1} dh{dh}")


ABOVE_LENS = (65, 33, 1, 64, 2)
ABOVE_MAX_LENS = (66, 97, 257, 288, 289)
_ABOVE = {}


def case_varlen_max_len_above(dev, max_len, heads=3):
    """max_len larger than every unit (the ABI asks for 1 <= len <= max_len only; cat_layouts takes the maximum over its batches): the kernel
    bars against fp64, and against the launch with max_len = 65 on the same data:
      * max_len = 66 has the wave counts of 65 in both directions (2 / 2) and only a larger LDS carve: every bit equal.
      * 97, 257, 288 launch 3, 8, 9 forward and 3, 4, 4 backward waves.  A wave that owns a 32-query (backward: 32-row) block sweeps ALL key
        sub-tiles itself in ascending order whatever the wave count, so the units without a cooperative tail (33, 1, 64, 2) are bit-equal in
        out, lse and dqkv, and so are out, lse and dQ of the first 64 rows of the 65-row unit.  Its TAIL row (row 64) is not claimed: the
        cooperative tail deals the key sub-tiles out as t = wave, wave + nwaves, ... and merges nwaves partials, so its summation order is
        a function of the launch.  Nor are dK / dV of that unit: every key row sums over the tail query, whose lse and delta (from the tail
        row of out) are the merged values.  Those elements are held to the bars only.
      * 289 takes the plain form (another kernel): the bars only."""
    kw = dict(seed=21, tag=f"max_len above every unit {ABOVE_LENS}")
    if str(dev) not in _ABOVE:
        _ABOVE[str(dev)] = case_varlen_attention(dev, BF16, ABOVE_LENS, heads, 64, 64, max_len=max(ABOVE_LENS), **kw)[0]
    got, _ = case_varlen_attention(dev, BF16, ABOVE_LENS, heads, 64, 64, max_len=max_len, **kw)
    if max_len > A3_MAX_N:
        return
    (out, lse, dqkv), (b_out, b_lse, b_dqkv) = got, _ABOVE[str(dev)]
    inner = heads * 64
    if (a3_waves(max_len), a3_bwd_waves(max_len)) == (a3_waves(65), a3_bwd_waves(65)):
        rows, q_rows = slice(0, None), slice(0, 0)
    else:
        assert ABOVE_LENS[0] == 65 and not any(a3_coop_tail(n) for n in ABOVE_LENS[1:])
        rows, q_rows = slice(65, None), slice(0, 64)         # the units behind the 65-row one; its rows in front of the tail
    for name, a, b in (("out", out[rows], b_out[rows]), ("lse", lse[:, rows], b_lse[:, rows]), ("dqkv", dqkv[rows], b_dqkv[rows]),
                       ("out, head of the 65-row unit", out[q_rows], b_out[q_rows]), ("lse, head of the 65-row unit", lse[:, q_rows], b_lse[:, q_rows]),
                       ("dQ, head of the 65-row unit", dqkv[q_rows, :inner], b_dqkv[q_rows, :inner])):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: max_len {max_len} and max_len 65 differ in bits"


def _draw(g):
    return lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))


def random_resident_cases(count=24, seed=5150):
    """head-resident form: 1 .. 12 samples, max_len uniform in 1 .. 288, lengths uniform in 1 .. max_len with one of them forced to max_len"""
    ri = _draw(torch.Generator().manual_seed(seed))
    cases = []
    for _ in range(count):
        samples, max_len, heads, dh = ri(1, 12), ri(1, A3_MAX_N), ri(1, 4), (64, 40)[ri(0, 1)]
        lens = [ri(1, max_len) for _ in range(samples)]
        lens[ri(0, samples - 1)] = max_len
        cases.append((tuple(lens), heads, dh))
    return cases


PLAIN_TYPES = ((F32, 64, (64, 24)), (F32, 128, (128, 80)), (BF16, 128, (128, 80)))


def random_plain_cases(count=10, seed=5151):
    """plain form, its three instantiations in turn: 1 .. 6 samples (a wave per (row, head) and O(length) work in each: the emulator's time),
    max_len uniform in 1 .. 320 -- on both sides of the resident limit, which these types never take"""
    ri = _draw(torch.Generator().manual_seed(seed))
    cases = []
    for i in range(count):
        dtype, slot, dhs = PLAIN_TYPES[i % len(PLAIN_TYPES)]
        samples, max_len, heads, dh = ri(1, 6), ri(1, 320), ri(1, 3), dhs[ri(0, 1)]
        lens = [ri(1, max_len) for _ in range(samples)]
        lens[ri(0, samples - 1)] = max_len
        cases.append((dtype, slot, tuple(lens), heads, dh))
    return cases


def case_varlen_random_resident(dev, index):
    lens, heads, dh = random_resident_cases()[index]
    print(f"resident #{index}: lens {lens} (max_len {max(lens)}: {a3_waves(max(lens))} / {a3_bwd_waves(max(lens))} waves) heads {heads} dim_head {dh}")
    case_varlen_attention(dev, BF16, lens, heads, 64, dh, seed=100 + index, tag="random sweep, resident")


def case_varlen_random_plain(dev, index):
    dtype, slot, lens, heads, dh = random_plain_cases()[index]
    print(f"plain #{index}: {dtype} slot {slot} lens {lens} heads {heads} dim_head {dh}")
    case_varlen_attention(dev, dtype, lens, heads, slot, dh, seed=200 + index, tag=f"random sweep, plain slot{slot}")


def row_search_lens(kind, many=1000):
    """the shapes of av_sample_of's binary search over cu: one sample (no step), R = batch (every row its own sample, `many` of them), a batch
    that is no power of two with mixed lengths 1 .. 9"""
    if kind == "one_sample":
        return (5,)
    if kind == "every_row_a_sample":
        return (1,) * many
    assert kind == "batch_37"
    ri = _draw(torch.Generator().manual_seed(37))
    return tuple(ri(1, 9) for _ in range(37))


def case_varlen_row_search(dev, dtype, slot, kind, many=1000):
    lens = row_search_lens(kind, many)
    (out, lse, dqkv), (r_out, r_lse, r_grad) = case_varlen_attention(dev, dtype, lens, 2, slot, slot, seed=31, tag=f"row search {kind} slot{slot}")
    # the last row of the last sample: the end of the search's range (cu[batch - 1] <= r < cu[batch]).  check_varlen covered it; by name:
    tag = f"last row of the last sample, {kind} slot{slot}"
    K.close(out[-1:], r_out[-1:], dtype, f"varlen attn out {tag}", scale=float(r_out.abs().max()), ulps=2.0, unit="scale")
    K.close(lse[:, -1:], r_lse[:, -1:], F32, f"varlen attn lse {tag}", scale=float(r_lse.abs().max()))
    K.close(dqkv[-1:], r_grad[-1:], dtype, f"varlen attn dqkv {tag}", scale=float(r_grad.abs().max()), mult=3.0, ulps=2.0, unit="scale")


def case_varlen_smallest_grid(dev, heads, n):
    """one sample: heads work-groups in all (1: xcd_remap of a single group; 7: fewer groups than XCDs)"""
    case_varlen_attention(dev, BF16, (n,), heads, 64, 64, seed=41, tag=f"one sample h{heads}")


def row_chunks_per_lane(dim, dtype):
    """csrc/xclip_api.hip chunks_per_lane: the MAXC a row kernel is instantiated with -- 16-byte chunks per lane, rounded up to a power of two"""
    need = (dim // (8 if dtype == BF16 else 4) + 63) // 64
    c = 1
    while c < need:
        c <<= 1
    return c


def dispatch_row_branches():
    """the (dtype, MAXC) instantiations XC_DISPATCH_ROW has, read from the macro"""
    src = open(_csrc("xclip_api.hip")).read()
    body = src[src.index("#define XC_DISPATCH_ROW"):]
    body = body[:body.index("while (0)")]
    return {dt: sorted(int(m) for m in re.findall(rf"case (\d+): F\({name}, \1\)", body)) for dt, name in ((BF16, "bf16_t"), (F32, "float"))}


EMBED_DIMS = (64, 72, 512, 768, 1024, 2048, 4096)             # 72: 9 (bf16) / 18 (fp32) chunks -- lanes idle, no multiple of 64 lanes
EMBED_BATCHES = (1, 32, 33, 100, 600)


EMBED_WIDTHS = [pytest.param(dt, d, id=f"{name}_dim{d}_maxc{row_chunks_per_lane(d, dt)}") for dt, name in ((F32, "fp32"), (BF16, "bf16"))
                for d in EMBED_DIMS]


def dcls_split(B):
    """xclip_text_embed_packed_bwd's grid: one work-group per 32 samples, 16 at the most (beyond: the sample loop strides)"""
    return min((B + 31) // 32, 16)


def case_embed_coverage():
    """host only: the dims reach every MAXC branch of XC_DISPATCH_ROW in both types, the batches both regimes of the dcls grid"""
    have = dispatch_row_branches()
    assert have[BF16] and have[F32], have
    for dt in (BF16, F32):
        assert sorted({row_chunks_per_lane(d, dt) for d in EMBED_DIMS}) == have[dt], (dt, have[dt])
    assert [dcls_split(B) for B in EMBED_BATCHES] == [1, 1, 2, 4, 16] and 600 > 16 * 32
    assert 72 % 8 == 0 and (72 // 8) % 64 != 0 and (72 // 4) % 64 != 0


BAD_KINDS = ("negative_id", "id_past_the_vocabulary", "position_past_the_table")


def case_packed_embedding_bad(dev, dtype, kind):
    """an id outside [0, vocab) or a layout whose position lies past the position table: that row comes out NaN, every other row keeps the bits
    of the clean launch, nothing is written behind row R, the flag is set and the host raises the IndexError of the dense kernel
    (kernel_cases.case_text_embed_bad_ids) -- at once on the CPU build, at ops.check_tokens() on the GPU.  The kernel reads id 0 in place of
    the bad one and no position row at all: nothing is read out of bounds"""
    B, n, dim, vocab = 4, 6, 64, 11
    tok = embed_tokens(B, n, vocab)
    E, P, cls = K.rnd((vocab, dim), dtype, 71).to(dev), K.rnd((n, dim), dtype, 72).to(dev), K.rnd((dim,), dtype, 73).to(dev)
    lay = text_layout(tok, pad_id=0).to(dev)
    R = lay.R
    r = int(lay.cu[3]) + 2                                      # a token row in the middle of sample 3
    assert int(lay.pos[r]) == 2 and int(lay.cu[3]) + 2 < int(lay.cu[4])
    tk, ps = lay.tok.clone(), lay.pos.clone()
    if kind == "negative_id":
        tk[r] = -1
    elif kind == "id_past_the_vocabulary":
        tk[r] = vocab
    else:
        assert kind == "position_past_the_table"
        ps[r] = n + 1                                           # table position n: one past P's last row
    L = _lib.lib()

    def launch(t, p):
        out = _poison((R + GUARD, dim), dtype, dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.xclip_text_embed_packed_fwd(t.data_ptr(), p.data_ptr(), E.data_ptr(), P.data_ptr(), cls.data_ptr(), out.data_ptr(), R, dim, vocab, n,
                                                 flag.data_ptr(), ops.dtype_code(E), ops._stream(E)), "xclip_text_embed_packed_fwd")
        assert bool(torch.isnan(out[R:].float()).all()), "packed embedding wrote behind row R"
        return out[:R], int(flag.cpu()[0])

    good, f0 = launch(lay.tok, lay.pos)
    bad, f1 = launch(tk, ps)
    assert (f0, f1) == (0, 1), (f0, f1)
    assert bool(torch.isfinite(good.float()).all())
    assert bool(torch.isnan(bad[r].float()).all()), f"{kind}: the row is not NaN"
    others = torch.arange(R, device=dev) != r
    assert torch.equal(_bits(bad[others]), _bits(good[others])), f"{kind}: another row changed"
    with pytest.raises(IndexError, match="index out of range"):
        ops.text_embed_packed_fwd(tk, ps, E, P, cls)
        ops.check_tokens()
    ok = ops.text_embed_packed_fwd(lay.tok, lay.pos, E, P, cls)   # and the state is clean again
    ops.check_tokens()
    assert torch.equal(_bits(ok), _bits(good))


def case_cat_layouts():
    """host only: cat_layouts of two and of three padded batches of one n is text_layout of the concatenated tokens, field by field -- with a
    max_len that the LAST batch alone does not reach (the launch sized above every unit of that batch); other n or CLS convention: raises"""
    from x_clip_amd.packing import cat_layouts
    n = 9
    toks = [embed_tokens(6, n, 50), embed_tokens(3, n, 50, seed=78), embed_tokens(4, n, 50, seed=79)]
    toks[2][:, 4:] = 0                                          # every sample of the last batch is shorter than the longest of the first
    for has_cls in (True, False):
        if not has_cls:
            for t in toks:
                t[1, 0] = 3                                     # (no all-padding sample without a CLS row)
        lays = [text_layout(t, pad_id=0, has_cls=has_cls) for t in toks]
        assert lays[2].max_len < lays[0].max_len
        assert cat_layouts(lays[:1]) is lays[0]
        for k in (2, 3):
            got, want = cat_layouts(lays[:k]), text_layout(torch.cat(toks[:k]), pad_id=0, has_cls=has_cls)
            for f in ("cu", "pos", "tok"):
                a, b = getattr(got, f), getattr(want, f)
                assert a.dtype == b.dtype and torch.equal(a, b), (k, has_cls, f)
            for f in ("R", "max_len", "batch", "n", "has_cls"):
                assert getattr(got, f) == getattr(want, f) and type(getattr(got, f)) is type(getattr(want, f)), (k, has_cls, f)
            assert got.batch == sum(t.shape[0] for t in toks[:k]) and got.max_len == max(l.max_len for l in lays[:k])
    a = text_layout(toks[0], pad_id=0)
    with pytest.raises(ValueError, match="same sequence length"):
        cat_layouts([a, text_layout(toks[1][:, :n - 1].contiguous(), pad_id=0)])
    with pytest.raises(ValueError, match="CLS convention"):
        cat_layouts([a, text_layout(toks[1], pad_id=0, has_cls=False)])


# The model the suite already runs against the oracle at the bf16 bars (cached_cases.MID = tests/test_clip_gpu.py's: dim 512, 70 tokens, depth 2),
# padded so that the packed launch is a mid-range one: rows per sample with the CLS row -- max_len 70 (3 forward and 3 backward waves), a
# single-tail sample (65), a two-row-tail one (66), one wave (4, 18, 32) and the CLS row alone; sample 3 has a hole (41 -> 40 rows)
MID_ROWS = (1, 65, 66, 41, 4, 18, 32, 70)


def padded_text_mid(cfg, text):
    text = text.clone()
    assert text.shape == (len(MID_ROWS), cfg.text_seq_len) and max(MID_ROWS) <= cfg.text_seq_len + 1
    text = torch.where(text == cfg.text_pad_id, torch.ones_like(text), text)
    for r, rows in enumerate(MID_ROWS):
        text[r, rows - 1:] = cfg.text_pad_id
    text[3, 7] = cfg.text_pad_id
    lay = text_layout(text, pad_id=cfg.text_pad_id)
    lens = (lay.cu[1:] - lay.cu[:-1]).tolist()
    assert 40 <= lay.max_len <= 71 and a3_waves(lay.max_len) in (2, 3) and a3_single_tail(65) and 65 in lens and 66 in lens, lens
    return text


def case_vs_oracle_mid(dev):
    """bf16 pack_text = True at a mid-range launch size (MID_ROWS: max_len 70) against the fp64 oracle, DESIGN section 7's bars unchanged"""
    import cached_cases as CC
    assert len(MID_ROWS) == 8
    case_vs_oracle(dev, BF16, "infonce", cfg=CC.MID, pad=padded_text_mid)
