"""Every launch size of the varlen attention kernels and every branch of the packed embedding on an MI355X (libxclip_hip.so).

The head-resident varlen launch is sized by the batch's longest sample (waves, LDS carve) and every shorter unit runs inside it; the fixed cases
of tests/test_packed_gpu.py see that at max_len 257 and 288 only.  Here max_len walks through every forward wave count and both sides of the
cooperative-tail dips (packed_sweep_cases.SWEEP_MAX_LENS, held to that by sweep_coverage), sits above every unit, and is drawn at random; the plain form's row
search and the smallest grids get their edge shapes; the packed embedding runs every MAXC branch of XC_DISPATCH_ROW and every grid of its dcls
kernel.  All against fp64 under the bars of packed_cases.check_varlen (tests/packed_sweep_cases.py holds the cases); tests/test_packed_sweep_emu.py is the thinned CPU twin."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
import packed_sweep_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def product_library():
    _lib._use_library_for_tests(None)
    _lib.lib()
    yield


def test_launch_size_list_covers_every_wave_count_and_both_sides_of_the_dips():
    S.sweep_coverage()
    S.case_geometry_twin()


# ---- varlen attention ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", S.SWEEP_MAX_LENS)
def test_varlen_resident_launch_size(max_len):
    S.case_varlen_launch_size(DEV, max_len)


@pytest.mark.parametrize("max_len", S.ABOVE_MAX_LENS)
def test_varlen_max_len_above_every_unit(max_len):
    S.case_varlen_max_len_above(DEV, max_len)


@pytest.mark.parametrize("index", range(24))
def test_varlen_random_resident(index):
    S.case_varlen_random_resident(DEV, index)


@pytest.mark.parametrize("index", range(10))
def test_varlen_random_plain(index):
    S.case_varlen_random_plain(DEV, index)


@pytest.mark.parametrize("dtype,slot", [(S.F32, 64), (S.BF16, 128)], ids=["fp32_slot64", "bf16_slot128"])
@pytest.mark.parametrize("kind", ["one_sample", "every_row_a_sample", "batch_37"])
def test_varlen_plain_row_search(kind, dtype, slot):
    S.case_varlen_row_search(DEV, dtype, slot, kind)


@pytest.mark.parametrize("n", [34, 65])
@pytest.mark.parametrize("heads", [1, 7])
def test_varlen_resident_smallest_grid(heads, n):
    S.case_varlen_smallest_grid(DEV, heads, n)


# ---- packed embedding ------------------------------------------------------------------------------------------------------------------------
def test_embedding_shapes_cover_every_row_dispatch_branch_and_both_split_regimes():
    S.case_embed_coverage()


@pytest.mark.parametrize("dtype,dim", S.EMBED_WIDTHS)
def test_packed_embedding_every_row_width(dtype, dim):
    """B = 33: two work-groups of the dcls kernel; the ids name the MAXC (16-byte chunks per lane) the case instantiates -- every branch
    XC_DISPATCH_ROW has, in both types"""
    P.case_packed_embedding(DEV, dtype, B=33, dim=dim)


@DTYPES
@pytest.mark.parametrize("B", S.EMBED_BATCHES, ids=[f"B{b}_split{S.dcls_split(b)}" for b in S.EMBED_BATCHES])
def test_packed_embedding_every_batch_regime(B, dtype):
    """dim 72 (lanes idle in the only chunk round); split 1: one work-group, 2 .. 4: cross-work-group atomics, 16 at B = 600: the sample loop strides"""
    P.case_packed_embedding(DEV, dtype, B=B, dim=72)


@DTYPES
@pytest.mark.parametrize("has_pos,has_cls", [(False, True), (True, False), (False, False)], ids=["no_pos", "no_cls", "no_pos_no_cls"])
def test_packed_embedding_without_table_or_cls(has_pos, has_cls, dtype):
    P.case_packed_embedding(DEV, dtype, B=33, has_pos=has_pos, has_cls=has_cls)


@DTYPES
@pytest.mark.parametrize("kind", S.BAD_KINDS)
def test_packed_embedding_bad_input(kind, dtype):
    S.case_packed_embedding_bad(DEV, dtype, kind)


def test_cat_layouts_is_the_layout_of_the_concatenated_tokens():
    S.case_cat_layouts()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
# GPU only: on the emulator the dim-512, depth-2, batch-8 step takes 25 s on top of its fp64 oracle (it passes there), far beyond the few
# seconds a case of the CPU suite may take; the emulator file has no twin of this one
def test_pack_text_against_the_oracle_at_a_mid_range_launch_size():
    S.case_vs_oracle_mid(DEV)
