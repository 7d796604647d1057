"""Every launch size of the varlen attention kernels and every branch of the packed embedding, on the CPU: the kernel sources compiled against
the wave64 emulator (tests/emu), the cases of tests/test_packed_sweep_gpu.py.  A wrong LDS carve, a wrong tail merge or a wave seeding the
wrong partial shows here too; a read that overtakes a DMA shows on the MI355X only."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
import packed_sweep_cases as S  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


# ---- host only -----------------------------------------------------------------------------------------------------------------------------
def test_launch_size_list_covers_every_wave_count_and_both_sides_of_the_dips():
    S.sweep_coverage()


def test_geometry_twin_is_the_headers():
    S.case_geometry_twin()


def test_embedding_shapes_cover_every_row_dispatch_branch_and_both_split_regimes():
    S.case_embed_coverage()


def test_cat_layouts_is_the_layout_of_the_concatenated_tokens():
    S.case_cat_layouts()


# ---- varlen attention ------------------------------------------------------------------------------------------------------------------------
# The emulator runs every GPU thread as a fibre, so the kernel sweeps of tests/test_packed_sweep_gpu.py are thinned to what keeps a case at a few
# seconds: the launch sizes S.SWEEP_EMU (2 .. 7 forward waves, a single tail, a two-row tail and the length past a dip as max_len) at 2 heads
# instead of all 27 at 3; the first 6 + 4 batches of the seeded sweeps instead of 24 + 10; the row search over 100 one-row samples instead
# of 1000.  max_len above every unit, the smallest grids, the embedding and the host-only cases run in full.
@pytest.mark.parametrize("max_len", S.SWEEP_EMU)
def test_varlen_resident_launch_size(max_len):
    S.case_varlen_launch_size(DEV, max_len, heads=2)


@pytest.mark.parametrize("max_len", S.ABOVE_MAX_LENS)
def test_varlen_max_len_above_every_unit(max_len):
    S.case_varlen_max_len_above(DEV, max_len)


@pytest.mark.parametrize("index", range(6))
def test_varlen_random_resident(index):
    S.case_varlen_random_resident(DEV, index)


@pytest.mark.parametrize("index", range(4))
def test_varlen_random_plain(index):
    S.case_varlen_random_plain(DEV, index)


@pytest.mark.parametrize("dtype,slot", [(S.F32, 64), (S.BF16, 128)], ids=["fp32_slot64", "bf16_slot128"])
@pytest.mark.parametrize("kind", ["one_sample", "every_row_a_sample", "batch_37"])
def test_varlen_plain_row_search(kind, dtype, slot):
    S.case_varlen_row_search(DEV, dtype, slot, kind, many=100)


@pytest.mark.parametrize("n", [34, 65])
@pytest.mark.parametrize("heads", [1, 7])
def test_varlen_resident_smallest_grid(heads, n):
    S.case_varlen_smallest_grid(DEV, heads, n)


# ---- packed embedding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", S.EMBED_WIDTHS)
def test_packed_embedding_every_row_width(dtype, dim):
    """B = 33: two work-groups of the dcls kernel; the ids name the MAXC (16-byte chunks per lane) the case instantiates -- every branch
    XC_DISPATCH_ROW has, in both types (test_embedding_shapes_cover_every_row_dispatch_branch_and_both_split_regimes)"""
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
