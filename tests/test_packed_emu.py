"""The packed text tower on the CPU: the kernel sources compiled against the wave64 emulator (tests/emu), the same cases as
tests/test_packed_gpu.py at the small shapes."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


# The emulator runs every GPU thread as a fibre, so the matrix of tests/test_packed_gpu.py is thinned to what keeps a case at a few seconds: the
# head-resident MFMA kernels (bf16, 64-wide slots) see every length of the GPU lists, at 2 heads and once at 8; the plain kernels (one wave per
# (row, head), O(length) each) see the same boundary lengths up to 65 and the dispatch beyond the resident limit with 2 heads
SHORT = (1, 2, 31, 32, 33, 63, 64, 65)


@pytest.mark.parametrize("dim_head", [64, 24])
@pytest.mark.parametrize("lens", [P.LENS_A, P.LENS_B], ids=["mixed", "three_ones_and_288"])
def test_varlen_attention_resident(lens, dim_head):
    P.case_varlen_attention(DEV, P.BF16, lens, 2, 64, dim_head)


def test_varlen_attention_resident_eight_heads():
    P.case_varlen_attention(DEV, P.BF16, P.LENS_A, 8, 64, 64)


@pytest.mark.parametrize("dtype,slot,dim_head", [(P.F32, 64, 64), (P.F32, 64, 24), (P.F32, 128, 80), (P.BF16, 128, 80)],
                         ids=["fp32_slot64", "fp32_slot64_dh24", "fp32_slot128_dh80", "bf16_slot128_dh80"])
@pytest.mark.parametrize("heads", [2, 8])
def test_varlen_attention_plain(heads, dtype, slot, dim_head):
    P.case_varlen_attention(DEV, dtype, SHORT if heads == 2 else (1, 33, 2), heads, slot, dim_head)


@DTYPES
def test_varlen_attention_beyond_the_resident_limit(dtype):
    P.case_varlen_attention(DEV, dtype, P.LENS_LONG, 2, 64, 64)


@DTYPES
@pytest.mark.parametrize("n,slot", [(65, 64), (33, 128)])
def test_varlen_equals_dense_for_equal_lengths(n, slot, dtype):
    P.case_varlen_equals_dense(DEV, dtype, 3, n, 2, slot)


@pytest.mark.parametrize("n", P.EQUAL_BITS_NS)
def test_varlen_equals_dense_bit_for_bit(n):
    P.case_varlen_equals_dense_bits(DEV, n)


@DTYPES
def test_packed_embedding(dtype):
    P.case_packed_embedding(DEV, dtype)


def test_layout():
    P.case_layout(DEV)


@DTYPES
@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_pack_text_against_the_oracle(variant, dtype):
    P.case_vs_oracle(DEV, dtype, variant)


# (run against run, the same launches twice: nothing in these depends on the storage type, and the emulator's fp32 matrix products take four times as
#  long as its bf16 ones -- bf16 here, both types in tests/test_packed_gpu.py; the fp32 plumbing is held by the oracle cases above)
def test_checkpointing_is_bit_identical():
    P.case_checkpoint(DEV, P.BF16, bitwise=True)


@pytest.mark.parametrize("variant", ["infonce", "dcl_multiview"])
def test_layout_passed_in_gives_the_same_bits(variant):
    P.case_layout_passed_in(DEV, P.BF16, variants=(variant,))


def test_pack_text_off_is_unchanged():
    P.case_off_is_unchanged(DEV, P.BF16)


@DTYPES
def test_embed_text_equals_the_text_half_of_forward(dtype):
    P.case_embed_text(DEV, dtype)


def test_rejected_combinations():
    P.case_rejected(DEV)


def test_fused_adamw_steps():
    P.case_adamw_steps(DEV)
