"""The packed text tower on an MI355X (libxclip_hip.so): the cases of tests/test_packed_emu.py, plus the launches that fill the chip."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def product_library():
    _lib._use_library_for_tests(None)
    _lib.lib()
    yield


@DTYPES
@pytest.mark.parametrize("slot,dim_head", P.WIDTHS, ids=["slot64", "slot64_dh24", "slot128_dh80"])
@pytest.mark.parametrize("heads", [2, 8])
@pytest.mark.parametrize("lens", [P.LENS_A, P.LENS_B, P.LENS_LONG], ids=["mixed", "three_ones_and_288", "beyond_resident"])
def test_varlen_attention(lens, heads, slot, dim_head, dtype):
    P.case_varlen_attention(DEV, dtype, lens, heads, slot, dim_head)


@DTYPES
@pytest.mark.parametrize("n,slot", [(65, 64), (33, 128)])
def test_varlen_equals_dense_for_equal_lengths(n, slot, dtype):
    P.case_varlen_equals_dense(DEV, dtype, 3, n, 2, slot)


@pytest.mark.parametrize("n", P.EQUAL_BITS_NS)
def test_varlen_equals_dense_bit_for_bit(n):
    P.case_varlen_equals_dense_bits(DEV, n)


def test_varlen_attention_every_cu_busy():
    P.case_varlen_full(DEV)


@DTYPES
def test_packed_embedding(dtype):
    P.case_packed_embedding(DEV, dtype)


def test_layout():
    P.case_layout(DEV)


@DTYPES
@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_pack_text_against_the_oracle(variant, dtype):
    P.case_vs_oracle(DEV, dtype, variant)


@DTYPES
def test_checkpointing_is_identical(dtype):
    P.case_checkpoint(DEV, dtype, bitwise=False)


def test_layout_passed_in_gives_the_same_bits():
    P.case_layout_passed_in(DEV, P.BF16, bitwise=False)


@DTYPES
def test_pack_text_off_is_unchanged(dtype):
    P.case_off_is_unchanged(DEV, dtype, bitwise=False)


@DTYPES
def test_embed_text_equals_the_text_half_of_forward(dtype):
    P.case_embed_text(DEV, dtype)


def test_rejected_combinations():
    P.case_rejected(DEV)


def test_fused_adamw_steps():
    P.case_adamw_steps(DEV)


def test_default_architecture_fill_one_eighth():
    P.case_default_architecture(DEV)
