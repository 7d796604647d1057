"""The packed text tower's pooled last layer on an MI355X (libxclip_hip.so): the cases of tests/test_pooled_packed_emu.py, plus the launch that
fills the chip and the default architecture."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import pooled_packed_cases as Q  # noqa: E402
import packed_cases as P  # noqa: E402
import cached_cases as CC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

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
@pytest.mark.parametrize("lens", [P.LENS_A, P.LENS_B, Q.LENS_KPL], ids=["mixed", "three_ones_and_288", "each_side_of_kpl"])
def test_pool_varlen_attention(lens, heads, slot, dim_head, dtype):
    Q.case_pool_varlen(DEV, dtype, lens, heads, slot, dim_head)


@DTYPES
def test_pool_varlen_unit_of_length_zero(dtype):
    Q.case_pool_varlen_empty_unit(DEV, dtype)


@DTYPES
@pytest.mark.parametrize("n,slot", [(65, 64), (33, 128)])
def test_pool_varlen_equals_dense_pool_for_equal_lengths(n, slot, dtype):
    Q.case_pool_varlen_equals_dense_pool(DEV, dtype, 3, n, 2, slot)


@DTYPES
@pytest.mark.parametrize("slot", [64, 128])
@pytest.mark.parametrize("n", Q.EQUAL_BITS_NS)
def test_pool_varlen_equals_dense_pool_bit_for_bit(n, slot, dtype):
    Q.case_pool_varlen_equals_dense_pool_bits(DEV, dtype, n, slot)


@pytest.mark.parametrize("dtype,slot", Q.PLAIN_ROUTES, ids=["fp32_slot64", "fp32_slot128", "bf16_slot128"])
def test_plain_varlen_equals_pool_varlen_bit_for_bit(dtype, slot):
    Q.case_plain_varlen_equals_pool_varlen_bits(DEV, dtype, slot)


def test_pool_varlen_attention_every_cu_busy():
    Q.case_pool_varlen_full(DEV)


@DTYPES
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
def test_rows_add_at(strided, dtype):
    Q.case_rows_add_at(DEV, dtype, strided)


@DTYPES
@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_pool_last_against_the_oracle(variant, dtype):
    Q.case_vs_oracle(DEV, dtype, variant)


@DTYPES
def test_pool_last_against_the_dense_last_layer(dtype):
    Q.case_vs_dense_last_layer(DEV, dtype)


@DTYPES
def test_routing(dtype):
    Q.case_routing(DEV, dtype, bitwise=False)


@DTYPES
def test_checkpointing_is_identical(dtype):
    Q.case_checkpoint(DEV, dtype, bitwise=False)


def test_layout_passed_in_gives_the_same_bits():
    Q.case_layout_passed_in(DEV, P.BF16, bitwise=False)


@DTYPES
def test_embed_text_equals_the_text_half_of_forward(dtype):
    Q.case_embed_text(DEV, dtype)


@DTYPES
def test_cached_step_one_slice_against_two(dtype):
    Q.case_cached_step(DEV, dtype, O.CFG1 if dtype == P.F32 else CC.MID)


def test_fused_adamw_steps():
    Q.case_adamw_steps(DEV)


@pytest.mark.parametrize("fill", [1 / 8, 1.0], ids=["fill_one_eighth", "no_padding"])
def test_default_architecture(fill):
    Q.case_default_architecture(DEV, fill=fill)
