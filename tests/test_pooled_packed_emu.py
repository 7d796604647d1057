"""The packed text tower's pooled last layer on the CPU: the kernel sources compiled against the wave64 emulator (tests/emu), the same cases as
tests/test_pooled_packed_gpu.py at the small shapes."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import pooled_packed_cases as Q  # noqa: E402
import packed_cases as P  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
# the emulator's twins of the cached step's models (tests/test_cached_emu.py): one layer per tower, 256 wide in bf16
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)
TOY_BF16 = dataclasses.replace(TOY, dim_text=256, dim_image=256, dim_latent=256)


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


# One wave per (sample, head) and O(length) work each: the kernel matrix of the GPU file needs no thinning here (a case is well under a second); what
# tests/test_packed_emu.py thins -- the run-against-run cases in one storage type -- is thinned the same way below
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


# (run against run: nothing below depends on the storage type -- bf16 here, both types in tests/test_pooled_packed_gpu.py, as tests/test_packed_emu.py)
def test_routing():
    Q.case_routing(DEV, P.BF16)


def test_checkpointing_is_bit_identical():
    Q.case_checkpoint(DEV, P.BF16)


@pytest.mark.parametrize("variant", ["infonce", "dcl_multiview"])
def test_layout_passed_in_gives_the_same_bits(variant):
    Q.case_layout_passed_in(DEV, P.BF16, variants=(variant,))


@DTYPES
def test_embed_text_equals_the_text_half_of_forward(dtype):
    Q.case_embed_text(DEV, dtype)


@DTYPES
def test_cached_step_one_slice_against_two(dtype):
    Q.case_cached_step(DEV, dtype, TOY if dtype == P.F32 else TOY_BF16)


def test_fused_adamw_steps():
    Q.case_adamw_steps(DEV)
