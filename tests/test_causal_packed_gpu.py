"""The packed causal text tower on an MI355X (libxclip_hip.so): the cases of tests/test_causal_packed_emu.py at every shape, plus the launch
that fills the chip."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import causal_packed_cases as Z  # noqa: E402
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
def test_causal_varlen_attention(lens, heads, slot, dim_head, dtype):
    Z.case_causal_attention(DEV, dtype, lens, heads, slot, dim_head)


@pytest.mark.parametrize("max_len", Z.size_max_lens(True))
def test_causal_varlen_every_launch_size(max_len):
    Z.case_causal_launch_size(DEV, max_len)


@DTYPES
@pytest.mark.parametrize("slot", [64, 128])
def test_causal_varlen_unit_of_length_one(slot, dtype):
    Z.case_causal_length_one_first(DEV, dtype, slot)


@pytest.mark.parametrize("n", P.EQUAL_BITS_NS)
def test_causal_varlen_equals_dense_causal_bits(n):
    Z.case_causal_equals_dense_bits(DEV, n)


@pytest.mark.parametrize("n", [66, 33])
@pytest.mark.parametrize("form", list(Z.FORMS))
def test_causality_is_a_property_of_the_kernels(form, n):
    Z.case_causality(DEV, form, n)


def test_plain_and_resident_forms_agree():
    Z.case_plain_and_resident_agree(DEV)


def test_causal_varlen_every_cu_busy_every_head_checked():
    Z.case_causal_full(DEV)


def test_layout_ends_at_the_first_eos():
    Z.case_layout(DEV)


@DTYPES
@pytest.mark.parametrize("pool_last", [False, True], ids=["dense_last", "pool_last"])
@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_packed_causal_vs_oracle(variant, pool_last, dtype):
    Z.case_vs_oracle(DEV, dtype, variant, pool_last)


@DTYPES
@pytest.mark.parametrize("pool_last", [False, True], ids=["dense_last", "pool_last"])
def test_packed_causal_vs_dense_causal(pool_last, dtype):
    Z.case_vs_dense(DEV, dtype, pool_last)


@DTYPES
def test_checkpointing_same_gradients(dtype):
    Z.case_checkpoint(DEV, dtype)


@DTYPES
def test_layout_passed_in_equals_implicit(dtype):
    Z.case_layout_passed_in(DEV, dtype)


@DTYPES
def test_embed_text_equals_forward_latents(dtype):
    Z.case_embed_text(DEV, dtype)


@DTYPES
def test_cached_step_equals_one_pass(dtype):
    Z.case_cached_step(DEV, dtype)


def test_adamw_steps_move_the_weights():
    Z.case_adamw_steps(DEV)


def test_switches():
    Z.case_switches(DEV)


@DTYPES
def test_off_is_unchanged(dtype):
    Z.case_off_is_unchanged(DEV, dtype)
