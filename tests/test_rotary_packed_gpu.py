"""The packed rotary text tower on an MI355X (libxclip_hip.so): the cases of tests/test_rotary_packed_emu.py, both storage types throughout."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
import rotary_packed_cases as Z  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
SHAPES = pytest.mark.parametrize("w,rot", Z.SHAPES, ids=["w64_rot32", "w128_rot32", "w64_rot16", "w64_rot24"])
POOL = pytest.mark.parametrize("pool_last", [False, True], ids=["dense_last", "pool_last"])


@pytest.fixture(scope="module", autouse=True)
def product_library():
    _lib._use_library_for_tests(None)
    _lib.lib()
    yield


@DTYPES
@SHAPES
@pytest.mark.parametrize("slots", [6, 4], ids=["qkv", "kv"])
@pytest.mark.parametrize("pad", [0, 16], ids=["tight", "ld_plus_16"])
def test_rotary_pos_equals_rotary_on_the_kept_rows(pad, slots, w, rot, dtype):
    Z.case_equals_dense_on_kept_rows(DEV, dtype, w, rot, slots, pad)


@DTYPES
@SHAPES
def test_rotary_pos_inverse_after_forward(w, rot, dtype):
    Z.case_inverse_after_forward(DEV, dtype, w, rot)


@DTYPES
@SHAPES
def test_rotary_pos_position_zero_is_the_identity(w, rot, dtype):
    Z.case_position_zero_is_identity(DEV, dtype, w, rot)


@DTYPES
def test_rotary_pos_no_rows(dtype):
    Z.case_no_rows(DEV, dtype)


@DTYPES
@pytest.mark.parametrize("rot", [32, 16, 24])
@pytest.mark.parametrize("size", ["one_row", "grid_wraps"])
def test_rotary_pos_every_launch_size(size, rot, dtype):
    Z.case_launch_sizes(DEV, dtype, rot, 1 if size == "one_row" else Z.wrap_rows(dtype, rot))


@DTYPES
def test_rotary_pos_wrapper_on_a_strided_view(dtype):
    Z.case_ops_wrapper(DEV, dtype)


@DTYPES
@POOL
def test_packed_rotary_vs_dense_rotary(pool_last, dtype):
    Z.case_vs_dense(DEV, dtype, pool_last)


@DTYPES
@POOL
@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_packed_rotary_vs_oracle(variant, pool_last, dtype):
    Z.case_vs_oracle(DEV, dtype, variant, pool_last)


@POOL
@pytest.mark.parametrize("cfg", [Z.NARROW, Z.SLOT128], ids=["dim_head16", "dim_head128"])
def test_packed_rotary_other_head_widths(cfg, pool_last):
    Z.case_vs_oracle(DEV, P.F32, "infonce", pool_last, cfg=cfg)
    Z.case_vs_dense(DEV, P.F32, pool_last, cfg=cfg)


@DTYPES
def test_checkpointing_same_gradients(dtype):
    Z.case_checkpoint(DEV, dtype)


@DTYPES
@POOL
def test_layout_passed_in_equals_implicit(pool_last, dtype):
    Z.case_layout_passed_in(DEV, dtype, pool_last=pool_last)


@DTYPES
@POOL
def test_dropped_rows_are_never_read(pool_last, dtype):
    Z.case_dead_rows(DEV, dtype, pool_last)


@DTYPES
@POOL
def test_embed_text_equals_forward_latents(pool_last, dtype):
    Z.case_embed_text(DEV, dtype, pool_last)


@DTYPES
def test_cached_step_equals_one_pass(dtype):
    Z.case_cached_step(DEV, dtype)


def test_switches():
    Z.case_switches(DEV)


def test_stack_guards():
    Z.case_stack_guards(DEV)


@DTYPES
def test_off_is_unchanged(dtype):
    Z.case_off_is_unchanged(DEV, dtype)


def test_off_matches_the_reference_fixture():
    Z.case_off_matches_reference_fixture(DEV)
