"""The fused MLM vocabulary head on the MI355X: every case of tests/mlm_head_cases.py (as tests/test_mlm_head_emu.py runs them on the
emulator) plus the shape whose 17 x 16 tiles exceed the 256 CUs, so that some work-group walks a second tile."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import mlm_head_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    _lib._use_library_for_tests(None)
    _lib.lib()
    return torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("nm,V,D", MC.GENERAL)
def test_general_form(dev, dtype, nm, V, D):
    MC.case_shape(dev, dtype, nm, V, D)


@pytest.mark.parametrize("nm,V,D", MC.RING)
def test_ring_form(dev, nm, V, D):
    MC.case_shape(dev, torch.bfloat16, nm, V, D)


def test_general_form_past_the_old_row_limit(dev):
    MC.case_shape(dev, torch.float32, *MC.WIDE_F32)


@pytest.mark.parametrize("shared", [False, True], ids=["placed", "shared"])
def test_label_placement(dev, shared):
    MC.case_label_placement(dev, shared)


@pytest.mark.parametrize("ring", [False, True], ids=["general-fp32", "ring-bf16"])
@pytest.mark.parametrize("which", MC.REGIMES)
def test_numerical_regimes(dev, which, ring):
    MC.case_regime(dev, ring, which)


def test_two_launches_give_the_same_bits(dev):
    MC.case_shape(dev, torch.bfloat16, 520, 777, 64, repeats=1)


def test_more_tiles_than_compute_units(dev):
    MC.case_more_tiles_than_compute_units(dev)


@DTYPES
@pytest.mark.parametrize("dim", [4096, 4104])
@pytest.mark.parametrize("rows", [1, 3, 1030])
def test_column_sum(dev, dtype, rows, dim):
    MC.case_colsum(dev, dtype, rows, dim)


def test_scatter_with_a_table_keeps_its_row_limit(dev):
    MC.case_scatter_still_refuses_wide_tables(dev)


@DTYPES
def test_fused_head_vs_oracle_2000_tokens(dev, dtype):
    MC.case_vs_oracle(dev, dtype, 2000, True)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_bf16_step_at_4100_tokens_vs_oracle(dev, fused):
    MC.case_vs_oracle(dev, torch.bfloat16, 4100, fused)


@DTYPES
def test_fused_vs_unfused(dev, dtype):
    MC.case_fused_vs_unfused(dev, dtype)


@DTYPES
def test_attribute_off_changes_nothing(dev, dtype):
    MC.case_off_is_unchanged(dev, dtype)


@pytest.mark.parametrize("row_multiple", [None, 256], ids=["packed", "packed-rows256"])
def test_packed_tower_follows(dev, row_multiple):
    MC.case_packed(dev, row_multiple)


def test_fused_node_saves_no_logits(dev):
    MC.case_saved_tensors(dev)


def test_value_error_without_mlm(dev):
    MC.case_value_error_without_mlm(dev)


def test_no_masked_rows_gives_nan(dev):
    MC.case_no_masked_rows(dev)


def test_public_surface(dev):
    MC.case_public_surface()
