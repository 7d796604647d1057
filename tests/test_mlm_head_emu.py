"""The fused MLM vocabulary head on the CPU: the kernels of csrc/kernels/vocabce.h and tokens.h colsum_wide_kernel compiled against the
wave64 emulator, every case of tests/mlm_head_cases.py (all but the 272-tile shape) against dense fp64 torch.  The same cases run on the
MI355X in tests/test_mlm_head_gpu.py."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import mlm_head_cases as MC  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("nm,V,D", MC.GENERAL)
def test_general_form(dtype, nm, V, D):
    MC.case_shape(DEV, dtype, nm, V, D)


@pytest.mark.parametrize("nm,V,D", MC.RING)
def test_ring_form(nm, V, D):
    MC.case_shape(DEV, torch.bfloat16, nm, V, D)


def test_general_form_past_the_old_row_limit():
    MC.case_shape(DEV, torch.float32, *MC.WIDE_F32)


@pytest.mark.parametrize("shared", [False, True], ids=["placed", "shared"])
def test_label_placement(shared):
    MC.case_label_placement(DEV, shared)


@pytest.mark.parametrize("ring", [False, True], ids=["general-fp32", "ring-bf16"])
@pytest.mark.parametrize("which", MC.REGIMES)
def test_numerical_regimes(which, ring):
    MC.case_regime(DEV, ring, which)


def test_two_launches_give_the_same_bits():
    MC.case_shape(DEV, torch.bfloat16, 520, 777, 64, repeats=1)


@DTYPES
@pytest.mark.parametrize("dim", [4096, 4104])
@pytest.mark.parametrize("rows", [1, 3, 1030])
def test_column_sum(dtype, rows, dim):
    MC.case_colsum(DEV, dtype, rows, dim)


def test_scatter_with_a_table_keeps_its_row_limit():
    MC.case_scatter_still_refuses_wide_tables(DEV)


@DTYPES
def test_fused_head_vs_oracle_2000_tokens(dtype):
    MC.case_vs_oracle(DEV, dtype, 2000, True)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_bf16_step_at_4100_tokens_vs_oracle(fused):
    MC.case_vs_oracle(DEV, torch.bfloat16, 4100, fused)


@DTYPES
def test_fused_vs_unfused(dtype):
    MC.case_fused_vs_unfused(DEV, dtype)


@DTYPES
def test_attribute_off_changes_nothing(dtype):
    MC.case_off_is_unchanged(DEV, dtype)


@pytest.mark.parametrize("row_multiple", [None, 256], ids=["packed", "packed-rows256"])
def test_packed_tower_follows(row_multiple):
    MC.case_packed(DEV, row_multiple)


def test_fused_node_saves_no_logits():
    MC.case_saved_tensors(DEV)


def test_value_error_without_mlm():
    MC.case_value_error_without_mlm(DEV)


def test_no_masked_rows_gives_nan():
    MC.case_no_masked_rows(DEV)


def test_public_surface():
    MC.case_public_surface()
