"""CLIP.pack_text_tokens on the CPU: the kernel sources compiled against the wave64 emulator (tests/emu), the cases of
tests/test_tokens_packed_gpu.py at the emulator's share of the dtypes."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
import tokens_packed_cases as T  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
KINDS = pytest.mark.parametrize("kind", list(T.KINDS))


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("name", list(T.layouts()))
@pytest.mark.parametrize("width", [0, 1, 2], ids=["one_chunk", "d64", "odd_chunks"])
def test_unpack_and_pack_rows(width, name, dtype):
    T.case_kernels(DEV, dtype, name, T.widths(dtype)[width])


@DTYPES
def test_unpack_and_pack_rows_edges(dtype):
    T.case_kernel_edges(DEV, dtype)


@DTYPES
def test_functional_pair_is_its_own_backward(dtype):
    T.case_functional_pair(DEV, dtype)


def test_layout_helpers():
    T.case_layout_helpers(DEV)


@DTYPES
@KINDS
def test_packed_tokens_vs_oracle(kind, dtype):
    T.case_vs_oracle(DEV, dtype, kind)


@DTYPES
def test_encodings_equal_the_dense_tower(dtype):
    T.case_encodings_equal_dense(DEV, dtype)


def test_encodings_stay_differentiable():
    T.case_encodings_grad(DEV)


def test_inference_return_goes_through_the_unpack():
    T.case_inference_return(DEV)


@pytest.mark.parametrize("kind", ["filip_dcl_multiview", "mlm_filip"])
def test_layout_passed_in_equals_implicit(kind):
    T.case_layout_passed_in(DEV, P.F32, kind)


@pytest.mark.parametrize("kind", ["filip", "mlm"])
def test_checkpointing_same_gradients(kind):
    T.case_checkpoint(DEV, P.F32, kind)


def test_row_multiple():
    T.case_row_multiple(DEV)


@pytest.mark.parametrize("kind", ["filip", "mlm"])
def test_off_is_unchanged(kind):
    T.case_off_is_unchanged(DEV, P.F32, kind)


def test_one_layout_per_call():
    T.case_one_layout(DEV)


def test_mlm_only_follows_pool_last():
    T.case_mlm_only_pool_last(DEV)


def test_switches():
    T.case_switches(DEV)


def test_adamw_step():
    T.case_adamw_step(DEV)
