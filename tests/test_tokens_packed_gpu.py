"""CLIP.pack_text_tokens on an MI355X (libxclip_hip.so): the cases of tests/test_tokens_packed_emu.py, both storage types throughout."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import packed_cases as P  # noqa: E402
import tokens_packed_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
KINDS = pytest.mark.parametrize("kind", list(T.KINDS))


@pytest.fixture(scope="module", autouse=True)
def product_library():
    _lib._use_library_for_tests(None)
    _lib.lib()
    yield


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


@DTYPES
def test_encodings_stay_differentiable(dtype):
    T.case_encodings_grad(DEV, dtype)


@DTYPES
def test_inference_return_goes_through_the_unpack(dtype):
    T.case_inference_return(DEV, dtype)


# (run against run: the fine-grained kinds in fp32, the MLM kind in both types -- tokens_packed_cases._same_run)
RUNS = pytest.mark.parametrize("kind,dtype", [("filip_dcl_multiview", P.F32), ("mlm_filip", P.F32), ("filip", P.F32), ("mlm", P.F32), ("mlm", P.BF16)],
                               ids=["filip_dcl_multiview-fp32", "mlm_filip-fp32", "filip-fp32", "mlm-fp32", "mlm-bf16"])


@RUNS
def test_layout_passed_in_equals_implicit(kind, dtype):
    T.case_layout_passed_in(DEV, dtype, kind)


@RUNS
def test_checkpointing_same_gradients(kind, dtype):
    T.case_checkpoint(DEV, dtype, kind)


def test_row_multiple():
    T.case_row_multiple(DEV)


@RUNS
def test_off_is_unchanged(kind, dtype):
    T.case_off_is_unchanged(DEV, dtype, kind)


def test_one_layout_per_call():
    T.case_one_layout(DEV)


@DTYPES
def test_mlm_only_follows_pool_last(dtype):
    T.case_mlm_only_pool_last(DEV, dtype)


def test_switches():
    T.case_switches(DEV)


def test_adamw_step():
    T.case_adamw_step(DEV)
