"""The row-bucketed packed layout on an MI355X (libxclip_hip.so): the cases of tests/test_bucket_packed_emu.py unthinned, plus a launch that
fills the chip."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import bucket_packed_cases as B  # noqa: E402
import packed_cases as P  # noqa: E402
import cached_cases as CC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
LENS = pytest.mark.parametrize("lens", [P.LENS_A, P.LENS_B, B.LENS_ONE], ids=["mixed", "three_ones_and_288", "one_sample"])


@pytest.fixture(scope="module", autouse=True)
def product_library():
    _lib._use_library_for_tests(None)
    _lib.lib()
    yield


def test_layout():
    B.case_layout(DEV)


def test_cat_layouts_pads_once_at_the_end():
    B.case_cat_layouts(DEV)


def test_routes_of_the_text_layer_products():
    B.case_routes()


@CAUSAL
@pytest.mark.parametrize("filler", B.FILLERS)
@LENS
def test_filler_rows_head_resident(lens, filler, causal):
    B.case_filler_rows(DEV, "resident", lens, filler, causal)


@CAUSAL
@pytest.mark.parametrize("filler", B.FILLERS)
@LENS
@pytest.mark.parametrize("form", ["plain_fp32", "plain_wide"])
def test_filler_rows_plain_form(form, lens, filler, causal):
    B.case_filler_rows(DEV, form, lens, filler, causal, heads=2)


@CAUSAL
@pytest.mark.parametrize("filler", B.FILLERS)
def test_filler_rows_plain_form_by_length(filler, causal):
    B.case_filler_rows(DEV, "plain_long", P.LENS_LONG, filler, causal, heads=2)


@CAUSAL
def test_filler_rows_every_cu_busy(causal):
    lens = tuple(P.LENS_A[i % len(P.LENS_A)] for i in range(256))
    B.case_filler_rows(DEV, "resident", lens, 255, causal, heads=8, seed=5)


@DTYPES
@pytest.mark.parametrize("slot", [64, 128])
@pytest.mark.parametrize("filler", B.FILLERS)
@LENS
def test_filler_rows_pooled_backward(lens, filler, slot, dtype):
    B.case_pool_filler_rows(DEV, dtype, slot, lens, filler)


@DTYPES
@pytest.mark.parametrize("multiple", [8, 256])
@pytest.mark.parametrize("pool_last", [False, True], ids=["dense_last", "pool_last"])
@pytest.mark.parametrize("kind", list(B.KINDS))
def test_bucketed_tower_against_the_oracle(kind, pool_last, multiple, dtype):
    B.case_vs_oracle(DEV, dtype, kind, "infonce", multiple, pool_last)


@DTYPES
@pytest.mark.parametrize("multiple", [8, 256])
def test_bucketed_aug_text(multiple, dtype):
    B.case_vs_oracle(DEV, dtype, "cls", "dcl_multiview", multiple, False)


@DTYPES
@pytest.mark.parametrize("multiple", [8, 256])
def test_bucketed_layout_passed_in_with_aug_text(multiple, dtype):
    B.case_vs_oracle(DEV, dtype, "cls", "dcl_multiview", multiple, True, how="layout")


@DTYPES
@pytest.mark.parametrize("multiple", [8, 256])
def test_bucketed_checkpointing(multiple, dtype):
    B.case_vs_oracle(DEV, dtype, "cls", "infonce", multiple, True, checkpoint_during_training=True)


@DTYPES
def test_off_is_unchanged(dtype):
    B.case_off_is_unchanged(DEV, dtype, bitwise=False)


@DTYPES
def test_no_filler_gives_the_unbucketed_bits(dtype):
    B.case_no_filler_same_bits(DEV, dtype)


@DTYPES
def test_cached_step_and_fused_adamw(dtype):
    B.case_cached_and_adamw(DEV, dtype, O.CFG1 if dtype == P.F32 else CC.MID, multiple=8 if dtype == P.F32 else 256)


@DTYPES
def test_embed_text(dtype):
    B.case_embed_text(DEV, dtype)
