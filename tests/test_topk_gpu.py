"""x_clip_amd.retrieval / ops.simtopk* on the MI355X: every case of tests/topk_cases.py (as tests/test_topk_emu.py runs them on the
emulator) plus the shape whose 17 x 16 tiles exceed the 256 CUs, so that some work-group walks a second tile."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import topk_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    _lib._use_library_for_tests(None)
    _lib.lib()
    return torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("nq,ng,d", TC.EXACT_GENERAL)
def test_exact_general_form(dev, dtype, nq, ng, d):
    TC.case_exact(dev, dtype, nq, ng, d)


@pytest.mark.parametrize("nq,ng,d,splits", TC.EXACT_RING)
def test_exact_ring_form(dev, nq, ng, d, splits):
    TC.case_exact(dev, torch.bfloat16, nq, ng, d, splits=splits)


def test_exact_more_tiles_than_compute_units(dev):
    TC.case_exact(dev, torch.bfloat16, 4352, 4096, 64, ks=(10,), repeats=2)


@DTYPES
def test_all_equal_gallery_returns_the_lowest_columns(dev, dtype):
    TC.case_all_equal_gallery(dev, dtype)


def test_nan_row_is_all_padding(dev):
    TC.case_nan_row(dev)


@DTYPES
def test_empty_inputs_launch_nothing(dev, dtype, monkeypatch):
    TC.case_empty(dev, dtype, monkeypatch)


@DTYPES
@pytest.mark.parametrize("nq,ng,d,c", TC.REALISTIC)
def test_realistic_latents_within_the_accumulation_band(dev, dtype, nq, ng, d, c):
    TC.case_realistic(dev, dtype, nq, ng, d, c)


@DTYPES
def test_embed_is_half_of_forward_and_similarity_topk(dev, dtype):
    TC.case_embed_matches_forward(dev, dtype)


@DTYPES
def test_zero_shot_classifier(dev, dtype):
    TC.case_zero_shot(dev, dtype)


def test_fine_grained_head_has_no_single_latent(dev):
    TC.case_fine_grained_head_raises(dev, torch.bfloat16)
