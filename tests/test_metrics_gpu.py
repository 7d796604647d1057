"""x_clip_amd.metrics / ops.simrank* on the MI355X: every case of tests/metrics_cases.py (as tests/test_metrics_emu.py runs them on
the emulator) plus the shape whose 17 x 16 tiles exceed the 256 CUs, so that some work-group walks a second tile."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    _lib._use_library_for_tests(None)
    _lib.lib()
    return torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("nq,nk,d", MC.EXACT_GENERAL)
def test_exact_general_form(dev, dtype, nq, nk, d):
    MC.case_exact(dev, dtype, nq, nk, d)


@pytest.mark.parametrize("nq,nk,d,off,splits", MC.EXACT_RING)
def test_exact_ring_form(dev, nq, nk, d, off, splits):
    MC.case_exact(dev, torch.bfloat16, nq, nk, d, off=off, splits=splits)


def test_exact_more_tiles_than_compute_units(dev):
    MC.case_exact(dev, torch.bfloat16, 4352, 4096, 64, repeats=2)


def test_nan_row_has_no_hardest_negative(dev):
    MC.case_nan_row(dev)


@DTYPES
@pytest.mark.parametrize("nq,nk,d,off,c", MC.REALISTIC)
def test_realistic_latents_within_the_accumulation_band(dev, dtype, nq, nk, d, off, c):
    MC.case_realistic(dev, dtype, nq, nk, d, off, c)


@DTYPES
def test_contrastive_metrics_against_dense_torch(dev, dtype):
    MC.case_public_metrics(dev, dtype)


@DTYPES
def test_track_metrics_leaves_loss_and_gradients_bit_equal(dev, dtype):
    MC.case_track_metrics_changes_nothing(dev, dtype)


def test_fine_grained_head_is_not_tracked(dev, monkeypatch):
    MC.case_filip_is_not_tracked(dev, torch.bfloat16, monkeypatch)
