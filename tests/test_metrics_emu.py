"""x_clip_amd.metrics / ops.simrank* on the CPU: the rank kernels (csrc/kernels/simrank.h) compiled against the wave64 emulator, every
case of tests/metrics_cases.py against dense torch in fp64.  The same cases run on the MI355X in tests/test_metrics_gpu.py."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import metrics_cases as MC  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("nq,nk,d", MC.EXACT_GENERAL)
def test_exact_general_form(dtype, nq, nk, d):
    MC.case_exact(DEV, dtype, nq, nk, d)


@pytest.mark.parametrize("nq,nk,d,off,splits", MC.EXACT_RING)
def test_exact_ring_form(nq, nk, d, off, splits):
    MC.case_exact(DEV, torch.bfloat16, nq, nk, d, off=off, splits=splits)


def test_nan_row_has_no_hardest_negative():
    MC.case_nan_row(DEV)


@DTYPES
@pytest.mark.parametrize("nq,nk,d,off,c", MC.REALISTIC)
def test_realistic_latents_within_the_accumulation_band(dtype, nq, nk, d, off, c):
    MC.case_realistic(DEV, dtype, nq, nk, d, off, c)


@DTYPES
def test_contrastive_metrics_against_dense_torch(dtype):
    MC.case_public_metrics(DEV, dtype)


@DTYPES
def test_track_metrics_leaves_loss_and_gradients_bit_equal(dtype):
    MC.case_track_metrics_changes_nothing(DEV, dtype)


def test_fine_grained_head_is_not_tracked(monkeypatch):
    MC.case_filip_is_not_tracked(DEV, torch.float32, monkeypatch)


def test_public_surface():
    import x_clip
    import x_clip_amd
    from x_clip.metrics import contrastive_metrics
    assert x_clip.contrastive_metrics is x_clip_amd.contrastive_metrics is contrastive_metrics
    assert _lib.lib().xclip_simrank_workspace_bytes(100, 130) == 3 * 3 * 100 * 4
