"""The pairwise sigmoid head on the MI355X: every case of tests/sigloss_cases.py (as tests/test_sigloss_emu.py runs them on the
emulator) plus the shape whose 17 x 16 tiles exceed the 256 CUs, so that some work-group walks a second tile."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import sigloss_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    _lib._use_library_for_tests(None)
    _lib.lib()
    return torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("nq,nk,d", SC.GENERAL)
def test_general_form(dev, dtype, nq, nk, d):
    SC.case_shape(dev, dtype, nq, nk, d)


@pytest.mark.parametrize("nq,nk,d,off,cuts", SC.RING)
def test_ring_form(dev, nq, nk, d, off, cuts):
    SC.case_shape(dev, torch.bfloat16, nq, nk, d, off=off, cuts=cuts)


def test_more_tiles_than_compute_units(dev):
    SC.case_more_tiles_than_compute_units(dev)


@pytest.mark.parametrize("ring", [False, True], ids=["general-fp32", "ring-bf16"])
@pytest.mark.parametrize("label,t,beta,matched", SC.REGIMES, ids=[r[0] for r in SC.REGIMES])
def test_numerical_regimes(dev, label, t, beta, matched, ring):
    SC.case_regime(dev, torch.bfloat16 if ring else torch.float32, label, t, beta, matched, ring)


@DTYPES
def test_log1p_is_accurate_relative_to_its_argument(dev, dtype):
    SC.case_log1p(dev, dtype)


def test_log1p_on_the_ring_loop(dev):
    SC.case_log1p(dev, torch.bfloat16, nq=256, nk=512, d=320)


@DTYPES
def test_multiview_weights(dev, dtype):
    SC.case_multiview(dev, dtype)


@DTYPES
def test_clip_with_sigmoid_loss_against_the_dense_formula(dev, dtype):
    SC.case_public(dev, dtype)


def test_three_optimizer_steps(dev):
    SC.case_adamw_steps(dev, torch.float32)     # (a bf16 bias of -10 has an ulp of 1/16: three steps of 1e-2 move its fp32 master only)


@DTYPES
def test_sigmoid_loss_off_changes_nothing(dev, dtype):
    SC.case_off_is_unchanged(dev, dtype)


def test_rejected_combinations(dev):
    SC.case_rejected_combinations()


def test_track_metrics_gives_the_same_loss(dev):
    SC.case_track_metrics(dev, torch.bfloat16)
