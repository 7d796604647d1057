"""The pairwise sigmoid head on the CPU: the kernels of csrc/kernels/sigloss.h compiled against the wave64 emulator, every case of
tests/sigloss_cases.py (all but the 272-tile shape) against dense fp64 torch.  The same cases run on the MI355X in
tests/test_sigloss_gpu.py."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import sigloss_cases as SC  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("nq,nk,d", SC.GENERAL)
def test_general_form(dtype, nq, nk, d):
    SC.case_shape(DEV, dtype, nq, nk, d)


@pytest.mark.parametrize("nq,nk,d,off,cuts", SC.RING)
def test_ring_form(nq, nk, d, off, cuts):
    SC.case_shape(DEV, torch.bfloat16, nq, nk, d, off=off, cuts=cuts)


@pytest.mark.parametrize("ring", [False, True], ids=["general-fp32", "ring-bf16"])
@pytest.mark.parametrize("label,t,beta,matched", SC.REGIMES, ids=[r[0] for r in SC.REGIMES])
def test_numerical_regimes(label, t, beta, matched, ring):
    SC.case_regime(DEV, torch.bfloat16 if ring else torch.float32, label, t, beta, matched, ring)


@DTYPES
def test_log1p_is_accurate_relative_to_its_argument(dtype):
    SC.case_log1p(DEV, dtype)


def test_log1p_on_the_ring_loop():
    SC.case_log1p(DEV, torch.bfloat16, nq=256, nk=512, d=320)


@DTYPES
def test_multiview_weights(dtype):
    SC.case_multiview(DEV, dtype)


@DTYPES
def test_clip_with_sigmoid_loss_against_the_dense_formula(dtype):
    SC.case_public(DEV, dtype)


def test_three_optimizer_steps():
    SC.case_adamw_steps(DEV, torch.float32)


@DTYPES
def test_sigmoid_loss_off_changes_nothing(dtype):
    SC.case_off_is_unchanged(DEV, dtype)


def test_rejected_combinations():
    SC.case_rejected_combinations()


def test_track_metrics_gives_the_same_loss():
    SC.case_track_metrics(DEV, torch.float32)


def test_public_surface():
    assert _lib.lib().xclip_sigloss_workspace_bytes(100, 130) == 3 * 100 * 4
