"""`trust_ratio` (LAMB) and `bounds` of x_clip_amd.optim.FusedAdamW on the MI355X (libxclip_hip.so): the cases of tests/lamb_cases.py
against their plain-torch reference run on the CPU in fp64; the end-to-end check trains the small CLIP of the optimizer's end-to-end tests
(oracle CFG1 through clip_cases.build_clip)."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import lamb_cases as LC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
BAD = pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
TRUST = pytest.mark.parametrize("trust", [False, True], ids=["adamw", "lamb"])
EMA = pytest.mark.parametrize("ema_decay", [None, 0.9], ids=["plain", "ema"])


@pytest.fixture(scope="module")
def dev():
    _lib._use_library_for_tests(None)
    _lib.lib()
    assert not _lib.is_emulator()
    return torch.device("cuda:0")


@DTYPES
def test_lamb_parity_over_ten_steps(dev, dtype):
    LC.case_parity(dev, dtype)


@DTYPES
def test_ratio_is_one_where_a_norm_is_zero(dev, dtype):
    LC.case_ratio_edges(dev, dtype)


@DTYPES
@TRUST
@EMA
def test_bounds_hold_on_master_parameter_and_ema(dev, dtype, trust, ema_decay):
    LC.case_bounds(dev, dtype, trust, ema_decay)


@DTYPES
def test_one_sided_bounds(dev, dtype):
    LC.case_one_sided_bounds(dev, dtype)


def test_invalid_bounds_are_refused(dev):
    LC.case_invalid_bounds(dev)


@DTYPES
@EMA
def test_off_means_off(dev, dtype, ema_decay):
    LC.case_off_means_off(dev, dtype, ema_decay)


@DTYPES
@BAD
def test_skipped_step_leaves_everything_and_the_ratios_alone(dev, dtype, bad):
    LC.case_skipped_step(dev, dtype, bad)


@DTYPES
def test_lamb_is_reproducible(dev, dtype):
    LC.case_reproducible(dev, dtype)


@DTYPES
def test_absent_and_late_gradients(dev, dtype):
    LC.case_absent_and_late_gradient(dev, dtype)


@DTYPES
def test_state_dict_round_trip_keeps_keys_and_bits(dev, dtype):
    LC.case_state_roundtrip(dev, dtype)


def test_torch_adamw_state_dict_keeps_the_constructor_keys(dev):
    LC.case_load_torch_adamw(dev)


@DTYPES
def test_lamb_with_ema_and_accumulated_gradients(dev, dtype):
    LC.case_lamb_ema_accumulate(dev, dtype)


def test_end_to_end_fp32_three_steps_lamb_and_bounded_temperature(dev):
    LC.case_end_to_end(dev, O.CFG1)
