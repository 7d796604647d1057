"""`trust_ratio` (LAMB) and `bounds` of x_clip_amd.optim.FusedAdamW on the CPU: lamb_norm_kernel, lamb_fold_kernel and optim_update_kernel
(csrc/kernels/optim.h) compiled against the wave64 emulator, every case of tests/lamb_cases.py against its plain-torch fp64 reference.
The same cases run on the MI355X in tests/test_lamb_gpu.py."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import lamb_cases as LC  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
BAD = pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
TRUST = pytest.mark.parametrize("trust", [False, True], ids=["adamw", "lamb"])
EMA = pytest.mark.parametrize("ema_decay", [None, 0.9], ids=["plain", "ema"])
# the toy-size twin of the GPU suite's end-to-end model: one layer per tower
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


def test_reference_without_the_keys_is_torch_adamw():
    LC.case_reference_is_adamw()


@DTYPES
def test_lamb_parity_over_ten_steps(dtype):
    LC.case_parity(DEV, dtype)


@DTYPES
def test_ratio_is_one_where_a_norm_is_zero(dtype):
    LC.case_ratio_edges(DEV, dtype)


@DTYPES
@TRUST
@EMA
def test_bounds_hold_on_master_parameter_and_ema(dtype, trust, ema_decay):
    LC.case_bounds(DEV, dtype, trust, ema_decay)


@DTYPES
def test_one_sided_bounds(dtype):
    LC.case_one_sided_bounds(DEV, dtype)


def test_invalid_bounds_are_refused():
    LC.case_invalid_bounds(DEV)


@DTYPES
@EMA
def test_off_means_off(dtype, ema_decay):
    LC.case_off_means_off(DEV, dtype, ema_decay)


def test_default_param_groups():
    LC.case_default_param_groups()


@DTYPES
@BAD
def test_skipped_step_leaves_everything_and_the_ratios_alone(dtype, bad):
    LC.case_skipped_step(DEV, dtype, bad)


@DTYPES
def test_lamb_is_reproducible(dtype):
    LC.case_reproducible(DEV, dtype)


@DTYPES
def test_absent_and_late_gradients(dtype):
    LC.case_absent_and_late_gradient(DEV, dtype)


@DTYPES
def test_state_dict_round_trip_keeps_keys_and_bits(dtype):
    LC.case_state_roundtrip(DEV, dtype)


def test_torch_adamw_state_dict_keeps_the_constructor_keys():
    LC.case_load_torch_adamw(DEV)


@DTYPES
def test_lamb_with_ema_and_accumulated_gradients(dtype):
    LC.case_lamb_ema_accumulate(DEV, dtype)


def test_end_to_end_fp32_three_steps_lamb_and_bounded_temperature():
    LC.case_end_to_end(DEV, TOY)
