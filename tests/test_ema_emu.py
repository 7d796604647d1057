"""The weight EMA of x_clip_amd.optim.FusedAdamW on the CPU: adamw_ema_kernel (csrc/kernels/optim.h) compiled against the wave64 emulator,
every case of tests/ema_cases.py against torch's clip_grad_norm_ + AdamW + the EMA recurrence in fp64.  The same cases run on the MI355X in
tests/test_ema_gpu.py."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import ema_cases as EC  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
BAD = pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
DECAYS = pytest.mark.parametrize("decay,warmup", [(0.99, False), (0.9999, True)], ids=["0.99", "0.9999-warmup"])
# the toy-size twin of the GPU suite's end-to-end model: one layer per tower (as tests/test_optim_emu.py)
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@DECAYS
def test_ema_parity_over_ten_steps(dtype, decay, warmup):
    EC.case_parity(DEV, dtype, decay, warmup)


@DTYPES
def test_ema_does_not_disturb_the_update(dtype):
    EC.case_update_untouched(DEV, dtype)


def test_fused_ema_moves_where_a_bf16_ema_stalls():
    EC.case_bf16_stall(DEV)


@DTYPES
@BAD
def test_skipped_step_leaves_the_ema_alone(dtype, bad):
    EC.case_skipped_step(DEV, dtype, bad)


@DTYPES
def test_parameter_without_a_gradient_is_not_averaged(dtype):
    EC.case_late_gradient(DEV, dtype)


@DTYPES
def test_ema_is_reproducible(dtype):
    EC.case_reproducible(DEV, dtype)


@DTYPES
def test_state_dict_round_trip_keeps_the_ema_bits(dtype):
    EC.case_state_roundtrip(DEV, dtype)


@DTYPES
def test_state_dict_without_ema_loads_the_weights_as_ema(dtype):
    EC.case_load_without_ema(DEV, dtype)


def test_torch_adamw_state_dict_loads_the_weights_as_ema():
    EC.case_load_torch_adamw(DEV)


@DTYPES
def test_ema_weights_swaps_in_and_restores(dtype):
    EC.case_ema_weights(DEV, dtype)


def test_invalid_decay_is_refused():
    EC.case_invalid_decay(DEV)


def test_end_to_end_fp32_three_steps_with_ema():
    EC.case_end_to_end(DEV, TOY)
