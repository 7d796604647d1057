"""The weight EMA of x_clip_amd.optim.FusedAdamW on the MI355X (libxclip_hip.so): the cases of tests/ema_cases.py against torch's
clip_grad_norm_ + AdamW + the EMA recurrence run on the CPU in fp64; the end-to-end check trains the small CLIP of the optimizer's
end-to-end tests (oracle CFG1 through clip_cases.build_clip)."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import ema_cases as EC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
BAD = pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
DECAYS = pytest.mark.parametrize("decay,warmup", [(0.99, False), (0.9999, True)], ids=["0.99", "0.9999-warmup"])


@pytest.fixture(scope="module")
def dev():
    _lib._use_library_for_tests(None)
    _lib.lib()
    assert not _lib.is_emulator()
    return torch.device("cuda:0")


@DTYPES
@DECAYS
def test_ema_parity_over_ten_steps(dev, dtype, decay, warmup):
    EC.case_parity(dev, dtype, decay, warmup)


@DTYPES
def test_ema_does_not_disturb_the_update(dev, dtype):
    EC.case_update_untouched(dev, dtype)


def test_fused_ema_moves_where_a_bf16_ema_stalls(dev):
    EC.case_bf16_stall(dev)


@DTYPES
@BAD
def test_skipped_step_leaves_the_ema_alone(dev, dtype, bad):
    EC.case_skipped_step(dev, dtype, bad)


@DTYPES
def test_parameter_without_a_gradient_is_not_averaged(dev, dtype):
    EC.case_late_gradient(dev, dtype)


@DTYPES
def test_ema_is_reproducible(dev, dtype):
    EC.case_reproducible(dev, dtype)


@DTYPES
def test_state_dict_round_trip_keeps_the_ema_bits(dev, dtype):
    EC.case_state_roundtrip(dev, dtype)


@DTYPES
def test_state_dict_without_ema_loads_the_weights_as_ema(dev, dtype):
    EC.case_load_without_ema(dev, dtype)


def test_torch_adamw_state_dict_loads_the_weights_as_ema(dev):
    EC.case_load_torch_adamw(dev)


@DTYPES
def test_ema_weights_swaps_in_and_restores(dev, dtype):
    EC.case_ema_weights(dev, dtype)


def test_invalid_decay_is_refused(dev):
    EC.case_invalid_decay(dev)


def test_end_to_end_fp32_three_steps_with_ema(dev):
    EC.case_end_to_end(dev, O.CFG1)
