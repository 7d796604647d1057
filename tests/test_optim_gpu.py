"""x_clip_amd.optim.FusedAdamW on the MI355X (libxclip_hip.so): the cases of tests/optim_cases.py against torch's clip_grad_norm_ + AdamW
run on the CPU in fp64; the end-to-end checks train the small CLIP of the existing end-to-end tests (oracle CFG1 through clip_cases.build_clip)."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import optim_cases as OC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def dev():
    _lib._use_library_for_tests(None)
    _lib.lib()
    assert not _lib.is_emulator()
    return torch.device("cuda:0")


@DTYPES
def test_parity_with_torch_adamw_over_ten_steps(dev, dtype):
    OC.case_parity(dev, dtype)


def test_bf16_parameters_do_not_stall(dev):
    OC.case_bf16_stall(dev)


@DTYPES
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_skips_the_step_on_the_device(dev, dtype, bad):
    OC.case_skip_nonfinite(dev, dtype, bad)


@DTYPES
def test_reproducible_and_independent_of_gradient_layout(dev, dtype):
    OC.case_reproducible(dev, dtype)


@DTYPES
def test_gradient_that_appears_in_the_second_step(dev, dtype):
    OC.case_late_gradient(dev, dtype)


@DTYPES
def test_state_dict_round_trip_is_bit_exact(dev, dtype):
    OC.case_state_roundtrip(dev, dtype)


def test_loads_a_torch_adamw_state_dict(dev):
    OC.case_load_torch_adamw(dev)


def test_end_to_end_fp32_three_steps(dev):
    OC.case_end_to_end_fp32(dev, O.CFG1)


def test_end_to_end_bf16_loss_decreases(dev):
    OC.case_end_to_end_bf16(dev, O.CFG1)


def test_gradient_on_another_device_is_an_error(dev):
    """torch refuses `p.grad = <tensor on another device>` itself; the optimizer's own check (it hands raw addresses to a kernel) is reached
    here the way a gradient that bypassed that assignment would reach it: through the table rebuild"""
    p = torch.nn.Parameter(torch.zeros(16, device=dev))
    opt = OC.FusedAdamW([p])
    with pytest.raises(RuntimeError, match="a gradient lives on cpu, its parameter on cuda:0"):
        opt._rebuild(opt._one(), [torch.zeros(16)])
    assert opt.table_uploads == 0
