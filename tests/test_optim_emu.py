"""x_clip_amd.optim.FusedAdamW on the CPU: the optimizer kernels (csrc/kernels/optim.h) compiled against the wave64 emulator, every case of
tests/optim_cases.py against torch's clip_grad_norm_ + AdamW in fp64.  The same cases run on the MI355X in tests/test_optim_gpu.py."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import optim_cases as OC  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
# the toy-size twin of the GPU suite's end-to-end model: one layer per tower
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
def test_parity_with_torch_adamw_over_ten_steps(dtype):
    OC.case_parity(DEV, dtype)


def test_bf16_parameters_do_not_stall():
    OC.case_bf16_stall(DEV)


@DTYPES
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_skips_the_step_on_the_device(dtype, bad):
    OC.case_skip_nonfinite(DEV, dtype, bad)


@DTYPES
def test_reproducible_and_independent_of_gradient_layout(dtype):
    OC.case_reproducible(DEV, dtype)


@DTYPES
def test_gradient_that_appears_in_the_second_step(dtype):
    OC.case_late_gradient(DEV, dtype)


@DTYPES
def test_state_dict_round_trip_is_bit_exact(dtype):
    OC.case_state_roundtrip(DEV, dtype)


def test_loads_a_torch_adamw_state_dict():
    OC.case_load_torch_adamw(DEV)


def test_end_to_end_fp32_three_steps():
    OC.case_end_to_end_fp32(DEV, TOY)


def test_end_to_end_bf16_loss_decreases():
    OC.case_end_to_end_bf16(DEV, TOY)


def test_public_surface():
    import x_clip_amd
    assert x_clip_amd.FusedAdamW is OC.FusedAdamW and issubclass(OC.FusedAdamW, torch.optim.Optimizer)
    lin = torch.nn.Sequential(torch.nn.Embedding(5, 8), torch.nn.Linear(8, 8), torch.nn.LayerNorm(8))
    decay, plain = OC.FusedAdamW.default_param_groups(lin, 0.2)
    assert [tuple(p.shape) for p in decay["params"]] == [(8, 8)] and decay["weight_decay"] == 0.2
    assert len(plain["params"]) == 4 and plain["weight_decay"] == 0.0
    opt = OC.FusedAdamW(lin.parameters(), lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5)
    assert opt.param_groups[0]["lr"] == 5e-3
    p = next(lin.parameters())
    p.grad = torch.zeros(8, 5).t()                              # the kernels walk plain memory: a strided gradient is refused, not misread
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    p.grad = torch.zeros(5, 8)
    opt.step()
    buf = p.grad                                                # the same address and dtype with another layout: still refused
    p.grad = None
    p.grad = buf.view(8, 5).t()
    assert p.grad.data_ptr() == buf.data_ptr()
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    del sched
