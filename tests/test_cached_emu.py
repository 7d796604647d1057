"""FusedAdamW.accumulate_* and x_clip_amd.cached.CachedContrastiveStep on the CPU: the kernels (csrc/kernels/optim.h grad_accum_kernel and
everything the towers and heads launch) compiled against the wave64 emulator, every case of tests/cached_cases.py.  The same cases run
on the MI355X in tests/test_cached_gpu.py."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import cached_cases as CC  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
# the emulator's twin of the GPU suite's small model: one layer per tower
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)
# bf16: a 256-wide model -- the dim-64 toy model's bf16 loss is off the oracle by more than DESIGN.md's 3e-4 in the one-pass step already
# (tests/test_clip_emu.py: measured 6.6e-4)
TOY_BF16 = dataclasses.replace(TOY, dim_text=256, dim_image=256, dim_latent=256)


def model_for(dtype):
    return TOY if dtype == torch.float32 else TOY_BF16


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("k", [1, 2, 5])
def test_accumulator_is_the_fp32_sum_and_is_rounded_once(dtype, k):
    CC.case_accumulate(DEV, dtype, k)


def test_sixty_four_bf16_gradients_are_summed_in_fp32():
    CC.case_why_fp32(DEV)


@DTYPES
def test_nonfinite_slice_gradient_skips_the_step(dtype):
    CC.case_nonfinite(DEV, dtype)


@DTYPES
def test_single_pass_through_the_accumulator_changes_no_bit(dtype):
    CC.case_noop_equivalence(DEV, dtype)


def test_step_inside_an_open_accumulation_raises():
    CC.case_open_accumulation_raises(DEV)


@DTYPES
@pytest.mark.parametrize("head", CC.HEADS)
@pytest.mark.parametrize("micro", [4, 3, 8, 16])
def test_cached_step_vs_one_pass_and_oracle(dtype, head, micro):
    CC.case_step(DEV, dtype, model_for(dtype), head, micro)


@DTYPES
def test_replay_is_exact_under_dropout_and_patch_dropout(dtype):
    CC.case_replay(DEV, dtype, model_for(dtype))


@DTYPES
def test_injected_patch_dropout_vs_one_pass_and_oracle(dtype):
    CC.case_replay_injected(DEV, dtype, model_for(dtype))


@DTYPES
def test_frozen_image_encoder(dtype):
    CC.case_freeze_image(DEV, dtype, model_for(dtype))


def test_track_metrics_changes_no_bit():
    CC.case_track_metrics_same_bits(DEV, torch.float32, TOY)


def test_checkpointing_changes_no_bit():
    CC.case_checkpoint_same_bits(DEV, torch.float32, TOY)


def test_unsupported_keywords_raise_at_construction():
    CC.case_raises(DEV)


def test_public_surface():
    import x_clip
    import x_clip_amd
    from x_clip.cached import CachedContrastiveStep
    assert x_clip.CachedContrastiveStep is x_clip_amd.CachedContrastiveStep is CachedContrastiveStep is CC.CachedContrastiveStep
