"""FusedAdamW.accumulate_* and x_clip_amd.cached.CachedContrastiveStep on the MI355X (libxclip_hip.so): the cases of tests/cached_cases.py.
fp32 on the small CLIP of the end-to-end tests (oracle CFG1), bf16 on the dim-512 model of the GPU suite's oracle checks."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import cached_cases as CC  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def model_for(dtype):
    return O.CFG1 if dtype == torch.float32 else CC.MID


@pytest.fixture(scope="module")
def dev():
    _lib._use_library_for_tests(None)
    _lib.lib()
    assert not _lib.is_emulator()
    return torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("k", [1, 2, 5])
def test_accumulator_is_the_fp32_sum_and_is_rounded_once(dev, dtype, k):
    CC.case_accumulate(dev, dtype, k)


def test_sixty_four_bf16_gradients_are_summed_in_fp32(dev):
    CC.case_why_fp32(dev)


@DTYPES
def test_nonfinite_slice_gradient_skips_the_step(dev, dtype):
    CC.case_nonfinite(dev, dtype)


@DTYPES
def test_single_pass_through_the_accumulator_changes_no_bit(dev, dtype):
    CC.case_noop_equivalence(dev, dtype)


def test_step_inside_an_open_accumulation_raises(dev):
    CC.case_open_accumulation_raises(dev)


@DTYPES
@pytest.mark.parametrize("head", CC.HEADS)
@pytest.mark.parametrize("micro", [4, 3, 8, 16])
def test_cached_step_vs_one_pass_and_oracle(dev, dtype, head, micro):
    CC.case_step(dev, dtype, model_for(dtype), head, micro)


@DTYPES
def test_replay_is_exact_under_dropout_and_patch_dropout(dev, dtype):
    CC.case_replay(dev, dtype, model_for(dtype))


@DTYPES
def test_injected_patch_dropout_vs_one_pass_and_oracle(dev, dtype):
    CC.case_replay_injected(dev, dtype, model_for(dtype))


@DTYPES
def test_frozen_image_encoder(dev, dtype):
    CC.case_freeze_image(dev, dtype, model_for(dtype))


@DTYPES
def test_track_metrics_changes_no_bit(dev, dtype):
    CC.case_track_metrics_same_bits(dev, dtype, model_for(dtype))


@DTYPES
def test_checkpointing_changes_no_bit(dev, dtype):
    CC.case_checkpoint_same_bits(dev, dtype, model_for(dtype))


def test_unsupported_keywords_raise_at_construction(dev):
    CC.case_raises(dev)


def test_cached_step_peaks_below_the_one_pass_step(dev):
    CC.case_memory(dev)
