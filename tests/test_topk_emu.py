"""x_clip_amd.retrieval / ops.simtopk* on the CPU: the top-k kernels (csrc/kernels/simtopk.h) compiled against the wave64 emulator, every
case of tests/topk_cases.py against dense torch in fp64.  The same cases run on the MI355X in tests/test_topk_gpu.py."""
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import topk_cases as TC  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@DTYPES
@pytest.mark.parametrize("nq,ng,d", TC.EXACT_GENERAL)
def test_exact_general_form(dtype, nq, ng, d):
    TC.case_exact(DEV, dtype, nq, ng, d)


@pytest.mark.parametrize("nq,ng,d,splits", TC.EXACT_RING)
def test_exact_ring_form(nq, ng, d, splits):
    TC.case_exact(DEV, torch.bfloat16, nq, ng, d, splits=splits)


@DTYPES
def test_all_equal_gallery_returns_the_lowest_columns(dtype):
    TC.case_all_equal_gallery(DEV, dtype)


def test_nan_row_is_all_padding():
    TC.case_nan_row(DEV)


@DTYPES
def test_empty_inputs_launch_nothing(dtype, monkeypatch):
    TC.case_empty(DEV, dtype, monkeypatch)


@DTYPES
@pytest.mark.parametrize("nq,ng,d,c", TC.REALISTIC)
def test_realistic_latents_within_the_accumulation_band(dtype, nq, ng, d, c):
    TC.case_realistic(DEV, dtype, nq, ng, d, c)


@DTYPES
def test_embed_is_half_of_forward_and_similarity_topk(dtype):
    TC.case_embed_matches_forward(DEV, dtype)


@DTYPES
def test_zero_shot_classifier(dtype):
    TC.case_zero_shot(DEV, dtype)


def test_fine_grained_head_has_no_single_latent():
    TC.case_fine_grained_head_raises(DEV, torch.float32)


def test_public_surface():
    import x_clip
    import x_clip_amd
    from x_clip.retrieval import similarity_topk, zero_shot_classifier
    assert x_clip.similarity_topk is x_clip_amd.similarity_topk is similarity_topk
    assert x_clip.zero_shot_classifier is x_clip_amd.zero_shot_classifier is zero_shot_classifier
    assert _lib.lib().xclip_simtopk_workspace_bytes(100, 130) == 5 * 3 * 100 * 4
