"""The row-bucketed packed layout on the CPU: the kernel sources compiled against the wave64 emulator (tests/emu), the cases of
tests/test_bucket_packed_gpu.py thinned where a case costs emulator time (the kernel matrix: every form, fewer filler counts per form; end to
end: one loss variant, one multiple per storage type)."""
import dataclasses
import os
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import bucket_packed_cases as B  # noqa: E402
import packed_cases as P  # noqa: E402
from emu.build_emu import build  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

DEV = torch.device("cpu")
DTYPES = pytest.mark.parametrize("dtype", [P.F32, P.BF16], ids=["fp32", "bf16"])
SHORT = (3, 1, 70)          # (the plain form costs O(length) emulated waves per row: the GPU file runs LENS_A and LENS_B through it)
TOY = dataclasses.replace(O.CFG1, text_enc_depth=1, visual_enc_depth=1)


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


def test_layout():
    B.case_layout(DEV)


def test_cat_layouts_pads_once_at_the_end():
    B.case_cat_layouts(DEV)


def test_routes_of_the_text_layer_products():
    B.case_routes()


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("filler", B.FILLERS)
@pytest.mark.parametrize("lens", [P.LENS_A, P.LENS_B, B.LENS_ONE], ids=["mixed", "three_ones_and_288", "one_sample"])
def test_filler_rows_head_resident(lens, filler, causal):
    B.case_filler_rows(DEV, "resident", lens, filler, causal)


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("form,lens,filler", [("plain_fp32", B.LENS_ONE, 0), ("plain_fp32", SHORT, 5), ("plain_wide", B.LENS_ONE, 1),
                                              ("plain_wide", SHORT, 255), ("plain_long", P.LENS_LONG, 5)])
def test_filler_rows_plain_form(form, lens, filler, causal):
    B.case_filler_rows(DEV, form, lens, filler, causal, heads=2)


@DTYPES
@pytest.mark.parametrize("slot", [64, 128])
@pytest.mark.parametrize("lens,filler", [(P.LENS_A, 5), (P.LENS_B, 255), (B.LENS_ONE, 1), (B.LENS_ONE, 0)])
def test_filler_rows_pooled_backward(lens, filler, slot, dtype):
    B.case_pool_filler_rows(DEV, dtype, slot, lens, filler)


@pytest.mark.parametrize("pool_last", [False, True], ids=["dense_last", "pool_last"])
@pytest.mark.parametrize("kind", list(B.KINDS))
def test_bucketed_tower_against_the_oracle_fp32(kind, pool_last):
    B.case_vs_oracle(DEV, P.F32, kind, "infonce", 8, pool_last)


# (bf16 runs the dim-512 model the bf16 bars are stated for: one case per encoder here, the whole matrix in the GPU file)
@pytest.mark.parametrize("kind,pool_last,multiple", [("cls", False, 8), ("cls", True, 256), ("causal", True, 8), ("rotary", True, 8)])
def test_bucketed_tower_against_the_oracle_bf16(kind, pool_last, multiple):
    B.case_vs_oracle(DEV, P.BF16, kind, "infonce", multiple, pool_last)


def test_bucketed_aug_text():
    B.case_vs_oracle(DEV, P.F32, "cls", "dcl_multiview", 8, False)


def test_bucketed_layout_passed_in_with_aug_text():
    B.case_vs_oracle(DEV, P.F32, "cls", "dcl_multiview", 256, True, how="layout")


def test_bucketed_checkpointing():
    B.case_vs_oracle(DEV, P.F32, "cls", "infonce", 8, True, checkpoint_during_training=True)


def test_off_is_unchanged():
    B.case_off_is_unchanged(DEV, P.BF16)


def test_no_filler_gives_the_unbucketed_bits():
    B.case_no_filler_same_bits(DEV, P.BF16)


def test_cached_step_and_fused_adamw():
    B.case_cached_and_adamw(DEV, P.F32, TOY)


def test_embed_text():
    B.case_embed_text(DEV, P.BF16)
