"""xclip_gemm on row-strided operands and outputs, MI355X run of libxclip_hip.so: every case of tests/gemm_strided_cases.py that
tests/test_gemm_strided_emu.py runs on the emulator, plus what only the device has -- gemm8.h's hand-scheduled body and the row tail cut
at the device's own CU count."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gemm_strided_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def hip_library():
    from x_clip_amd import _lib
    _lib._use_library_for_tests(None)
    assert not _lib.is_emulator()
    _lib.lib()          # raises if libxclip_hip.so is missing -- no fallback
    yield


@pytest.mark.parametrize("name", list(G.SMALL))
def test_gemm_small_strided(name):
    """route 0, gemm_small.h"""
    G.run_case(DEV, G.SMALL[name])


@pytest.mark.parametrize("name", list(G.BIG))
def test_gemm_256_strided(name):
    """route 1: the ring loop (PLAIN / RES / TERMS / SLAB + reduce, banded order) and the two-stage TN loop (PLAIN, SLAB on the placed grid)"""
    G.run_case(DEV, G.BIG[name])


@pytest.mark.parametrize("name", list(G.GEMM8))
def test_gemm8_strided(name):
    """route 1, gemm8.h: the only small strided test of the asm body.  That these shapes run on it follows from g8_takes (plain, alpha 1,
    interior tiles, G8_MIN_KSTEPS K steps, one K slice, a grid of a multiple of 8 work-groups) -- the route query cannot tell it from the
    ring loop, which answers route 1 as well"""
    G.run_case(DEV, G.GEMM8[name])


@pytest.mark.parametrize("name", list(G.GENERIC))
def test_gemm_generic_strided(name):
    """route 3, gemm.h"""
    G.run_case(DEV, G.GENERIC[name])


@pytest.mark.parametrize("name", list(G.TAIL_GPU))
def test_gemm_row_tail_cut_strided(name):
    """route 2: 130 row tiles x 2 column tiles on 256 CUs = one round + 4 tail tiles as a split-K problem behind pointers xclip_gemm offsets
    by main_rows x lda / ldc / ldr itself; every element against fp32 row blocks built on the device (the tail rows are a block of their own)"""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    G.run_case(DEV, G.TAIL_GPU[name])


def test_gemm_strided_random_shapes():
    """the seeded sweep: 48 cases, none dropped; with FUZZ_SEED the routes 0 / 1 / 3 are taken 6 / 36 / 6 times (counted by the host query on the
    emulator build as well: tests/test_gemm_strided_emu.py)"""
    counts = G.case_gemm_strided_fuzz(DEV, 48, G.FUZZ_SEED)
    assert counts == {0: 6, 1: 36, 3: 6}, counts
