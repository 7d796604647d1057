"""xclip_gemm on row-strided operands and outputs, CPU run: every kernel family behind the entry point (compiled against the wave64
emulator) on views into NaN- / pattern-filled buffers, each of the five leading dimensions different from its width and from the others
(tests/gemm_strided_cases.py).  The same cases run on the MI355X in tests/test_gemm_strided_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import gemm_strided_cases as G  # noqa: E402
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


@pytest.mark.parametrize("name", list(G.SMALL))
def test_gemm_small_strided(name):
    """route 0, gemm_small.h"""
    G.run_case(DEV, G.SMALL[name])


@pytest.mark.parametrize("name", list(G.BIG))
def test_gemm_256_strided(name):
    """route 1: the ring loop (PLAIN / RES / TERMS / SLAB + reduce, banded order) and the two-stage TN loop (PLAIN, SLAB on the placed grid)"""
    G.run_case(DEV, G.BIG[name])


def test_gemm8_shapes_strided_on_the_ring_loop():
    """the smallest product g8_takes gives to gemm8.h on the MI355X; here (no twin of an asm unit) it runs on the ring loop"""
    layout, M, N, K_, kw = G.GEMM8["nn 4352x2048x512"]
    G.run_case(DEV, (layout, M, N, K_, dict(kw, contiguous_twin=False)))         # (one emulated launch of 4.6 GFLOP is enough: 7 s)


@pytest.mark.parametrize("name", list(G.GENERIC))
def test_gemm_generic_strided(name):
    """route 3, gemm.h"""
    G.run_case(DEV, G.GENERIC[name])


def test_gemm_row_tail_cut_strided():
    """route 2 (xclip_api.hip gemm2_tail_cut; the pointer arithmetic of xclip_gemm's cut branch): the policy plans for the device's CU count, so
    the emulator is told it has 4 in an interpreter of its own, as tests/test_kernels_emu.py::test_gemm_row_tail_as_split_k does: 1280 rows =
    5 row tiles x 2 column tiles = 2 rounds + 2 tiles -> 4 row tiles in the main launch, 1 as slabs; plain, + residual, in place"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from x_clip_amd import _lib\n"
        "from emu.build_emu import build\n"
        "_lib._use_library_for_tests(build())\n"
        "import gemm_strided_cases as G\n"
        "for case in G.TAIL_EMU:\n"
        "    assert G.run_case(torch.device('cpu'), case) == 2\n"
        "print('strided tail ok')\n") % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, XCLIP_EMU_CUS="4"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "strided tail ok" in out.stdout, out.stderr[-2000:]


def test_gemm_strided_random_shapes():
    """the seeded sweep at the emulator's sizes: 12 cases, none dropped (FUZZ_SEED: routes 0 / 1 / 3 taken 2 / 9 / 1 times)"""
    counts = G.case_gemm_strided_fuzz(DEV, 12, G.FUZZ_SEED, **G.EMU_CAPS)
    assert counts == {0: 2, 1: 9, 3: 1}, counts


def test_gemm_strided_sweep_reaches_every_route_on_the_device_list():
    """the 48 cases tests/test_gemm_strided_gpu.py runs (the emulator plans for the MI355X's 256 CUs: the same routes): each of the routes
    0, 1 and 3 at least 6 times -- with FUZZ_SEED 6 / 36 / 6"""
    counts = G.fuzz_routes(48, G.FUZZ_SEED)
    assert counts == {0: 6, 1: 36, 3: 6}, counts
