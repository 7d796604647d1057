"""The attention kernels with every CU busy, every head checked (MI355X, libxclip_hip.so -- the product build).

attention3.h / attention4.h / attention5.h bring whole K / V / Q / dO images in by LDS DMA behind counted waits, keep one or two
work-groups resident per CU and stagger the second work-group of a CU in time.  The emulator lands every DMA piece at once and runs one
work-group after the other, so it can see neither an early read, nor a missing wait, nor an LDS allocation handed over to the next
work-group; the kernel-level cases of tests/test_kernels_gpu.py launch 4 to 36 work-groups on 256 CUs.  This module is the hardware
gate for that regime, as test_gemm_full_size_every_element_and_repeatable is for the GEMM family: each case launches at least 1024
work-groups, compares out, lse and dqkv of EVERY head with a blocked fp64 reference built on the device (kernel_cases.attention_ref_blocked,
anchored against the CPU reference in tests/test_kernels_emu.py) under the bounds the small cases are held to, and launches forward and
backward three more times for the same bits.  One row per branch of xclip_attention_fwd / xclip_attention_bwd (csrc/xclip_attn.hip) that
the product build can reach; the id names the branch, read off the dispatch code:

  forward                                                       backward
  hd 128, bf16, n <= 288, no dropout  -> attention4.h           the same predicate -> attention4.h
  hd 128 otherwise                    -> attention.h, 2 halves  attn_delta_kernel + attention.h dQ / dK dV on two halves
  hd 64, bf16, n <= 288, no dropout   -> attention3.h           a5_takes(n, causal) and n / 32 >= 7 -> attention5.h, else attention3.h
     (cooperative tail when n % 32 in {1, 2} and n >= 64; staggered when batch x heads >= 1024 and its LDS <= 80 KB)
  hd 64, bf16 with dropout / fp32     -> attention.h            attn_delta_kernel + attention.h
  hd 64, bf16, n > 288                -> attention2.h           attn_delta_kernel + attention2.h
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kernel_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, FP32 = torch.bfloat16, torch.float32
DROP = (0.25, 0xC0FFEE1234567)


@pytest.fixture(scope="module", autouse=True)
def hip_library():
    from x_clip_amd import _lib
    _lib._use_library_for_tests(None)
    assert not _lib.is_emulator()
    _lib.lib()          # raises if libxclip_hip.so is missing -- no fallback
    yield


# batch, n, heads, head slot, dtype, text mask, causal, dropout
FULL = [
    pytest.param(1024, 257, 8, 64, BF16, True, False, None, id="b1024-n257-attention3_coop_tail_stagger-attention5"),
    pytest.param(1024, 256, 8, 64, BF16, True, False, None, id="b1024-n256-attention3_no_tail_stagger-attention5"),
    pytest.param(1024, 257, 8, 64, BF16, True, True, None, id="b1024-n257-causal-attention3_causal-attention3_bwd"),
    # the vision tower: 32 kept patches + CLS = 33 rows pad to two 32-row blocks, TWO waves per head, the second with one live query
    # (n < 64: no cooperative tail); one whole block, fewer than A5_MIN_BLOCKS = 7: attention3 backward
    pytest.param(1024, 33, 8, 64, BF16, False, False, None, id="b1024-n33-vision-attention3_two_waves_padded-attention3_bwd"),
    pytest.param(1024, 32, 8, 64, BF16, False, False, None, id="b1024-n32-attention3_one_wave_per_head-attention3_bwd"),
    pytest.param(1024, 65, 8, 64, BF16, False, False, None, id="b1024-n65-vision-attention3_coop_tail-attention3_bwd"),
    pytest.param(512, 193, 8, 64, BF16, True, False, None, id="b512-n193-attention3_coop_tail-attention3_bwd_below_A5_MIN_BLOCKS"),
    pytest.param(256, 257, 8, 128, BF16, True, False, None, id="b256-n257-wide-attention4_160KB_one_per_CU-attention4_bwd"),
    pytest.param(256, 257, 8, 128, BF16, True, True, None, id="b256-n257-wide-causal-attention4_causal-attention4_bwd_causal"),
    pytest.param(256, 257, 8, 64, FP32, True, False, None, id="b256-n257-fp32-tiled_attention_3_chunks_per_head-delta_dq_dkv"),
    pytest.param(256, 257, 8, 64, BF16, True, False, DROP, id="b256-n257-dropout-tiled_attention_bf16-delta_dq_dkv"),
    pytest.param(256, 257, 8, 128, FP32, True, False, None, id="b256-n257-wide-fp32-tiled_attention_two_halves-delta_pass_two_halves"),
    pytest.param(64, 577, 16, 64, BF16, False, False, None, id="b64-n577-attention2_19_chunks_per_head-delta_attention2_bwd"),
    pytest.param(64, 577, 16, 128, BF16, False, False, None, id="b64-n577-wide-tiled_attention_two_halves-delta_pass_two_halves"),
    pytest.param(64, 577, 16, 64, BF16, True, True, None, id="b64-n577-causal-masked-attention2_causal-delta_attention2_bwd_causal"),
]


@pytest.mark.parametrize("batch,n,heads,hd,dtype,masked,causal,drop", FULL)
def test_attention_full_occupancy_every_head_and_repeatable(request, batch, n, heads, hd, dtype, masked, causal, drop):
    """>= 1024 work-groups of the branch the id names: out, lse, dqkv of every head against the blocked fp64 reference (2 bf16 ulps of the
    whole tensor's scale / the fp32 bars of kernel_cases.close), outputs NaN-poisoned before each launch, four launches bit-identical"""
    K.case_attention_full(DEV, dtype, batch, n, heads, hd, masked, causal, drop, tag=request.node.callspec.id)


@pytest.mark.parametrize("batch,n,heads,row,causal", [pytest.param(1024, 257, 8, 0, False, id="b1024-n257-row0-2048_work_groups"),
                                                      pytest.param(512, 257, 8, 131, True, id="b512-n257-causal-row131-1024_work_groups")])
def test_attention_pool_full_occupancy_every_row_and_repeatable(request, batch, n, heads, row, causal):
    """attention_pool.h at the benchmark's shape (one wave per (sample, head), four per work-group), masked, pooled row 0; and causal with
    the pooled row in the middle: every row of out / lse / dq / dkv against the blocked reference, four launches bit-identical"""
    K.case_attention_pool_full(DEV, BF16, batch, n, heads, 64, row, causal, tag=request.node.callspec.id)
