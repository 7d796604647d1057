"""The pairwise sigmoid loss on two ranks (gloo, CPU: emulator kernels) with ragged batches (5 + 3) and an empty rank (8 + 0): the loss is
the same bits on both ranks and equals the single-process run on the concatenated batch; the local latent gradients are the
single-process slices; dtau and dbeta the single-process values."""
import os
import sys

import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dist_cases as D  # noqa: E402
import sigloss_cases as SC  # noqa: E402


def test_two_ranks_ragged_and_empty_batches(tmp_path):
    from x_clip_amd import _lib
    from emu.build_emu import build
    port = D.free_port()
    mp.spawn(SC.worker_sigloss, args=(2, port, str(tmp_path), "cpu"), nprocs=2, join=True)
    _lib._use_library_for_tests(build())
    try:
        SC.check_two_ranks(str(tmp_path), torch.device("cpu"))
    finally:
        _lib._use_library_for_tests(None)
