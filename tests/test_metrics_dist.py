"""contrastive_metrics on two ranks (gloo, CPU: emulator kernels) with ragged batches (5 + 3): the recall / mean-rank scalars are global
-- the same bits on both ranks and as the single-process result on the concatenated batch -- the per-row vectors are the rank's slice;
unequal global counts of texts and images raise on every rank."""
import os
import sys

import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dist_cases as D  # noqa: E402
import metrics_cases as MC  # noqa: E402


def test_two_ranks_ragged_batches(tmp_path):
    from x_clip_amd import _lib
    from emu.build_emu import build
    port = D.free_port()
    mp.spawn(MC.worker_metrics, args=(2, port, str(tmp_path), "cpu"), nprocs=2, join=True)
    _lib._use_library_for_tests(build())
    try:
        MC.check_two_ranks(str(tmp_path), torch.device("cpu"))
    finally:
        _lib._use_library_for_tests(None)
