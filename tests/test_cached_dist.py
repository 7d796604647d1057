"""CachedContrastiveStep on two ranks (gloo, emulator kernels): after sync.finish() the loss and every gradient are those of the one-pass
step run in the same group with the same GradSync(overlap=False), identical on both ranks; an overlapping GradSync is refused."""
import os
import sys

import pytest
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cached_cases as CC  # noqa: E402
import dist_cases as D  # noqa: E402


@pytest.mark.parametrize("head", ["infonce", "sigmoid"])
@pytest.mark.parametrize("sizes", [(4, 4), (4, 3)], ids=["even", "ragged"])
def test_two_ranks_cached_step_equals_one_pass(tmp_path, head, sizes):
    port = D.free_port()
    mp.spawn(CC.worker_two_ranks, args=(2, port, head, list(sizes), str(tmp_path), "cpu"), nprocs=2, join=True)
    CC.check_two_ranks(str(tmp_path), head)
