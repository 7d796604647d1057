"""GradSync + FusedAdamW on two ranks (gloo; CPU: emulator kernels, GPU: both ranks on cuda:0): after finish() every rank holds the same
averaged gradients, so parameters and grad_norm are the same bits on both ranks without a collective in the optimizer; the optimizer
leaves GradSync's in-place gradient slices alone and uploads its chunk table once."""
import dataclasses
import os
import sys

import pytest
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dist_cases as D  # noqa: E402
import optim_cases as OC  # noqa: E402


def _run(tmp_path, kind):
    from oracle import clip_oracle as O
    cfg = dataclasses.replace(O.CFG1, decoupled_contrastive_learning=True)
    port = D.free_port()
    mp.spawn(OC.worker_two_ranks, args=(2, port, dataclasses.asdict(cfg), 4, str(tmp_path), kind), nprocs=2, join=True)
    OC.check_two_ranks(str(tmp_path))


def test_two_ranks_gradsync_then_fused_adamw(tmp_path):
    _run(tmp_path, "cpu")


@pytest.mark.gpu
def test_two_ranks_gradsync_then_fused_adamw_gpu(tmp_path):
    _run(tmp_path, "cuda")
