"""The product against the reference (lucidrains/x-clip) on configurations that no other committed fixture holds: the reference ran
forward + backward once on each configuration below (`python oracle/make_golden.py --live '<SPECS[name] as JSON>' <name>.json`, where
the reference is importable) and the records are stored together in tests/golden/live_reference.npz (`pack_records` below); the product
runs the same parameters and inputs through the C-ABI kernels on the wave64 emulator, and loss, d(temperature), latents and every
parameter gradient must agree at the fixture bars (tests/clip_cases.py case_golden: loss 1e-5, gradient norms 5e-4)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import clip_oracle as O
from x_clip_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import clip_cases as C
from emu.build_emu import build  # noqa: E402

DEV = torch.device("cpu")
RECORDS = os.path.join(C.GOLDEN, "live_reference.npz")


def pack_records(json_paths, out=RECORDS):
    """<name>.json records -> one .npz: a record's long float lists whose values are all float32 (the reference's fp32 latents) as
    float32 arrays `<name>/<key>`, everything else as the record's JSON text `<name>/json` -- lossless, load_record gives the same dict back"""
    arrays = {}
    for path in json_paths:
        name = os.path.basename(path)[:-len(".json")]
        with open(path) as f:
            rec = json.load(f)
        for k, v in list(rec.items()):
            if isinstance(v, list) and len(v) > 64 and all(isinstance(x, float) and float(np.float32(x)) == x for x in v):
                arrays[f"{name}/{k}"] = np.asarray(rec.pop(k), np.float32)
        arrays[f"{name}/json"] = np.array(json.dumps(rec))
    np.savez_compressed(out, **arrays)


def load_record(name):
    with np.load(RECORDS) as z:
        rec = json.loads(str(z[f"{name}/json"]))
        rec.update({k.split("/", 1)[1]: z[k].tolist() for k in z.files if k.startswith(name + "/") and not k.endswith("/json")})
    return rec


@pytest.fixture(scope="module", autouse=True)
def emulator_library():
    _lib._use_library_for_tests(build())
    yield
    _lib._use_library_for_tests(None)


SPECS = {
    # three heads of 40 / 24 features in towers of different widths, DCL + CLOOB projections + one augmented view a side, odd batch
    "odd_heads_dcl_extra_multiview": dict(config=dict(dim_text=96, dim_image=64, dim_latent=48, text_heads=3, text_dim_head=40, visual_heads=3,
                                                      visual_dim_head=24, decoupled_contrastive_learning=True, extra_latent_projection=True),
                                          batch=5, n_aug_text=1, n_aug_image=1, param_seed=101, input_seed=202),
    # the similarity regulariser on the CLOOB projections (the reference cannot combine it with augmented views or FILIP: x_clip.py:779
    # indexes with a [1, b, b] mask), latent wider than both towers, one text head of 16 features
    "simreg_extra_wide_latent": dict(config=dict(dim_text=40, dim_image=72, dim_latent=88, text_heads=1, text_dim_head=16, visual_heads=2,
                                                 visual_dim_head=32, extra_latent_projection=True, sim_reg_loss_weight=0.3),
                                     batch=6, param_seed=107, input_seed=208),
    # FILIP + DCL + CLOOB projections on a batch of 7, rotary text encoder with 24-wide heads
    "filip_dcl_extra_rotary": dict(config=dict(use_all_token_embeds=True, decoupled_contrastive_learning=True, extra_latent_projection=True,
                                               text_rotary_pos_emb=True, text_dim_head=24, text_heads=3),
                                    batch=7, param_seed=103, input_seed=204),
    # wide heads (96 / 80) + patch dropout + three text views against one image view
    "wide_heads_patchdrop_m3n1": dict(config=dict(text_dim_head=96, text_heads=2, visual_dim_head=80, visual_heads=2, multiview_loss_weight=0.25),
                                      batch=3, n_aug_text=2, n_aug_image=0, patch_dropout=0.5, param_seed=105, input_seed=206),
    # the MLM side loss through a text tower of width 96 (three 32-wide heads), DCL, odd batch; the draw of masked positions is the reference's own
    "mlm_dcl_odd_width": dict(config=dict(use_mlm=True, dim_text=96, text_heads=3, text_dim_head=32, decoupled_contrastive_learning=True),
                              batch=5, param_seed=109, input_seed=210),
    # autoregressive text encoder (causal attention, EOS pooling) with CLOOB projections and one augmented text view
    "causal_extra_m2n1": dict(config=dict(text_causal_mask=True, text_has_cls_token=False, text_eos_id=3, extra_latent_projection=True,
                                          text_dim_head=48, text_heads=2),
                              batch=4, n_aug_text=1, n_aug_image=0, param_seed=111, input_seed=212),
}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_product_matches_live_reference(name):
    spec, rec = SPECS[name], load_record(name)
    # the stored record is the reference's run of exactly this specification (an edited spec without a regenerated record fails here)
    cfg = O.ClipConfig(**{**O.CFG1.ctor_kwargs(), **spec["config"]})
    assert rec["config"] == json.loads(json.dumps(cfg.ctor_kwargs()))
    assert (rec["batch"], rec["n_aug_text"], rec["n_aug_image"], rec["visual_patch_dropout"], rec["param_seed"], rec["input_seed"]) == \
        (spec["batch"], spec.get("n_aug_text", 0), spec.get("n_aug_image", 0), float(spec.get("patch_dropout", 0.0)), spec["param_seed"], spec["input_seed"])
    assert rec["loss"] == rec["loss"] and abs(rec["loss"]) < 1e3                      # (a finite reference loss)
    C.case_golden(DEV, name, rec=rec)
