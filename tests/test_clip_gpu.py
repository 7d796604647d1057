"""MI355X end-to-end parity of the product `x_clip_amd.CLIP` through libxclip_hip.so: reference golden fixtures, the fp64
oracle at small and medium shapes (fp32 and bf16), and size-independent properties at the full BASELINE configs[1]
shape (local batch 1024, bf16)."""
import dataclasses
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import clip_cases as C  # noqa: E402
from oracle import clip_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MID = O.ClipConfig(dim_text=512, dim_image=512, dim_latent=512, num_text_tokens=2000, text_enc_depth=2, text_seq_len=70,
                   text_heads=8, visual_enc_depth=2, visual_image_size=128, visual_patch_size=32, visual_heads=8)


@pytest.fixture(scope="module", autouse=True)
def hip_library():
    from x_clip_amd import _lib
    _lib._use_library_for_tests(None)
    _lib.lib()                       # raises if libxclip_hip.so is missing: there is no fallback
    yield


@pytest.mark.parametrize("name", ["cfg1_infonce", "cfg1_dcl", "cfg1_extra_dcl", "cfg1_multiview", "cfg1_multiview_m3n1",
                                  "cfg1_patchdrop", "cfg1_filip", "cfg1_filip_dcl", "cfg1_simreg_extra", "cfg1_simreg_extra_dcl", "cfg1_rotary", "cfg1_rotary_dcl_multiview", "cfg1_filip_downsample", "cfg1_filip_downsample_extra_dcl", "cfg1_mlm", "cfg1_mlm_dcl_multiview", "cfg1_simsiam", "cfg1_simsiam_mlm_dcl", "cfg1_simclr", "cfg1_causal", "cfg1_causal_dcl_multiview", "cfg1_wide_heads", "cfg1_wide_heads_rotary_dcl", "cfg1_rotary_narrow24", "cfg1_rotary_narrow16_dcl"])
def test_clip_matches_reference_fixture(name):
    C.case_golden(DEV, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cfg1_vs_oracle(dtype):
    # (bf16: the dim-64 toy model's loss is the least accurate of the suite -- measured 6.6e-4; every other case holds 3e-4)
    C.case_vs_oracle(DEV, dtype, O.CFG1, 4, bf16_loss=1.4e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_high_temperature_vs_oracle(dtype):
    """exp(tau) = 200 end to end ON THE GPU (the NaN this pins was GPU-visible for two rounds and its end-to-end
    test ran on the emulator only) -- the reference multiplies by exp(tau) without a clamp (x_clip.py:574,736) and exponentiates
    without subtracting a maximum (:826); the product's log-sum-exp forms and one-exponential gradient must not depend on that.
    CLS head on the toy and the dim-512 model (the latter through the ring-loop kernels of simloss5.h), FILIP + DCL on the toy."""
    import dataclasses
    loose = dict(bf16_cos=0.97, bf16_rel=0.3, bf16_loss=5e-2)   # (bf16 logits of magnitude 100: the loss bar is absolute)
    C.case_vs_oracle(DEV, dtype, O.CFG1, 5, temperature=5.3, **loose)
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(O.CFG1, decoupled_contrastive_learning=True, use_all_token_embeds=True), 5, temperature=5.3, **loose)
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, decoupled_contrastive_learning=True), 264, temperature=5.3, label=f"mid b=264 exp(tau)=200 [{'fp32' if dtype == torch.float32 else 'bf16'}]", **loose)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_vs_oracle(dtype):
    C.case_vs_oracle(DEV, dtype, MID, 24)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pruned_text_rows_equal_dense_last_layer(dtype):
    """CLIP.prune_unused_rows (the text tower's last layer runs its row-wise part on the CLS rows only) against the dense last layer: same loss,
    same gradient of every parameter; mid-size model at b = 40 (+ an augmented text view under checkpointing, + two text slices), and the
    default architecture at b = 24 (the shapes bench.py runs: 257 positions, 8 heads)"""
    C.case_pruned_rows_equal_dense(DEV, dtype, MID, 40)
    C.case_pruned_rows_equal_dense(DEV, dtype, dataclasses.replace(MID, decoupled_contrastive_learning=True, extra_latent_projection=True), 16, n_aug_text=1,
                                   checkpoint=True)
    C.case_pruned_rows_equal_dense(DEV, dtype, dataclasses.replace(MID, text_rotary_pos_emb=True), 32, micro=2)
    C.case_pruned_rows_equal_dense(DEV, dtype, O.ClipConfig(num_text_tokens=3000), 24)


@pytest.mark.parametrize("checkpoint", [False, True], ids=["tape", "checkpoint"])
@pytest.mark.parametrize("row", [0, 7, 32])
@pytest.mark.parametrize("rotary,causal", [(False, False), (True, False), (False, True), (True, True)], ids=["plain", "rotary", "causal", "rotary_causal"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pool_row_equals_dense_row(dtype, rotary, causal, row, checkpoint):
    """text_encode(pool_row=r) for the first, a middle and the last row of 32 tokens + CLS (one whole 32-block of keys plus a tail row, a key
    count that is no multiple of the pooled kernel's keys per wave-load): the pooled last layer against row r of the dense one"""
    C.case_pool_row_equals_dense_row(DEV, dtype, rotary, causal, row, checkpoint, B=5, dim=128, heads=2, dim_head=64, n_tok=32)


# ---- the HEADLINE architecture (what bench.py times: O.ClipConfig() defaults = depth 6 / 6, text length 256 -> 257 positions, 64
# patches of which 32 are kept) against the fp64 oracle, every parameter gradient in full ---------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_default_arch_vs_oracle(dtype):
    """BASELINE configs[1] model at batch 12 (not a whole 16-byte chunk of rows in bf16), InfoNCE, patch dropout 0.5 with a fixed
    draw.  fp32: loss 1e-5, every gradient 2e-4 relative (the north star's fp32 bar); bf16: see clip_cases.case_vs_oracle"""
    C.case_vs_oracle(DEV, dtype, O.ClipConfig(), 12, patch_keep=32, seed=31, label=f"default arch InfoNCE b=12 keep=32 [{'fp32' if dtype == torch.float32 else 'bf16'}]")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_default_arch_dcl_multiview_vs_oracle(dtype):
    """BASELINE configs[2] / [4] head on the default towers: decoupled contrastive loss, one augmented text + one augmented image
    (four view pairs), patch dropout with a fixed draw for both image views"""
    import dataclasses
    cfg = dataclasses.replace(O.ClipConfig(), decoupled_contrastive_learning=True)
    C.case_vs_oracle(DEV, dtype, cfg, 8, n_aug_text=1, n_aug_image=1, patch_keep=32, seed=41,
                     label=f"default arch DCL multiview b=8 keep=32 [{'fp32' if dtype == torch.float32 else 'bf16'}]")


def test_mid_patch_dropout_multiview_dcl_fp32():
    import dataclasses
    cfg = dataclasses.replace(MID, decoupled_contrastive_learning=True, extra_latent_projection=True)
    C.case_vs_oracle(DEV, torch.float32, cfg, 16, n_aug_text=1, n_aug_image=1, patch_keep=8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_filip_mid_vs_oracle(dtype):
    """fine-grained head (use_all_token_embeds): token-level max / masked-mean reductions + routing backward"""
    import dataclasses
    cfg = dataclasses.replace(MID, use_all_token_embeds=True)
    # bf16: the token scores are rounded to bf16 before the max, so near-ties can route through a different token than the fp64
    # oracle (as the reference's own bf16 run would); the small, attention-only gradients (cls_token) show it most
    C.case_vs_oracle(DEV, dtype, cfg, 24, bf16_cos=0.985, bf16_rel=0.16)     # measured on the MI355X: rel 0.123, cosine 0.9924


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_sim_reg_extra_vs_oracle(dtype):
    """similarity regularisation (x_clip.py:773-784) on top of the CLOOB extra projections; batch 20 is not a whole 16-byte chunk"""
    import dataclasses
    cfg = dataclasses.replace(MID, extra_latent_projection=True, sim_reg_loss_weight=0.5)
    # bf16: D is a difference of two bf16-rounded similarity matrices (the reference's einsum outputs are rounded the same way), so
    # its relative error is larger than that of the other heads; the direction of every gradient still has to match
    C.case_vs_oracle(DEV, dtype, cfg, 20)                                      # measured: rel 0.016


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_narrow_heads_vs_oracle(dtype):
    """text_dim_head = 32 (rotary: the whole head is rotated), visual_dim_head = 48: zero-padded to the kernels' 64-wide heads"""
    import dataclasses
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, text_dim_head=32, visual_dim_head=48, text_rotary_pos_emb=True), 16)
    # rotary heads narrower than 32 (round 4): min(dim_head, 32) = 24 rotated features -- 12 pairs, the element-pair kernel
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, text_dim_head=24, text_heads=16, visual_dim_head=48, text_rotary_pos_emb=True), 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dh_text,dh_image", [(80, 96), (128, 80), (96, 128)])
def test_mid_wide_heads_vs_oracle(dtype, dh_text, dh_image):
    """text_dim_head / visual_dim_head in {80, 96, 128} (ordinary ViT head widths; the reference accepts any, x_clip.py:201-212):
    128-feature head slots = two 64-wide halves per head in the tiled attention kernels, narrower-than-slot heads zero-padded; the
    text heads are rotary (first 32 features of every slot rotated)"""
    import dataclasses
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, text_dim_head=dh_text, visual_dim_head=dh_image, text_rotary_pos_emb=True), 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_rotary_vs_oracle(dtype):
    """rotary text encoder (no absolute position table; q, k and v rotated over n + 1 positions, x_clip.py:155-176,221-223,328-330)"""
    import dataclasses
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, text_rotary_pos_emb=True), 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_causal_vs_oracle(dtype):
    """autoregressive text encoder: no CLS token, causal attention, the first EOS position pooled (x_clip.py:231-234,314,670-685)"""
    import dataclasses
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, text_causal_mask=True, text_eos_id=1999), 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_mlm_vs_oracle(dtype):
    """masked-language-model side loss through the shared text tower (mlm.py:96-109; x_clip.py:620-622, 857-860)"""
    import dataclasses
    # (with the oracle on the bf16 LayerNorm epsilon the temperature gradient -- a difference of O(1) sums over 16 x 16 logits -- is 3 % off)
    C.case_vs_oracle(DEV, dtype, dataclasses.replace(MID, use_mlm=True, text_ssl_loss_weight=0.3), 16)      # measured (bf16): rel 0.022


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mid_simsiam_vs_oracle(dtype):
    """SimSiam side loss around the shared vision tower (visual_ssl.py:207-259; x_clip.py:623): BatchNorm MLP projector / predictor,
    negative-cosine loss, running statistics"""
    import dataclasses
    cfg = dataclasses.replace(MID, use_visual_ssl=True, image_ssl_loss_weight=0.3, ssl_projection_size=256, ssl_projection_hidden_size=1024)
    # (bf16: the worst tensor is the last predictor bias, a sum over rows of vectors tangent to the unit sphere -- heavy cancellation)
    C.case_vs_oracle(DEV, dtype, cfg, 16, bf16_cos=0.992, bf16_rel=0.16)      # measured (bf16): rel 0.088, cosine 0.9961 (the last predictor bias)


def test_simclr_bf16_patch_dropout_runs():
    """SimCLR / NT-Xent variant (visual_ssl.py:263-299) in bf16 with the tower's random patch dropout: finite loss, every parameter reached
    (parity: tests/golden/cfg1_simclr.json above and the NT-Xent kernel cases)"""
    from x_clip_amd import CLIP, VisionTransformer
    from x_clip_amd.visual_ssl import SimCLR
    vit = VisionTransformer(**MID.vit_kwargs(0.5))
    ssl = SimCLR(vit, image_size=MID.visual_image_size, hidden_layer=-1, augment_fn=O.SslAugPair(), temperature=4.0)
    kw = {k: v for k, v in MID.ctor_kwargs().items() if k != "use_visual_ssl"}
    m = CLIP(**kw, image_encoder=vit, visual_ssl=ssl, use_visual_ssl=True).to(torch.bfloat16).to(DEV).train()
    text, image, _, _ = O.make_inputs(MID, 8, 3)
    loss = m(text.to(DEV), image.to(torch.bfloat16).to(DEV), return_loss=True)
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        if "_extra" not in k:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_simsiam_default_construction_and_patch_dropout():
    """CLIP(use_visual_ssl = True) builds SimSiam around its own vision tower (x_clip.py:536-552; default sizes 256 / 4096), which needs
    torchvision for the default augmentations -- absent here, so the constructor must say so; with augmentations supplied the side loss
    runs with the tower's random patch dropout (the target passes draw their own patches, as in the reference) and reaches every parameter"""
    from x_clip_amd import CLIP, VisionTransformer
    from x_clip_amd.visual_ssl import SimSiam
    try:
        import torchvision  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="torchvision"):
            CLIP(**{**MID.ctor_kwargs(), "use_visual_ssl": True})
    vit = VisionTransformer(**MID.vit_kwargs(0.5))
    ssl = SimSiam(vit, image_size=MID.visual_image_size, hidden_layer=-1, augment_fn=O.ssl_aug_one, augment_fn2=O.ssl_aug_two)
    kw = {k: v for k, v in MID.ctor_kwargs().items() if k != "use_visual_ssl"}
    m = CLIP(**kw, image_encoder=vit, visual_ssl=ssl, use_visual_ssl=True).to(torch.bfloat16).to(DEV).train()
    assert ssl.online_encoder.projector[0].weight.shape == (4096, MID.dim_image)
    text, image, _, _ = O.make_inputs(MID, 8, 3)
    loss = m(text.to(DEV), image.to(torch.bfloat16).to(DEV), return_loss=True)
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        if "_extra" not in k:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert int(ssl.online_encoder.projector[1].num_batches_tracked) == 4 and int(ssl.online_predictor[1].num_batches_tracked) == 2


def test_filip_multiview_extra_dcl_patchdrop_fp32():
    import dataclasses
    cfg = dataclasses.replace(MID, use_all_token_embeds=True, decoupled_contrastive_learning=True, extra_latent_projection=True)
    C.case_vs_oracle(DEV, torch.float32, cfg, 12, n_aug_text=1, n_aug_image=1, patch_keep=8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_filip_mid_fused_shape_vs_oracle(dtype):
    """MID with 64 image tokens and 70 text tokens: in bf16 the forward runs with its reductions inside the token-similarity GEMM
    (filip5.h; fp32 keeps the chunked form), DCL + one augmented text view"""
    import dataclasses
    from x_clip_amd import ops
    cfg = dataclasses.replace(MID, use_all_token_embeds=True, visual_image_size=256, decoupled_contrastive_learning=True)
    assert ops.filip_fused_ok(70, 64, 512, torch.bfloat16) and not ops.filip_fused_ok(70, 64, 512, torch.float32)
    C.case_vs_oracle(DEV, dtype, cfg, 12, n_aug_text=1, bf16_cos=0.985, bf16_rel=0.16)


def test_filip_chunked_workspace_matches_single_chunk(monkeypatch):
    """the image-chunked evaluation (bounded workspace) gives the same loss and gradients as one chunk"""
    import dataclasses
    from x_clip_amd import CLIP, losses
    cfg = dataclasses.replace(MID, use_all_token_embeds=True)
    torch.manual_seed(5)
    m = CLIP(**cfg.ctor_kwargs(), visual_patch_dropout=0.0).to(DEV).train()
    text, image, _, _ = O.make_inputs(cfg, 40, 8)
    text, image = text.to(DEV), image.float().to(DEV)
    l1 = m(text, image, return_loss=True); l1.backward()
    g1 = m.to_visual_latent.weight.grad.clone(); m.zero_grad()
    monkeypatch.setattr(losses, "_FILIP_CHUNK_BYTES", 40 * cfg.text_seq_len * cfg.num_patches * 4 * 9)      # ~9 images per chunk -> 8
    l2 = m(text, image, return_loss=True); l2.backward()
    assert abs(float(l1.detach()) - float(l2.detach())) < 1e-6
    torch.testing.assert_close(g1, m.to_visual_latent.weight.grad, rtol=1e-4, atol=1e-7)


def test_filip_odd_chunks_vs_oracle(monkeypatch):
    """fine-grained head with 9 image tokens and 22 images: no chunk of images gives a whole 16-byte chunk of similarity columns, and
    the workspace bound is lowered so that several partial chunks are walked (N / K padding of the token GEMMs)"""
    import dataclasses
    from x_clip_amd import losses
    cfg = dataclasses.replace(MID, use_all_token_embeds=True, visual_image_size=96)
    monkeypatch.setattr(losses, "_FILIP_CHUNK_BYTES", 22 * cfg.text_seq_len * 9 * 4 * 5)       # ~5 images per chunk
    C.case_vs_oracle(DEV, torch.float32, cfg, 22)
    C.case_vs_oracle(DEV, torch.bfloat16, cfg, 22, bf16_cos=0.993, bf16_rel=0.16)   # measured: rel 0.080, cosine 0.9968


def test_vit_l_like_shapes_vs_oracle():
    """BASELINE configs[4]-like widths (text dim 768 / 12 heads, vision dim 1024 / 16 heads, patch 14 -> 588-wide patch rows padded
    to the 16-byte chunk, latent 768, one augmented text + image, patch dropout) at a small depth / batch"""
    cfg = O.ClipConfig(dim_text=768, dim_image=1024, dim_latent=768, num_text_tokens=3000, text_enc_depth=1, text_seq_len=77,
                       text_heads=12, visual_enc_depth=2, visual_image_size=56, visual_patch_size=14, visual_heads=16)
    C.case_vs_oracle(DEV, torch.float32, cfg, 8, n_aug_text=1, n_aug_image=1, patch_keep=8)
    C.case_vs_oracle(DEV, torch.bfloat16, cfg, 8, n_aug_text=1, n_aug_image=1, patch_keep=8)


# ---- BASELINE configs[4] and configs[3] at their REAL architectures against the fp64 oracle -------
VITL = O.ClipConfig(dim_text=768, dim_image=1024, dim_latent=768, num_text_tokens=49408, text_enc_depth=12, text_seq_len=77,
                    text_heads=12, visual_enc_depth=24, visual_image_size=336, visual_patch_size=14, visual_heads=16,
                    decoupled_contrastive_learning=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_vit_l_14_336_full_depth_vs_oracle(dtype):
    """what `bench.py --config vitl` times, tower for tower: ViT-L/14 at 336 (576 patches, 288 kept = attention3's A3_MAX_N, depth 24,
    dim 1024, 16 heads, 588-wide patch rows padded to 592), text dim 768 depth 12 length 77, latent 768, DCL, one augmented text + one
    augmented image (four view pairs), activation checkpointing; batch 2 (x 2 views), every parameter gradient in full"""
    # (bf16 loss bar: at batch 2 with DCL the loss itself is 0.07 and 36 bf16 layers put ~1e-3 on the unit-norm latents: measured 6.8e-4;
    #  every gradient holds the default bars -- measured 2.1 % / cosine 0.99977)
    # (fp32 -- not what the bench times -- walks the same shapes through 4 / 2 layers: the fp64 oracle of the full depth is a minute of host time,
    #  and the GPU suite must stay well inside the driver's limit; the bf16 run keeps every layer)
    import dataclasses
    fp32 = dtype == torch.float32
    cfg = dataclasses.replace(VITL, visual_enc_depth=4, text_enc_depth=2) if fp32 else VITL
    C.case_vs_oracle(DEV, dtype, cfg, 2, n_aug_text=1, n_aug_image=1, patch_keep=288, seed=51, checkpoint_during_training=True, bf16_loss=1.4e-3,
                     label=f"configs[4] arch ViT-L/14-336 depth {'4/2' if fp32 else '24/12'} DCL multiview b=2 keep=288 ckpt [{'fp32' if fp32 else 'bf16'}]")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_filip_config3_real_arch_vs_oracle(dtype):
    """what `bench.py --filip` times: default towers (dim 512, depth 6 / 6) on image 224 / patch 16 (196 patches, 98 kept), text length
    77, fine-grained token-patch similarity (77 x 98 per pair); batch 8"""
    import dataclasses
    cfg = dataclasses.replace(O.ClipConfig(), use_all_token_embeds=True, visual_image_size=224, visual_patch_size=16, text_seq_len=77)
    C.case_vs_oracle(DEV, dtype, cfg, 8, patch_keep=98, seed=61, bf16_cos=0.985, bf16_rel=0.16,
                     label=f"configs[3] arch FILIP 224/16 seq 77 depth 6/6 b=8 keep=98 [{'fp32' if dtype == torch.float32 else 'bf16'}]")


def test_full_size_step_eight_live_rows_vs_oracle():
    """BASELINE configs[1] at its full size (local batch 1024, bf16, patch dropout 0.5) pinned to the ORACLE, not to itself: the encoders
    are row independent, so with an upstream latent gradient that is non-zero on 8 samples only, every parameter gradient of the
    1024-sample step must equal the oracle's gradient on those 8 samples alone.  The other 1016 samples still walk through every
    kernel at full size (M = 263,168-row GEMMs, split-K weight gradients, streamed stores, 8192-head attention launches) and must
    contribute exact zeros -- any stale slab, stray tile or cross-row leak shows up in the comparison.  Also compared with the
    PRODUCT's own 8-sample step (same bf16 arithmetic per row: only the split-K summation order differs)."""
    C.case_live_rows(DEV, O.ClipConfig(), 1024, [0, 5, 255, 256, 511, 640, 1022, 1023], torch.bfloat16, label="configs[1] FULL SIZE b=1024 bf16")


def test_filip_config4_like_bf16_runs_at_scale():
    """BASELINE configs[3]-like FILIP step (image 224 patch 16 -> 98 kept patches, seq 77) at local batch 256: finite loss near
    ln(B), finite gradients, chunked workspace path exercised"""
    from x_clip_amd import CLIP
    torch.manual_seed(0)
    m = CLIP(use_all_token_embeds=True, visual_image_size=224, visual_patch_size=16, text_seq_len=77, text_enc_depth=2,
             visual_enc_depth=2).to(torch.bfloat16).to(DEV).train()
    b = 256
    g = torch.Generator().manual_seed(7)
    text = torch.randint(0, 10000, (b, 77), generator=g).to(DEV)
    image = torch.randn(b, 3, 224, 224, generator=g).to(torch.bfloat16).to(DEV)
    loss = m(text, image, return_loss=True)
    loss.backward()
    assert torch.isfinite(loss) and abs(float(loss.detach()) - math.log(b)) < 1.0
    for k, p in m.named_parameters():
        if "_extra" not in k:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_checkpointing_is_bit_identical():
    from x_clip_amd import CLIP
    torch.manual_seed(3)
    a = CLIP(**MID.ctor_kwargs(), visual_patch_dropout=0.0).to(DEV).train()
    b = CLIP(**MID.ctor_kwargs(), visual_patch_dropout=0.0, checkpoint_during_training=True).to(DEV).train()
    b.load_state_dict(a.state_dict())
    text, image, _, _ = O.make_inputs(MID, 8, 5)
    for m in (a, b):
        m(text.to(DEV), image.float().to(DEV), return_loss=True).backward()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if pa.grad is None:
            assert pb.grad is None
        elif "token_emb" in k or k.endswith(".g") or "pos_emb" in k or "cls_token" in k or k.endswith("bias") or k == "temperature":
            torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-4, atol=1e-6)      # fp32 atomics: order varies
        else:
            assert torch.equal(pa.grad, pb.grad), k


def test_freeze_and_early_returns():
    C.case_freeze_and_early_returns(DEV, MID)


def test_pluggable_encoders_head_only():
    C.case_pluggable_encoders_head_only(DEV, B=96, d=128)


def test_full_size_properties_bf16():
    """BASELINE configs[1] (default CLIP, local batch 1024, bf16): encoders are row-independent (latents of a 1024 batch
    equal the latents of its two halves), the fused loss equals an fp64 evaluation from the latents, gradients are
    finite and the step is repeatable."""
    from x_clip_amd import CLIP
    torch.manual_seed(0)
    m = CLIP(visual_patch_dropout=0.0).to(torch.bfloat16).to(DEV).train()
    b = 1024
    g = torch.Generator().manual_seed(1234)
    text = torch.randint(0, 10000, (b, 256), generator=g).to(DEV)
    image = torch.randn(b, 3, 256, 256, generator=g).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        tl, il = m(text, image, return_latents=True)
        tl2 = torch.cat([m(text[i: i + 512], image[i: i + 512], return_latents=True)[0] for i in (0, 512)])
    # Rounds 1-3 held this to bit equality.  Since round 4 the last partial round of a persistent GEMM runs as a split-K problem
    # (xclip_api.hip gemm2_tail_cut): WHICH rows form that tail depends on the batch size, and their fp32 sums are associated per K slice --
    # the same products, another order of addition.  What is held now: every sample whose rows lie in no tail (all but the last few of
    # the full batch and of each half) keeps its latents BIT for bit; the others move by a few bf16 ulps of the latent scale (six layers
    # downstream of a one-ulp difference).
    d = (tl.float() - tl2.float()).abs()
    moved = int((d > 0).any(dim=1).sum())
    ulp = float(tl.float().abs().max()) * 2.0 ** -7
    assert moved <= 16 and float(d.max()) <= 8 * ulp, (moved, float(d.max()), ulp)
    # ... and with ops.BATCH_INVARIANT_GEMM the round-3 property holds again: no product is cut, every sample bit for bit
    import x_clip_amd
    was = x_clip_amd.set_batch_invariant(True)
    try:
        with torch.no_grad():
            tl3, _ = m(text, image, return_latents=True)
            tl4 = torch.cat([m(text[i: i + 512], image[i: i + 512], return_latents=True)[0] for i in (0, 512)])
    finally:
        x_clip_amd.set_batch_invariant(was)
    assert torch.equal(tl3, tl4), "with BATCH_INVARIANT_GEMM text latents must not depend on which other rows share the batch"
    # batch sizes on BOTH sides of the small-kernel boundary (gemm_small.h takes the pooled layer's / the latent products by their
    # row count: B = 1024 yes, B = 1000 (not a multiple of 64) and B = 2048 (beyond its FLOP limit for the 4096-wide products) no)
    from x_clip_amd import ops
    limit = ops.gemm_small_limit()
    was = x_clip_amd.set_batch_invariant(True)
    try:
        assert ops.gemm_small_limit() == 0
        with torch.no_grad():
            a1000 = m(text[:1000], image[:1000], return_latents=True)
            a1024 = m(text, image, return_latents=True)
            t2, i2 = torch.cat([text, text.flip(0)]), torch.cat([image, image.flip(0)])
            a2048 = m(t2, i2, return_latents=True)
    finally:
        x_clip_amd.set_batch_invariant(was)
    assert ops.gemm_small_limit() == limit
    for k in (0, 1):
        assert torch.equal(a1000[k], a1024[k][:1000]), ("1000 vs 1024", k)
        assert torch.equal(a1024[k], a2048[k][:1024]), ("1024 vs 2048", k)
    loss = m(text, image, return_loss=True)
    loss.backward()
    S = math.e * tl.double() @ il.double().t()
    want = 0.5 * ((S.exp().sum(1).log() - S.diag()).mean() + (S.exp().sum(0).log() - S.diag()).mean())
    assert abs(float(loss.detach()) - float(want)) < 2e-3 * float(want), (float(loss.detach()), float(want))
    for k, p in m.named_parameters():
        if "_extra" in k:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    g1 = m.to_text_latent.weight.grad.clone()
    m.zero_grad()
    m(text, image, return_loss=True).backward()
    assert torch.equal(g1, m.to_text_latent.weight.grad)


def test_short_and_fully_padded_text():
    C.case_short_and_padded_text(DEV)


def test_no_kernel_reads_unwritten_memory():
    """ViT-L-like widths (the shape whose uneven split-K once reduced an unwritten slab) with every torch.empty the product makes
    poisoned with NaN"""
    cfg = O.ClipConfig(dim_text=768, dim_image=1024, dim_latent=768, num_text_tokens=3000, text_enc_depth=1, text_seq_len=77,
                       text_heads=12, visual_enc_depth=2, visual_image_size=56, visual_patch_size=14, visual_heads=16)
    with C.poisoned_empty():
        C.case_vs_oracle(DEV, torch.bfloat16, cfg, 8, n_aug_text=1, n_aug_image=1, patch_keep=8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_transformer_dropout_vs_oracle(dtype):
    """Transformer(attn_dropout = 0.2, ff_dropout = 0.1) (x_clip.py:185-212,241) at dim 512 / 8 heads / 71 tokens in training mode: output
    and every gradient against the oracle evaluating the reference's dropout arithmetic on the product's keep-masks"""
    from x_clip_amd import functional as XF
    from x_clip_amd.clip import Transformer
    torch.manual_seed(5)
    dim, depth, heads, dh, b, n = 512, 2, 8, 64, 6, 71
    net = Transformer(dim, depth=depth, heads=heads, dim_head=dh, attn_dropout=0.2, ff_dropout=0.1).to(dtype).to(DEV).train()
    x = torch.randn(b, n, dim).to(dtype)
    mask = torch.ones(b, n, dtype=torch.bool)
    mask[1, 40:] = False
    g = torch.randn(b, n, dim).to(dtype)
    seed = 0x2545F4914F6CDD1
    orig = XF._draw_seed
    XF._draw_seed = lambda: seed
    try:
        xi = x.to(DEV).requires_grad_(True)
        y = net(xi, mask=mask.to(DEV))
        y.backward(g.to(DEV))
    finally:
        XF._draw_seed = orig
    sd = {"t." + k: v.detach().double().cpu().requires_grad_(True) for k, v in net.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    fp32 = dtype == torch.float32
    with O.layer_norm_eps(1e-5 if fp32 else 1e-3):
        ref = O.transformer(x64, sd, "t.", depth, heads, dh, mask, dropout=(0.2, 0.1, seed))
        ref.backward(g.double())
    err = float((y.detach().double().cpu() - ref.detach()).abs().max()) / float(ref.detach().abs().max())
    assert err < (2e-5 if fp32 else 3e-2), err
    assert float((xi.grad.double().cpu() - x64.grad).norm() / x64.grad.norm()) < (2e-4 if fp32 else 5e-2)
    for k, p in net.named_parameters():
        rg = sd["t." + k].grad
        rel = float((p.grad.double().cpu() - rg).norm() / rg.norm())
        assert rel < (2e-4 if fp32 else 8e-2), (k, rel)
