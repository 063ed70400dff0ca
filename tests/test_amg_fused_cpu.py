"""CPU side of the fused automatic-mask-generator path (no GPU needed): the C ABI surface, the generator's fall-back on
predictors without ``predict_points_batch``, and the two host restatements the GPU tests (tests/test_gpu_amg_fused.py)
compare the device against — HQ-SAM's ``multimask_output=True`` rule and the per-mask score record."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sam_ref as R
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_sam_decode_points", "sampt_sam_decode_points_workspace_bytes", "sampt_amg_score", "sampt_amg_binarize")


# --------------------------------------------------------------------------------------------------------------------
# helper 3: MaskDecoderHQ.forward with multimask_output=True, from the oracle's public pieces
# --------------------------------------------------------------------------------------------------------------------
def hq_mask_decoder_ref(sd, cfg, image_embeddings, image_pe, sparse, dense, hq_feat, multimask_output=True,
                        _hf_samhq_quirk=False):
    """-> (low_res (B,1,4g,4g), iou (B,1), iou of mask tokens 1..3 (B,3)).  ``oracle.sam_ref.mask_decoder`` restated up to its
    output slice, then upstream sam-hq's rule (**upstream-recall**: the source is not in the reference tree): with
    ``multimask_output`` the SAM mask of the mask token (1..3) with the largest predicted IoU, else mask token 0; + the HQ mask
    (``hq_token_only=False``).  ``_hf_samhq_quirk`` as in ``oracle.sam_ref.mask_decoder`` (transformers' SamHQMaskDecoder upscales
    the pre-transformer embedding with H / W swapped)."""
    nmt = cfg.num_multimask_outputs + 1
    out_tok = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"],
                         sd["mask_decoder.hf_token.weight"]], dim=0)
    tokens = torch.cat([out_tok.unsqueeze(0).expand(sparse.shape[0], -1, -1), sparse], dim=1)
    src = torch.repeat_interleave(image_embeddings, tokens.shape[0], dim=0) + dense
    pos = torch.repeat_interleave(image_pe, tokens.shape[0], dim=0)
    b, c, h, w = src.shape
    hs, keys = R.two_way_transformer(sd, cfg, src, pos, tokens)
    iou_tok, mask_toks = hs[:, 0, :], hs[:, 1:1 + nmt, :]
    src = src.transpose(2, 3).reshape(b, c, h, w) if _hf_samhq_quirk else keys.transpose(1, 2).reshape(b, c, h, w)
    U = "mask_decoder.output_upscaling"
    up = F.conv_transpose2d(src, sd[U + ".0.weight"], sd[U + ".0.bias"], stride=2)
    up = F.gelu(R._ln2d(up, sd, U + ".1"))
    up = F.gelu(F.conv_transpose2d(up, sd[U + ".3.weight"], sd[U + ".3.bias"], stride=2))
    hyper = torch.stack([R._mlp3(sd, f"mask_decoder.output_hypernetworks_mlps.{i}", mask_toks[:, i, :], 3)
                         for i in range(nmt)], dim=1)
    b, c, h, w = up.shape
    masks = (hyper @ up.view(b, c, h * w)).view(b, -1, h, w)
    iou = R._mlp3(sd, "mask_decoder.iou_prediction_head", iou_tok, cfg.iou_head_depth)
    E = "mask_decoder.embedding_maskfeature"
    uh = F.conv2d(up, sd[E + ".0.weight"], sd[E + ".0.bias"], padding=1)
    uh = F.gelu(R._ln2d(uh, sd, E + ".1"))
    uh = F.conv2d(uh, sd[E + ".3.weight"], sd[E + ".3.bias"], padding=1) + hq_feat
    hyper_hq = R._mlp3(sd, "mask_decoder.hf_mlp", hs[:, 1 + nmt, :], 3)
    mask_hq = (hyper_hq.unsqueeze(1) @ uh.view(b, c, h * w)).view(b, 1, h, w)
    if multimask_output:
        best = iou[:, 1:].argmax(dim=1)
        ar = torch.arange(b)
        return masks[:, 1:][ar, best][:, None] + mask_hq, iou[:, 1:][ar, best][:, None], iou[:, 1:]
    return masks[:, 0:1] + mask_hq, iou[:, 0:1], iou[:, 1:]


# --------------------------------------------------------------------------------------------------------------------
# helper 4: the score record of a stack of full-resolution logits, with the generator's own expressions
# --------------------------------------------------------------------------------------------------------------------
def score_record_ref(logits: torch.Tensor, thr: float, off: float) -> torch.Tensor:
    """logits (N,H,W) -> int32 (N,8) = [hi, lo, area, x0, y0, x1, y1, 0]: the two counts ``calculate_stability_score`` divides,
    the pixel count of ``logits > thr`` and ``batched_mask_to_box`` of it."""
    hi = (logits > (thr + off)).flatten(-2).sum(-1, dtype=torch.int32)
    lo = (logits > (thr - off)).flatten(-2).sum(-1, dtype=torch.int32)
    st, ref = hi / lo, A.calculate_stability_score(logits, thr, off)
    assert torch.equal(torch.nan_to_num(st, nan=-1.0), torch.nan_to_num(ref, nan=-1.0))
    masks = logits > thr
    area = masks.flatten(-2).sum(-1, dtype=torch.int32)
    box = A.batched_mask_to_box(masks).to(torch.int32)
    return torch.cat([hi[:, None], lo[:, None], area[:, None], box, torch.zeros_like(hi)[:, None]], dim=1)


def _image(h, w, seed):
    from sam_pt_amd.synth import synthetic_clip
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


# --------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_binds_and_exports_the_new_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
    # the launch functions follow the house style: int return code, stream last
    for name in ("sampt_sam_decode_points", "sampt_amg_score", "sampt_amg_binarize"):
        res, args = _lib._SIGS[name]
        assert res is _lib.c_int and args[-1] is _lib._P


def test_generator_falls_back_without_predict_points_batch():
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    img = _image(96, 128, 3)
    kw = dict(points_per_side=4, points_per_batch=5, pred_iou_thresh=0.0, stability_score_thresh=0.0,
              stability_score_offset=0.02)
    auto = A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), fused=None, **kw)
    plain = A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), fused=False, **kw)
    assert auto.fused is False and plain.fused is False
    a, b = auto.generate(img), plain.generate(img)
    assert len(a) == len(b) > 0
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["segmentation"], rb["segmentation"])
        for k in ("area", "bbox", "predicted_iou", "point_coords", "crop_box"):
            assert ra[k] == rb[k], k
        assert ra["stability_score"] == rb["stability_score"] or (np.isnan(ra["stability_score"]) and np.isnan(rb["stability_score"]))
    with pytest.raises(ValueError, match="predict_points_batch"):
        A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), fused=True, **kw)


def test_hq_multimask_helper_vs_oracle_and_transformers():
    """Helper 3 is the oracle's HQ decoder when ``multimask_output=False`` (exactly) and transformers' SamHQMaskDecoder's FIRST
    returned mask / IoU when ``multimask_output=True`` (HF sorts the three by IoU; bars of test_sam_hq_oracle_vs_hf_golden)."""
    pytest.importorskip("transformers.models.sam_hq.modeling_sam_hq")
    from oracle import hf_crosscheck as HF
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72, hq=True)
    x = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        emb, interm = R.image_encoder(sd, cfg, x, return_interm=True)
        hq = R.hq_features(sd, emb, interm)
        pe = R.dense_pe(sd, cfg)
        model = HF.build_hf_hq_model(cfg, sd)
        hf_emb, hf_interm = HF.hf_hq_embed(model, x)
        chosen = set()
        for x0, y0 in A.build_point_grid(3) * 256.0:             # nine single-point prompts on a 3 x 3 grid
            pts = torch.tensor([[[float(x0), float(y0)]]])
            lab = torch.ones(1, 1, dtype=torch.int)
            sp, de = R.prompt_encoder(sd, cfg, (pts, lab), None, None)
            low0, iou0, _ = hq_mask_decoder_ref(sd, cfg, emb, pe, sp, de, hq, multimask_output=False)
            low_o, iou_o = R.mask_decoder(sd, cfg, emb, pe, sp, de, False, hq_feat=hq)
            assert torch.equal(low0, low_o) and torch.equal(iou0, iou_o)
            low1, iou1, iou3 = hq_mask_decoder_ref(sd, cfg, emb, pe, sp, de, hq, multimask_output=True, _hf_samhq_quirk=True)
            out = model(image_embeddings=hf_emb, intermediate_embeddings=hf_interm, multimask_output=True, hq_token_only=False,
                        input_points=pts[:, None], input_labels=lab[:, None].long())
            hf_low, hf_iou = out.pred_masks[:, 0], out.iou_scores[:, 0]
            assert hf_low.shape[1] == 3 and low1.shape == (1, 1, 64, 64) and iou1.shape == (1, 1)
            e_low, e_iou = float((low1[:, 0] - hf_low[:, 0]).abs().max()), float((iou1[:, 0] - hf_iou[:, 0]).abs().max())
            print(f"helper vs HF first entry: low-res {e_low:.3g}, IoU {e_iou:.3g}, chosen token {int(iou3.argmax()) + 1}")
            assert e_low < 3e-4 and e_iou < 1e-4
            assert float(iou1) == float(iou3.max())
            chosen.add(int(iou3.argmax()))
    assert len(chosen) >= 2, "the prompts never exercise the selection"


def test_score_record_helper_on_hand_made_masks():
    lg = torch.full((3, 9, 13), -1.0)
    lg[0, 2:5, 3:11] = 0.5                      # 3 x 8 block of 0.5 ...
    lg[0, 3, 4] = 2.0                           # ... one pixel of it well above the offset
    lg[0, 7, 0] = -0.005                        # just below the threshold: counted by `lo` only
    lg[2] = 1.0                                 # full frame; mask 1 stays empty
    rec = score_record_ref(lg, 0.0, 0.02)
    assert rec.dtype == torch.int32 and rec.shape == (3, 8)
    assert rec[0].tolist() == [24, 25, 24, 3, 2, 10, 4, 0]
    assert rec[1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    assert rec[2].tolist() == [117, 117, 117, 0, 0, 12, 8, 0]
    rec1 = score_record_ref(lg, 0.0, 1.0)       # offset 1.0: only the 2.0 pixel clears thr + off; -0.005 and the block clear thr - off
    assert rec1[0].tolist() == [1, 25, 24, 3, 2, 10, 4, 0]
    assert rec1[2].tolist() == [0, 117, 117, 0, 0, 12, 8, 0]
