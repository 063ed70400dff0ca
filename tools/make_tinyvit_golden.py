"""Records tests/golden/tinyvit_ref.npz from the TinyViT restatement of tests/tinyvit_ref.py run on the CPU.  Data only.

PARITY UNPINNED: upstream's tiny_vit_sam.py (MobileSAM, Light HQ-SAM) and its checkpoints are not available where this project is
built, so the recorded numbers are the restatement's, not upstream's (tests/tinyvit_ref.py says what is pinned instead).

Seeded weights (weights.init_sam_state_dict on SAM_CONFIGS["vit_t_test"] with the HQ extras; the SAM model is the same dict without
them), two landscape frames of 144 x 256 from the synthetic clip — the image rows below 144 are Sam.preprocess's zero padding, and
every layer pads its windows (32 -> 35, 16 -> 28, 16 -> 21) — and one prompt of three points (two on the disc, one off it) per
frame through oracle/sam_ref.py's prompt encoder and mask decoder, for SAM and for HQ-SAM.  Stored:

  frame_ids (2,), points (2,3,2), labels (2,3)     which frames of synthetic_clip(T=4, H=144, W=256, seed=72), the prompts (frame px)
  emb_rows (2,52,256), emb_idx                     every 5th token of the embedding
  interm_rows (2,52,96)                            the same tokens of the HQ tap (the input of layers.2)
  hq_rows (2,111,32), hq_idx                       every 37th pixel of the HQ feature map (embedding_encoder + compress_vit_feat)
  low_sam, low_hq (2,64,64)                        low-resolution logits; mask_sam, mask_hq (2,144,256) the masks (logits > 0)
  floor_<stage> (2,), bar_<stage>                  per stage (patch_embed, layer0..3, neck): the restatement's own noise and 8 x it
  bar_emb, bar_interm, bar_hq, bar_logit           the same for the embedding, the HQ tap, the HQ features and the logits

Noise (the recipe of oracle/noise_floor.py, as tools/make_tapir_golden.py and make_tapnet_golden.py apply it): the larger of (a) the
f32 run against a float64 run of the same weights and (b) the f32 run against an f32 run with every weight multiplied by
1 + 1e-7 N(0, 1), as the largest absolute difference over the stage.  Nothing is fixed in advance and nothing comes from the device
path: a bar is 8 x what is measured here (TAPIR's and TapNet's factor: room for another summation order, none for a wrong operator).

The script REFUSES to write the file unless every prompt's mask covers between 5 % and 95 % of the frame and no more than 0.1 % of
its full-resolution logits lie within bar_logit of the threshold.

    python tools/make_tinyvit_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import sam_ref as S                                # noqa: E402
from oracle.noise_floor import perturbed                       # noqa: E402
from sam_pt_amd.synth import synthetic_clip                    # noqa: E402
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict  # noqa: E402
from tests import tinyvit_ref as R                             # noqa: E402

H, W, FRAME_IDS = 144, 256, (0, 3)
EMB_STEP, HQ_STEP = 5, 37


def golden_inputs():
    """(cfg, sd with the HQ extras, frames uint8 (2,3,144,256), points (2,3,2) f32, labels (2,3) i32) — shared with the tests."""
    cfg = SAM_CONFIGS["vit_t_test"]
    sd = init_sam_state_dict(cfg, 72, hq=True)
    clip, centres = synthetic_clip(T=4, H=H, W=W, seed=72)
    frames = clip[list(FRAME_IDS)].contiguous()
    pts, labels = [], []
    for t in FRAME_IDS:
        cx, cy = float(centres[t][0]), float(centres[t][1])
        pts.append([[cx - 6.0, cy + 3.0], [cx + 7.0, cy - 4.0], [cx + 90.0, cy - 40.0]])
        labels.append([1, 1, 0])
    return cfg, sd, frames, torch.tensor(pts, dtype=torch.float32), torch.tensor(labels, dtype=torch.int32)


def decode(cfg, sd, emb, interm, pts, labels, hq, dtype=torch.float32):
    """oracle/sam_ref.py's decoder on one frame's embedding (1,256,g,g) [+ HQ tap (1,g,g,C2)] -> (low (64,64), logits (H,W), hq features)."""
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    default = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                  # the oracle creates its constants (grids, 2 pi) in the default dtype
    try:
        p = S.SamPredictorRef(sdd, cfg, hq=hq)
        p.features, p.original_size, p.input_size = emb.to(dtype), (H, W), (H, W)
        if hq:
            p.hq_feat = S.hq_features(sdd, p.features, interm.to(dtype))
        logits, _, low = p.predict_torch(pts[None].to(dtype), labels[None], multimask_output=False, return_logits=True)
    finally:
        torch.set_default_dtype(default)
    return low[0, 0], logits[0, 0], (p.hq_feat[0] if hq else None)


def run_all(cfg, sd, frames, pts, labels, dtype):
    with torch.no_grad():
        st = R.run(cfg, sd, frames, dtype)
        out = dict(st)
        for name, hq in (("sam", False), ("hq", True)):
            res = [decode(cfg, sd, st["neck"][i:i + 1], st["interm"][i:i + 1], pts[i], labels[i], hq, dtype) for i in range(len(frames))]
            out["low_" + name] = torch.stack([r[0] for r in res])
            out["logits_" + name] = torch.stack([r[1] for r in res])
            if hq:
                out["hqfeat"] = torch.stack([r[2] for r in res])            # (2,32,64,64)
    return out


def spread(a, b):
    return float((a.double() - b.double()).abs().max())


def main():
    cfg, sd, frames, pts, labels = golden_inputs()
    o32 = run_all(cfg, sd, frames, pts, labels, torch.float32)
    o64 = run_all(cfg, sd, frames, pts, labels, torch.float64)
    op = run_all(cfg, perturbed(sd, 1e-7), frames, pts, labels, torch.float32)
    out = {}
    keys = {s: s for s in R.STAGES}
    keys.update(emb="neck", interm="interm", hq="hqfeat")
    for name, k in keys.items():
        fl = (spread(o32[k], o64[k]), spread(o32[k], op[k]))
        out["floor_" + name], out["bar_" + name] = np.array(fl), np.float64(8 * max(fl))
        print(f"{name:12s} |x| max {float(o32[k].abs().max()):9.3f}  f32 vs f64 {fl[0]:.3e}  vs 1e-7 perturbed weights {fl[1]:.3e}  -> bar {8 * max(fl):.3e}")
    fl = tuple(max(spread(o32["low_" + m], o[("low_" + m)]) for m in ("sam", "hq")) for o in (o64, op))
    bar_logit = 8 * max(fl)
    out["floor_logit"], out["bar_logit"] = np.array(fl), np.float64(bar_logit)
    print(f"{'logit':12s} |x| max {float(o32['low_hq'].abs().max()):9.3f}  f32 vs f64 {fl[0]:.3e}  vs perturbed {fl[1]:.3e}  -> bar {bar_logit:.3e}")
    for m in ("sam", "hq"):
        for i in range(len(frames)):
            lg = o64["logits_" + m][i]
            cover, near = float((lg > 0).double().mean()), float((lg.abs() <= bar_logit).double().mean())
            print(f"{m} frame {i}: mask covers {100 * cover:.1f} % of the frame, {100 * near:.4f} % of its logits within bar_logit of 0, "
                  f"logits in [{float(lg.min()):.2f}, {float(lg.max()):.2f}]")
            assert 0.05 <= cover <= 0.95, "a mask covers less than 5 % or more than 95 % of the frame: move the prompt"
            assert near <= 1e-3, "more than 0.1 % of a mask's logits lie within bar_logit of the threshold"
    g2 = cfg.grid * cfg.grid
    emb_idx, hq_idx = np.arange(0, g2, EMB_STEP, dtype=np.int32), np.arange(0, 16 * g2, HQ_STEP, dtype=np.int32)
    emb = o32["neck"].permute(0, 2, 3, 1).reshape(len(frames), g2, -1)
    hqf = o32["hqfeat"].permute(0, 2, 3, 1).reshape(len(frames), 16 * g2, -1)
    out.update(frame_ids=np.array(FRAME_IDS, dtype=np.int32), points=pts.numpy(), labels=labels.numpy(), emb_idx=emb_idx, hq_idx=hq_idx,
               emb_rows=emb[:, emb_idx].numpy(), interm_rows=o32["interm"].reshape(len(frames), g2, -1)[:, emb_idx].numpy(),
               hq_rows=hqf[:, hq_idx].numpy(), low_sam=o32["low_sam"].numpy(), low_hq=o32["low_hq"].numpy(),
               mask_sam=(o32["logits_sam"] > 0).numpy(), mask_hq=(o32["logits_hq"] > 0).numpy())
    np.savez_compressed(R.GOLDEN, **out)
    print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
