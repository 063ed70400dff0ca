"""Records tests/golden/tapnet_ref.npz from the TapNet restatement of tests/tapnet_ref.py run on the CPU.  Data only.

PARITY UNPINNED: the reference model needs JAX, Haiku and a checkpoint, none of which exists where this project is built, so the
recorded numbers are the restatement's, not the reference's (tests/tapnet_ref.py says what is pinned instead).

Seeded weights (weights.init_tapnet_state_dict), a synthetic clip of 5 frames at 96 x 128 — the adapter resizes every clip to the
model's 256 x 256 — and six queries (t, x, y) in clip pixels, one on each of frames 0 .. 4 and a second one on frame 2, one of them
on a cell border of the grid in x and y (model pixel 72, 160).  They were picked, among a lattice of candidates, for heat maps with a
clear maximum on every frame (the refusal below); corners of the grid are the kernel tests' business.  Stored:

  frames, query_points, video_q (6,3)              the clip, the queries, and the queries as the model sees them (t, y, x in 256 px)
  map_rows, stem_rows, unit0_rows, unit1_rows, unit2_rows, grid_rows   every 389th pixel of every frame's stages (unit1 / unit2 / grid:
                                                   those below 1024)
  qf (6,256), logits_top2 (6,5,2), logits_best (6,5)   query features; the two largest heat-map logits of every item and the best cell
  tracks (6,5,2), occlusion (6,5)                  the model's outputs in 256 px / logits
  trajectories (5,6,2), visibilities (5,6)         the adapter's output in clip pixels, for visibility_threshold 0.5
  floor_*, bar_px, bar_logit                       the restatement's own arithmetic noise at this shape and 8 x it

Noise floor (the recipe of oracle/noise_floor.py, as tools/make_tapir_golden.py applies it): the larger of (a) the f32 run against a
float64 run of the same weights and (b) the f32 run against an f32 run with every weight multiplied by 1 + 1e-7 N(0, 1); in pixels
for the tracks, in logits for the occlusion.  Nothing is fixed in advance: the bars are 8 x what is measured here.

The script REFUSES to write the file unless, in float64, for every one of the 30 (query, frame) items the best heat-map cell beats
the runner-up by FACTOR x the larger of bar_logit and 8 x the heat-map logits' own noise, every occlusion logit is further than
FACTOR x bar_logit from the threshold's logit, and visibilities of both signs occur.

    python tools/make_tapnet_golden.py
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.noise_floor import perturbed                       # noqa: E402
from sam_pt_amd.synth import synthetic_clip                    # noqa: E402
from sam_pt_amd.weights import init_tapnet_state_dict          # noqa: E402
from tests import tapnet_ref as R                              # noqa: E402

T, H, W, THRESHOLD, FACTOR = 5, 96, 128, 0.5, 4.0
# (t, x, y) in 256-pixel model coordinates; stored in clip pixels (x 128 / 256 and y 96 / 256 are exact in f32)
QUERIES_256 = [(0, 120.0, 20.0), (4, 24.0, 20.0), (2, 144.0, 20.0), (1, 72.0, 160.0), (3, 24.0, 104.0), (2, 96.0, 132.0)]


def model_inputs(frames, queries):
    """tracker.py:71-88 for one clip: the resized video in [-1, 1] NHWC and the queries as (t, y, x) in 256 px."""
    video = F.interpolate(frames / 255, (R.SIZE, R.SIZE), mode="bilinear", align_corners=False, antialias=True) * 2 - 1
    rescale = torch.tensor((R.SIZE, R.SIZE)) / torch.tensor((frames.shape[2], frames.shape[3]))
    q = queries.clone()
    q[:, 1:] *= rescale.flip(0)
    q[:, 1:] = q[:, 1:].flip(-1)
    return video.permute(0, 2, 3, 1).contiguous(), q, rescale


def spread(a, b):
    return float((a - b.to(a.dtype)).abs().max())


def main():
    sd = init_tapnet_state_dict(72)
    frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
    queries = torch.tensor([(t, x * W / R.SIZE, y * H / R.SIZE) for t, x, y in QUERIES_256], dtype=torch.float32)
    video, q, rescale = model_inputs(frames, queries)
    assert torch.allclose(q, torch.tensor([(t, y, x) for t, x, y in QUERIES_256], dtype=torch.float32), rtol=1e-6, atol=0)
    o32 = R.forward(sd, video, q, stages=True)
    o64 = R.forward(sd, video, q, dtype=torch.float64, stages=True)
    op = R.forward(perturbed(sd, 1e-7), video, q, stages=True)
    floors = {k: (spread(o32[k], o64[k]), spread(o32[k], op[k])) for k in ("tracks", "occlusion", "logits")}
    floor_px, floor_logit, floor_heat = max(floors["tracks"]), max(floors["occlusion"]), max(floors["logits"])
    bar_px, bar_logit = 8 * floor_px, 8 * floor_logit
    print(f"noise floor: tracks f32 vs f64 {floors['tracks'][0]:.3e} px, vs 1e-7 perturbed weights {floors['tracks'][1]:.3e} px -> bar_px {bar_px:.3e}")
    print(f"             occlusion f32 vs f64 {floors['occlusion'][0]:.3e}, vs perturbed {floors['occlusion'][1]:.3e} -> bar_logit {bar_logit:.3e}")
    print(f"             heat-map logits f32 vs f64 {floors['logits'][0]:.3e}, vs perturbed {floors['logits'][1]:.3e}")

    # ---- the margins, in float64, for every item
    lg = o64["logits"].reshape(len(QUERIES_256), T, -1)
    top = lg.topk(2, -1).values
    gap = top[..., 0] - top[..., 1]
    need = FACTOR * max(bar_logit, 8 * floor_heat)
    print(f"heat maps: |logit| max {float(lg.abs().max()):.3f}, smallest best-vs-runner-up gap {float(gap.min()):.3e} (need {need:.3e})")
    assert float(gap.min()) > need, "a heat map's best cell does not clearly beat the runner-up: move the queries"
    centre = math.log((1 - THRESHOLD) / THRESHOLD)                     # 1 - sigmoid(occ) > threshold  <=>  occ < this
    margin = float((o64["occlusion"] - centre).abs().min())
    vis64 = R.visibility_probability(o64["occlusion"]) > THRESHOLD
    print(f"visibility: {int(vis64.sum())} of {vis64.numel()} items visible, occlusion logits in [{float(o64['occlusion'].min()):.3f}, "
          f"{float(o64['occlusion'].max()):.3f}], closest to the threshold: {margin:.3e} (need {FACTOR * bar_logit:.3e})")
    assert margin > FACTOR * bar_logit, "an occlusion logit lies within the bar's reach of the threshold"
    assert 0 < int(vis64.sum()) < vis64.numel(), "both visibility outcomes must occur"
    soft = float((o64["tracks"] - (o64["tracks"] / 8).floor() * 8 - 4).abs().max())
    assert soft > 0.01, "no item is a real average"

    vis = R.visibility_probability(o32["occlusion"]).t() > THRESHOLD
    top32 = o32["logits"].reshape(len(QUERIES_256), T, -1).topk(2, -1)
    assert torch.equal(vis, vis64.t())
    traj = o32["tracks"].permute(1, 0, 2) / rescale.flip(-1)
    rows = torch.arange(0, 64 * 64, 389)
    rows_l = rows[rows < 32 * 32]
    out = dict(frames=frames.numpy(), query_points=queries.numpy(), video_q=q.numpy(), map_rows=rows.numpy().astype(np.int32),
               stem_rows=o32["stem"].reshape(T, -1, 64)[:, rows].numpy(), unit0_rows=o32["unit0"].reshape(T, -1, 64)[:, rows].numpy(),
               unit1_rows=o32["unit1"].reshape(T, -1, 128)[:, rows_l].numpy(), unit2_rows=o32["unit2"].reshape(T, -1, 256)[:, rows_l].numpy(),
               grid_rows=o32["grid"].reshape(T, -1, 256)[:, rows_l].numpy(), qf=o32["qf"].numpy(), logits_top2=top32.values.numpy(), logits_best=top32.indices[..., 0].numpy().astype(np.int32),
               tracks=o32["tracks"].numpy(), occlusion=o32["occlusion"].numpy(), trajectories=traj.numpy(), visibilities=vis.numpy(),
               threshold=np.float64(THRESHOLD), min_gap=np.float64(gap.min()), min_margin=np.float64(margin), floor_px=np.float64(floor_px),
               floor_logit=np.float64(floor_logit), floor_heat=np.float64(floor_heat), bar_px=np.float64(bar_px), bar_logit=np.float64(bar_logit))
    np.savez_compressed(R.GOLDEN, **out)
    print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
