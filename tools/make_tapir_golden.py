"""Records tests/golden/tapir_ref.npz from the TAPIR restatement of tests/tapir_ref.py run on the CPU.

PARITY UNPINNED: the reference model needs JAX, Haiku and a checkpoint, none of which exists where this project is built, so the
recorded numbers are the restatement's, not the reference's (tests/tapir_ref.py says what is pinned instead).

Seeded weights (weights.init_tapir_state_dict), a synthetic clip of 5 frames at 40 x 56 — the adapter resizes every clip to the
model's 256 x 256 — and six queries (t, x, y) in clip pixels: on frame 0, on the last frame, one whose 7 x 7 patch hangs over the
lower left corner of both feature maps, one on a cell border of both maps (model pixel 96, 128), two interior ones.  Stored:

  frames, query_points, video_q (6,3)              the clip, the queries, and the queries as the model sees them (t, y, x in 256 px)
  map_rows, hires_rows, lowres_rows                every 97th pixel of every frame's two feature maps
  qf (6,384), logits (6,5,32,32)                   query features, the heat-map logits of the cost-volume heads
  x0, x1 (6,5,486), block0 (6,5,512)               mixer input rows of refinements 0 and 1, mixer block 0 applied to mixer.in(x0)
  iter_tracks (5,6,5,2), iter_occlusion, iter_expected_dist (5,6,5)   after the heads and after each of the 4 refinements
  trajectories (5,6,2), visibilities (5,6)         the adapter's output in clip pixels, for visibility_threshold 0.1
  floor_*, bar_px, bar_logit                       the restatement's own arithmetic noise at this shape and 8 x it

Noise floor (the recipe of oracle/noise_floor.py, RAFT's rule): the larger of (a) the f32 run against a float64 run of the same
weights and (b) the f32 run against an f32 run with every weight multiplied by 1 + 1e-7 N(0, 1), over all five iterations.

The script REFUSES to write the file unless, in float64, for every one of the 30 (query, frame) items the best heat-map cell beats
the runner-up by MIN_GAP in the logits, and every visibility probability is further from the threshold than bar_logit can move it.

    python tools/make_tapir_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.noise_floor import perturbed                       # noqa: E402
from sam_pt_amd.synth import synthetic_clip                    # noqa: E402
from sam_pt_amd.weights import init_tapir_state_dict           # noqa: E402
from tests import tapir_ref as R                               # noqa: E402

T, H, W, THRESHOLD, MIN_GAP = 5, 40, 56, 0.1, 1e-3
# (t, x, y) in 256-pixel model coordinates; stored in clip pixels (x 56 / 256 and y 40 / 256 are exact in f32)
QUERIES_256 = [(0, 120.75, 100.25), (4, 200.5, 60.25), (2, 3.0, 250.0), (1, 96.0, 128.0), (3, 33.25, 77.75), (2, 140.25, 180.5)]


def model_inputs(frames, queries):
    """tracker.py:76-94 for one clip: the resized video in [-1, 1] NHWC and the queries as (t, y, x) in 256 px."""
    video = F.interpolate(frames / 255, (R.SIZE, R.SIZE), mode="bilinear", align_corners=False, antialias=True) * 2 - 1
    rescale = torch.tensor((R.SIZE, R.SIZE)) / torch.tensor((frames.shape[2], frames.shape[3]))
    q = queries.clone()
    q[:, 1:] *= rescale.flip(0)
    q[:, 1:] = q[:, 1:].flip(-1)
    return video.permute(0, 2, 3, 1).contiguous(), q, rescale


def spread(a, b):
    return max(float((x - y.to(x.dtype)).abs().max()) for x, y in zip(a, b))


def main():
    sd = init_tapir_state_dict(72)
    frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
    queries = torch.tensor([(t, x * W / R.SIZE, y * H / R.SIZE) for t, x, y in QUERIES_256], dtype=torch.float32)
    video, q, rescale = model_inputs(frames, queries)
    # (the adapter multiplies by the f32 quotients 256 / 56 and 256 / 40, so the model sees these to within one ulp or two)
    assert torch.allclose(q, torch.tensor([(t, y, x) for t, x, y in QUERIES_256], dtype=torch.float32), rtol=1e-6, atol=0)
    o32 = R.forward(sd, video, q, stages=True)
    o64 = R.forward(sd, video, q, dtype=torch.float64, stages=True)
    op = R.forward(perturbed(sd, 1e-7), video, q)
    floors = {}
    for name, key in (("px", "iter_tracks"), ("logit", "iter_occlusion"), ("logit_e", "iter_expected_dist")):
        floors[name] = (spread(o32[key], o64[key]), spread(o32[key], op[key]))
    floor_px = max(floors["px"])
    floor_logit = max(max(floors["logit"]), max(floors["logit_e"]))
    bar_px, bar_logit = 8 * floor_px, 8 * floor_logit
    print(f"noise floor: tracks f32 vs f64 {floors['px'][0]:.3e} px, vs 1e-7 perturbed weights {floors['px'][1]:.3e} px -> bar_px {bar_px:.3e}")
    print(f"             logits f32 vs f64 {max(floors['logit'][0], floors['logit_e'][0]):.3e}, vs perturbed "
          f"{max(floors['logit'][1], floors['logit_e'][1]):.3e} -> bar_logit {bar_logit:.3e}")

    # ---- the margins, in float64, for every item
    lg = o64["logits"].reshape(len(QUERIES_256), T, -1)
    top = lg.topk(2, -1).values
    gap = top[..., 0] - top[..., 1]
    print(f"heat maps: |logit| max {float(lg.abs().max()):.3f}, smallest best-vs-runner-up gap {float(gap.min()):.3e} (need {MIN_GAP:.0e})")
    assert float(gap.min()) > MIN_GAP, "a heat map's best cell does not clearly beat the runner-up: move the queries"
    move = float((o64["iter_tracks"][-1] - o64["iter_tracks"][0]).abs().max())
    print(f"4 refinements move a point by at most {move:.3f} px")
    assert 0.01 < move < 32.0
    for i in range(R.ITERS + 1):
        prob = R.visibility_probability(o64["iter_occlusion"][i], o64["iter_expected_dist"][i])
        # |d prob / d logit| <= 1/4 per logit: bar_logit on both logits moves a probability by at most bar_logit / 2
        margin = float((prob - THRESHOLD).abs().min())
        assert margin > max(bar_logit, 1e-3), f"iteration {i}: a visibility probability lies {margin:.2e} from the threshold"
    vis64 = prob > THRESHOLD
    print(f"visibility: {int(vis64.sum())} of {vis64.numel()} items visible, closest probability to {THRESHOLD}: {margin:.3e}")
    assert 0 < int(vis64.sum()) < vis64.numel(), "both visibility outcomes must occur"

    # ---- stages
    sdc = R.cast(sd, torch.float32)
    with torch.no_grad():
        x0, _ = R.mixer_input(o32["hires"], o32["lowres"], o32["qf"], o32["iter_tracks"][0], o32["iter_occlusion"][0],
                              o32["iter_expected_dist"][0], None)
        p1, c1, e1, f1 = R.refine(sdc, o32["hires"], o32["lowres"], o32["qf"], o32["iter_tracks"][0], o32["iter_occlusion"][0],
                                  o32["iter_expected_dist"][0], None)
        x1, _ = R.mixer_input(o32["hires"], o32["lowres"], o32["qf"], p1, c1, e1, f1)
        block0 = R.mixer_block(sdc, 0, x0 @ sdc["mixer.in.weight"].t() + sdc["mixer.in.bias"])
    assert torch.equal(p1, o32["iter_tracks"][1])
    vis = R.visibility_probability(o32["occlusion"], o32["expected_dist"]).t() > THRESHOLD
    assert torch.equal(vis, vis64.t())
    traj = o32["tracks"].permute(1, 0, 2) / rescale.flip(-1)
    rows = torch.arange(0, 64 * 64, 97)
    rows_l = rows[rows < 32 * 32]
    out = dict(frames=frames.numpy(), query_points=queries.numpy(), video_q=q.numpy(),
               map_rows=rows.numpy().astype(np.int32), hires_rows=o32["hires"].reshape(T, -1, 128)[:, rows].numpy(),
               lowres_rows=o32["lowres"].reshape(T, -1, 256)[:, rows_l].numpy(), qf=o32["qf"].numpy(), logits=o32["logits"].numpy(),
               x0=x0.numpy(), x1=x1.numpy(), block0=block0.numpy(),
               iter_tracks=torch.stack(o32["iter_tracks"]).numpy(), iter_occlusion=torch.stack(o32["iter_occlusion"]).numpy(),
               iter_expected_dist=torch.stack(o32["iter_expected_dist"]).numpy(), trajectories=traj.numpy(), visibilities=vis.numpy(),
               threshold=np.float64(THRESHOLD), min_gap=np.float64(gap.min()), floor_px=np.float64(floor_px),
               floor_logit=np.float64(floor_logit), floor_px_f64=np.float64(floors["px"][0]), floor_px_perturbed=np.float64(floors["px"][1]),
               bar_px=np.float64(bar_px), bar_logit=np.float64(bar_logit))
    np.savez_compressed(R.GOLDEN, **out)
    print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
