#!/usr/bin/env python
"""Interactive point correction: one click selection at the reference's size, host against device, and one simulated video,
incremental against not (sam_pt_amd/interactive.py, sam_pt_amd/sam_pt_interactive.py, csrc/dbscan.hip).

  python tools/interactive_bench.py [--repeats 7] [--skip-video] [--model vit_h] [--frames 24] [--interactions 60]

Part 1: 18 000 points sampled from two rectangles of a 480 x 854 frame (the reference's ``dbscan_points`` and DAVIS frame size).
  host    DBSCAN (scikit-learn where it imports, else the NumPy restatement, said so in the output) + the host k-medoids on 720 points
  device  extract_largest_cluster_points(device=...) on the same mask, checked for the same points first
  and the DBSCAN kernels alone between two events.  One warm-up, then ``--repeats`` runs: median, min, max and spread.
Part 2: the bench clip (24 frames of 480 x 854 upscaled to 576 x 1024, ViT-H, PIPS, seeded weights), ground truth = the moving disc,
  ``interactions_max`` 60, once with ``incremental=True`` and once with ``incremental=False``: seconds per video and decoder calls per
  click.  Nothing else runs this loop on the GPU, so the non-incremental run of the same tree is the baseline.
Part 3: ``decode_batch=4`` against ``decode_batch=1`` on the clip of tests/test_gpu_interactive.py (5 frames of 128 x 256, the smallest
  SAM test configuration, PIPS): the largest logit difference on fixed point states (the figure that test holds to 8 x 1.9e-7)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import interactive as I  # noqa: E402
from sam_pt_amd.query_points import kmedoids_alternate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--skip-video", action="store_true")
ap.add_argument("--model", default="vit_h")
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--interactions", type=int, default=60)
args = ap.parse_args()
assert torch.cuda.is_available(), "interactive_bench needs a GPU"
dev = torch.device("cuda:0")


def stats(ts, unit="ms"):
    return f"median {statistics.median(ts):.3f} {unit}, min {min(ts):.3f}, max {max(ts):.3f} (spread {max(ts) - min(ts):.3f})"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


# ------------------------------------------------------------------------------------------------------------------ part 1
H, W = 480, 854
mask = torch.zeros((H, W), dtype=torch.bool)
mask[40:254, 60:340] = True
mask[300:420, 500:786] = True
eps = 2.4 * H * W / 18000
try:
    from sklearn.cluster import DBSCAN
    host_dbscan, host_name = (lambda X: DBSCAN(eps=eps, min_samples=10).fit(X).labels_), "scikit-learn DBSCAN"
except ImportError:
    host_dbscan, host_name = (lambda X: I.dbscan_labels(X, eps, 10)), "NumPy restatement (scikit-learn does not import here)"


def host_click():
    px = mask.nonzero().float()
    px = px[torch.randperm(len(px))[:18000]]
    best = I.largest_cluster(host_dbscan(px.numpy()), 180)
    pts = px[torch.from_numpy(best.members)] if best.cluster_id >= 0 else mask.nonzero().float()
    pts = pts[torch.randperm(len(pts))[:720]]
    return pts[torch.as_tensor(kmedoids_alternate(pts.numpy(), 3))].flip(1)


mask_dev = mask.to(dev)
torch.manual_seed(1)
a = I.extract_largest_cluster_points(mask, 3)
torch.manual_seed(1)
b = I.extract_largest_cluster_points(mask_dev, 3, device=dev)
assert (a == b).all(), (a, b)
print(f"click selection, {int(mask.sum())} mask pixels -> 18000 points, eps {eps:.3f}: host and device pick {b.tolist()}")
host_click(), I.extract_largest_cluster_points(mask_dev, 3, device=dev)                  # warm-up
th = [wall(host_click)[0] for _ in range(args.repeats)]
td = [wall(lambda: I.extract_largest_cluster_points(mask_dev, 3, device=dev))[0] for _ in range(args.repeats)]
print(f"  host   ({host_name} + host k-medoids): {stats(th)}")
print(f"  device (pixel list, DBSCAN, cluster choice, k-medoids): {stats(td)}")
px = mask_dev.nonzero().float()
px = px[torch.randperm(len(px))[:18000].to(dev)].contiguous()
r2 = I.eps_to_r2(eps)
I._dbscan_device_raw(px, r2, 10)
tk = []
for _ in range(args.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    labels, ws = I._dbscan_device_raw(px, r2, 10)
    I._largest_device_raw(labels, 180, ws)
    e1.record()
    torch.cuda.synchronize()
    tk.append(e0.elapsed_time(e1))
print(f"  DBSCAN kernels alone (labels + largest, events, n = 18000, r2 = {r2}): {stats(tk)}")
print(f"  host / device medians: {statistics.median(th) / statistics.median(td):.1f} x")

# ------------------------------------------------------------------------------------------------------------------ part 2
if not args.skip_video:
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    from sam_pt_amd.synth import disc_queries, synthetic_clip, upscale_to_longest_side
    from sam_pt_amd.weights import init_pips_state_dict
    T = args.frames
    frames, centres = synthetic_clip(T=T, H=480, W=854, seed=72, disc_r=60.0)
    frames, centres = upscale_to_longest_side(frames, centres, 1024)
    Hh, Ww = frames.shape[-2:]
    r = 60.0 * 1024 / 854
    yy, xx = torch.meshgrid(torch.arange(Hh), torch.arange(Ww), indexing="ij")
    gts = [(((xx - c[0]) ** 2 + (yy - c[1]) ** 2) <= r * r)[None] for c in centres]
    video = {"image": [f.to(dev) for f in frames], "gt_masks": gts, "query_points": disc_queries(centres, n_pos=8, r=36.0)[None],
             "target_hw": (Hh, Ww), "video_id": "bench"}
    tracker = PipsPointTracker(state_dict=init_pips_state_dict(72), fnet_chunk=8)
    pred = SamPredictor(SamHip(args.model, precision="f16", seed=72).to(dev))
    kw = dict(sam_iou_threshold=0.7, positive_points_per_mask=8, negative_points_per_mask=0, iterative_refinement_iterations=0,
              interactions_max=args.interactions, interactions_max_per_frame=3)
    print(f"simulated video: {T} frames of {Hh} x {Ww}, {args.model} (fp16 ViT), PIPS, interactions_max {args.interactions}; "
          "baseline = the non-incremental run of the same tree")
    for incremental in (True, False, True, False):
        model = SamPtInteractive(point_tracker=tracker, sam_predictor=pred, incremental=incremental, **kw).eval()
        torch.manual_seed(3)
        ms, _ = wall(lambda: model(video))
        last = model.last_run
        clicks = len(last["interaction_history"])
        print(f"  incremental={incremental}: {ms / 1e3:.2f} s per video, {clicks} clicks, {last['decoder_calls']} decoder calls "
              f"({last['decoder_calls'] / max(clicks, 1):.1f} per click), {last['tracker_calls']} tracker calls, "
              f"{last['device_clicks']} device click selections, final mean IoU {np.mean(last['final_ious']):.3f}")

# ------------------------------------------------------------------------------------------------------------------ part 3
from tests import interactive_ref as IR  # noqa: E402
from sam_pt_amd.sam_pt_interactive import SamPtInteractive as _Sim  # noqa: E402

setup = IR.gpu_loop_setup(dev)
m = _Sim(point_tracker=setup[1], sam_predictor=setup[2], decode_batch=1, **setup[3]).eval()
torch.manual_seed(5)
m(setup[0])
print("decode_batch=4 against decode_batch=1, 5 frames of 128 x 256 (vit_test, f32, PIPS), fixed point states:")
for name, diff, big, has_neg in IR.decode_batch_differences(setup, m.last_run, batch=4):
    print(f"  {name}: largest logit difference {diff:.3e} (largest |logit| {big:.3e}); frames with a visible negative {has_neg}; "
          f"the test's bar is 8 x 1.9e-7 = {8 * 1.9e-7:.3e}")
