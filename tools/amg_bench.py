#!/usr/bin/env python
"""SamAutomaticMaskGenerator.generate() on one synthetic 576 x 1024 frame at the VIS settings (configs/vis_eval_root.yaml: 32 x 32
points, 64 per batch): the fused path (batched decode + scoring on low-res masks) against ``fused=False`` (``predict_torch`` prompt by
prompt + tensor work on full-resolution logits), alternating in one process.

  python tools/amg_bench.py [--model vit_h|vit_b] [--hq] [--repeats 5] [--warmup 1] [--offset 0.02]
  python tools/amg_bench.py --launches [...]      # kernel launches / copies of ONE batch of 64 points on either path (torch.profiler)
  rocprofv3 --kernel-trace --stats -d DIR -o amg -- python tools/amg_bench.py --only fused --repeats 1 --warmup 0
                                                   # then tools/rocprof_summary.py / tools/rocprof_by_grid.py on the .db

Seeded random weights give small logits, so the stability offset is small and both thresholds are taken from the candidates
themselves (pred_iou_thresh = their lower-quartile IoU, stability_score_thresh = their median stability): the printed share
survives the filters.  ``set_image`` (the ViT) is timed apart and excluded from the generate() figures."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import automatic_mask_generator as A  # noqa: E402
from sam_pt_amd.sam_predictor import SamHip, SamPredictor  # noqa: E402
from sam_pt_amd.synth import synthetic_clip  # noqa: E402
from sam_pt_amd.weights import SAM_CONFIGS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="vit_h", choices=["vit_h", "vit_b", "vit_l", "vit_test"])
ap.add_argument("--hq", action="store_true", help="HQ-SAM decoder (fused path only: one candidate per point)")
ap.add_argument("--precision", default="f16", choices=["f16", "f16x3", "f32"])
ap.add_argument("--points-per-side", type=int, default=32)
ap.add_argument("--points-per-batch", type=int, default=64)
ap.add_argument("--offset", type=float, default=0.02)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--height", type=int, default=576)
ap.add_argument("--width", type=int, default=1024)
ap.add_argument("--launches", action="store_true")
ap.add_argument("--only", default="both", choices=["both", "fused", "unfused"], help="time one path alone (e.g. under a kernel trace)")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = SAM_CONFIGS[args.model]
frames, _ = synthetic_clip(T=1, H=args.height, W=args.width, seed=72)
img = frames[0].permute(1, 2, 0).contiguous().numpy()
pred = SamPredictor(SamHip(config=cfg, seed=72, precision=args.precision, hq=args.hq).to(dev))
sync = torch.cuda.synchronize

# ---- set_image alone
pred.set_image(img)
sync()
t_set = []
for _ in range(3):
    pred.reset_image()
    t0 = time.perf_counter()
    pred.set_image(img)
    sync()
    t_set.append((time.perf_counter() - t0) * 1e3)
print(f"model {args.model}{' + HQ' if args.hq else ''} ({args.precision} ViT), frame {args.height} x {args.width}, "
      f"{args.points_per_side} x {args.points_per_side} points, {args.points_per_batch} per batch")
print(f"set_image: {statistics.median(t_set):.1f} ms (median of 3; excluded below)")
nb = args.points_per_batch
print(f"sampt_sam_decode_points_workspace_bytes(n = {nb}, k = 1) = {pred.points_workspace_bytes(nb, 1) / 2**20:.0f} MiB")

# ---- thresholds from the candidates
grid = A.build_point_grid(args.points_per_side) * np.array([[args.width, args.height]])
pts = torch.as_tensor(pred.transform.apply_coords(grid, (args.height, args.width)), dtype=torch.float, device=dev)[:, None, :]
lab = torch.ones(pts.shape[0], 1, dtype=torch.int, device=dev)
low, iou = pred.predict_points_batch(pts, lab, multimask_output=True, max_chunk=nb)
rec = pred.score_masks(low.flatten(0, 1), args.offset).cpu()
stab = (rec[:, 0] / rec[:, 1]).numpy()
ious = iou.flatten().cpu().numpy()
iou_thr = float(np.quantile(ious, 0.25))
stab_thr = float(np.nanmedian(stab))
passed = (ious > iou_thr) & (np.nan_to_num(stab, nan=-1.0) >= stab_thr)
print(f"{len(ious)} candidates: |low-res logit| median {float(low.abs().median()):.3g}; pred_iou_thresh {iou_thr:.5f} (lower quartile), "
      f"stability_score_thresh {stab_thr:.4f} at offset {args.offset} (median) -> {int(passed.sum())} survive both "
      f"({100.0 * passed.mean():.1f} %)")
del low, iou, rec
kw = dict(points_per_side=args.points_per_side, points_per_batch=nb, pred_iou_thresh=iou_thr, stability_score_thresh=stab_thr,
          stability_score_offset=args.offset)
paths = {"both": [False, True], "fused": [True], "unfused": [False]}[args.only]
if args.hq:
    paths = [True]                                     # fused=False with HQ-SAM decodes prompt by prompt: nothing batched to compare
gens = {f: A.SamAutomaticMaskGenerator(None, predictor=pred, fused=f, **kw) for f in paths}

if args.launches:
    from torch.profiler import ProfilerActivity, profile
    crop_box, hw = [0, 0, args.width, args.height], (args.height, args.width)
    pred.set_image(img)
    for f in paths:
        fn = gens[f]._process_batch_fused if f else gens[f]._process_batch
        for _ in range(2):
            fn(grid[:nb], hw, crop_box, hw)
        sync()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(grid[:nb], hw, crop_box, hw)
            sync()
        kern = copies = 0
        for ev in prof.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA:
                if ev.name.lower().startswith(("memcpy", "memset", "copy")):
                    copies += 1
                else:
                    kern += 1
        print(f"fused={f}: one batch of {nb} points = {kern} kernel launches + {copies} copies / memsets")
    sys.exit(0)

# ---- generate(), alternating, set_image timed inside and subtracted
t_in_set = [0.0]
orig_set = pred.set_image


def timed_set_image(*a, **k):
    sync()
    t0 = time.perf_counter()
    orig_set(*a, **k)
    sync()
    t_in_set[0] += time.perf_counter() - t0


pred.set_image = timed_set_image
times = {f: [] for f in paths}
n_rec = {}
for r in range(args.warmup + args.repeats):
    for f in paths:
        t_in_set[0] = 0.0
        sync()
        t0 = time.perf_counter()
        recs = gens[f].generate(img)
        sync()
        dt = (time.perf_counter() - t0 - t_in_set[0]) * 1e3
        n_rec[f] = len(recs)
        if r >= args.warmup:
            times[f].append(dt)
for f in paths:
    t = times[f]
    print(f"generate() fused={f}: median {statistics.median(t):.1f} ms, min {min(t):.1f}, max {max(t):.1f} (spread {max(t) - min(t):.1f}) "
          f"over {len(t)} repeats; {n_rec[f]} records after NMS")
if len(paths) == 2:
    a, b = statistics.median(times[False]), statistics.median(times[True])
    print(f"fused / unfused: {a / b:.2f} x faster ({a - b:.1f} ms; the unfused path's own spread is {max(times[False]) - min(times[False]):.1f} ms)")
