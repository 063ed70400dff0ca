#!/usr/bin/env python
"""SuperGlue point tracker on the device (sam_pt_amd.point_tracker.SuperGluePointTracker, csrc/superglue.hip,
csrc/engine_superglue.hip).

  python tools/superglue_bench.py [--frames 24] [--height 480] [--width 854] [--masks 3] [--repeats 3] [--cpu-frames 3]

The default clip is 24 frames of 480 x 854 with 3 masks and the shipped superglue.yaml's settings (nms_radius 3, threshold
0.005, 20 Sinkhorn iterations, match threshold 0.2), seeded random weights.  Printed:
  * keypoints per frame;
  * device time per clip between two events, split into SuperPoint (detect: all frames) and matching (23 pairs + selection),
    and forward() as a whole (with its two host synchronisations);
  * the share of every kernel in the device time of one forward() (torch.profiler), and the Sinkhorn passes' achieved bytes per
    second: a row pass and a column pass each read the n0 x n1 score matrix once, against the 8 TB/s HBM figure (at a few
    thousand keypoints the matrix fits the 256 MiB Infinity Cache, so this is a cache figure, not an HBM one);
  * the CPU restatement (tests/superglue_ref.py, PyTorch on the host) on the first --cpu-frames frames of the same clip, scaled
    to the clip: the reference tree is absent where this runs, the restatement is pinned to it by tests/test_superglue_cpu.py.
No target is attached to these figures; they are the starting point for tuning."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd.point_tracker import SuperGluePointTracker  # noqa: E402
from sam_pt_amd.synth import synthetic_clip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--masks", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--cpu-frames", type=int, default=3, help="frames the CPU restatement runs (0: not measured)")
ap.add_argument("--no-profile", action="store_true", help="skip the torch.profiler pass (when an outer profiler is attached)")
args = ap.parse_args()
assert torch.cuda.is_available(), "superglue_bench needs a GPU"
dev = torch.device("cuda:0")
HBM_GBS = 8000.0
T, H, W, NM, POS, NEG = args.frames, args.height, args.width, args.masks, 8, 1
CONFIG = {"superpoint": {"nms_radius": 3, "keypoint_threshold": 0.005, "max_keypoints": -1, "descriptor_dim": 256, "remove_borders": 4},
          "superglue": {"sinkhorn_iterations": 20, "match_threshold": 0.2}}

frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
masks = torch.stack([(((xx - W * (0.25 + 0.25 * m)) ** 2 + (yy - H * 0.5) ** 2) <= (H * 0.2) ** 2).float() for m in range(NM)])
q = torch.zeros(1, NM * (POS + NEG), 3)
q[0, :, 1:] = torch.rand(NM * (POS + NEG), 2, generator=torch.Generator().manual_seed(1)) * torch.tensor([W - 1.0, H - 1.0])
trk = SuperGluePointTracker(POS, NEG, [-1, -1], CONFIG)
fd, md, qd = frames.to(dev), masks.to(dev), q.to(dev)
print(f"SuperGlue tracker: {T} frames of {H} x {W}, {NM} masks, {POS} + {NEG} points per mask, shipped settings; {args.repeats} repeats "
      "after 1 warm-up")


def timed(fn):
    ts = []
    for r in range(1 + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 1:
            ts.append(e0.elapsed_time(e1))
    return ts


def line(ts):
    return f"median {statistics.median(ts):.1f} ms, min {min(ts):.1f}, max {max(ts):.1f}"


det = trk.detect(fd)
counts = det["counts"]
print(f"keypoints per frame: min {min(counts)}, median {int(statistics.median(counts))}, max {max(counts)} (capacity {det['cap']})")
ts_d = timed(lambda: trk.detect(fd))
print(f"SuperPoint, {T} frames (detect): {line(ts_d)}")
ws = trk.match_workspace(det)


def all_pairs():
    for i in range(1, T):
        trk.match(det, i, ws)


ts_m = timed(all_pairs)
print(f"SuperGlue, {T - 1} pairs (match): {line(ts_m)} -> {statistics.median(ts_m) / max(T - 1, 1):.2f} ms per pair")


def forward():
    trk.set_masks(md)
    np.random.seed(0)
    trk(fd[None], qd)


ts_f = timed(forward)
print(f"forward() (detect + match + selection + draws + gather, 2 host synchronisations): {line(ts_f)}")

if not args.no_profile:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        forward()
        torch.cuda.synchronize()
    per = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            d = per.setdefault(ev.name.split("(")[0][:72], [0, 0.0])
            d[0] += 1
            d[1] += ev.time_range.elapsed_us()
    total = sum(v[1] for v in per.values())
    print(f"kernels of one forward(): {sum(v[0] for v in per.values())} launches, {total / 1e3:.1f} ms of device time")
    for name, (n, us) in sorted(per.items(), key=lambda kv: -kv[1][1])[:16]:
        print(f"  {100 * us / total:5.1f} %  {us / 1e3:9.2f} ms  {n:6d} x {us / n:9.1f} us  {name}")
    sink = [v for k, v in per.items() if "k_sg_sinkhorn" in k]
    if sink:
        us = sum(v[1] for v in sink)
        nbytes = sum(2 * 20 * counts[0] * c * 4 for c in counts[1:])          # 20 iterations x (row pass + column pass) x the matrix
        gbs = nbytes / (us * 1e-6) / 1e9
        print(f"Sinkhorn: {sum(v[0] for v in sink)} launches, {us / 1e3:.2f} ms, {nbytes / 1e9:.2f} GB read -> {gbs:.0f} GB/s = "
              f"{100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM figure")
    else:
        print("Sinkhorn: not measured (no k_sg_sinkhorn kernel in the profile)")

if args.cpu_frames >= 2:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from tests import superglue_ref as R
    n = min(args.cpu_frames, T)
    np.random.seed(0)
    t0 = time.perf_counter()
    R.track(trk._sp_sd, trk._sg_sd, frames[:n], masks, q, CONFIG, POS, NEG)
    dt = time.perf_counter() - t0
    print(f"CPU restatement ({torch.get_num_threads()} threads): {n} frames ({n - 1} pairs) in {dt:.2f} s -> about "
          f"{dt / n * T:.1f} s for the {T}-frame clip (linear in the frames)")
else:
    print("CPU restatement: not measured")
