#!/usr/bin/env python
"""What ``SamPt(device_reinit=True)`` takes off a clip with point re-initialisation.

  python tools/reinit_bench.py [--tag this] [--baseline-only] [--repeats 7] [--frames 72] [--log profiles/reinit_bench.log]

One blocking ``SamPt.forward`` (host wall time around a device synchronise) of a 72-frame 480 x 854 clip with 3 objects, ViT-B fp16 +
PIPS, ``use_point_reinit=True`` with ``reinit_horizon`` 24 and the point settings of the shipped sam_pt.yaml (16 k-medoid positives, 1
``mixed`` negative per object, 12 refinement iterations, the default ``reinit-at-median-of-area-diff``), in three modes that alternate
inside every repeat after a warm-up of each: the default mode (the host's re-initialisation loop), ``device_reinit=True``, and
``device_reinit=True, device_tracks=True``.  The generator is seeded before every forward, so every leg makes the same draws.
--baseline-only times the default mode alone and needs no new keyword: that is the run to make on a build of the parent commit, with
this file copied beside it, in the same job — the fourth configuration, the baseline of the default mode.
One JSON line per leg, printed and appended to --log; "spread" is (max - min) / median over the repeats of a leg.  Random weights:
``sam_iou_threshold`` is -1e9 so that no frame's mask is rejected (a seeded IoU head would reject most, leaving empty masks and
nothing to re-initialise from); the times do not otherwise depend on the weights."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sam_pt_amd.point_tracker import PipsPointTracker  # noqa: E402
from sam_pt_amd.sam_predictor import SamHip, SamPredictor  # noqa: E402
from sam_pt_amd.sam_pt import SamPt  # noqa: E402
from sam_pt_amd.synth import bench_clip  # noqa: E402
from sam_pt_amd.weights import init_pips_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="this", help="which build ran (written into every line)")
ap.add_argument("--baseline-only", action="store_true", help="only the default mode: what the parent commit's API has")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--frames", type=int, default=72)
ap.add_argument("--objects", type=int, default=3)
ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reinit_bench.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "reinit_bench needs a GPU"
dev = torch.device("cuda:0")
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
log = open(args.log, "a")


def emit(rec):
    line = json.dumps({"build": args.tag, **rec})
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def stats(ms):
    med = statistics.median(ms)
    return {"ms_median_min_max": [round(med, 2), round(min(ms), 2), round(max(ms), 2)], "spread": round((max(ms) - min(ms)) / med, 4),
            "repeats": len(ms)}


frames, qp = bench_clip(T=args.frames, seed=72, n_pos=16, n_objects=args.objects, native=True, n_neg=1)
H, W = frames.shape[-2:]
video = {"image": [f for f in frames.to(dev)], "target_hw": (H, W), "query_points": qp}
pred = SamPredictor(SamHip("vit_b", precision="f16", seed=72, max_batch=8, max_decode_batch=128).to(dev))
tracker = PipsPointTracker(state_dict=init_pips_state_dict(72), fnet_chunk=8)
legs = [("default mode", {})]
if not args.baseline_only:
    legs += [("device_reinit", {"device_reinit": True}), ("device_reinit + device_tracks", {"device_reinit": True, "device_tracks": True})]
models = {name: SamPt(tracker, pred, sam_iou_threshold=-1e9, positive_point_selection_method="kmedoids",
                      negative_point_selection_method="mixed", positive_points_per_mask=16, negative_points_per_mask=1,
                      iterative_refinement_iterations=12, use_point_reinit=True, reinit_horizon=24, reinit_point_tracker_horizon=24,
                      reinit_variant="reinit-at-median-of-area-diff", **kw).eval() for name, kw in legs}
segments = {name: 0 for name, _ in legs}


def forward(name):
    model = models[name]
    track, n = model._track_points, [0]

    def counted(*a, **k):
        n[0] += 1
        return track(*a, **k)
    model._track_points = counted
    torch.manual_seed(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model(video)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    del model._track_points
    segments[name] = n[0]
    return ms, out


times = {name: [] for name, _ in legs}
outs = {}
for name, _ in legs:
    forward(name)                                           # warm-up: graphs, workspaces, staging
    outs[name] = forward(name)[1]
for _ in range(args.repeats):
    for name, _ in legs:
        times[name].append(forward(name)[0])
for name, kw in legs:
    s = stats(times[name])
    emit({"forward": f"SamPt(PipsPointTracker, ViT-B f16), use_point_reinit, horizon 24, {args.frames} frames {H}x{W}, {args.objects} objects, "
                     "16 kmedoids + 1 mixed points", "leg": name, **kw, "tracker_calls_per_forward": segments[name], **s,
          "frames_per_s": round(args.frames / (s["ms_median_min_max"][0] * 1e-3), 1)})
if not args.baseline_only:
    base = outs["default mode"]
    for name, _ in legs[1:]:
        o = outs[name]
        emit({"equal_to_default_mode": name, "logits": all(torch.equal(a, b) for a, b in zip(base["logits"], o["logits"])),
              "trajectories": bool(torch.equal(base["trajectories"], o["trajectories"])),
              "visibilities": bool(torch.equal(base["visibilities"], o["visibilities"]))})
        a, b = times["default mode"], times[name]
        gain = statistics.median(a) - statistics.median(b)
        noise = (max(a) - min(a)) + (max(b) - min(b))
        emit({"default_mode_minus": name, "ms": round(gain, 2), "sum_of_the_two_legs_min_max_ranges_ms": round(noise, 2),
              "beyond_the_spread": bool(abs(gain) > noise)})
log.close()
