#!/usr/bin/env python
"""TapNet point tracker on the device (sam_pt_amd.point_tracker.TapnetPointTracker, csrc/tapnet.hip, csrc/engine_tapnet.hip).

  python tools/tapnet_bench.py [--frames 24] [--height 480] [--width 854] [--queries 8 64] [--repeats 5] [--no-cpu]

The protocol of tools/tapir_bench.py: one clip of 24 frames at 480 x 854 (the adapter resizes it to the model's 256 x 256), with 8
and with 64 queries.  Printed, one JSON line for the backbone and one per query count:
  * device time between two events of the backbone alone (sampt_tapnet_backbone_f32: every block over all frames at once, the stem
    and the max-pool in chunks of 8 frames), of the whole engine call (backbone + query features + heads; heads = the second minus
    the first) and of the whole forward() (resize included);
  * nominal kernel launches per clip (sampt_tapnet_launches: the engine's own sum over the stages that ran, not a count at the launch
    sites);
  * the backbone convolutions against the fp16 matrix pipe: 2 x MACs x 3 fp16 MFMA products per fp32-grade product over the backbone
    time, as a fraction of the dense fp16 peak (2500 TFLOP/s) — the stem runs on the exact-f32 path and is counted the same way, and
    the time includes the norm / shift passes, the max-pool and the frame preparation, so this is a lower bound for the convolutions
    themselves;
  * the restatement of tests/tapnet_ref.py on the CPU on the same clip, the only comparison there is (no reference run exists:
    parity unpinned).
No target is attached to these figures; they are the starting point for tuning."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sam_pt_amd import _lib  # noqa: E402
from sam_pt_amd.point_tracker import TapnetPointTracker  # noqa: E402
from sam_pt_amd.synth import synthetic_clip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--queries", type=int, nargs="+", default=[8, 64])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement")
args = ap.parse_args()
assert torch.cuda.is_available(), "tapnet_bench needs a GPU"
dev = torch.device("cuda:0")
PEAK_FP16_TFLOPS = 2500.0
T, H, W = args.frames, args.height, args.width


def backbone_macs_per_frame():
    macs, side, cin = 128 * 128 * 64 * 7 * 7 * 3, 64, 64             # the stem; the max-pool halves the side before unit 0
    for c, stride in ((64, 1), (128, 2), (256, 1)):
        o = side // stride
        macs += o * o * c * (9 * cin + cin) + o * o * c * 9 * c          # block 0: conv_0 + shortcut, conv_2
        macs += 2 * o * o * c * 9 * c                                     # block 1
        side, cin = o, c
    return macs


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
frames_d = frames.to(dev)
trk = TapnetPointTracker()
frames01 = F.interpolate(frames_d / 255, (256, 256), mode="bilinear", align_corners=False, antialias=True).contiguous()
trk._ensure(dev)
grid = torch.empty((T, 32, 32, 256), device=dev)
ws = _lib.workspace("sampt_tapnet_backbone_workspace_bytes", dev, trk._h, T)


def backbone():
    _lib.check(trk._lib.sampt_tapnet_backbone_f32(trk._h, _lib.ptr(frames01), T, _lib.ptr(grid), None, _lib.ptr(ws), ws.numel(),
                                                  _lib.stream_ptr()), "sampt_tapnet_backbone_f32")


t_bb = timed(backbone, args.repeats)
macs = backbone_macs_per_frame() * T
print(json.dumps({"clip": [T, H, W], "backbone_ms": [round(v, 3) for v in t_bb], "backbone_launches": int(trk._lib.sampt_tapnet_launches(trk._h)),
                  "backbone_workspace_MB": round(ws.numel() / 1e6, 1), "backbone_GMAC_per_frame": round(macs / T / 1e9, 2),
                  "backbone_fp16_pipe_fraction": round(3 * 2 * macs / (t_bb[0] * 1e-3) / 1e12 / PEAK_FP16_TFLOPS, 4)}))
for n in args.queries:
    g = torch.Generator().manual_seed(n)
    q = torch.stack([torch.randint(0, T, (n,), generator=g).float(), torch.rand(n, generator=g) * W, torch.rand(n, generator=g) * H], 1)
    q256 = (q * torch.tensor([1.0, 256 / W, 256 / H])).to(dev)
    te = timed(lambda: trk.track(frames01, q256), args.repeats)
    launches = trk.stats["launches"]
    tf = timed(lambda: trk(frames_d[None], q[None].to(dev)), args.repeats)
    rec = {"queries": n, "engine_ms": [round(v, 3) for v in te], "forward_ms": [round(v, 3) for v in tf], "heads_ms": round(te[0] - t_bb[0], 3),
           "launches_per_clip": launches}
    if not args.no_cpu and n == min(args.queries):
        from tests import tapnet_ref as R
        video = (frames01.cpu() * 2 - 1).permute(0, 2, 3, 1)
        t = time.time()
        R.forward(trk._sd, video, q256.cpu()[:, [0, 2, 1]])
        rec["cpu_restatement_ms"] = round((time.time() - t) * 1e3, 1)
        rec["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(rec))
