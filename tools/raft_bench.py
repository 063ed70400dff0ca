#!/usr/bin/env python
"""RAFT point tracker on the device (sam_pt_amd.point_tracker.RaftPointTracker, csrc/raft.hip, csrc/engine_raft.hip).

  python tools/raft_bench.py [--frames 24] [--height 480] [--width 854] [--iters 32] [--pairs 8] [--repeats 3] [--points 64]

The default clip is 24 frames of 480 x 854 with the reference's 32 iterations: 46 pair-directions.  Printed:
  * flows() alone between two events: ms per clip and pair-directions per second; forward() (flows + chain) beside it;
  * the share of every kernel in the device time of one flows() call (torch.profiler; the same table comes from
    ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/raft_bench.py --repeats 1 --no-profile``);
  * the lookup kernel's achieved bytes per second: per pixel and level it reads one 10 x 10 patch of its correlation plane and it
    writes 352 floats per pixel, against the 8 TB/s HBM figure — the volume of a chunk (--pairs) exceeds the 256 MiB Infinity Cache
    from 1 pair on at this frame size, so the patches come from HBM.
No target is attached to these figures; they are the starting point for tuning."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sam_pt_amd.point_tracker import RaftPointTracker, raft_padded_size  # noqa: E402
from sam_pt_amd.synth import synthetic_clip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--pairs", type=int, default=8, help="pairs in flight (both directions of a pair travel together)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--points", type=int, default=64)
ap.add_argument("--no-profile", action="store_true", help="skip the torch.profiler pass (when an outer profiler is attached)")
args = ap.parse_args()
assert torch.cuda.is_available(), "raft_bench needs a GPU"
dev = torch.device("cuda:0")
HBM_GBS = 8000.0
T, H, W = args.frames, args.height, args.width
Hp, Wp = raft_padded_size(H, W)
hw, npd = (Hp // 8) * (Wp // 8), 2 * (T - 1)

frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
frames = frames.to(dev)
g = torch.Generator().manual_seed(1)
q = torch.stack([torch.randint(0, T, (args.points,), generator=g).float(), torch.rand(args.points, generator=g) * (W - 1),
                 torch.rand(args.points, generator=g) * (H - 1)], 1).to(dev)
trk = RaftPointTracker(iters=args.iters, max_pairs_in_flight=args.pairs)
print(f"RAFT: {T} frames of {H} x {W} (padded {Hp} x {Wp}, coarse grid {Hp // 8} x {Wp // 8} = {hw} pixels), {args.iters} iterations, "
      f"{npd} pair-directions, {args.pairs} pairs in flight; {args.repeats} repeats after 1 warm-up")


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


ts = timed(lambda: trk.flows(frames))
print(f"flows(): {line(ts)} -> {npd / (statistics.median(ts) * 1e-3):.1f} pair-directions/s")
ts = timed(lambda: trk(frames[None], q[None]))
print(f"forward() with {args.points} query points (flows + chain): {line(ts)}")

if not args.no_profile:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        trk.flows(frames)
        torch.cuda.synchronize()
    per = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            d = per.setdefault(ev.name.split("(")[0][:72], [0, 0.0])
            d[0] += 1
            d[1] += ev.time_range.elapsed_us()
    total = sum(v[1] for v in per.values())
    print(f"kernels of one flows() call: {sum(v[0] for v in per.values())} launches, {total / 1e3:.1f} ms of device time")
    for name, (n, us) in sorted(per.items(), key=lambda kv: -kv[1][1])[:16]:
        print(f"  {100 * us / total:5.1f} %  {us / 1e3:9.2f} ms  {n:6d} x {us / n:9.1f} us  {name}")
    look = [v for k, v in per.items() if "k_raft_lookup" in k]
    if look:
        n, us = look[0]
        rows = npd * hw * args.iters                                # pixels looked up over the call
        nbytes = rows * (4 * 100 * 4 + 352 * 4 + 8)
        gbs = nbytes / (us * 1e-6) / 1e9
        print(f"lookup: {n} launches, {us / n:.1f} us each, {nbytes / 1e9:.2f} GB read + written -> {gbs:.0f} GB/s = "
              f"{100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM figure")
