#!/usr/bin/env python
"""Prediction overlays (sam_pt_amd/visualize.py, csrc/viz.hip): the host restatement against the device path.

  python tools/viz_bench.py [--frames 24] [--height 480] [--width 854] [--masks 3] [--points 16] [--repeats 20] [--host-repeats 2]
                            [--large-frames 240]

The default workload is 24 frames of 480 x 854 with 3 masks (float32 logits) and 16 points each, the predictions panel.  The
reference's own visualize_predictions needs cv2 and cannot be timed where cv2 is absent: the host side of the comparison is this
project's NumPy restatement of it (download of the logits included, as a user of the reference would have to), and it is named so.
The device path is pack (sampt_bits_pack) + band (sampt_viz_band) + compose (sampt_viz_compose): timed by device events around the
whole call and by a host clock around call + synchronise, after a warm-up, with the repeat spread; its three kernels are then timed
under torch.profiler in a pass of their own and their achieved rates are computed on the bytes the algorithm needs (pack: the
logits in, the bit-planes out; band: the bit-planes in and out; compose: 3 B read + 3 B written per pixel plus the two bit-planes
of every mask).  The device part is repeated on --large-frames frames, whose frames and output exceed the 256 MB Infinity Cache."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import visualize as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--masks", type=int, default=3)
ap.add_argument("--points", type=int, default=16)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-repeats", type=int, default=2)
ap.add_argument("--large-frames", type=int, default=240)
args = ap.parse_args()
assert torch.cuda.is_available(), "viz_bench needs a GPU"
dev = torch.device("cuda:0")
KERNELS = {"pack": "k_bits_pack", "band": "k_viz_band", "compose": "k_viz_compose"}


def sync():
    torch.cuda.synchronize()


def stats(ts, unit="ms"):
    return f"median {statistics.median(ts):.3f} {unit}, min {min(ts):.3f}, max {max(ts):.3f} (spread {max(ts) - min(ts):.3f})"


def workload(T, h, w, n, p, seed=72):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, 3, h, w), generator=g, dtype=torch.uint8)
    z = torch.randn(n * T, 1, h // 16 + 2, w // 16 + 2, generator=g)
    logits = torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False).reshape(n, T, h, w).contiguous()
    tr = torch.rand(T, n, p, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32)
    vis = (torch.rand(T, n, p, generator=g) < 0.8).float()
    return frames, logits, tr, vis


def kernel_times(fn, repeats):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        sync()
    out = {k: [] for k in KERNELS}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            for k, name in KERNELS.items():
                if name in ev.name:
                    out[k].append(ev.time_range.elapsed_us())
    return out


def measure(T, with_host):
    h, w, n, p = args.height, args.width, args.masks, args.points
    frames, logits, tr, vis = workload(T, h, w, n, p)
    kw = dict(positive_points_per_mask=p // 2)
    d = [x.to(dev) for x in (frames, logits, tr, vis)]
    planes = n * T * ((h + 63) // 64) * w * 8
    need = {"pack": n * T * h * w * 4 + planes, "band": 2 * planes, "compose": T * h * w * 6 + 2 * planes}
    print(f"{T} frames of {h} x {w}, {n} masks (float32 logits), {p} points each, predictions panel; frames + output "
          f"{T * h * w * 6 / 1e6:.1f} MB, logits {n * T * h * w * 4 / 1e6:.1f} MB, bit-planes {planes / 1e6:.2f} MB per set")

    def device():
        return V.render_predictions(*d, **kw)

    got = device()
    sync()
    if with_host:
        t_host, want = [], None
        for i in range(1 + args.host_repeats):
            t0 = time.perf_counter()
            want = V.render_predictions_host(d[0].cpu(), d[1].cpu(), d[2].cpu(), d[3].cpu(), **kw)
            if i >= 1:
                t_host.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got.cpu().numpy(), want), "host and device frames differ"
        print("  device == host restatement: equal bytes")
        print(f"  host: download + render_predictions_host (this project's NumPy restatement of the reference's function, which needs "
              f"cv2 and is not timed), {args.host_repeats} repeats after 1 warm-up: {stats(t_host)}")
    t_ev, t_wall = [], []
    for i in range(2 + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        t0 = time.perf_counter()
        e0.record()
        device()
        e1.record()
        sync()
        if i >= 2:
            t_wall.append((time.perf_counter() - t0) * 1e3), t_ev.append(e0.elapsed_time(e1))
    print(f"  device: render_predictions, pack + band + compose with the marker table's torch operations, {args.repeats} repeats after "
          f"2 warm-ups, events: {stats(t_ev)}")
    print(f"  device: the same by a host clock around call + synchronise: {stats(t_wall)}")
    if with_host:
        print(f"  host / device = {statistics.median(t_host) / statistics.median(t_wall):.0f} x (medians, host clock on both sides)")
    kt = kernel_times(device, max(3, args.repeats // 4))
    for k, name in KERNELS.items():
        if not kt[k]:
            print(f"    {name}: no profiler record")
            continue
        us = statistics.median(kt[k])
        print(f"    {name}, {len(kt[k])} launches: {stats(kt[k], 'us')}; needs {need[k] / 1e6:.2f} MB -> {need[k] / us / 1e6:.3f} TB/s achieved")
    del d, got


print(f"viz_bench on {torch.cuda.get_device_name(0)}")
measure(args.frames, True)
if args.large_frames:
    print("beyond the Infinity Cache:")
    measure(args.large_frames, False)
