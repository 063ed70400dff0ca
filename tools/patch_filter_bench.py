#!/usr/bin/env python
"""Patch-similarity filter (sam_pt_amd/patch_filter.py, csrc/patch_filter.hip): the host path against the device path.

  python tools/patch_filter_bench.py [--frames 50] [--height 480] [--width 854] [--objects 5] [--points 9] [--patch-size 3]
                                     [--repeats 200] [--host-repeats 3] [--parent-source FILE]

The default workload is one call of ``SamPt._track_points``' filter stage: 50 frames of 480 x 854, 5 objects x 9 points, patch_size 3,
threshold 0.01, the border rule included; the points walk at random (0.8 px per frame) from seeded starts on seeded query frames
over ``synthetic_clip``.  Host path: ``SamPt._patch_similarity_filter`` + the four border lines on CPU tensors, by a host clock, with
the download of the clip (which a device-resident pipeline has to add) timed apart.  --parent-source names a copy of another
commit's sam_pt_amd/sam_pt.py (``git show REV:sam_pt_amd/sam_pt.py``): its ``_patch_similarity_filter`` is timed on the same inputs,
alternating with this tree's.  Device path: ``patch_similarity_filter`` with everything resident, after a warm-up, by device events
around each call and by a host clock around a batch of calls that ends in a synchronise; then the kernel alone under torch.profiler
in a pass of its own.  Before anything is timed the two paths' codes are compared on these inputs."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sam_pt_amd import patch_filter as PF  # noqa: E402
from sam_pt_amd.sam_pt import SamPt  # noqa: E402
from sam_pt_amd.synth import synthetic_clip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=50)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--objects", type=int, default=5)
ap.add_argument("--points", type=int, default=9)
ap.add_argument("--patch-size", type=int, default=3)
ap.add_argument("--threshold", type=float, default=0.01)
ap.add_argument("--repeats", type=int, default=200)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--parent-source", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")


def stats(ts, unit="ms"):
    return f"median {statistics.median(ts):.3f} {unit}, min {min(ts):.3f}, max {max(ts):.3f} (spread {max(ts) - min(ts):.3f})"


def workload(T, H, W, M, P, seed=72):
    g = torch.Generator().manual_seed(seed)
    frames, _ = synthetic_clip(T=T, H=H, W=W, seed=seed, disc_r=60.0)
    N = M * P
    t0 = torch.randint(0, T, (N,), generator=g)
    start = torch.rand(N, 2, generator=g) * torch.tensor([W - 40.0, H - 40.0]) + 20.0
    steps = 0.8 * torch.randn(T, N, 2, generator=g)
    walk = steps.cumsum(0)
    traj = start[None] + walk - walk[t0, torch.arange(N)][None]                  # passes through its start on its query frame
    q = torch.cat([t0[:, None].float(), start], dim=1)
    vis = (torch.rand(T, N, generator=g) < 0.9).float()
    return frames, q, traj.float(), vis


def host_call(cls, frames, q, traj, vis):
    self = type("HostFilter", (), {"patch_size": args.patch_size, "patch_similarity_threshold": args.threshold})()
    out = cls._patch_similarity_filter(self, frames, q, traj, vis, args.objects, args.points)
    h, w = frames.shape[-2:]
    out[traj[:, :, 0] / w < 0.01] = -2
    out[traj[:, :, 1] / h < 0.01] = -2
    out[traj[:, :, 0] / w > 0.99] = -2
    out[traj[:, :, 1] / h > 0.99] = -2
    return out


def main():
    assert torch.cuda.is_available(), "patch_filter_bench needs a GPU"
    T, H, W, M, P = args.frames, args.height, args.width, args.objects, args.points
    frames, q, traj, vis = workload(T, H, W, M, P)
    N = M * P
    taps = 2 * (args.patch_size // 2) + 1
    print(f"patch_filter_bench on {torch.cuda.get_device_name(0)}, torch.get_num_threads() = {torch.get_num_threads()}")
    print(f"{T} frames of {H} x {W} ({frames.numel() / 1e6:.1f} MB), {M} objects x {P} points, patch_size {args.patch_size} ({taps} x {taps} taps), "
          f"threshold {args.threshold}: {T * N} items, {int(vis.sum())} raw-visible; the host converts {frames.numel() / 1e6:.1f} M values to Lab, "
          f"the result depends on at most {T * N * taps * taps * 4} pixels")
    d = [x.to(dev) for x in (frames, q, traj, vis)]

    def device():
        return PF.patch_similarity_filter(*d, args.patch_size, args.threshold, border_rule=True)

    got, sim = PF.patch_similarity_filter(*d, args.patch_size, args.threshold, border_rule=True, return_similarities=True)
    torch.cuda.synchronize()
    classes = [("this tree", SamPt)]
    if args.parent_source:
        spec = importlib.util.spec_from_file_location("parent_sam_pt", args.parent_source)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        classes.append((f"{args.parent_source}", mod.SamPt))
    t_host = {name: [] for name, _ in classes}
    for i in range(1 + args.host_repeats):
        for name, cls in classes:                                                   # alternating
            t0 = time.perf_counter()
            want = host_call(cls, frames, q, traj, vis)
            if i >= 1:
                t_host[name].append((time.perf_counter() - t0) * 1e3)
            differ = got.cpu() != want
            margin = (sim.cpu() - args.threshold).abs()[vis == 1].min()
            if i == 0:
                print(f"  codes, device against the host path of {name}: {int(differ.sum())} of {want.numel()} differ; codes present "
                      f"{sorted(set(want.flatten().int().tolist()))}; closest raw-visible similarity to the threshold {float(margin):.3e}")
                assert not differ.any(), "host and device codes differ"
    for name, _ in classes:
        print(f"  host path of {name}: _patch_similarity_filter + border lines on CPU tensors, {args.host_repeats} repeats after 1 warm-up: "
              f"{stats(t_host[name])}")
    t_down = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d[0].cpu()
        if i >= 1:
            t_down.append((time.perf_counter() - t0) * 1e3)
    print(f"  download of the clip, which the host path adds when the frames live on the device: {stats(t_down)}")

    t_ev = []
    for i in range(10 + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device()
        e1.record()
        torch.cuda.synchronize()
        if i >= 10:
            t_ev.append(e0.elapsed_time(e1) * 1e3)
    print(f"  device path: patch_similarity_filter (wrapper + one launch), {args.repeats} repeats after 10 warm-ups, device events around each "
          f"call: {stats(t_ev, 'us')}")
    t_batch = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            device()
        torch.cuda.synchronize()
        if i >= 1:
            t_batch.append((time.perf_counter() - t0) * 1e6 / args.repeats)
    print(f"  device path: host clock around {args.repeats} calls + synchronise, per call, 5 batches after 1 warm-up: {stats(t_batch, 'us')}")
    host_ms = statistics.median(t_host["this tree"])
    print(f"  host / device = {host_ms * 1e3 / statistics.median(t_batch):.0f} x (medians, host clock on both sides; the host side without the "
          f"download)")

    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            device()
        torch.cuda.synchronize()
    ks = [ev.time_range.elapsed_us() for ev in prof.events()
          if ev.device_type == torch.autograd.DeviceType.CUDA and "k_patch_filter" in ev.name]
    print(f"    k_patch_filter, {len(ks)} launches under torch.profiler: {stats(ks, 'us')}" if ks else "    k_patch_filter: no profiler record")


if __name__ == "__main__":
    main()
