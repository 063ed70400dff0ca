#!/usr/bin/env python
"""DAVIS J&F evaluation: the host restatement against the device path (sam_pt_amd/vos_metrics.py, csrc/vos_metrics.hip).

  python tools/jf_bench.py [--objects 4] [--frames 24] [--height 480] [--width 854] [--repeats 7]

The default stack is 4 objects x 24 frames of 480 x 854: the bench clip's frame size with the tests' 4-object stack.  Three input
kinds are timed, each first checked for equal counts on both paths:
  byte masks   (M * T, H, W) bool           host: jf_counts on the stack downloaded with .cpu()
  f32 logits   (M * T, H, W) float32, thr 0  the prediction as logits, binarised in the kernel
  index maps   (T, H, W) uint8 x 2           the M objects of a frame share its plane
(a) host and (b) device alternate in one process.  Then the device call alone between two events, and its two kernels' times from
torch.profiler over the same calls: pass A (k_jf_words, reads every pixel once) as bytes of input per second, pass B (k_jf_match)
beside it.  Stacks beyond the 256 MiB Infinity Cache are timed as well, since a repeated pass over a smaller one is served from it."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import _lib  # noqa: E402
from sam_pt_amd import vos_metrics as VM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=4)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "jf_bench needs a GPU"
dev = torch.device("cuda:0")
HBM_GBS = 8000.0


def sync():
    torch.cuda.synchronize()


def stats(ts, unit="ms"):
    return f"median {statistics.median(ts):.3f} {unit}, min {min(ts):.3f}, max {max(ts):.3f} (spread {max(ts) - min(ts):.3f})"


def wall(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def blobs(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 1, h // 16 + 2, w // 16 + 2, generator=g)
    return torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)[:, 0].contiguous()


def kernel_times(fn, repeats):
    """{kernel: [us per launch]} of the vos_metrics kernels over `repeats` calls of fn (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        sync()
    out = {"k_jf_words": [], "k_jf_match": []}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            for k in out:
                if k in ev.name:
                    out[k].append(ev.time_range.elapsed_us())
    return out


def device_alone(what, call, in_bytes, repeats):
    """The device call alone: events around it, then its kernels under the profiler."""
    ts = []
    for r in range(1 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        sync()
        if r >= 1:
            ts.append(e0.elapsed_time(e1))
    print(f"  device call alone ({what}, {in_bytes / 1e6:.1f} MB of input, events around jf_counts_device): {stats(ts)}")
    kt = kernel_times(call, repeats)
    for k, label in (("k_jf_words", "pass A"), ("k_jf_match", "pass B")):
        if not kt[k]:
            print(f"    {label} ({k}): no profiler record")
            continue
        med = statistics.median(kt[k])
        line = f"    {label} ({k}), {len(kt[k])} launches: {stats(kt[k], 'us')}"
        if k == "k_jf_words":
            gbs = in_bytes / (med * 1e-6) / 1e9
            line += f" -> {gbs:.0f} GB/s of input = {100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM peak"
        print(line)


def alternate(what, host, device, repeats):
    exp, got = host(), device()
    assert np.array_equal(exp, got), f"{what}: host and device counts differ"
    t_host, t_dev = [], []
    for r in range(1 + repeats):
        a, _ = wall(host)
        b, _ = wall(device)
        if r >= 1:
            t_host.append(a)
            t_dev.append(b)
    a, b = statistics.median(t_host), statistics.median(t_dev)
    print(f"{what}: device == host counts")
    print(f"  (a) host: download + jf_counts (numpy): {stats(t_host)}")
    print(f"  (b) device: jf_counts_device + the counts to the host: {stats(t_dev)}")
    print(f"  (a) - (b) = {a - b:.1f} ms ({a / b:.1f} x); spread of (a)'s repeats {max(t_host) - min(t_host):.1f} ms, of (b)'s "
          f"{max(t_dev) - min(t_dev):.3f} ms")
    return exp


M, T, h, w = args.objects, args.frames, args.height, args.width
n = M * T
r = VM.boundary_radius(h, w)
print(f"J&F: {M} objects x {T} frames of {h} x {w} = {n} items, radius {r} (bound_th 0.008); {args.repeats} repeats after 1 warm-up")
logits_pred = blobs(n, h, w, 72).reshape(M, T, h, w)
logits_gt = torch.roll(logits_pred, (3, 5), (2, 3)) + 0.3 * blobs(n, h, w, 73).reshape(M, T, h, w)
bg = torch.zeros(1, T, h, w)
pred_idx = torch.cat([bg, logits_pred]).argmax(0).to(torch.uint8)          # (T, h, w): what dist.index_masks hands over
gt_idx = torch.cat([bg, logits_gt]).argmax(0).to(torch.uint8)
ids = torch.arange(1, M + 1, dtype=torch.uint8)[:, None, None, None]
seg = (pred_idx[None] == ids).reshape(n, h, w)
ann = (gt_idx[None] == ids).reshape(n, h, w)
seg_logits = torch.where(seg, logits_pred.reshape(n, h, w).abs() + 0.01, -logits_pred.reshape(n, h, w).abs()).contiguous()
seg_d, ann_d, lg_d, pi_d, gi_d = seg.to(dev), ann.to(dev), seg_logits.to(dev), pred_idx.to(dev), gt_idx.to(dev)
values = np.repeat(np.arange(1, M + 1), T)
planes = np.tile(np.arange(T), M)
ikw = dict(seg_values=values, seg_planes=planes, ann_values=values, ann_planes=planes)

c0 = alternate("byte masks", lambda: VM.jf_counts(seg_d.cpu(), ann_d.cpu()), lambda: VM.jf_counts_device(seg_d, ann_d).cpu().numpy(),
               args.repeats)
device_alone("byte masks", lambda: VM.jf_counts_device(seg_d, ann_d), 2 * n * h * w, args.repeats)
c1 = alternate("f32 logits against byte masks", lambda: VM.jf_counts(lg_d.cpu(), ann_d.cpu(), seg_threshold=0.0),
               lambda: VM.jf_counts_device(lg_d, ann_d, seg_threshold=0.0).cpu().numpy(), args.repeats)
device_alone("f32 logits + byte masks", lambda: VM.jf_counts_device(lg_d, ann_d, seg_threshold=0.0), 5 * n * h * w, args.repeats)
c2 = alternate("index maps", lambda: VM.jf_counts(pi_d.cpu()[None] == ids, gi_d.cpu()[None] == ids),
               lambda: VM.jf_counts_device(pi_d, gi_d, **ikw).cpu().numpy(), args.repeats)
device_alone(f"index maps, {M} objects per plane; input counted once per item", lambda: VM.jf_counts_device(pi_d, gi_d, **ikw),
             2 * n * h * w, args.repeats)
assert np.array_equal(c0, c1) and np.array_equal(c0, c2), "the three input kinds disagree"
J, F = VM.jaccard_from_counts(c0), VM.f_measure(c0)[0]
print(f"all three kinds give the same counts; J mean {J.mean():.4f}, F mean {F.mean():.4f}")

# beyond the Infinity Cache: the same pass over stacks of more than 256 MiB
reps_b, reps_f = -(-300_000_000 // (2 * seg_d.numel())), -(-400_000_000 // (5 * lg_d.numel()))
big_s, big_a = seg_d.repeat(reps_b, 1, 1), ann_d.repeat(reps_b, 1, 1)
print(f"larger stacks (the workspace limit raised so that one call takes the whole stack):")
ws_b = int(_lib.load().sampt_jf_workspace_bytes(big_s.shape[0], h, w, r))
device_alone(f"byte masks, the stack {reps_b} times over", lambda: VM.jf_counts_device(big_s, big_a, workspace_bytes=ws_b),
             2 * big_s.numel(), args.repeats)
del big_s, big_a
big_l, big_a = lg_d.repeat(reps_f, 1, 1), ann_d.repeat(reps_f, 1, 1)
ws_f = int(_lib.load().sampt_jf_workspace_bytes(big_l.shape[0], h, w, r))
device_alone(f"f32 logits + byte masks, the stack {reps_f} times over",
             lambda: VM.jf_counts_device(big_l, big_a, seg_threshold=0.0, workspace_bytes=ws_f), 5 * big_l.numel(), args.repeats)
