#!/usr/bin/env python
"""YouTube-VIS AP / AR evaluation: the host restatement against the device path (sam_pt_amd/vis_metrics.py, csrc/vis_eval.hip).

  python tools/vis_eval_bench.py [--dets 100] [--gts 20] [--frames 36] [--height 480] [--width 854] [--warmup 15] [--timed 40]
                                 [--host-repeats 3]

The default is the project's VIS setting: 100 tracked proposals against 20 annotated objects over 36 frames of 480 x 854, one
category.  The detections are timed from f32 logits (threshold 0) and from byte masks; the ground truths are byte masks.
  (a) host    download + threshold + seq_iou_counts + match_video (numpy), `--host-repeats` times
  (b) device  bits_pack_device (both sides) + seq_iou_counts_device + match_video_device with the tables to the host, --warmup +
              --timed times, the whole call in wall time and each step between two events
Both give the same counts and tables (checked first).  The pack kernel's time (torch.profiler) is given as bytes of input per
second — both stacks are larger than the 256 MiB Infinity Cache — next to the 3.5 - 4.7 TB/s on file for k_rle_words / k_jf_words
(profiles/jf_bench.log); the IoU kernel's time goes alongside the number of (pair, word) operations it performs, from the shapes."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import vis_metrics as VM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dets", type=int, default=100)
ap.add_argument("--gts", type=int, default=20)
ap.add_argument("--frames", type=int, default=36)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--warmup", type=int, default=15)
ap.add_argument("--timed", type=int, default=40)
ap.add_argument("--host-repeats", type=int, default=3)
args = ap.parse_args()
assert torch.cuda.is_available(), "vis_eval_bench needs a GPU"
dev = torch.device("cuda:0")
HBM_GBS = 8000.0
D, G, T, h, w = args.dets, args.gts, args.frames, args.height, args.width


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


def events(fn, warmup, timed):
    ts = []
    for r in range(warmup + timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        sync()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
    return ts


def kernel_times(fn, repeats, names):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        sync()
    out = {k: [] for k in names}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            for k in names:
                if k in ev.name and not (k == "k_seq_iou" and "k_seq_iou_sum" in ev.name):
                    out[k].append(ev.time_range.elapsed_us())
    return out


def blobs(n, t, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn(n, t, h // 16 + 2, w // 16 + 2, generator=g, device=dev)
    return torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)


print(f"VIS AP / AR: {D} detections x {G} ground truths x {T} frames of {h} x {w}; device steps {args.warmup} warm-up + {args.timed} "
      f"timed, host {args.host_repeats} repeats after 1 warm-up")
gt_logits = blobs(G, T, 72) - 0.8
gt_masks = (gt_logits > 0).contiguous()
det_logits = torch.empty((D, T, h, w), dtype=torch.float32, device=dev)
for i in range(D):                                                        # jittered copies of the ground truths
    det_logits[i] = torch.roll(gt_logits[i % G], shifts=(2 * (i // G), 3 * (i // G)), dims=(1, 2)) + 0.25 * blobs(1, T, 100 + i)[0]
del gt_logits
det_masks = (det_logits > 0).contiguous()
dp, gp = np.arange(D * T, dtype=np.int32).reshape(D, T), np.arange(G * T, dtype=np.int32).reshape(G, T)
p = VM.Params()
rng = np.asarray(p.areaRng)


def flags(darea, garea):
    d_avg = np.array([VM._avg_area(r) for r in np.asarray(darea).reshape(D, T).tolist()])
    g_avg = np.array([VM._avg_area(r) for r in np.asarray(garea).reshape(G, T).tolist()])
    crowd = np.zeros(G, dtype=bool)
    order = np.argsort(-np.linspace(0.0, 1.0, D), kind="mergesort")       # (scores: any fixed order)
    g_ig = (g_avg[None, :] < rng[:, :1]) | (g_avg[None, :] > rng[:, 1:])
    d_out = (d_avg[None, order] < rng[:, :1]) | (d_avg[None, order] > rng[:, 1:])
    return order, g_ig, crowd, d_out


def host(det, thr):
    x = det.cpu().numpy().reshape(D * T, h, w)
    dm = x > np.float32(thr) if thr is not None else x
    gm = gt_masks.cpu().numpy().reshape(G * T, h, w)
    order, g_ig, crowd, d_out = flags(dm.sum(axis=(1, 2)), gm.sum(axis=(1, 2)))
    counts = VM.seq_iou_counts(dm, dp[order], gm, gp)
    return counts, VM.match_video(counts, g_ig, crowd, d_out, p.iouThrs)


def device(det, thr):
    db, da = VM.bits_pack_device(det.reshape(D * T, h, w), threshold=thr)
    gb, ga = VM.bits_pack_device(gt_masks.reshape(G * T, h, w))
    order, g_ig, crowd, d_out = flags(da.cpu().numpy(), ga.cpu().numpy())
    counts = VM.seq_iou_counts_device(db, da, dp[order], gb, ga, gp, h, w)
    return counts.cpu().numpy(), VM.match_video_device(counts, g_ig, crowd, d_out, p.iouThrs)


wp = ((h + 63) // 64) * w
pair_words = D * G * T * wp
tile_words = -(-D // 32) * 32 * -(-G // 32) * 32 * T * (-(-wp // 64) * 64)
for what, det, thr, in_bytes in (("f32 logits", det_logits, 0.0, 4 * D * T * h * w), ("byte masks", det_masks, None, D * T * h * w)):
    (hc, hm), (dc, dmt) = host(det, thr), device(det, thr)
    assert np.array_equal(hc, dc), f"{what}: host and device counts differ"
    for k in hm:
        assert np.array_equal(hm[k], dmt[k]), f"{what}: host and device tables differ in {k}"
    print(f"{what}: device == host counts and match tables; {int((hm['dt_match'][0, 0] > 0).sum())} of {D} detections matched at IoU 0.5")
    t_host = [wall(lambda: host(det, thr))[0] for _ in range(args.host_repeats)]
    t_dev = [wall(lambda: device(det, thr))[0] for _ in range(args.warmup + args.timed)][args.warmup:]
    a, b = statistics.median(t_host), statistics.median(t_dev)
    print(f"  (a) host: download + seq_iou_counts + match_video (numpy): {stats(t_host)}")
    print(f"  (b) device: pack + seq_iou_counts_device + match_video_device + tables to the host: {stats(t_dev)}")
    print(f"  (a) - (b) = {a - b:.1f} ms ({a / b:.1f} x); spread of (a)'s repeats {max(t_host) - min(t_host):.1f} ms, of (b)'s "
          f"{max(t_dev) - min(t_dev):.3f} ms")
    db, da = VM.bits_pack_device(det.reshape(D * T, h, w), threshold=thr)
    gb, ga = VM.bits_pack_device(gt_masks.reshape(G * T, h, w))
    counts = VM.seq_iou_counts_device(db, da, dp, gb, ga, gp, h, w)
    _, g_ig, crowd, d_out = flags(da.cpu().numpy(), ga.cpu().numpy())
    steps = (("pack of the detections", lambda: VM.bits_pack_device(det.reshape(D * T, h, w), threshold=thr)),
             ("sequence IoU", lambda: VM.seq_iou_counts_device(db, da, dp, gb, ga, gp, h, w)),
             ("matching, tables to the host", lambda: VM.match_video_device(counts, g_ig, crowd, d_out, p.iouThrs)))
    for name, fn in steps:
        print(f"    {name} (events around the call): {stats(events(fn, args.warmup, args.timed))}")
    kt = kernel_times(lambda: [fn() for _, fn in steps], args.timed, ("k_bits_pack", "k_seq_iou", "k_vis_match"))
    for k, ts in kt.items():
        if not ts:
            print(f"    {k}: no profiler record")
            continue
        med = statistics.median(ts)
        line = f"    {k}, {len(ts)} launches: {stats(ts, 'us')}"
        if k == "k_bits_pack":
            gbs = in_bytes / (med * 1e-6) / 1e9
            line += f" -> {in_bytes / 1e6:.0f} MB of input at {gbs:.0f} GB/s = {100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM peak"
        if k == "k_seq_iou":
            line += (f" -> {pair_words / 1e6:.0f} M (pair, word) operations ({tile_words / 1e6:.0f} M with the tiles' padding): "
                     f"{tile_words / (med * 1e-6) / 1e12:.2f} T popc(d & g) per second")
        print(line)
