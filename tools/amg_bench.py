#!/usr/bin/env python
"""SamAutomaticMaskGenerator.generate() on one synthetic 576 x 1024 frame at the VIS settings (configs/vis_eval_root.yaml: 32 x 32
points, 64 per batch): the fused path (batched decode + scoring on low-res masks) against ``fused=False`` (``predict_torch`` prompt by
prompt + tensor work on full-resolution logits), alternating in one process.

  python tools/amg_bench.py [--model vit_h|vit_b] [--hq] [--repeats 5] [--warmup 1] [--offset 0.02]
  python tools/amg_bench.py --tail both --min-area 100 [...]   # the tail after the survivors' masks (box NMS, small-region clean-up):
                                                   # device_tail=True against False on the fused path, alternating, + the two steps alone
  python tools/amg_bench.py --standalone [--masks 100] [--min-area 100]   # the two steps alone on seeded inputs, no model: clean-up of
                                                   # blob masks (device call against the host loop), NMS at n = 300, 1000, 3072
  python tools/amg_bench.py --standalone --rle [--masks 100] [--height 576] [--width 1024]   # run-length encoding alone on the
                                                   # seeded blob masks: (a) masks.cpu() + mask_to_rle + coco_rle_string, the host
                                                   # path, against (b) rle_encode_device(compressed=True); + the pixel pass's GB/s
                                                   # for byte and for float input (hip events around sampt_rle_count)
  python tools/amg_bench.py --output-mode coco_rle [...]   # generate() with an RLE output mode (coco_rle: device tail only)
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
ap.add_argument("--min-area", type=int, default=0, help="min_mask_region_area of generate() (0: no small-region clean-up, the VIS setting)")
ap.add_argument("--tail", default="device", choices=["both", "device", "host"],
                help="box NMS / clean-up on the device, on the host, or both alternating on the fused path")
ap.add_argument("--standalone", action="store_true", help="time the clean-up and NMS alone on seeded inputs (no model)")
ap.add_argument("--masks", type=int, default=100, help="--standalone: number of blob masks")
ap.add_argument("--rle", action="store_true", help="--standalone: time the run-length encoding (host path against the device encoder)")
ap.add_argument("--output-mode", default="binary_mask", choices=["binary_mask", "uncompressed_rle", "coco_rle"],
                help="output_mode of generate()")
args = ap.parse_args()

dev = torch.device("cuda:0")
sync = torch.cuda.synchronize
HBM_GBS = 8000.0        # MI355X HBM3E peak, the figure DESIGN.md quotes for the bandwidth-shaped kernels
REGION_BYTES_PER_PIXEL = 48


def stats(t):
    return f"median {statistics.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f} (spread {max(t) - min(t):.3f})"


def timed(fn, repeats, warmup=1):
    out = []
    for r in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def blob_masks(n, h, w, seed):
    """The seeded masks of tests/test_amg_tail_cpu.py: upsampled noise > 0.3, 0.4 % speckle, six stamped squares per mask."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 1, h // 8 + 2, w // 8 + 2, generator=g)
    m = torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)[:, 0] > 0.3
    m = m ^ (torch.rand(n, h, w, generator=g) < 0.004)
    for i in range(n):
        for _ in range(6):
            s = int(torch.randint(2, 12, (1,), generator=g))
            y = int(torch.randint(0, max(1, h - s + 1), (1,), generator=g))
            x = int(torch.randint(0, max(1, w - s + 1), (1,), generator=g))
            m[i, y:y + s, x:x + s] = bool(torch.randint(0, 2, (1,), generator=g))
    return m


def host_cleanup(masks, min_area):
    """The clean-up as the host tail runs it: masks to the host, two labellings per mask, masks back, boxes."""
    out = []
    for m in masks.cpu().numpy():
        m, _ = A.remove_small_regions(m, min_area, mode="holes")
        m, _ = A.remove_small_regions(m, min_area, mode="islands")
        out.append(torch.as_tensor(m))
    return A.batched_mask_to_box(torch.stack(out).to(masks.device))


def bench_cleanup(masks, min_area, repeats, host=True):
    n, h, w = masks.shape
    if n == 0:
        print("clean-up alone: no masks survive, nothing to time")
        return
    nbytes = n * h * w * REGION_BYTES_PER_PIXEL
    t_dev = timed(lambda: A.remove_small_regions_device(masks, min_area), repeats)
    gbs = nbytes / (statistics.median(t_dev) * 1e-3) / 1e9
    print(f"clean-up alone, {n} masks of {h} x {w}, min_area {min_area}: device {stats(t_dev)}")
    print(f"  byte count {nbytes / 1e6:.1f} MB = {REGION_BYTES_PER_PIXEL} B per pixel (per pass: mask 1 B read + 1 B written, label 4 B written + read "
          f"twice - three times in the islands pass -, size 4 B zeroed + 4 B read; chain reads, compress writes and atomics not counted) "
          f"-> {gbs:.0f} GB/s = {100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM peak")
    if host:
        t_host = timed(lambda: host_cleanup(masks, min_area), repeats)
        a, b = statistics.median(t_host), statistics.median(t_dev)
        print(f"  host loop (copy, scipy.ndimage.label twice per mask, copy back, boxes): {stats(t_host)}")
        print(f"  host - device = {a - b:.1f} ms ({a / b:.0f} x); sum of both spreads {max(t_host) - min(t_host) + max(t_dev) - min(t_dev):.1f} ms")


def bench_nms(n, repeats, thr=0.7, seed=5):
    g = torch.Generator().manual_seed(seed + n)
    xy = torch.rand(n, 2, generator=g) * (40.0 + 0.15 * n)
    boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 30.0], dim=1).to(dev)
    scores = torch.rand(n, generator=g).to(dev)
    t_dev = timed(lambda: A.nms_device(boxes, scores, thr), repeats)
    t_host = timed(lambda: A.nms(boxes, scores, thr), repeats)
    kept = len(A.nms_device(boxes, scores, thr))
    print(f"NMS alone, n = {n} (thr {thr}, {kept} kept): device {stats(t_dev)}")
    print(f"  host sweep: {stats(t_host)}; host - device = {statistics.median(t_host) - statistics.median(t_dev):.2f} ms")


def host_rle(masks):
    """What the RLE output modes cost without the device encoder: every mask to the host, the numpy loop, the string codec."""
    recs = A.mask_to_rle(masks.cpu())
    for r in recs:
        r["counts"] = A.coco_rle_string(r["counts"])
    return recs


def bench_rle_pixel_pass(x, threshold, repeats, what):
    """sampt_rle_count alone (the pass over the pixels + the two small scans) between two events on the stream."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    n, h, w = x.shape
    ws = torch.empty(lib.sampt_rle_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    is_f32 = int(x.dtype.is_floating_point)
    t = []
    for r in range(1 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.sampt_rle_count(_lib.ptr(x), is_f32, float(threshold), n, h, w, _lib.ptr(offsets), _lib.ptr(area), _lib.ptr(ws),
                                       ws.numel(), _lib.stream_ptr()), "sampt_rle_count")
        e1.record()
        sync()
        if r >= 1:
            t.append(e0.elapsed_time(e1))
    nbytes = x.numel() * x.element_size()
    gbs = nbytes / (statistics.median(t) * 1e-3) / 1e9
    print(f"  pixel pass ({what}, {nbytes / 1e6:.1f} MB read once; words, scan and offsets included): {stats(t)} -> {gbs:.0f} GB/s of input "
          f"= {100 * gbs / HBM_GBS:.1f} % of the {HBM_GBS:.0f} GB/s HBM peak")


def bench_rle(masks, repeats):
    n, h, w = masks.shape
    exp = host_rle(masks)
    got, _ = A.rle_encode_device(masks, compressed=True)
    assert got == exp, "device and host encodings differ"
    nruns = sum(len(A.coco_rle_counts(r["counts"])) for r in exp)
    nchars = sum(len(r["counts"]) for r in exp)
    print(f"RLE alone, {n} masks of {h} x {w}: {nruns} runs ({nruns // n} per mask), {nchars / 1e6:.2f} MB of COCO strings against "
          f"{n * h * w / 1e6:.1f} MB of mask bytes; device == host records")
    t_host, t_dev = [], []
    import gc
    for r in range(1 + repeats):                                     # alternating in one process
        gc.collect()                                                 # (the millions of Python ints of the previous records)
        a = timed(lambda: host_rle(masks), 1, warmup=0)
        gc.collect()
        b = timed(lambda: A.rle_encode_device(masks, compressed=True), 1, warmup=0)
        if r >= 1:
            t_host += a
            t_dev += b
    a, b = statistics.median(t_host), statistics.median(t_dev)
    print(f"  (a) host: masks.cpu() + mask_to_rle + coco_rle_string: {stats(t_host)}")
    print(f"  (b) device: rle_encode_device(compressed=True), strings on the host at the end: {stats(t_dev)}")
    print(f"  (a) - (b) = {a - b:.1f} ms ({a / b:.1f} x); spread of (a)'s repeats {max(t_host) - min(t_host):.1f} ms, of (b)'s "
          f"{max(t_dev) - min(t_dev):.1f} ms")
    t_alone = timed(lambda: A.rle_encode_device(masks, compressed=True), repeats)
    print(f"  (b) again, back to back (not alternating with the host path): {stats(t_alone)}")
    bench_rle_pixel_pass(masks, 0.0, repeats, "bytes")
    g = torch.Generator().manual_seed(73)
    logits = (torch.randn(n, h // 8 + 2, w // 8 + 2, generator=g)).to(dev)
    logits = torch.nn.functional.interpolate(logits[:, None], size=(h, w), mode="bilinear", align_corners=False)[:, 0].contiguous()
    bench_rle_pixel_pass(logits, 0.0, repeats, "f32 logits, threshold 0")
    # the stacks above fit the 256 MiB Infinity Cache, so a repeated pass can be served from it: the same pass over stacks that do not
    reps_b, reps_f = -(-300_000_000 // masks.numel()), -(-75_000_000 // logits.numel())
    bench_rle_pixel_pass(masks.repeat(reps_b, 1, 1), 0.0, repeats, f"bytes, the stack {reps_b} times over")
    bench_rle_pixel_pass(logits.repeat(reps_f, 1, 1), 0.0, repeats, f"f32 logits, the stack {reps_f} times over")
    t_f = timed(lambda: A.rle_encode_device(logits, threshold=0.0, compressed=True), repeats)
    print(f"  rle_encode_device(f32 logits, threshold=0.0, compressed=True) end to end: {stats(t_f)}")


if args.standalone and args.rle:
    print(f"standalone RLE: {args.masks} seeded blob masks of {args.height} x {args.width}; {args.repeats} repeats after 1 warm-up")
    bench_rle(blob_masks(args.masks, args.height, args.width, 72).to(dev), args.repeats)
    sys.exit(0)

if args.standalone:
    min_area = args.min_area or 100
    print(f"standalone: {args.masks} seeded blob masks of {args.height} x {args.width}, min_area {min_area}; {args.repeats} repeats after 1 warm-up")
    bench_cleanup(blob_masks(args.masks, args.height, args.width, 72).to(dev), min_area, args.repeats)
    for n_boxes in (300, 1000, 3072):
        bench_nms(n_boxes, args.repeats)
    sys.exit(0)

cfg = SAM_CONFIGS[args.model]
frames, _ = synthetic_clip(T=1, H=args.height, W=args.width, seed=72)
img = frames[0].permute(1, 2, 0).contiguous().numpy()
pred = SamPredictor(SamHip(config=cfg, seed=72, precision=args.precision, hq=args.hq).to(dev))

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
          stability_score_offset=args.offset, min_mask_region_area=args.min_area, output_mode=args.output_mode)
n_cand = len(ious)

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
if args.tail == "both":
    # ---- the tail: device_tail=True against False on the fused path, alternating in one process
    gens = {t: A.SamAutomaticMaskGenerator(None, predictor=pred, fused=True, device_tail=t, **kw) for t in (False, True)}
    times = {t: [] for t in gens}
    n_rec = {}
    for r in range(args.warmup + args.repeats):
        for t in (False, True):
            t_in_set[0] = 0.0
            sync()
            t0 = time.perf_counter()
            recs = gens[t].generate(img)
            sync()
            dt = (time.perf_counter() - t0 - t_in_set[0]) * 1e3
            n_rec[t] = len(recs)
            if r >= args.warmup:
                times[t].append(dt)
    for t in (True, False):
        print(f"generate() min_area {args.min_area}, device_tail={t}: {stats(times[t])} over {len(times[t])} repeats; {n_rec[t]} records")
    a, b = statistics.median(times[False]), statistics.median(times[True])
    sp = [max(times[t]) - min(times[t]) for t in (False, True)]
    print(f"host tail - device tail = {a - b:.1f} ms ({a / b:.2f} x); spreads {sp[0]:.1f} (host) + {sp[1]:.1f} (device) = {sum(sp):.1f} ms, "
          f"the larger {max(sp):.1f} ms")
    # ---- the two steps alone: the clean-up of the masks that reach it, NMS at the candidate count
    g0 = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=True, device_tail=True, **{**kw, "min_mask_region_area": 0})
    survivors = g0._generate_masks(img)["masks"]
    bench_cleanup(survivors, args.min_area or 100, args.repeats)
    bench_nms(n_cand, args.repeats)
    sys.exit(0)

paths = {"both": [False, True], "fused": [True], "unfused": [False]}[args.only]
if args.hq:
    paths = [True]                                     # fused=False with HQ-SAM decodes prompt by prompt: nothing batched to compare
gens = {f: A.SamAutomaticMaskGenerator(None, predictor=pred, fused=f, device_tail=args.tail == "device", **kw) for f in paths}

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
