#!/usr/bin/env python
"""TinyViT image encoder on the device (MobileSAM / Light HQ-SAM: csrc/tinyvit.hip, csrc/engine_tinyvit.hip).

  python tools/tinyvit_bench.py [--batch 8] [--repeats 7] [--frames 24] [--no-vit] [--no-forward]

One machine, one run.  Printed, one JSON line each:
  * encode: device time between two events of ``encode_frames`` over ``--batch`` frames of the bench clip (576 x 1024, padded to
    1024^2 by Sam.preprocess) for ``vit_t`` — and, unless --no-vit, for ``vit_b`` and ``vit_h`` in ``f16x3`` beside it, the ViT's
    mode of the same arithmetic grade (dead-row skipping on, as shipped).  Median, min, max over --repeats after one warm-up call;
  * stages: per-stage device time of one vit_t call from HIP events recorded inside the engine (sampt_tinyvit_encode_stages): patch
    embed, the four layers, the neck.  layers.0 holds the MBConv hidden map (256 channels at 256^2) that makes two round trips
    through memory per block in this first form: the figure a fused MBConv would have to beat;
  * depthwise: the depthwise 3 x 3 kernel alone at layers.0's shape (batch, 256, 256, 256), stride 1, GELU on: time and achieved
    bytes per second, counting the bytes the algorithm needs — one read of the input, one write of the output, the weights — over
    the kernel's event time, as a fraction of the 8 TB/s HBM peak (a lower bound for what the kernel moves: halo rows are re-read
    through the caches);
  * forward: one blocking ``SamPt.forward`` of the bench clip (24 frames, 8 positive points, 12 refinement iterations) with
    PipsPointTracker and MobileSAM (vit_t) — BASELINE config #1's pairing — as host wall time around a device synchronise, and the
    frames per second that makes: first as shipped, one item per decoder chain (``SamHip.clip_decode_batch`` = 1, bitwise equal to
    the per-frame path), then with the chains batched up to ``max_decode_batch``, which prices that guarantee.
Random weights (no checkpoint exists here): times do not depend on them.  No target is attached to these figures."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sam_pt_amd import _lib  # noqa: E402
from sam_pt_amd.sam_predictor import SamHip, SamPredictor  # noqa: E402
from sam_pt_amd.synth import bench_clip  # noqa: E402
from sam_pt_amd.weights import SAM_CONFIGS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--no-vit", action="store_true", help="skip vit_b / vit_h")
ap.add_argument("--no-forward", action="store_true", help="skip the SamPt.forward")
args = ap.parse_args()
assert torch.cuda.is_available(), "tinyvit_bench needs a GPU"
dev = torch.device("cuda:0")
PEAK_HBM_TBS = 8.0


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
    return [round(v, 3) for v in (statistics.median(out), min(out), max(out))]


frames, qp = bench_clip(T=args.frames, seed=72, n_pos=8)
frames_d = frames.to(dev)
B = args.batch
H, W = frames.shape[-2:]

# ---- encode_frames, vit_t and the ViTs of the same grade
preds = {}
for name, prec in [("vit_t", "f16x3")] + ([] if args.no_vit else [("vit_b", "f16x3"), ("vit_h", "f16x3")]):
    pred = SamPredictor(SamHip(variant=name, precision=prec, max_batch=B).to(dev))
    t = timed(lambda: pred.encode_frames(frames_d[:B], chw=True), args.repeats)
    print(json.dumps({"encode": name, "precision": "fp32 grade (one arithmetic)" if name == "vit_t" else prec, "frames": B, "frame_hw": [H, W],
                      "ms_median_min_max": t, "ms_per_frame": round(t[0] / B, 3), "workspace_MB": round(pred._vit_ws(B).numel() / 1e6, 1)}))
    if name == "vit_t":
        preds[name] = pred
    else:
        del pred
        torch.cuda.empty_cache()

# ---- per-stage times of one vit_t call
pred = preds["vit_t"]
cfg = SAM_CONFIGS["vit_t"]
out = torch.empty((B, cfg.grid ** 2, cfg.out_chans), device=dev)
ws = pred._vit_ws(B)
ms = (C.c_float * 6)()
rows = []
for _ in range(args.repeats):
    _lib.check(pred._lib.sampt_tinyvit_encode_stages(pred._vit, _lib.ptr(frames_d[:B]), 1, B, H, W, _lib.ptr(out), None, None, ms, _lib.ptr(ws),
                                                     ws.numel(), _lib.stream_ptr()), "sampt_tinyvit_encode_stages")
    rows.append(list(ms))
med = [round(statistics.median(r[i] for r in rows), 3) for i in range(6)]
print(json.dumps({"stages_ms": dict(zip(["patch_embed", "layers.0", "layers.1", "layers.2", "layers.3", "neck"], med)), "sum_ms": round(sum(med), 3),
                  "frames": B}))

# ---- the depthwise kernel at layers.0's shape
R0, Ch = cfg.resolutions[0], cfg.embed_dims[0] * cfg.mbconv_expand_ratio
x = torch.randn((B, R0, R0, Ch), device=dev)
y = torch.empty_like(x)
w, b = torch.randn((3, 3, Ch), device=dev), torch.randn((Ch,), device=dev)
t = timed(lambda: _lib.check(pred._lib.sampt_tinyvit_dwconv3x3_nhwc(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, R0, R0, Ch, 1, 1,
                                                                    _lib.stream_ptr()), "sampt_tinyvit_dwconv3x3_nhwc"), args.repeats)
nbytes = 2 * x.numel() * 4 + w.numel() * 4 + b.numel() * 4
print(json.dumps({"depthwise_shape": [B, R0, R0, Ch], "ms_median_min_max": t, "algorithm_MB": round(nbytes / 1e6, 1),
                  "achieved_TBps": round(nbytes / (t[0] * 1e-3) / 1e12, 3), "fraction_of_hbm_peak": round(nbytes / (t[0] * 1e-3) / 1e12 / PEAK_HBM_TBS, 3)}))
del x, y

# ---- one blocking SamPt.forward: PIPS + MobileSAM
if not args.no_forward:
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_pt import SamPt
    model = SamPt(PipsPointTracker(), pred, sam_iou_threshold=0.7, positive_points_per_mask=8, negative_points_per_mask=0,
                  iterative_refinement_iterations=12).eval()
    video = {"image": [f for f in frames_d], "target_hw": (H, W), "query_points": qp}
    for per_chain in (pred.model.clip_decode_batch, pred.model.max_decode_batch):
        pred.model.clip_decode_batch = per_chain
        model(video)                                        # warm-up: engines, graphs, workspaces
        torch.cuda.synchronize()
        times = []
        for _ in range(max(3, args.repeats // 2)):
            t0 = time.perf_counter()
            model(video)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        m = statistics.median(times)
        print(json.dumps({"forward": "SamPt(PipsPointTracker, MobileSAM vit_t)", "clip_decode_batch": per_chain, "frames": args.frames,
                          "ms_median_min_max": [round(m, 2), round(min(times), 2), round(max(times), 2)],
                          "frames_per_s": round(args.frames / (m * 1e-3), 1)}))
