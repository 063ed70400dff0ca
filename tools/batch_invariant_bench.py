#!/usr/bin/env python
"""The price of batch-invariant mask decoding (SamHip(batch_invariant_decode=True), sampt_dec_set_batch_invariant).

  python tools/batch_invariant_bench.py [--tag this] [--baseline-only] [--repeats 7] [--no-headline] [--log profiles/batch_invariant_bench.log]

One machine, one run; every leg of a comparison runs in this process, the legs alternating inside every repeat, after a warm-up
of each.  One JSON line per figure, printed and appended to --log:
  * predict: ``predict_torch`` with one prompt (6 points) at the shipped decoder geometry — grid 64, 576 x 1024 output — on a seeded
    embedding: device time between two events around --calls calls, per call.  Default mode against invariant mode.
  * forward: one blocking ``SamPt.forward`` of tools/tinyvit_bench.py's clip (24 frames, PIPS + MobileSAM vit_t, 8 positive points,
    12 refinement iterations), host wall time around a device synchronise.  Three legs: decoder chains of one item (what a TinyViT
    predictor ships with when the mode is off), ``clip_decode_batch = 128`` without the mode, the mode with chains of 128.
  * headline: bench.py's default configuration (its own ``build_model`` and ``one_step``, two clips alternating) with the mode off and
    on: informational.
--baseline-only runs the legs that need no new API (default-mode predict, chains of one, chains of 128) and nothing else: that is
the run to make on a build of the parent commit, with this file copied beside it, for the baseline of each figure.
"spread" is (max - min) / median over the repeats of a leg.  Random weights: times do not depend on them."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sam_pt_amd.sam_predictor import SamHip, SamPredictor  # noqa: E402
from sam_pt_amd.synth import bench_clip  # noqa: E402
from sam_pt_amd.weights import SAM_CONFIGS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="this", help="which build ran (written into every line)")
ap.add_argument("--baseline-only", action="store_true", help="only the legs the parent commit's API has")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="predict_torch calls per timed window")
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--headline-steps", type=int, default=6)
ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_invariant_bench.log"))
args = ap.parse_args()
assert torch.cuda.is_available(), "batch_invariant_bench needs a GPU"
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
    return {"ms_median_min_max": [round(med, 4), round(min(ms), 4), round(max(ms), 4)], "spread": round((max(ms) - min(ms)) / med, 4),
            "repeats": len(ms)}


def set_mode(pred, on):
    if not args.baseline_only:
        pred.set_batch_invariant_decode(on)
    else:
        assert not on


modes = [False] if args.baseline_only else [False, True]

# ---- predict_torch, one prompt, grid 64, 576 x 1024
cfg = SAM_CONFIGS["vit_t"]
pred = SamPredictor(SamHip(variant="vit_t", seed=72).to(dev))
pred._ensure()
g = torch.Generator().manual_seed(72)
emb = torch.randn(cfg.grid ** 2, cfg.out_chans, generator=g).to(dev)
pred.set_features(emb, (576, 1024), (576, 1024))
pts = (torch.rand(1, 6, 2, generator=g) * torch.tensor([1023.0, 575.0])).to(dev)
lab = torch.tensor([[1, 1, 1, 1, 0, 0]], dtype=torch.int32, device=dev)


def predict_window():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.calls):
        pred.predict_torch(pts, lab, multimask_output=False, return_logits=True)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.calls


times = {m: [] for m in modes}
outs = {}
for m in modes:
    set_mode(pred, m)
    predict_window()
    outs[m] = pred.predict_torch(pts, lab, multimask_output=False, return_logits=True)[0].cpu()
for _ in range(args.repeats):
    for m in modes:
        set_mode(pred, m)
        times[m].append(predict_window())
for m in modes:
    emit({"predict": "predict_torch, 1 prompt of 6 points, grid 64, 576x1024 logits", "batch_invariant": m, "calls_per_window": args.calls,
          **stats(times[m])})
if len(modes) == 2:
    d = (outs[True] - outs[False]).abs().max().item()
    emit({"predict_modes_max_abs_logit_diff": d, "max_abs_logit": outs[False].abs().max().item()})
set_mode(pred, False)

# ---- SamPt.forward, PIPS + MobileSAM, tools/tinyvit_bench.py's clip
from sam_pt_amd.point_tracker import PipsPointTracker  # noqa: E402
from sam_pt_amd.sam_pt import SamPt  # noqa: E402

frames, qp = bench_clip(T=args.frames, seed=72, n_pos=8)
frames_d = frames.to(dev)
H, W = frames.shape[-2:]
model = SamPt(PipsPointTracker(), pred, sam_iou_threshold=0.7, positive_points_per_mask=8, negative_points_per_mask=0,
              iterative_refinement_iterations=12).eval()
video = {"image": [f for f in frames_d], "target_hw": (H, W), "query_points": qp}
legs = [("chains of one item, mode off", 1, False), ("chains of 128, mode off", pred.model.max_decode_batch, False)]
if not args.baseline_only:
    legs.append(("chains of 128, mode on", pred.model.max_decode_batch, True))


def forward(leg):
    _, per_chain, on = leg
    pred.model.clip_decode_batch = per_chain
    set_mode(pred, on)
    t0 = time.perf_counter()
    out = model(video)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


ftimes = {leg[0]: [] for leg in legs}
flog = {}
for leg in legs:
    forward(leg)                                            # warm-up: graphs, workspaces, staging of this leg
    flog[leg[0]] = forward(leg)[1]["logits"][0].cpu()
for _ in range(args.repeats):
    for leg in legs:
        ftimes[leg[0]].append(forward(leg)[0])
for leg in legs:
    s = stats(ftimes[leg[0]])
    emit({"forward": "SamPt(PipsPointTracker, MobileSAM vit_t), 24 frames 576x1024", "leg": leg[0], "clip_decode_batch": leg[1],
          "batch_invariant": leg[2], **s, "frames_per_s": round(args.frames / (s["ms_median_min_max"][0] * 1e-3), 1)})
if not args.baseline_only:
    one, many_off, many_on = (flog[leg[0]] for leg in legs)
    fin = torch.isfinite(one)
    emit({"forward_logits": "against the chains-of-one leg (mode off)", "finite_pixels_compared": int(fin.sum()), "pixels": fin.numel(),
          "chains_of_128_mode_off_equal": bool(torch.equal(one, many_off)),
          "chains_of_128_mode_off_max_abs_diff": float((one - many_off)[fin].abs().max()) if fin.any() else 0.0,
          "note": "informational: seeded weights and sam_iou_threshold 0.7 reject frames (all -inf, nothing to compare there); what the "
                  "mode computes is held by tests/test_gpu_batch_invariant.py", "chains_of_128_mode_on_max_abs_diff": float((one - many_on)[fin].abs().max()) if fin.any() else 0.0})
    a, b = ftimes[legs[0][0]], ftimes[legs[2][0]]
    gain = statistics.median(a) - statistics.median(b)
    noise = (max(a) - min(a)) + (max(b) - min(b))
    emit({"claim": "batched and bitwise", "chains_of_one_minus_mode_on_ms": round(gain, 3), "sum_of_the_two_legs_min_max_ranges_ms": round(noise, 3),
          "stands": bool(gain > noise)})
set_mode(pred, False)
del model, pred
torch.cuda.empty_cache()

# ---- bench.py's headline configuration, mode off / on (informational)
if not args.no_headline and not args.baseline_only:
    import bench  # noqa: E402
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1"]
    bargs = bench.parse()
    sys.argv = argv
    fr_a, qp_a = bench_clip(T=bargs.frames, seed=72, n_pos=bargs.points, n_objects=bargs.objects)
    fr_b, qp_b = bench_clip(T=bargs.frames, seed=1072, n_pos=bargs.points, n_objects=bargs.objects)
    Hh, Ww = fr_a.shape[-2:]
    clips = [{"image": [f for f in fr.to(dev)], "target_hw": (Hh, Ww), "query_points": q} for fr, q in ((fr_a, qp_a), (fr_b, qp_b))]
    hmodel = bench.build_model(bargs, dev)
    hpred = hmodel.sam_predictor

    def hstep(i):
        t0 = time.perf_counter()
        bench.one_step(hmodel, clips[i % 2], bargs.frames, "sequences", False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ht = {False: [], True: []}
    for on in (False, True):
        hpred.set_batch_invariant_decode(on)
        hstep(0), hstep(1)
    for i in range(args.headline_steps):
        for on in (False, True):
            hpred.set_batch_invariant_decode(on)
            ht[on].append(hstep(i))
    for on in (False, True):
        s = stats(ht[on])
        emit({"headline": f"bench.py defaults ({bargs.model}, {bargs.precision}, {bargs.frames} frames, {bargs.tracker}), sequential steps",
              "batch_invariant": on, **s, "frames_per_s": round(bargs.frames / (s["ms_median_min_max"][0] * 1e-3), 1)})
log.close()
