#!/usr/bin/env python
"""All-pairs J&F counts (the DAVIS unsupervised protocol's input) and a BDD100K sequence: host against device
(sam_pt_amd/vos_metrics.py, csrc/vos_pairs.hip, csrc/vos_metrics.hip).

  python tools/jf_pairs_bench.py [--proposals 20] [--objects 4] [--frames 24] [--height 480] [--width 854] [--repeats 7] [--host-repeats 2]

The default shape is 20 proposals x 4 objects x 24 frames of 480 x 854 (the protocol's proposal limit on the bench clip's frame
size).  Three ways to the (P, K, T, 6) counts are timed, after their results are compared for equality:
  (a) host        download + jf_pairs_counts (numpy; every boundary dilated once)
  (b) pairwise    jf_counts_device over the P * K * T flattened pairs sharing planes: what the pairwise kernel alone can do; it reads
                  every mask K (or P) times and runs 2 * P * K dilations per frame
  (c) all pairs   jf_pairs_counts_device: P + K reads and dilations per frame, then a popcount GEMM over bit-planes
(b) and (c) alternate in one process, timed by a host clock around call + download and by events around the call alone; the kernels
of (c) are then timed under torch.profiler.  Last, a BDD100K sequence of the same frame size (index maps, --objects objects):
evaluate_bdd100k_sequence on the host against the device path.  Every timing reports its repeat spread."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import vos_metrics as VM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--proposals", type=int, default=20)
ap.add_argument("--objects", type=int, default=4)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=854)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--host-repeats", type=int, default=2)
args = ap.parse_args()
assert torch.cuda.is_available(), "jf_pairs_bench needs a GPU"
dev = torch.device("cuda:0")


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


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1)


def blobs(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 1, h // 16 + 2, w // 16 + 2, generator=g)
    return torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)[:, 0].contiguous()


def kernel_times(fn, names, repeats):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        sync()
    out = {k: [] for k in names}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            for k in names:
                if k in ev.name:
                    out[k].append(ev.time_range.elapsed_us())
    return out


P, K, T, h, w = args.proposals, args.objects, args.frames, args.height, args.width
r = VM.boundary_radius(h, w)
print(f"all pairs: {P} proposals x {K} objects x {T} frames of {h} x {w} = {P * K * T} pairs of {(P + K) * T} masks, radius {r} "
      f"(bound_th 0.008); {args.repeats} repeats after 1 warm-up ({args.host_repeats} for the host)")
gt_logits = blobs(K * T, h, w, 72).reshape(K, T, h, w)
A = torch.cat([torch.zeros(1, T, h, w), gt_logits]).argmax(0)              # (T, h, w): disjoint objects 1 .. K
A = torch.stack([A == k + 1 for k in range(K)])                            # (K, T, h, w) bool
S = torch.stack([torch.roll(A[p % K], (1 + p, 2 * p - 7), (1, 2)) ^ (blobs(T, h, w, 100 + p) > 1.2) for p in range(P)])   # (P, T, h, w)
S_d, A_d = S.to(dev), A.to(dev)
pp, kk, tt = np.meshgrid(np.arange(P), np.arange(K), np.arange(T), indexing="ij")
flat = dict(seg_planes=(pp * T + tt).reshape(-1), ann_planes=(kk * T + tt).reshape(-1))


def host():
    return VM.jf_pairs_counts(S_d.cpu().numpy(), A_d.cpu().numpy())


def pairwise():
    return VM.jf_counts_device(S_d, A_d, **flat)


def allpairs():
    return VM.jf_pairs_counts_device(S_d, A_d)


exp = None
t_host = []
for i in range(1 + args.host_repeats):
    t, exp = wall(host)
    if i >= 1:
        t_host.append(t)
b, c = pairwise().cpu().numpy().reshape(P, K, T, 6), allpairs().cpu().numpy()
assert np.array_equal(exp, b) and np.array_equal(exp, c), "host, pairwise and all-pairs counts differ"
print("host == pairwise == all pairs: equal counts")
t_b, t_c, e_b, e_c = [], [], [], []
for i in range(1 + args.repeats):
    tb, _ = wall(lambda: pairwise().cpu())
    tc, _ = wall(lambda: allpairs().cpu())
    eb, ec = event_ms(pairwise), event_ms(allpairs)
    if i >= 1:
        t_b.append(tb), t_c.append(tc), e_b.append(eb), e_c.append(ec)
print(f"  (a) host: download + jf_pairs_counts (numpy): {stats(t_host)}")
print(f"  (b) pairwise kernel over {P * K * T} items + the counts to the host: {stats(t_b)}")
print(f"  (c) all pairs + the counts to the host: {stats(t_c)}")
print(f"  (b) the call alone (events; with its host-side set-up and plane tables): {stats(e_b)}")
print(f"  (c) the call alone (events; the same): {stats(e_c)}")
mb, mc = statistics.median(e_b), statistics.median(e_c)
sp = max(max(e_b) - min(e_b), max(e_c) - min(e_c))
verdict = "beyond" if abs(mb - mc) > sp else "WITHIN"
print(f"  (b) - (c) = {mb - mc:.3f} ms ({mb / mc:.2f} x), {verdict} the larger spread of the two ({sp:.3f} ms)")
names = ("k_jfp_words", "k_jfp_dilate", "k_jfp_pairs")
kt = kernel_times(allpairs, names, args.repeats)
for k in names:
    print(f"    {k}, {len(kt[k])} launches: {stats(kt[k], 'us') if kt[k] else 'no profiler record'}")
names = ("k_jf_words", "k_jf_match")
kt = kernel_times(pairwise, names, args.repeats)
for k in names:
    print(f"    {k} (pairwise), {len(kt[k])} launches: {stats(kt[k], 'us') if kt[k] else 'no profiler record'}")

# ---- a BDD100K sequence: index maps of K objects, objects appearing late and disappearing
gt = torch.cat([torch.zeros(1, T, h, w), gt_logits]).argmax(0).to(torch.uint8)
gt[:T // 3][gt[:T // 3] == K] = 0                                          # the last object appears after a third of the frames
gt[T // 2:T // 2 + 3][gt[T // 2:T // 2 + 3] == 1] = 0                      # the first one is gone for three frames
pred = torch.roll(gt, (2, 3), (1, 2))
gt_d, pred_d = gt.to(dev), pred.to(dev)


def same(x, y):
    return all(np.array_equal(u, v, equal_nan=True) for k in ("J", "F", "J_vis", "F_vis", "J_nonvis", "F_nonvis") for u, v in zip(x[k], y[k]))


t_h, t_d = [], []
for i in range(1 + args.repeats):
    th, rh = wall(lambda: VM.evaluate_bdd100k_sequence(pred_d.cpu().numpy(), gt_d.cpu().numpy()))
    td, rd = wall(lambda: VM.evaluate_bdd100k_sequence(pred_d, gt_d))
    assert same(rh, rd), "BDD100K: host and device differ"
    if i >= 1:
        t_h.append(th), t_d.append(td)
print(f"BDD100K sequence: {K} objects x {T} frames of {h} x {w}, visible frames {rh['visible_frames'].tolist()}: device == host")
print(f"  (a) host: download + evaluate_bdd100k_sequence: {stats(t_h)}")
print(f"  (b) device: evaluate_bdd100k_sequence on HIP tensors (counts and areas to the host, statistics there): {stats(t_d)}")
print(f"  (a) - (b) = {statistics.median(t_h) - statistics.median(t_d):.1f} ms ({statistics.median(t_h) / statistics.median(t_d):.1f} x); "
      f"spread of (a)'s repeats {max(t_h) - min(t_h):.1f} ms, of (b)'s {max(t_d) - min(t_d):.3f} ms")
