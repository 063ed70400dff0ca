"""Records tests/golden/superglue_ref.npz from the reference's SuperGlue point tracker run in place on the CPU
(tests/superglue_ref.py).

Seeded weights (weights.init_superpoint_state_dict / init_superglue_state_dict), the golden clip of superglue_ref.golden_clip
— 3 frames of 75 x 109 (no multiple of 8: the score map covers 72 x 104), two masks, 4 positive + 2 negative points each,
nms_radius 3, 20 Sinkhorn iterations — and NumPy's global generator seeded with GOLDEN_NP_SEED.  Stored:

  frames, masks, query_points, np_seed                     the tracker's input
  trajectories (1,3,12,2), visibilities (1,3,12)           its output (the live reference's)
  counts (3,), kpts{t}, kscores{t}                         SuperPoint's keypoints (x, y) and scores per frame
  dense_rows, dense (3, rows, 104)                         every 3rd row of the dense score maps
  desc_cols, desc{t} (256, cols)                           the sampled descriptors of every 4th keypoint
  gnn_cols{p}, gnn{p} (256, cols)                          the GNN's output descriptors of every 4th keypoint (set 0 then set 1)
  z_rows, Z{p} (rows, n1 + 1)                              every 4th row of the transport matrix
  matches{p}, mscores{p}                                   matches0 / matching_scores0 of pair p = (frame 0, frame p + 1)
  marginal{p}                                              keypoint-0 indices whose match could flip within the bars (see b)
  noise_* / bar_*                                          the reference's own arithmetic noise and 8 x it, per quantity

Noise (the recipe of oracle/noise_floor.py, the RAFT protocol): the larger of (1) the f32 run against a float64 run of the same
weights and (2) the f32 run against an f32 run with every weight multiplied by 1 + 1e-7 N(0, 1); later stages are fed the f32
run's keypoints so that the same entries are compared.  The float64 and perturbed runs use the restatement, which this tool
first checks against the live reference (== for keypoints, matches, trajectories, visibilities).

The tool asserts what the tests rely on and writes nothing otherwise:
  a. every frame's keypoint set is unchanged when its score map is perturbed by +- bar_scores (5 seeds) and in float64;
  b. matches0 of every pair is unchanged under +- bar_sinkhorn on Z (5 seeds) and in float64, outside the keypoints listed as
     marginal: row or column top-1 - top-2 gap below bar_sinkhorn, or |score - threshold| below bar_mscores; at most 2 % of a
     pair's keypoints are marginal;
  c. every pair has >= 10 valid matches and >= 10 unmatched keypoints;
  d. over the clip some (frame, mask) has more candidates than requested and some fewer, for positives and for negatives;
  e. 100..300 keypoints per frame, no count a multiple of 64, all unequal; the threshold and the border removal both remove
     local maxima; no score reaches 0.45 (the empty-case test runs with keypoint_threshold=0.5).

    python tools/make_superglue_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.noise_floor import perturbed                                                   # noqa: E402
from sam_pt_amd.weights import init_superglue_state_dict, init_superpoint_state_dict       # noqa: E402
from tests import superglue_ref as R                                                       # noqa: E402

SEEDS = range(5)


def stages(sp_sd, sg_sd, frames, kpts, dtype):
    """The pipeline in ``dtype`` with every stage fed the given (f32 run's) keypoints -> dense maps, descriptors, GNN outputs, Z,
    matching scores."""
    cfg = R.GOLDEN_CONFIG
    grey = R.grey_frames(frames, dtype)
    sp = [R.superpoint(sp_sd, grey[t], cfg["superpoint"]) for t in range(frames.shape[0])]
    dense = torch.stack([s["dense"] for s in sp])
    desc = [R.sample_descriptors(sp[t]["dmap"], kpts[t].to(dtype)) for t in range(len(sp))]
    ksc = [sp[t]["dense"][kpts[t][:, 1].long(), kpts[t][:, 0].long()] for t in range(len(sp))]
    pairs = [R.superglue(sg_sd, kpts[0].to(dtype), ksc[0], desc[0], kpts[t].to(dtype), ksc[t], desc[t], R.GOLDEN_H, R.GOLDEN_W,
                         cfg["superglue"]) for t in range(1, len(sp))]
    return dense, desc, pairs


def dev(a, b):
    return float((a.double() - b.double()).abs().max())


def main(clip_seed=R.GOLDEN_SEED):
    sp_sd, sg_sd = init_superpoint_state_dict(R.GOLDEN_WEIGHT_SEED), init_superglue_state_dict(R.GOLDEN_WEIGHT_SEED)
    frames, masks, q = R.golden_clip(clip_seed)
    cfg = R.GOLDEN_CONFIG
    thr = cfg["superglue"]["match_threshold"]

    # ---- the live reference, and the restatement against it
    trk = R.reference_tracker(sp_sd, sg_sd)
    trk.set_masks(masks)
    np.random.seed(R.GOLDEN_NP_SEED)
    with torch.no_grad():
        ref_traj, ref_vis = trk.forward(frames[None], q)
    np.random.seed(R.GOLDEN_NP_SEED)
    traj, vis, sp, pairs = R.track(sp_sd, sg_sd, frames, masks, q, detail=True)
    assert torch.equal(traj, ref_traj) and torch.equal(vis, ref_vis), "restatement != live reference"
    with torch.no_grad():
        grey = R.grey_frames(frames)
        for t in (1, 2):
            pred = trk.matching({"image0": grey[0][None, None], "image1": grey[t][None, None]})
            assert torch.equal(pred["keypoints0"][0], sp[0]["keypoints"]) and torch.equal(pred["keypoints1"][0], sp[t]["keypoints"])
            assert torch.equal(pred["matches0"][0].int(), pairs[t - 1]["matches0"])
            assert dev(pred["matching_scores0"][0], pairs[t - 1]["matching_scores0"]) <= 1e-6
            assert dev(pred["descriptors1"][0], sp[t]["descriptors"]) <= 1e-6
    kpts = [s["keypoints"] for s in sp]
    counts = [len(k) for k in kpts]
    print("keypoints per frame:", counts, "largest score", float(max(s["dense"].max() for s in sp)))
    assert all(100 <= c <= 300 and c % 64 for c in counts) and len(set(counts)) == 3, "keypoint counts: ragged and unequal"
    assert max(float(s["dense"].max()) for s in sp) < 0.45, "the empty-case test sets keypoint_threshold=0.5"
    for t in range(3):                                      # the threshold and the border removal both take keypoints away
        s = R.nms(sp[t]["dense"], cfg["superpoint"]["nms_radius"])
        assert int((s > 0).sum()) > int((s > cfg["superpoint"]["keypoint_threshold"]).sum()) > counts[t]

    # ---- noise floors and bars
    with torch.no_grad():
        d32, e32, p32 = stages(sp_sd, sg_sd, frames, kpts, torch.float32)
        d64, e64, p64 = stages(sp_sd, sg_sd, frames, kpts, torch.float64)
        dpt, ept, ppt = stages(perturbed(sp_sd, 1e-7), perturbed(sg_sd, 1e-7), frames, kpts, torch.float32)
    assert all(torch.equal(e32[t], sp[t]["descriptors"]) for t in range(3))
    noise = {}
    for name, get in (("scores", lambda d, e, p: [d]), ("desc", lambda d, e, p: e),
                      ("gnn", lambda d, e, p: [x for r in p for x in (r["gnn0"], r["gnn1"])]),
                      ("sinkhorn", lambda d, e, p: [r["Z"] for r in p]),
                      ("mscores", lambda d, e, p: [r["matching_scores0"] for r in p])):
        a, b, c = get(d32, e32, p32), get(d64, e64, p64), get(dpt, ept, ppt)
        n64, npt = max(dev(x, y) for x, y in zip(a, b)), max(dev(x, y) for x, y in zip(a, c))
        noise[name] = (n64, npt)
        print(f"noise {name}: f32 vs f64 {n64:.3e}, f32 vs 1e-7 perturbed weights {npt:.3e} -> bar = 8 x {max(n64, npt):.3e}")
    bar = {k: 8 * max(v) for k, v in noise.items()}

    # ---- (a) keypoint sets under +- bar_scores, and in float64
    sc = cfg["superpoint"]
    for t in range(3):
        variants = [d64[t]] + [d32[t].double() + bar["scores"] * (2 * torch.rand(d32[t].shape, dtype=torch.float64,
                                                                               generator=torch.Generator().manual_seed(s)) - 1)
                               for s in SEEDS]
        for v in variants:
            k, _ = R.keypoints_from_scores(v, sc["nms_radius"], sc["keypoint_threshold"], sc["remove_borders"])
            assert torch.equal(k.float(), kpts[t]), f"(a) frame {t}: the keypoint set moves within bar_scores"

    # ---- (b) matches under +- bar_sinkhorn, marginal keypoints
    marginal = []
    for p, r in enumerate(pairs):
        Z = r["Z"].double()
        inner = Z[:-1, :-1]
        top_r = inner.topk(min(2, inner.shape[1]), dim=1).values
        top_c = inner.topk(min(2, inner.shape[0]), dim=0).values
        gap_r = top_r[:, 0] - top_r[:, 1]
        gap_c = (top_c[0] - top_c[1])[inner.argmax(1)]
        ms = r["matching_scores0"].double()
        mutual = ms > 0
        marg = (gap_r < bar["sinkhorn"]) | (gap_c < bar["sinkhorn"]) | (mutual & ((ms - thr).abs() < bar["mscores"]))
        idx = torch.nonzero(marg)[:, 0]
        assert len(idx) <= 0.02 * len(ms), f"(b) pair {p}: {len(idx)} marginal keypoints of {len(ms)}"
        keep = ~marg
        for v in [p64[p]["Z"]] + [Z + bar["sinkhorn"] * (2 * torch.rand(Z.shape, dtype=torch.float64,
                                                                       generator=torch.Generator().manual_seed(s)) - 1) for s in SEEDS]:
            m, _ = R.matches_from_transport(v, thr)
            assert torch.equal(m[keep], r["matches0"][keep]), f"(b) pair {p}: matches move within bar_sinkhorn outside the marginal set"
        marginal.append(idx.numpy().astype(np.int32))
        # ---- (c)
        valid = int((r["matches0"] > -1).sum())
        print(f"pair {p}: {valid} matches, {len(ms) - valid} unmatched, {int((~mutual).sum())} mutual-check failures, "
              f"{int((mutual & (ms <= thr)).sum())} mutual below the threshold, {len(idx)} marginal")
        assert valid >= 10 and len(ms) - valid >= 10, "(c)"
        assert int((~mutual).sum()) > 0 and int((mutual & (ms <= thr)).sum()) > 0

    # ---- (d) more and fewer candidates than requested, positives and negatives
    more, fewer = [False, False], [False, False]
    for p, r in enumerate(pairs):
        valid = (r["matches0"] > -1)
        mk1 = kpts[p + 1][r["matches0"][valid].long()]
        for mi in range(masks.shape[0]):
            inside = masks[mi][mk1[:, 1].long(), mk1[:, 0].long()] > 0.5
            for w, (have, want) in enumerate(((int(inside.sum()), R.GOLDEN_POS), (int((~inside).sum()), R.GOLDEN_NEG))):
                more[w] |= have > want
                fewer[w] |= have < want
    assert all(more) and all(fewer), f"(d) more {more} fewer {fewer}"
    assert bool((vis[0, 1:] == 0).any()) and bool((vis[0, 1:] == 1).any())

    dense_rows = np.arange(0, d32.shape[1], 3)
    out = dict(frames=frames.numpy(), masks=masks.numpy(), query_points=q.numpy(), np_seed=np.int64(R.GOLDEN_NP_SEED),
               trajectories=ref_traj.numpy(), visibilities=ref_vis.numpy(), counts=np.asarray(counts, dtype=np.int32),
               dense_rows=dense_rows.astype(np.int32), dense=d32[:, dense_rows].numpy())
    for t in range(3):
        cols = np.arange(0, counts[t], 4)
        out[f"kpts{t}"], out[f"kscores{t}"] = kpts[t].numpy(), sp[t]["scores"].numpy()
        out[f"desc_cols{t}"], out[f"desc{t}"] = cols.astype(np.int32), sp[t]["descriptors"][:, cols].numpy()
    for p, r in enumerate(pairs):
        g = torch.cat([r["gnn0"], r["gnn1"]], 1)
        cols = np.arange(0, g.shape[1], 4)
        rows = np.arange(0, r["Z"].shape[0], 4)
        out[f"gnn_cols{p}"], out[f"gnn{p}"] = cols.astype(np.int32), g[:, cols].numpy()
        out[f"z_rows{p}"], out[f"Z{p}"] = rows.astype(np.int32), r["Z"][rows].numpy()
        out[f"matches{p}"], out[f"mscores{p}"], out[f"marginal{p}"] = r["matches0"].numpy(), r["matching_scores0"].numpy(), marginal[p]
    for k, (n64, npt) in noise.items():
        out[f"noise_{k}_f64"], out[f"noise_{k}_perturbed"], out[f"bar_{k}"] = np.float64(n64), np.float64(npt), np.float64(bar[k])
    np.savez_compressed(R.GOLDEN, **out)
    print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    # ``--search`` tries clip seeds until the assertions hold and prints the first that does (then set GOLDEN_SEED to it)
    if "--search" in sys.argv:
        for seed in range(72, 172):
            try:
                main(seed)
            except AssertionError as e:
                print(f"clip seed {seed}: {e}")
                continue
            print(f"clip seed {seed} passes")
            break
    else:
        main()
