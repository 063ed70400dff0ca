"""CPU side of the YouTube-VIS AP / AR evaluation (no GPU needed): the host restatement of sam_pt_amd/vis_metrics.py against the
golden file the REFERENCE's evaluator wrote (tests/golden/vis_eval_ref.npz, tools/make_vis_eval_golden.py) and, where the reference
tree is present, against that evaluator run live (tests/ytvis_ref.py) — every comparison is ``==`` — plus hand cases for each rule
of the matching, the corners of ``accumulate``, the host pixel primitives, and the C ABI surface with its refusals."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from sam_pt_amd import vis_metrics as VM
from sam_pt_amd.automatic_mask_generator import mask_to_rle, rle_to_mask
from tests import ytvis_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_bits_pack", "sampt_rle_decode_workspace_bytes", "sampt_rle_decode_bits", "sampt_bits_unpack",
               "sampt_seq_iou_workspace_bytes", "sampt_seq_iou_counts", "sampt_vis_match")
THR10 = np.linspace(0.5, 0.95, 10)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(Y.GOLDEN))                                        # (shared by the tests, never written to)


def run_ours(dataset, results, **kw):
    ev = VM.YTVISEval(dataset, params=Y.golden_params(), **kw)
    ev.add_results(results)
    ev.evaluate(), ev.accumulate(), ev.summarize()
    return ev


# ------------------------------------------------------------------------------------------------ pinned on the reference
def test_golden_set_meets_its_conditions():
    g = golden()
    stats, gmeta, dmeta, sc = g["stats"], g["in_gt_meta"], g["in_dt_meta"], g["in_dt_score"]
    assert stats.shape == (12,) and (stats >= 0).all() and 0 < stats[0] < 1
    assert set(gmeta[:, 2].tolist()) == {1, 2}                            # two categories
    assert gmeta[:, 3].any()                                              # a crowd
    assert (~g["in_gt_present"]).any()                                    # an annotation with a None frame
    _, d = Y.masks_of(g)
    assert (d.reshape(len(d), -1).sum(axis=1) == 0).any()                 # a detection that is empty on every frame
    gv, dv = set(gmeta[:, 1].tolist()), set(dmeta[:, 0].tolist())
    assert dv - gv and gv - dv                                            # detections without ground truth, and the reverse
    groups = [sc[(dmeta[:, 0] == v) & (dmeta[:, 1] == c)] for v in dv for c in (1, 2)]
    assert any(len(set(s.tolist())) < len(s) for s in groups)             # a score tie inside a group
    assert any(np.isin(g[k], THR10).any() for k in g if k.startswith("ious_"))       # an IoU that equals a threshold
    assert any((g[k] == 11 / 20).any() for k in g if k.startswith("ious_"))
    assert (g["precision"] > -1).all()                                    # precision defined everywhere


def test_host_restatement_equals_the_golden():
    g = golden()
    ev = run_ours(*Y.dataset_of(g))
    Y.assert_same(Y.our_arrays(ev), g)
    res = ev.results()
    assert list(res) == list(VM.METRICS) and [res[k] for k in VM.METRICS] == (g["stats"] * 100).tolist()


def test_masks_logits_and_process_equal_the_golden_on_the_host():
    g = golden()
    dataset, _ = Y.dataset_of(g)
    _, dm = Y.masks_of(g)
    for key, use_logits in (("pred_masks", False), ("pred_logits", True)):
        ev = VM.YTVISEval(dataset, params=Y.golden_params())
        for v in sorted(ev.videos):
            idx = np.flatnonzero(g["in_dt_meta"][:, 0] == v)
            data = torch.from_numpy(dm[idx])
            data = [m for m in data] if key == "pred_masks" else torch.where(data, 1.5, -0.5).float()
            ev.process([{"video_id": v}], {"pred_scores": g["in_dt_score"][idx].tolist(),
                                           "pred_labels": g["in_dt_meta"][idx, 1].tolist(), key: data}, use_logits=use_logits)
        ev.evaluate(), ev.accumulate(), ev.summarize()
        keys = [k for k in g if k in ("precision", "recall", "stats") or k.startswith("ious_") or k.endswith(("Matches", "Ignore"))]
        got = Y.our_arrays(ev)
        # detection ids follow the order of arrival (per video here, one list in the golden): gtMatches holds them
        Y.assert_same(got, g, [k for k in keys if not k.endswith("gtMatches")])
        for k in keys:
            if k.endswith("gtMatches"):
                assert np.array_equal(got[k] > 0, g[k] > 0)


def test_evaluate_ytvis_with_default_params_runs_and_refuses_bad_input():
    g = golden()
    dataset, results = Y.dataset_of(g)
    res = VM.evaluate_ytvis(dataset, results, params=Y.golden_params())
    assert [res[k] for k in VM.METRICS] == (g["stats"] * 100).tolist()
    res = VM.evaluate_ytvis(dataset, results)                             # the default ranges: nothing here is medium or large
    assert np.isnan(res["APm"]) and np.isnan(res["ARl"]) and res["AP"] == res["APs"] > 0
    bad = {**dataset, "annotations": [{**dataset["annotations"][0], "id": 0}]}
    with pytest.raises(ValueError, match="ids must be integers >= 1"):
        VM.YTVISEval(bad)
    poly = {**dataset, "annotations": [{**dataset["annotations"][0], "segmentations": [[[1, 1, 5, 1, 5, 5]]] * 5}]}
    with pytest.raises(ValueError, match="polygon"):
        VM.YTVISEval(poly)
    short = [{**results[0], "segmentations": [{"size": [40, 70], "counts": [10, 5]}] * 5}]
    with pytest.raises(ValueError, match="does not cover"):
        VM.evaluate_ytvis(dataset, short)


@pytest.mark.skipif(not Y.available(), reason="the reference tree is absent")
@pytest.mark.parametrize("seed", (None, 3), ids=("golden_inputs", "seed3"))
def test_host_restatement_equals_the_live_reference(seed):
    arr = golden() if seed is None else Y.seeded_arrays(seed)
    dataset, results = Y.dataset_of(arr)
    ref = Y.reference_arrays(Y.run_reference(dataset, results))
    if seed is None:
        Y.assert_same(ref, {k: v for k, v in golden().items() if k != "seed"})          # the golden is what the reference gives today
    Y.assert_same(Y.our_arrays(run_ours(dataset, results)), ref)


# ------------------------------------------------------------------------------------------------------------ hand cases
def C(*pairs):
    """counts (D, G, 2) from rows of (inter, union) pairs."""
    return np.array(pairs, dtype=np.int64)


# name -> (counts, gt_ignore (ranges, G), iscrowd, dt_out (ranges, D), thrs, expected dt_match, gt_match, dt_ignore, gt_order)
HAND_CASES = {
    # two ground truths with the same IoU: the later one wins (a candidate must not be BELOW the best so far)
    "last_of_equals": (C([(1, 2), (1, 2)]), [[0, 0]], [0, 0], [[0]], [0.5], [[[2]]], [[[0, 1]]], [[[0]]], [[0, 1]]),
    # a crowd is matched by both detections; it keeps the last one, and both detections are ignored
    "crowd_rematch": (C([(4, 5)], [(4, 5)]), [[1]], [1], [[0, 0]], [0.5], [[[1, 1]]], [[[2]]], [[[1, 1]]], [[0]]),
    # without the crowd flag the second detection stays unmatched (ignored ground truth, no crowd)
    "no_rematch": (C([(4, 5)], [(4, 5)]), [[1]], [0], [[0, 0]], [0.5], [[[1, 0]]], [[[1]]], [[[1, 0]]], [[0]]),
    # a regular match exists when the ignored ground truths begin: the better ignored one is never looked at
    "ignore_break": (C([(6, 10), (9, 10)]), [[0, 1]], [0, 1], [[0]], [0.5], [[[1]]], [[[1, 0]]], [[[0]]], [[0, 1]]),
    # no regular match: the ignored one is taken and the detection is ignored with it
    "ignore_taken": (C([(4, 10), (9, 10)]), [[0, 1]], [0, 1], [[0]], [0.5], [[[2]]], [[[0, 1]]], [[[1]]], [[0, 1]]),
    # the ignored ground truth comes first in the group: the stable sort moves it behind the regular ones
    "ignore_sorted_last": (C([(9, 10), (6, 10), (2, 10)]), [[1, 0, 0]], [1, 0, 0], [[0]], [0.5], [[[2]]], [[[1, 0, 0]]], [[[0]]],
                           [[1, 2, 0]]),
    # unmatched detections are ignored iff outside the area range; a matched one takes its ground truth's flag
    "area_range": (C([(9, 10)], [(1, 10)], [(0, 10)]), [[0], [0]], [0], [[1, 1, 0], [0, 0, 0]], [0.5], [[[1, 0, 0]], [[1, 0, 0]]],
                   [[[1]], [[1]]], [[[0, 1, 0]], [[0, 0, 0]]], [[0], [0]]),
    # IoU == threshold matches (11 / 20 against linspace's 0.55); IoU 1 matches at threshold 1 through the start value 1 - 1e-10;
    # an empty union is IoU 0
    "thresholds": (C([(11, 20), (0, 0)], [(7, 7), (0, 0)]), [[0, 0]], [0, 0], [[0, 0]], [THR10[1], THR10[2], 1.0],
                   [[[1, 0], [0, 1], [0, 1]]], [[[1, 0], [2, 0], [2, 0]]], [[[0, 0], [0, 0], [0, 0]]], [[0, 1]]),
    # a matched regular ground truth is passed over by the next detection, which takes the second best
    "taken": (C([(9, 10), (8, 10)], [(9, 10), (7, 10)]), [[0, 0]], [0, 0], [[0, 0]], [0.5, 0.75], [[[1, 2], [1, 0]]], [[[1, 2], [1, 0]]],
              [[[0, 0], [0, 0]]], [[0, 1]]),
}


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_matching_rules_by_hand(name):
    counts, g_ig, crowd, d_out, thrs, dtm, gtm, dtig, order = HAND_CASES[name]
    m = VM.match_video(counts, g_ig, crowd, d_out, thrs)
    assert m["dt_match"].tolist() == dtm and m["gt_match"].tolist() == gtm
    assert m["dt_ignore"].astype(int).tolist() == dtig and m["gt_order"].tolist() == order


def disc_rle(cy, cx, r, h=20, w=30, T=2):
    y, x = np.mgrid[:h, :w]
    m = torch.from_numpy((y - cy) ** 2 + (x - cx) ** 2 <= r * r)
    rec = mask_to_rle(m[None])[0]
    return [dict(rec) for _ in range(T)]


def test_max_dets_cut_and_empty_sides():
    p = VM.Params()
    p.maxDets, p.areaRng = [1, 2, 3], [[0, 1e10], [0, 10], [10, 50], [50, 1e10]]
    ev = VM.YTVISEval(params=p, categories=[1, 2, 3])
    scores = [0.3, 0.9, 0.5, 0.9, 0.1]
    ev.add_video({"id": 7, "height": 20, "width": 30},
                 [{"id": 4, "category_id": 1, "iscrowd": 0, "segmentations": disc_rle(10, 10, 4), "areas": [49, 49]},
                  {"id": 5, "category_id": 2, "iscrowd": 0, "segmentations": disc_rle(10, 10, 4), "areas": [49, 49]}],
                 [{"score": s, "category_id": 1, "segmentations": disc_rle(10, 10 + i, 4)} for i, s in enumerate(scores)] +
                 [{"score": 0.4, "category_id": 3, "segmentations": disc_rle(5, 5, 1)}])
    imgs = ev.evaluate()
    assert len(imgs) == 3 * 4 * 1 and ev.catIds == [1, 2, 3]
    e = imgs[0]                                                           # category 1, all areas: the 3 best of 5, ties in input order
    assert e["dtIds"] == [2, 4, 3] and e["dtScores"] == [0.9, 0.9, 0.5] and e["maxDet"] == 3
    assert e["dtMatches"].shape == (10, 3) and ev.ious[7, 1].shape == (3, 1)
    assert e["dtMatches"][0].tolist() == [4.0, 0.0, 0.0] and e["gtMatches"][0].tolist() == [2.0]
    e = imgs[4]                                                           # category 2: a ground truth and no detection — "empty" IoUs
    assert ev.ious[7, 2] == [] and e["dtMatches"].shape == (10, 0) and e["gtMatches"].tolist() == [[0.0]] * 10
    assert e["dtIgnore"].shape == (10, 0) and e["gtIgnore"].tolist() == [0] and e["gtIds"] == [5]
    for a, out in enumerate((False, False, True, True)):                  # category 3: a detection (5 pixels) and no ground truth
        e = imgs[8 + a]
        assert ev.ious[7, 3].shape == (1, 0) and e["dtMatches"].tolist() == [[0.0]] * 10 and e["gtMatches"].shape == (10, 0)
        assert e["dtIgnore"].tolist() == [[out]] * 10 and e["dtIds"] == [6]
    ev2 = VM.YTVISEval(params=p)
    ev2.add_video({"id": 1, "height": 20, "width": 30}, [], [])
    assert ev2.evaluate() == []                                           # no category at all
    ev.accumulate(), ev.summarize()
    assert ev.eval["precision"].shape == (10, 101, 3, 4, 3) and (ev.eval["precision"][:, :, 2] == -1).all()
    assert np.isnan(ev.results()["APs"]) and ev.results()["APm"] >= 0


def test_accumulate_when_recall_stops_short_and_without_regular_ground_truth():
    p = VM.Params()
    p.iouThrs, p.maxDets = np.array([0.5]), [1, 10, 100]
    img = {"dtMatches": np.array([[4.0, 0.0]]), "dtIgnore": np.array([[False, False]]), "dtScores": [0.8, 0.6], "gtIgnore": np.array([0, 0])}
    ev = VM.accumulate([img, None, None, None, None, None, None, None], p, n_cats=1, n_vids=2)
    one = 1.0 / (1.0 + np.spacing(1))
    assert ev["recall"][0, 0, 0].tolist() == [0.5, 0.5, 0.5] and (ev["recall"][0, 0, 1:] == -1).all()
    pr, sc = ev["precision"][0, :, 0, 0, 2], ev["scores"][0, :, 0, 0, 2]
    assert (pr[:51] == one).all() and (pr[51:] == 0).all()                # recall thresholds above 0.5 are never reached: left at 0
    assert (sc[:51] == 0.8).all() and (sc[51:] == 0).all()
    assert (ev["precision"][:, :, :, 1:] == -1).all()                     # no group at all in the other ranges
    ig = {**img, "gtIgnore": np.array([1, 1])}
    ev = VM.accumulate([ig, None], p, n_cats=1, n_vids=2)["precision"]
    assert (ev == -1).all()                                               # no regular ground truth: the setting is skipped
    none = {"dtMatches": np.zeros((1, 0)), "dtIgnore": np.zeros((1, 0), dtype=bool), "dtScores": [], "gtIgnore": np.array([0])}
    ev = VM.accumulate([none], p, n_cats=1, n_vids=1)
    assert (ev["recall"][0, 0, 0] == 0).all() and (ev["precision"][0, :, 0, 0] == 0).all()
    s = VM.summarize({"precision": -np.ones((1, 101, 1, 4, 3)), "recall": -np.ones((1, 1, 4, 3))}, p)
    assert (s == -1).all()


# ----------------------------------------------------------------------------------------------- host pixel primitives
def test_pack_decode_and_sequence_counts_on_the_host():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (63, 5), (64, 4), (65, 7), (130, 3)):
        m = rng.random((3, h, w)) < 0.4
        bits, area = VM.bits_pack(m)
        nb = (h + 63) // 64
        assert bits.dtype == np.uint64 and bits.shape == (3, nb, w) and area.tolist() == m.sum(axis=(1, 2)).tolist()
        for j in (0, h - 1):                                              # bit j of band b is row 64 b + j
            assert np.array_equal((bits[:, j // 64, :] >> np.uint64(j % 64)) & np.uint64(1), m[:, j, :].astype(np.uint64))
        if h % 64:
            assert not (bits[:, -1, :] >> np.uint64(h % 64)).any()        # rows >= h are 0
        assert np.array_equal(VM.unpack_bits(bits, h), m)
        recs = mask_to_rle(torch.from_numpy(m))
        dbits, darea, status = VM.rle_decode([r["counts"] for r in recs], h, w)
        assert np.array_equal(dbits, bits) and darea.tolist() == area.tolist() and not status.any()
        assert all(np.array_equal(rle_to_mask(r), m[i]) for i, r in enumerate(recs))
    f = np.array([[[0.5, np.nan, 0.25, 0.2500001]]], dtype=np.float32)
    assert VM.bits_pack(f, threshold=0.25)[0].reshape(-1).tolist() == [1, 0, 0, 1]
    idx = np.array([[[1, 2], [2, 0]]], dtype=np.uint8)
    b, a = VM.bits_pack(idx, values=[2, 1, 7], planes=[0, 0, 0])
    assert b.reshape(3, 2).tolist() == [[2, 1], [1, 0], [0, 0]] and a.tolist() == [2, 1, 0]
    bits, area, status = VM.rle_decode([[6], [0, 6], [5], [7], [2, 0, 0, 3, 1], []], 2, 3)
    assert status.tolist() == [0, 0, 1, 1, 0, 1] and area.tolist() == [0, 6, 0, 0, 3, 0]
    assert bits.reshape(6, 3).tolist() == [[0, 0, 0], [3, 3, 3], [0, 0, 0], [0, 0, 0], [0, 3, 1], [0, 0, 0]]
    # sequence counts against the definition, absent frames on either side and on both, shared planes
    dm, gm = rng.random((5, 9, 11)) < 0.5, rng.random((4, 9, 11)) < 0.5
    dp, gp = np.array([[0, 1, -1], [2, 2, 2], [-1, -1, -1], [4, -1, 3]]), np.array([[0, -1, 1], [-1, -1, 3], [2, 2, -1]])
    c = VM.seq_iou_counts(dm, dp, gm, gp)
    for d in range(4):
        for g in range(3):
            i = u = 0
            for t in range(3):
                a = dm[dp[d, t]] if dp[d, t] >= 0 else None
                b = gm[gp[g, t]] if gp[g, t] >= 0 else None
                if a is not None and b is not None:
                    i, u = i + (a & b).sum(), u + (a | b).sum()
                elif a is not None or b is not None:
                    u += (a if a is not None else b).sum()
            assert c[d, g].tolist() == [i, u]
    assert VM.seq_iou(C([(11, 20), (0, 0)]))[0].tolist() == [11 / 20, 0.0]
    assert VM.seq_iou_counts(dm, np.zeros((0, 3), dtype=int), gm, gp).shape == (0, 3, 2)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_declares_binds_and_exports_the_vis_eval_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
    for name in ("sampt_bits_pack", "sampt_rle_decode_bits", "sampt_bits_unpack", "sampt_seq_iou_counts", "sampt_vis_match"):
        res, args = _lib._SIGS[name]                                      # house style: int return code, stream last
        assert res is _lib.c_int and args[-1] is _lib._P
    for name in ("sampt_rle_decode_bits", "sampt_seq_iou_counts"):        # workspace and its size before the stream
        args = _lib._SIGS[name][1]
        assert args[-2] is _lib.c_size_t and args[-3] is _lib._P
    assert "vis_eval.hip" in open(os.path.join(ROOT, "sam_pt_amd", "csrc", "Makefile")).read()


def test_abi_refuses_bad_arguments_without_touching_memory():
    from sam_pt_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    fake = P(1 << 20)                                                     # never dereferenced: every call below is refused first
    assert lib.sampt_seq_iou_workspace_bytes(0, 1, 1, 8, 8) == 0 and lib.sampt_seq_iou_workspace_bytes(1, 1, 1, 46341, 46341) == 0
    ws = lib.sampt_seq_iou_workspace_bytes(100, 20, 36, 480, 854)
    assert 0 < ws <= 1024 * 32 * 32 * 8 and ws % (128 * 32 * 8) == 0      # whole tiles of 32 x 32 pairs, at most 1024 workgroups
    assert lib.sampt_rle_decode_workspace_bytes(10) >= 80 and lib.sampt_rle_decode_workspace_bytes(-1) == 0
    assert lib.sampt_bits_pack(fake, 3, 0.0, None, None, 1, 8, 8, fake, fake, None) == -1          # unknown kind
    assert lib.sampt_bits_pack(fake, 0, 0.0, None, None, 1, 0, 8, fake, fake, None) == -1          # bad shape
    assert lib.sampt_bits_pack(fake, 0, 0.0, None, None, 1, 46341, 46341, fake, fake, None) == -1  # h * w >= 2^31
    assert lib.sampt_bits_pack(fake, 2, 0.0, None, None, 1, 8, 8, fake, fake, None) == -1          # an index map without values
    assert lib.sampt_bits_pack(None, 0, 0.0, None, None, 1, 8, 8, fake, fake, None) == -1
    assert lib.sampt_bits_pack(P((1 << 20) + 2), 1, 0.0, None, None, 1, 8, 8, fake, fake, None) == -1   # f32 at an odd address
    assert lib.sampt_bits_pack(None, 0, 0.0, None, None, 0, 8, 8, None, None, None) == 0           # n = 0: nothing to do
    assert lib.sampt_rle_decode_bits(fake, fake, 1, 4, 8, 8, fake, fake, fake, fake, 8, None) == -4     # workspace too small
    assert lib.sampt_rle_decode_bits(fake, fake, 1, -1, 8, 8, fake, fake, fake, fake, 1 << 20, None) == -1
    assert lib.sampt_rle_decode_bits(fake, None, 1, 4, 8, 8, fake, fake, fake, fake, 1 << 20, None) == -1
    assert lib.sampt_bits_unpack(None, 1, 8, 8, fake, None) == -1
    args = (fake, fake, fake, 2, 4, fake, fake, fake, 2, 4, 3, 8, 8, fake, fake)
    assert lib.sampt_seq_iou_counts(*args, 8, None) == -4
    assert b"workspace" in lib.sampt_last_error()
    assert lib.sampt_seq_iou_counts(fake, fake, fake, 0, 4, fake, fake, fake, 2, 4, 3, 8, 8, fake, fake, 1 << 20, None) == -1
    assert lib.sampt_seq_iou_counts(fake, fake, None, 2, 4, fake, fake, fake, 2, 4, 3, 8, 8, fake, fake, 1 << 20, None) == -1
    for D, G, A, n in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 961, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 65)):
        assert lib.sampt_vis_match(fake, D, G, A, n, fake, fake, fake, fake, fake, fake, fake, fake, None) == -1
    assert lib.sampt_vis_match(None, 1, 1, 1, 1, fake, fake, fake, fake, fake, fake, fake, fake, None) == -1


def test_device_functions_refuse_the_host():
    from sam_pt_amd import _lib
    with pytest.raises(_lib.SamptError, match="HIP device only"):
        VM.bits_pack_device(torch.zeros(1, 4, 4, dtype=torch.bool))
    with pytest.raises(_lib.SamptError, match="HIP device only"):
        VM.rle_decode_device([[16]], 4, 4, "cpu")
    with pytest.raises(_lib.SamptError, match="HIP device only"):
        VM.match_video_device(torch.zeros(1, 1, 2, dtype=torch.int64), [[0]], [0], [[0]], [0.5])
