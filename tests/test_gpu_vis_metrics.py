"""YouTube-VIS AP / AR on the device (csrc/vis_eval.hip) against the host twins of sam_pt_amd/vis_metrics.py computed live, and end to
end against the golden file the reference's evaluator wrote (tests/golden/vis_eval_ref.npz; the reference tree itself is never read
here).  The device does integer work and one correctly rounded float64 division per IoU, so every comparison is ``==``."""
import functools

import numpy as np
import pytest
import torch

from sam_pt_amd import vis_metrics as VM
from sam_pt_amd.automatic_mask_generator import rle_encode_device, rle_to_mask
from tests import ytvis_ref as Y
from tests.test_vis_metrics_cpu import HAND_CASES, golden

pytestmark = pytest.mark.gpu

HS, WS = (1, 63, 64, 65, 130), (1, 3, 4, 5, 255, 256, 257)


def words(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def shape_masks(h, w, n=3):
    rng = np.random.default_rng(1000 * h + w)                             # (shared by the tests below, never written to)
    m = rng.random((n, h, w)) < 0.45
    m[0, -1, :] = True                                                    # the last row and the last column are exercised
    m[1, :, -1] = True
    return m


def odd_slice(x: np.ndarray, dev) -> torch.Tensor:
    """The stack as a view that starts one element into its buffer: a base address that is odd (bytes) or not 16-byte aligned (f32)."""
    buf = torch.zeros(x.size + 1, dtype=torch.from_numpy(x[:0].copy()).dtype, device=dev)
    buf[1:] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1).to(dev)
    return buf[1:].view(x.shape)


# ------------------------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("h", HS)
def test_pack_shapes_and_kinds(dev, h, w):
    m = shape_masks(h, w)
    nb = (h + 63) // 64
    pad = np.zeros((3, nb * 64, w), dtype=bool)
    pad[:, :h] = m
    exp = np.packbits(pad.reshape(3, nb, 64, w).transpose(0, 1, 3, 2), axis=-1, bitorder="little").view("<u8").reshape(3, nb, w)
    area = m.sum(axis=(1, 2))
    rng = np.random.default_rng(h * 7 + w)
    f = np.where(m, 0.25 + rng.random(m.shape), 0.25 - rng.random(m.shape)).astype(np.float32)
    off = np.argwhere(~m)
    if len(off) >= 2:
        f[tuple(off[0])], f[tuple(off[1])] = np.nan, 0.25                 # NaN and x == thr are clear
    idx = np.where(m[0], 3, np.where(m[1], 9, 0)).astype(np.uint8)[None]  # an index map: item 0 is value 3, item 1 value 9, item 2 value 200
    idx_exp, idx_area = VM.bits_pack(idx, values=[3, 9, 200], planes=[0, 0, 0])
    for aligned in (True, False):
        put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if aligned else (lambda a: odd_slice(a, dev))
        for x, kw in ((m, {}), (m.astype(np.uint8) * 7, {}), (f, {"threshold": 0.25})):
            bits, a = VM.bits_pack_device(put(x), **kw)
            assert bits.dtype == torch.int64 and tuple(bits.shape) == (3, nb, w) and a.dtype == torch.int32
            assert np.array_equal(words(bits), exp) and a.cpu().tolist() == area.tolist()
            hb, ha = VM.bits_pack(x, **kw)
            assert np.array_equal(words(bits), hb) and a.cpu().tolist() == ha.tolist()
        bits, a = VM.bits_pack_device(put(idx), values=[3, 9, 200], planes=[0, 0, 0])
        assert np.array_equal(words(bits), idx_exp) and a.cpu().tolist() == idx_area.tolist()
    if h % 64:
        assert not (exp[:, -1, :] >> np.uint64(h % 64)).any()             # the bits of rows >= h are 0


def test_pack_nothing(dev):
    bits, a = VM.bits_pack_device(torch.zeros((0, 65, 5), dtype=torch.bool, device=dev))
    assert tuple(bits.shape) == (0, 2, 5) and tuple(a.shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("h", HS)
def test_decode_round_trip(dev, h, w):
    m = shape_masks(h, w)
    x = torch.from_numpy(m).to(dev)
    recs, areas = rle_encode_device(x)
    bits, area, status, by = VM.rle_decode_device([r["counts"] for r in recs], h, w, dev, as_bytes=True)
    pb, pa = VM.bits_pack_device(x)
    assert torch.equal(bits, pb) and torch.equal(area, pa) and area.cpu().tolist() == areas.cpu().tolist()
    assert not status.any().item()
    assert by.dtype == torch.uint8 and np.array_equal(by.cpu().numpy(), np.stack([rle_to_mask(r) for r in recs]).astype(np.uint8))
    hb, ha, hs = VM.rle_decode([r["counts"] for r in recs], h, w)
    assert np.array_equal(words(bits), hb) and area.cpu().tolist() == ha.tolist()


@pytest.mark.parametrize("shape", ((130, 5), (65, 257), (300, 300)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_special_runs_and_bad_masks(dev, shape):
    h, w = shape
    hw = h * w
    rng = np.random.default_rng(hw)
    cuts = np.sort(rng.choice(np.arange(1, hw), size=min(40, hw - 1), replace=False))
    seeded = np.diff(np.concatenate([[0], cuts, [hw]])).tolist()
    cases = [[hw], [0, hw], [1] * hw, [0] + [1] * (hw - 1) + [1],         # all zero, all one, single-pixel runs from a 0 and from a 1
             [h - 1, 2, hw - h - 1],                                       # a run across a column's end
             [63, 2, hw - 65] if h > 65 else [hw - 2, 2],                  # a run across a band's end
             [0, 3, 0, 0, 5, 0, 0, 0, hw - 8, 0],                          # zero-length runs, also at the end
             [0, 0, 0, hw], seeded, [0] + seeded,
             [hw - 1], [hw - 5, 2],                                        # too short
             [hw + 1], [3, hw], [hw, 0, 1],                                # too long
             [], seeded]                                                   # no run at all; a good neighbour at the end
    if hw > 1 << 17:
        cases.insert(0, [10, 70000, hw - 70010])                          # a run longer than 2^16
    bits, area, status, by = VM.rle_decode_device(cases, h, w, dev, as_bytes=True)
    hb, ha, hs = VM.rle_decode(cases, h, w)
    assert status.cpu().tolist() == hs.tolist() and sum(hs.tolist()) == 6
    assert np.array_equal(words(bits), hb) and area.cpu().tolist() == ha.tolist()
    for i, c in enumerate(cases):
        if hs[i]:
            assert not by[i].any().item() and not bits[i].any().item() and area[i].item() == 0
        else:
            assert np.array_equal(by[i].cpu().numpy().astype(bool), rle_to_mask({"size": [h, w], "counts": c}))


def test_decode_nothing(dev):
    bits, area, status = VM.rle_decode_device([], 65, 5, dev)
    assert tuple(bits.shape) == (0, 2, 5) and tuple(area.shape) == (0,) and tuple(status.shape) == (0,)


# ---------------------------------------------------------------------------------------------------------- sequence IoU
@functools.lru_cache(maxsize=None)
def seq_case(D, G, T, h, w):
    rng = np.random.default_rng(D * 1000 + G * 10 + T + h)
    nd, ng = max(1, D * T - 2), max(1, G * T - 1)                         # fewer planes than entries: some are shared
    dm, gm = rng.random((nd, h, w)) < 0.5, rng.random((ng, h, w)) < 0.3
    dp, gp = rng.integers(0, nd, size=(D, T)), rng.integers(0, ng, size=(G, T))
    if D * T > 1:
        dp[rng.random((D, T)) < 0.2] = -1                                 # absent frames on either side, and (T > 1) on both
        gp[rng.random((G, T)) < 0.2] = -1
        dp[-1, -1] = gp[-1, -1] = -1
        gp[0, 0], dp[0, 0] = -1, 0
    return dm, dp, gm, gp, VM.seq_iou_counts(dm, dp, gm, gp)


@pytest.mark.parametrize("shape", ((65, 257), (130, 5)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dgt", ((1, 1, 1), (7, 5, 3), (33, 33, 2), (100, 20, 3)), ids=lambda s: f"D{s[0]}_G{s[1]}_T{s[2]}")
def test_sequence_counts(dev, dgt, shape):
    h, w = shape
    dm, dp, gm, gp, exp = seq_case(*dgt, h, w)
    db, da = VM.bits_pack_device(torch.from_numpy(dm).to(dev))
    gb, ga = VM.bits_pack_device(torch.from_numpy(gm).to(dev))
    got = VM.seq_iou_counts_device(db, da, dp, gb, ga, gp, h, w)
    assert got.dtype == torch.int64 and tuple(got.shape) == exp.shape
    assert np.array_equal(got.cpu().numpy(), exp), np.argwhere(got.cpu().numpy() != exp)[:3].tolist()
    again = VM.seq_iou_counts_device(db, da, dp, gb, ga, gp, h, w)
    assert torch.equal(got, again)                                        # two runs give identical bits
    assert VM.seq_iou_counts_device(db, da, dp[:0], gb, ga, gp, h, w).shape == (0, dgt[1], 2)


def test_sequence_counts_beyond_int32(dev):
    """40 frames that all name one all-ones plane of 8192 x 8192: inter = union = 40 * 2^26 > 2^31."""
    bits = torch.full((1, 128, 8192), -1, dtype=torch.int64, device=dev)
    area = torch.full((1,), 1 << 26, dtype=torch.int32, device=dev)
    planes = np.zeros((1, 40), dtype=np.int32)
    got = VM.seq_iou_counts_device(bits, area, planes, bits, area, planes, 8192, 8192)
    assert got.cpu().tolist() == [[[40 << 26, 40 << 26]]] and 40 << 26 > 1 << 31


# -------------------------------------------------------------------------------------------------------------- matching
def assert_match(got, exp):
    for k in ("gt_order", "gt_ignore", "dt_match", "gt_match", "dt_ignore"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), k


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_matching_rules_by_hand(dev, name):
    counts, g_ig, crowd, d_out, thrs, dtm, gtm, dtig, order = HAND_CASES[name]
    m = VM.match_video_device(torch.from_numpy(counts).to(dev), g_ig, crowd, d_out, thrs)
    assert m["dt_match"].tolist() == dtm and m["gt_match"].tolist() == gtm
    assert m["dt_ignore"].astype(int).tolist() == dtig and m["gt_order"].tolist() == order
    assert_match(m, VM.match_video(counts, g_ig, crowd, d_out, thrs))


@pytest.mark.parametrize("case", ((100, 33, 10), (100, 33, 64), (17, 5, 10), (1, 1, 1), (3, 64, 64)), ids=lambda c: f"D{c[0]}_G{c[1]}_T{c[2]}")
def test_matching_seeded_groups(dev, case):
    D, G, n = case
    rng = np.random.default_rng(D + G + n)
    union = rng.choice([0, 20, 20, 20, 40, 7], size=(D, G))               # small ratios: many equal IoUs, many equal to a threshold
    inter = (rng.integers(0, 21, size=(D, G)) * union) // 20
    counts = np.stack([inter, union], axis=-1).astype(np.int64)
    crowd = rng.random(G) < 0.2
    g_ig = crowd[None, :] | (rng.random((4, G)) < 0.3)
    d_out = rng.random((4, D)) < 0.3
    thrs = np.linspace(0.5, 0.95, 10) if n == 10 else np.linspace(0.05, 1.0, n) if n > 1 else np.array([0.5])
    exp = VM.match_video(counts, g_ig, crowd, d_out, thrs)
    got = VM.match_video_device(torch.from_numpy(counts).to(dev), g_ig, crowd, d_out, thrs)
    assert_match(got, exp)
    assert (exp["dt_match"] > 0).any() or D * G == 1


# ------------------------------------------------------------------------------------------------------------ end to end
RECORDED = lambda g: [k for k in g if k in ("precision", "recall", "scores", "stats", "img_none") or k.startswith("ious_") or
                      (k.startswith("img") and k.split("_")[-1] in Y.IMG_KEYS)]


def by_video(g):
    for v in g["in_videos"][:, 0].tolist():
        idx = np.flatnonzero(g["in_dt_meta"][:, 0] == v)
        yield v, idx, g["in_dt_score"][idx].tolist(), g["in_dt_meta"][idx, 1].tolist()


def finish(ev):
    ev.evaluate(), ev.accumulate(), ev.summarize()
    return Y.our_arrays(ev)


def assert_golden(got, g, ids_in_video_order):
    keys = RECORDED(g)
    if not ids_in_video_order:
        return Y.assert_same(got, g, keys)
    # detections added video by video get their ids in that order: the ids differ from the golden's, nothing else does
    Y.assert_same(got, g, [k for k in keys if not k.endswith(("gtMatches", "dtIds"))])
    for k in keys:
        if k.endswith("gtMatches"):
            assert np.array_equal(got[k] > 0, g[k] > 0), k


def test_end_to_end_from_rles_on_the_device(dev):
    g = golden()
    dataset, results = Y.dataset_of(g)
    ev = VM.YTVISEval(dataset, device=dev, params=Y.golden_params())
    ev.add_results(results)
    assert_golden(finish(ev), g, False)
    assert [ev.results()[k] for k in VM.METRICS] == (g["stats"] * 100).tolist()
    ev = VM.YTVISEval(dataset, device=dev, params=Y.golden_params())
    for v, idx, scores, labels in by_video(g):                            # the same through process() with pred_rles
        ev.process([{"video_id": v}], {"pred_scores": scores, "pred_labels": labels,
                                       "pred_rles": [results[i]["segmentations"] for i in idx]})
    assert_golden(finish(ev), g, True)


@pytest.mark.parametrize("kind", ("masks", "mask_list", "logits"))
def test_end_to_end_from_device_tensors(dev, kind):
    g = golden()
    dataset, _ = Y.dataset_of(g)
    _, dm = Y.masks_of(g)
    ev = VM.YTVISEval(dataset, params=Y.golden_params())                  # no device named: the tensors decide
    for v, idx, scores, labels in by_video(g):
        m = torch.from_numpy(dm[idx]).to(dev)
        out = {"pred_scores": scores, "pred_labels": labels, "image_size": (40, 70)}
        if kind == "logits":
            out["pred_logits"] = torch.where(m, 2.0, -1.0).float()
            out["pred_logits"][:, :, 0, 0] = torch.where(m[:, :, 0, 0], 1e-6, 0.0)       # 0 is not above the threshold 0
        else:
            out["pred_masks"] = m if kind == "masks" else [x for x in m]
        ev.process([{"video_id": v}], out, use_logits=kind == "logits")
    assert_golden(finish(ev), g, True)
    assert [ev.results()[k] for k in VM.METRICS] == (g["stats"] * 100).tolist()


def test_end_to_end_add_video_with_device_ground_truth(dev):
    """Ground truths and detections as device tensors through add_video: the stats of the golden (its None frame is an empty mask
    here, which the sequence IoU cannot tell apart; the annotation's own areas are kept)."""
    g = golden()
    gm, dm = Y.masks_of(g)
    ev = VM.YTVISEval(params=Y.golden_params(), categories=[1, 2])
    for v, idx, scores, labels in by_video(g):
        gi = np.flatnonzero(g["in_gt_meta"][:, 1] == v)
        gts = [{"id": int(g["in_gt_meta"][i, 0]), "category_id": int(g["in_gt_meta"][i, 2]), "iscrowd": int(g["in_gt_meta"][i, 3]),
                "masks": torch.from_numpy(gm[i]).to(dev),
                "areas": [None if np.isnan(a) else float(a) for a in g["in_gt_areas"][i]]} for i in gi]
        dts = [{"score": s, "category_id": l, "masks": torch.from_numpy(dm[i]).to(dev)} for i, s, l in zip(idx, scores, labels)]
        ev.add_video({"id": v, "height": 40, "width": 70}, gts, dts)
    got = finish(ev)
    Y.assert_same(got, g, ["precision", "recall", "scores", "stats"] + [k for k in g if k.startswith("ious_")])
