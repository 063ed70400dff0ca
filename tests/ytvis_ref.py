"""TEST INFRASTRUCTURE ONLY: what it takes to run the reference's own YouTube-VIS evaluator (``YTVOS.loadRes`` and
``YTVOSeval.evaluate / accumulate / summarize`` of vis_eval/mask2former_video/data_video/datasets/ytvis_api) in place on the CPU,
and the seeded data set the golden file tests/golden/vis_eval_ref.npz is made of.

The evaluator needs four mask primitives of pycocotools, which is absent: ``area``, ``merge``, ``frPyObjects`` for an uncompressed
RLE dict, and ``toBbox``.  ``MaskStandIn`` supplies them from the project's RLE functions and is registered as ``pycocotools.mask``
before the two reference files are imported by path; nothing of the reference is copied.  ``available()`` is false where the
reference tree is absent (the GPU tests never need it: they read the golden file).
"""
import contextlib
import copy
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

from oracle.reference_loader import REF
from sam_pt_amd.automatic_mask_generator import coco_rle_counts, coco_rle_string, mask_to_rle, rle_to_mask

API = os.path.join(REF, "sam_pt", "vis_eval", "mask2former_video", "data_video", "datasets", "ytvis_api")
TEST_AREA_RNG = [[0, 1e10], [0, 150], [150, 400], [400, 1e10]]          # ranges that fit 40 x 70 images
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_eval_ref.npz")
IMG_KEYS = ("dtMatches", "gtMatches", "dtIgnore", "gtIgnore", "dtIds", "gtIds", "dtScores")


def available() -> bool:
    return os.path.isfile(os.path.join(API, "ytvoseval.py")) and os.path.isfile(os.path.join(API, "ytvos.py"))


# ---------------------------------------------------------------------------------------------- pycocotools.mask stand-in
def _record(mask: np.ndarray) -> dict:
    r = mask_to_rle(torch.from_numpy(np.ascontiguousarray(mask))[None])[0]
    return {"size": list(r["size"]), "counts": coco_rle_string(r["counts"])}


class MaskStandIn:
    """The four functions; an RLE is ``{"size": [h, w], "counts": str}`` (a list of counts is accepted as well)."""

    @staticmethod
    def area(rle):
        c = rle["counts"]
        c = coco_rle_counts(c) if isinstance(c, (str, bytes)) else c
        return int(sum(c[1::2]))

    @staticmethod
    def merge(rles, intersect=False):
        m = rle_to_mask(rles[0]).copy()
        for r in rles[1:]:
            m = (m & rle_to_mask(r)) if intersect else (m | rle_to_mask(r))
        return _record(m)

    @staticmethod
    def frPyObjects(obj, h, w):
        if not isinstance(obj, dict):
            raise NotImplementedError("the stand-in converts uncompressed RLE dicts only")
        assert list(obj["size"]) == [h, w]
        return {"size": [h, w], "counts": coco_rle_string(obj["counts"])}

    @staticmethod
    def toBbox(rle):
        ys, xs = np.nonzero(rle_to_mask(rle))
        if ys.size == 0:
            return np.zeros(4)
        return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], dtype=np.float64)


def load():
    """(YTVOS, YTVOSeval) of the reference, imported in place."""
    assert available(), "reference tree not present"
    sys.dont_write_bytecode = True                                      # never write __pycache__ into the reference tree
    if "pycocotools.mask" not in sys.modules:
        pkg, mask = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.mask")
        for name in ("area", "merge", "frPyObjects", "toBbox"):
            setattr(mask, name, getattr(MaskStandIn, name))
        pkg.mask = mask
        sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pkg, mask
    # ytvos.py imports three matplotlib names for its drawing helpers, which the evaluation never calls: empty modules stand in
    # while it is imported (other tests may have stubbed or imported matplotlib; sys.modules is left as it was)
    plot = {"matplotlib": {}, "matplotlib.pyplot": {}, "matplotlib.collections": {"PatchCollection": object},
            "matplotlib.patches": {"Polygon": object}}
    saved = {k: sys.modules.get(k) for k in plot}
    mods = []
    try:
        for k, attrs in plot.items():
            sys.modules[k] = types.ModuleType(k)
            for a, v in attrs.items():
                setattr(sys.modules[k], a, v)
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
        for name in ("ytvos", "ytvoseval"):
            key = "_sampt_ref_" + name
            if key not in sys.modules:
                spec = importlib.util.spec_from_file_location(key, os.path.join(API, name + ".py"))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                sys.modules[key] = mod
            mods.append(sys.modules[key])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods[0].YTVOS, mods[1].YTVOSeval


def run_reference(dataset, results, area_rng=TEST_AREA_RNG):
    """The reference's evaluator object after evaluate / accumulate / summarize on copies of the inputs."""
    YTVOS, YTVOSeval = load()
    with contextlib.redirect_stdout(io.StringIO()):
        gt = YTVOS()
        gt.dataset = copy.deepcopy(dataset)
        gt.createIndex()
        dt = gt.loadRes(copy.deepcopy(list(results)))
        ev = YTVOSeval(gt, dt)
        ev.params.areaRng = [list(r) for r in area_rng]
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return ev


def reference_arrays(ev) -> dict:
    """What the golden file records of a reference run, as flat arrays."""
    out = {"precision": ev.eval["precision"], "recall": ev.eval["recall"], "scores": ev.eval["scores"], "stats": np.asarray(ev.stats),
           "area_rng": np.asarray(ev.params.areaRng, dtype=np.float64), "vid_ids": np.asarray(ev.params.vidIds),
           "cat_ids": np.asarray(ev.params.catIds), "img_none": np.array([e is None for e in ev.evalImgs])}
    for i, e in enumerate(ev.evalImgs):
        if e is not None:
            for k in IMG_KEYS:
                out[f"img{i}_{k}"] = np.asarray(e[k])
    for (v, c), iou in ev.ious.items():
        out[f"ious_{v}_{c}"] = np.asarray(iou, dtype=np.float64)
    return out


def our_arrays(ev) -> dict:
    """The same arrays of a ``sam_pt_amd.vis_metrics.YTVISEval`` after evaluate / accumulate / summarize."""
    out = {"precision": ev.eval["precision"], "recall": ev.eval["recall"], "scores": ev.eval["scores"], "stats": np.asarray(ev.stats),
           "area_rng": np.asarray(ev.params.areaRng, dtype=np.float64), "vid_ids": np.asarray(ev.vidIds),
           "cat_ids": np.asarray(ev.catIds), "img_none": np.array([e is None for e in ev.evalImgs])}
    for i, e in enumerate(ev.evalImgs):
        if e is not None:
            for k in IMG_KEYS:
                out[f"img{i}_{k}"] = np.asarray(e[k])
    for (v, c), iou in ev.ious.items():
        out[f"ious_{v}_{c}"] = np.asarray(iou, dtype=np.float64)
    return out


def assert_same(got: dict, exp: dict, keys=None):
    """``==`` on every recorded array (shape, then values; an empty IoU matrix is empty whatever its shape)."""
    keys = [k for k in exp if not k.startswith("in_") and k != "seed"] if keys is None else keys
    for k in keys:
        assert k in got, f"{k} is missing"
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if g.size == 0 and e.size == 0 and k.startswith("ious_"):
            assert len(g) == len(e), f"{k}: lengths {len(g)} != {len(e)}"
            continue
        assert g.shape == e.shape, f"{k}: shape {g.shape} != {e.shape}"
        assert np.array_equal(g.astype(np.float64), e.astype(np.float64)), f"{k} differs at {np.argwhere(g != e)[:3].tolist()}"
    extra = [k for k in got if k not in exp and (k.startswith("img") or k.startswith("ious_"))]
    assert not extra, f"unexpected arrays {extra[:4]}"


# ------------------------------------------------------------------------------------------------------ seeded data set
def _disc(h, w, cy, cx, r):
    y, x = np.mgrid[:h, :w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def seeded_arrays(seed: int, n_videos: int = 12, T: int = 5, h: int = 40, w: int = 70) -> dict:
    """The inputs as arrays (the ``in_*`` entries of the golden file).  Discs drifting one pixel per frame; detections are jittered
    copies of ground truths plus random ones; scores are rounded to 0.01.  Added by hand, and asserted by the tests on the golden
    set: two categories; a crowd ground truth with two detections on it (video 1); an annotation with a ``None`` frame (video 2); a
    detection whose masks are all empty (video 3); two detections with one score (video 4); a pair with inter / union = 11 / 20
    exactly (video 5, category 2); a video with detections and no ground truth (the last but one) and one with ground truths and
    no detection (the last)."""
    rng = np.random.default_rng(seed)
    gm, gmeta, gpres, gareas = [], [], [], []
    dm, dmeta, dscore, dpres = [], [], [], []

    def add_gt(v, cat, masks, crowd=0):
        gm.append(masks), gmeta.append([len(gmeta) + 1, v, cat, crowd]), gpres.append(np.ones(T, dtype=bool))
        gareas.append(masks.sum(axis=(1, 2)).astype(np.float64))

    def add_dt(v, cat, masks, score):
        dm.append(masks), dmeta.append([v, cat]), dscore.append(float(score)), dpres.append(np.ones(T, dtype=bool))

    for v in range(1, n_videos + 1):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, r = rng.integers(8, h - 8), rng.integers(10, w - 10), int(rng.integers(4, 13))
            dy, dx = rng.integers(-1, 2, size=2)
            cat = int(rng.integers(1, 3))
            if v < n_videos - 1:
                add_gt(v, cat, np.stack([_disc(h, w, cy + dy * t, cx + dx * t, r) for t in range(T)]))
            if v != n_videos and (rng.random() < 0.85 or v == n_videos - 1):
                jy, jx, jr = rng.integers(-2, 3), rng.integers(-2, 3), int(rng.integers(-1, 2))
                dcat = cat if rng.random() < 0.9 else 3 - cat
                add_dt(v, dcat, np.stack([_disc(h, w, cy + jy + dy * t, cx + jx + dx * t, max(2, r + jr)) for t in range(T)]),
                       round(float(rng.uniform(0.3, 1.0)), 2))
        if v == n_videos:                                               # ground truths only
            add_gt(v, 1, np.stack([_disc(h, w, 20, 30 + t, 7) for t in range(T)]))
        else:
            for _ in range(int(rng.integers(0, 3))):
                cy, cx, r = rng.integers(5, h - 5), rng.integers(5, w - 5), int(rng.integers(3, 10))
                add_dt(v, int(rng.integers(1, 3)), np.stack([_disc(h, w, cy, cx + t, r) for t in range(T)]),
                       round(float(rng.uniform(0.0, 0.5)), 2))
    first = {v: next(i for i, m in enumerate(gmeta) if m[1] == v) for v in (1, 2)}
    gmeta[first[1]][3] = 1                                              # video 1: a crowd, and two detections on it
    for s in (0.9, 0.8):
        add_dt(1, gmeta[first[1]][2], gm[first[1]].copy(), s)
    gpres[first[2]][2] = False                                          # video 2: no annotation on frame 2
    gareas[first[2]][2] = np.nan
    gm[first[2]][2] = False
    add_dt(3, 1, np.zeros((T, h, w), dtype=bool), 0.5)                  # video 3: a detection that is empty on every frame
    add_dt(4, 1, np.stack([_disc(h, w, 12, 20, 5)] * T), 0.77)          # video 4: one score twice
    add_dt(4, 1, np.stack([_disc(h, w, 28, 50, 6)] * T), 0.77)
    g, d = np.zeros((T, h, w), dtype=bool), np.zeros((T, h, w), dtype=bool)   # video 5: |g| = 15, |d| = 16, |g & d| = 11 -> 11 / 20
    g[0, 0:3, 0:5] = True
    d[0, 0:3, 0:3], d[0, 0:2, 3], d[0, 3, 0:5] = True, True, True
    add_gt(5, 2, g)
    add_dt(5, 2, d, 0.95)
    order = np.argsort([m[1] for m in gmeta], kind="mergesort")         # annotations grouped by video, ids in that order
    gmeta = [[i + 1] + gmeta[j][1:] for i, j in enumerate(order)]
    return {"in_T": np.int64(T), "in_videos": np.array([[v, h, w] for v in range(1, n_videos + 1)]),
            "in_gt_meta": np.array(gmeta), "in_gt_present": np.stack([gpres[j] for j in order]),
            "in_gt_areas": np.stack([gareas[j] for j in order]), "in_gt_bits": np.packbits(np.stack([gm[j] for j in order])),
            "in_dt_meta": np.array(dmeta), "in_dt_score": np.array(dscore), "in_dt_present": np.stack(dpres),
            "in_dt_bits": np.packbits(np.stack(dm))}


def masks_of(arr: dict):
    """(gt masks bool (Ng, T, h, w), dt masks bool (Nd, T, h, w)) of the ``in_*`` arrays."""
    T, (_, h, w) = int(arr["in_T"]), arr["in_videos"][0]
    ng, nd = len(arr["in_gt_meta"]), len(arr["in_dt_meta"])
    g = np.unpackbits(arr["in_gt_bits"])[:ng * T * h * w].reshape(ng, T, h, w).astype(bool)
    d = np.unpackbits(arr["in_dt_bits"])[:nd * T * h * w].reshape(nd, T, h, w).astype(bool)
    return g, d


def dataset_of(arr: dict):
    """(annotation dict, results list) of the ``in_*`` arrays: uncompressed RLE for the ground truths (the reference converts them
    through ``frPyObjects``), compressed RLE for the detections, ``None`` for an absent frame."""
    g, d = masks_of(arr)
    h, w = int(arr["in_videos"][0][1]), int(arr["in_videos"][0][2])
    dataset = {"videos": [{"id": int(v), "height": int(hh), "width": int(ww), "length": int(arr["in_T"])} for v, hh, ww in arr["in_videos"]],
               "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}], "annotations": []}
    for (i, v, c, crowd), pres, areas, masks in zip(arr["in_gt_meta"], arr["in_gt_present"], arr["in_gt_areas"], g):
        segs = [mask_to_rle(torch.from_numpy(m)[None])[0] if p else None for m, p in zip(masks, pres)]
        dataset["annotations"].append({"id": int(i), "video_id": int(v), "category_id": int(c), "iscrowd": int(crowd), "segmentations": segs,
                                       "areas": [float(a) if p else None for a, p in zip(areas, pres)], "height": h, "width": w})
    results = [{"video_id": int(v), "category_id": int(c), "score": float(s),
                "segmentations": [_record(m) if p else None for m, p in zip(masks, pres)]}
               for (v, c), s, pres, masks in zip(arr["in_dt_meta"], arr["in_dt_score"], arr["in_dt_present"], d)]
    return dataset, results


def golden_params():
    from sam_pt_amd.vis_metrics import Params
    p = Params()
    p.areaRng = [list(r) for r in TEST_AREA_RNG]
    return p
