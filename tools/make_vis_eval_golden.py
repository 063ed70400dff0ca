"""Writes tests/golden/vis_eval_ref.npz: a seeded YouTube-VIS data set (tests/ytvis_ref.seeded_arrays) and what the REFERENCE's own
evaluator (YTVOS.loadRes + YTVOSeval.evaluate / accumulate / summarize, run in place through tests/ytvis_ref.py) makes of it — per
(category, area range, video) group dtMatches, gtMatches, dtIgnore, gtIgnore, the ids and scores, per (video, category) the IoU
matrix, and precision, recall, scores and the 12 summary figures.  Nothing of sam_pt_amd.vis_metrics takes part.

Regenerate (needs the reference tree, SAMPT_REFERENCE or the default of oracle/reference_loader.py):

    python tools/make_vis_eval_golden.py [--seed 2]

The conditions the tests assert on the set are checked here first: all 12 figures >= 0, 0 < AP < 1, two categories, a crowd, a
None frame, an all-empty detection, a video without ground truth and one without detections, a score tie, and an IoU that equals
a threshold exactly.  The area ranges are tests/ytvis_ref.TEST_AREA_RNG, set through the reference's params.areaRng.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ytvis_ref as Y  # noqa: E402


def check_conditions(arr, ref):
    stats = ref["stats"]
    assert (stats >= 0).all(), f"a summary figure is undefined: {stats}"
    assert 0 < stats[0] < 1, f"AP = {stats[0]}"
    gmeta, dmeta = arr["in_gt_meta"], arr["in_dt_meta"]
    assert set(gmeta[:, 2]) == {1, 2} and gmeta[:, 3].any()
    assert (~arr["in_gt_present"]).any()
    _, d = Y.masks_of(arr)
    assert (d.reshape(len(d), -1).sum(1) == 0).any()
    gv, dv = set(gmeta[:, 1]), set(dmeta[:, 0])
    assert dv - gv and gv - dv
    sc = arr["in_dt_score"]
    assert any(len(set(sc[(dmeta[:, 0] == v) & (dmeta[:, 1] == c)])) < ((dmeta[:, 0] == v) & (dmeta[:, 1] == c)).sum()
               for v in dv for c in (1, 2))
    thrs = np.linspace(0.5, 0.95, 10)
    assert any(np.isin(ref[k], thrs).any() for k in ref if k.startswith("ious_")), "no IoU equals a threshold"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--out", default=Y.GOLDEN)
    args = ap.parse_args()
    assert Y.available(), "the reference tree is required"
    arr = Y.seeded_arrays(args.seed)
    dataset, results = Y.dataset_of(arr)
    ref = Y.reference_arrays(Y.run_reference(dataset, results))
    check_conditions(arr, ref)
    np.savez_compressed(args.out, seed=np.int64(args.seed), **arr, **ref)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(arr['in_gt_meta'])} annotations, {len(arr['in_dt_meta'])} detections, "
          f"stats = {np.round(ref['stats'], 4).tolist()}")


if __name__ == "__main__":
    main()
