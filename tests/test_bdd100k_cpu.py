"""The BDD100K protocol (sam_pt_amd.vos_metrics.evaluate_bdd100k_sequence / BDD100KEval) on the host, pinned on the reference's own
evaluator: live where the reference tree is present (tests/bdd100k_ref.py runs it in place) and through the golden file
tests/golden/bdd100k_ref.npz everywhere.  Every comparison is ``==``: labels and counts exactly, floats with NaN equal to NaN."""
import functools

import numpy as np
import pytest
import torch

from sam_pt_amd import vos_metrics as VM
from tests import bdd100k_ref as B


@functools.lru_cache(maxsize=None)
def dataset():
    return B.seeded_dataset()                                             # (shared by the tests below, never written to)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(B.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_seeded_set_is_the_one_in_the_golden_file():
    got, exp = B.input_arrays(dataset()), golden()
    for k, v in got.items():
        assert np.array_equal(v, exp[k]), k


def test_golden_pin():
    """``BDD100KEval`` equals the reference's recorded tables and per-frame arrays, in index and in overlapping mode."""
    exp = golden()
    ref = {k: v for k, v in exp.items() if not k.startswith("in_") and k != "seed"}
    B.check_conditions(B.dataset_of(exp), ref)                            # finite figures: no comparison hides behind NaN
    B.assert_same(B.our_arrays(B.dataset_of(exp)), ref)


@pytest.mark.skipif(not B.available(), reason="the reference tree is absent")
def test_live_pin():
    """The same against the reference run now: ``BDD100KEvaluator.evaluate()`` on the PNGs, ``_evaluate_semisupervised`` per sequence."""
    ref = B.reference_arrays(dataset())
    B.check_conditions(dataset(), ref)
    B.assert_same(B.our_arrays(dataset()), ref)
    B.assert_same(ref, {k: v for k, v in golden().items() if not k.startswith("in_") and k != "seed"})   # the file is up to date


@pytest.mark.skipif(not B.available(), reason="the reference tree is absent")
def test_live_thresholds():
    """Other bin thresholds reach the labels and the bins (an empty bin is NaN on both sides)."""
    table_g, table_seq = B.run_reference(dataset(), short_object_threshold=10, long_object_threshold=13)
    ev = VM.BDD100KEval(short_object_threshold=10, long_object_threshold=13)
    for name, (gt, pr, _) in dataset().items():
        ev.add(name, pr, gt)
    g, table = ev.summarize()
    assert list(g) == list(table_g.index)
    assert np.array_equal(np.array(list(g.values())), np.array([table_g[k][0] for k in table_g.index], dtype=np.float64), equal_nan=True)
    assert table["short-medium-long"] == list(table_seq["short-medium-long"]) and len(set(table["short-medium-long"])) == 3


def test_torch_cpu_tensors_take_the_host_path():
    gt, pr, planes = dataset()["b"]
    a = VM.evaluate_bdd100k_sequence(pr, gt)
    b = VM.evaluate_bdd100k_sequence(torch.from_numpy(pr), torch.from_numpy(gt))
    for k in B.KINDS:
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    c = VM.evaluate_bdd100k_sequence(torch.from_numpy(planes), gt, object_overlapping_allowed=True)
    assert len(c["J"]) == 2


def test_per_object_records():
    gt, pr, _ = dataset()["a"]
    r = VM.evaluate_bdd100k_sequence(pr, gt)
    assert r["n_frames"].tolist() == [40, 37, 1] and r["visible_frames"].tolist() == [40, 15, 1]
    assert r["nonvisible_frames"].tolist() == [0, 22, 0]
    assert len(r["J"][0]) == 39 and len(r["J_nonvis"][0]) == 0 and np.isnan(r["stats"]["J_nonvis"][0]).all()
    for k in B.KINDS:                                                     # first seen on the last frame: the record of all ones
        assert r[k][2].tolist() == [1.0] and r["stats"][k][2][0] == 1.0
    # frame 12 of object 2 (index 8 after its first frame 3): both empty -> J = F = 1; frame 11: predicted, truth invisible -> J = 0
    assert r["J"][1][8] == 1.0 and r["F"][1][8] == 1.0 and r["J"][1][7] == 0.0
    # visibility is the area: a full-frame mask has an empty boundary map and is visible all the same
    gt, pr, _ = dataset()["b"]
    assert (gt[5] == 2).all() and not VM.seg2bmap(gt[5] == 2).any()
    r = VM.evaluate_bdd100k_sequence(pr, gt)
    assert r["visible_frames"].tolist() == [4, 9] and r["J"][1][4] == 1.0 and r["F"][1][4] == 1.0


def test_refusals():
    gt, pr, planes = dataset()["b"]
    bad = gt.copy()
    bad[0, 0, 0] = 255
    with pytest.raises(ValueError, match="255"):
        VM.evaluate_bdd100k_sequence(pr, bad)
    hi = pr.copy()
    hi[0, 0, 0] = 3
    with pytest.raises(ValueError, match="index 3"):
        VM.evaluate_bdd100k_sequence(hi, gt)
    skip = np.where(gt == 2, 3, gt).astype(np.uint8)                      # ids 1 and 3: 2 is never visible
    with pytest.raises(ValueError, match="object id 2 is never visible"):
        VM.evaluate_bdd100k_sequence(pr, skip)
    with pytest.raises(ValueError, match="no objects"):
        VM.evaluate_bdd100k_sequence(np.zeros_like(gt), np.zeros_like(gt))
    with pytest.raises(ValueError, match="K \\+ 1"):
        VM.evaluate_bdd100k_sequence(planes[:, :2], gt, object_overlapping_allowed=True)
    ev = VM.BDD100KEval()
    with pytest.raises(ValueError, match="no sequence"):
        ev.summarize()
    ev.add("b", pr, gt)
    with pytest.raises(ValueError, match="added before"):
        ev.add("b", pr, gt)
