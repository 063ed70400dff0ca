"""Interactive point correction on the host: the order-free DBSCAN restatement against scikit-learn, the click selection against the
reference's own function and the loop against the reference's own ``forward`` (both run in place where the reference tree is present,
and always against tests/golden/interactive_ref.npz, which tools/make_interactive_golden.py recorded from them)."""
import json
import os

import numpy as np
import pytest
import torch

from sam_pt_amd import interactive as I
from tests import interactive_ref as IR


@pytest.fixture(scope="module")
def golden():
    return np.load(IR.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return IR.dbscan_cases()


@pytest.fixture(scope="module")
def our_labels(cases):
    return {name: I.dbscan_labels(X, eps, ms) for name, (X, eps, ms) in cases.items()}


# ------------------------------------------------------------------------------------------------------------------- DBSCAN
def test_dbscan_labels_equal_the_recorded_sklearn_labels(cases, our_labels, golden):
    for name in cases:
        ref = golden[f"dbscan_{name}"]
        assert ref.dtype == np.int16 and our_labels[name].shape == ref.shape, name
        assert (our_labels[name] == ref).all(), name


@pytest.mark.skipif(not IR.sklearn_available(), reason="scikit-learn is not installed")
def test_dbscan_labels_equal_sklearn_live(cases, our_labels):
    for name, (X, eps, ms) in cases.items():
        if name != "ref_18000":                                   # (the golden holds that one; a live run of it takes a second more)
            assert (our_labels[name] == IR.sklearn_labels(X, eps, ms)).all(), name
    rng = np.random.default_rng(5)
    for _ in range(25):                                           # random pixel sets, shuffled, with duplicates now and then
        h, w = rng.integers(12, 41, 2)
        X = np.argwhere(rng.random((h, w)) < rng.uniform(0.1, 0.7)).astype(np.float32)
        X = X[rng.permutation(len(X))]
        if rng.random() < 0.3:
            X = np.concatenate([X, X[: len(X) // 3]])
        eps, ms = float(rng.uniform(0.6, 6.5)), int(rng.integers(1, 11))
        assert (I.dbscan_labels(X, eps, ms) == IR.sklearn_labels(X, eps, ms)).all(), (h, w, eps, ms)


def test_dbscan_cases_are_what_they_claim(cases, our_labels):
    assert our_labels["n1"].tolist() == [-1]
    assert (our_labels["all_noise"] == -1).all()
    for name in ("bridge", "bridge_shuffled"):
        X, lab = cases[name][0], our_labels[name]
        bridge = int(np.flatnonzero(X[:, 1] == 6)[0])
        left, right = lab[X[:, 1] < 6], lab[X[:, 1] > 6]
        assert len(set(left)) == 1 and len(set(right)) == 1 and left[0] != right[0]
        assert lab[bridge] == min(left[0], right[0]) == 0, name                      # the border pixel of both takes the lower id
    lab = our_labels["first_member_is_border"]
    assert lab[0] == 1 and (lab[1:6] == 0).all() and (lab[6:] == 1).all()
    assert our_labels["exact_r2_in"].tolist() == [0] * 6 and our_labels["exact_r2_out"].tolist() == [-1] * 6
    assert our_labels["n1000"].max() + 1 == 12 and our_labels["ref_18000"].max() + 1 == 2


def test_eps_within_rounding_of_an_integer_square_is_refused():
    for eps in (3.0, 8.0, float(np.sqrt(5.0)), float(np.nextafter(3.0, 0))):
        with pytest.raises(ValueError, match="within 1e-6 of an integer"):
            I.eps_to_r2(eps)
    assert I.eps_to_r2(2.24) == 5 and I.eps_to_r2(2.23) == 4 and I.eps_to_r2(0.5) == 0
    assert I.eps_to_r2(2.4 * 480 * 854 / 18000) == 2987
    with pytest.raises(ValueError, match="integer pixel"):
        I.dbscan_labels(np.array([[0.5, 1.0]]), 1.5, 2)


def test_largest_cluster_is_most_common_without_noise(our_labels):
    from collections import Counter
    for name, lab in our_labels.items():
        cnt = Counter(lab.tolist())
        cnt.pop(-1, None)
        got = I.largest_cluster(lab, 1)
        if not cnt:
            assert got.cluster_id == -1 and got.size == 0 and got.n_clusters == 0 and len(got.members) == 0, name
            continue
        cid, size = cnt.most_common(1)[0]
        assert (got.cluster_id, got.size, got.n_clusters) == (cid, size, len(cnt)), name
        assert got.members.tolist() == np.flatnonzero(lab == cid).tolist(), name
        below = I.largest_cluster(lab, size + 1)
        assert below.cluster_id == -1 and below.size == size and len(below.members) == 0, name
    assert I.largest_cluster(our_labels["first_member_is_border"], 1).cluster_id == 1      # 5 against 5: the one that appears first
    assert I.largest_cluster(our_labels["tie_in_id_order"], 1).cluster_id == 0


# ----------------------------------------------------------------------------------------------------------- click selection
def test_extract_largest_cluster_points_equals_the_recorded_reference(golden):
    for name, (mask, n, seed) in IR.extract_cases().items():
        got = IR.our_extract(mask, n, seed)
        assert got.dtype == np.float32 and got.shape == (n, 2)
        assert (got == golden[f"extract_{name}"]).all(), name


@pytest.mark.skipif(not IR.available(), reason="the reference tree is not present")
def test_extract_largest_cluster_points_equals_the_reference_live():
    for name, (mask, n, seed) in IR.extract_cases().items():
        assert (IR.our_extract(mask, n, seed) == IR.reference_extract(mask, n, seed)).all(), name


def test_extract_cases_take_the_branch_they_are_named_after():
    for name, (mask, n, seed) in IR.extract_cases().items():
        torch.manual_seed(seed)
        px = torch.from_numpy(mask).nonzero().float()
        px = px[torch.randperm(len(px))[:18000]]
        best = I.largest_cluster(I.dbscan_labels(px.numpy(), 2.4 * mask.size / 18000, 10), 180)
        want = {"large_cluster": lambda b: b.cluster_id >= 0 and b.size >= 180, "below_min_points": lambda b: b.cluster_id == -1 and 0 < b.size < 180,
                "no_cluster": lambda b: b.n_clusters == 0, "two_pixels": lambda b: b.n_clusters == 0 and mask.sum() < 3}[name]
        assert want(best), (name, best[:3])


def test_extract_consumes_the_generator_as_the_reference_does():
    mask, n, seed = IR.extract_cases()["below_min_points"]
    IR.our_extract(mask, n, seed)
    after = torch.rand(1).item()
    torch.manual_seed(seed)
    torch.randperm(int(mask.sum()))         # the sampled pixel list ...
    torch.randperm(int(mask.sum()))         # ... and the whole mask, since the largest cluster is below 180 points
    assert torch.rand(1).item() == after


# --------------------------------------------------------------------------------------------------------------- frame state
def test_frame_state_rounds_half_to_even_wraps_and_raises():
    logits = torch.full((6, 8), -1.0)
    logits[2:4, 2:5] = 1.0
    gt = torch.zeros((6, 8), dtype=torch.bool)
    gt[2:5, 3:6] = True
    #            tp            fp (2.5 -> 2)  fn             tn            invisible on fn  -1 wraps to (7, 5): tn
    xy = torch.tensor([[3.0, 2.0], [2.5, 3.0], [5.0, 3.5], [0.0, 0.0], [5.0, 4.0], [-1.0, -1.0]])
    vis = torch.tensor([1., 1., 1., 1., 0., 1.])
    lab = torch.tensor([1, 1, 0, 1, 1, 0], dtype=torch.int)
    st = I.frame_state(logits, gt, xy, vis, lab)
    assert (st.tp, st.fn, st.fp) == (4, 5, 2)
    C = I
    assert st.categories.tolist() == [C.CAT_VISIBLE | C.CAT_POSITIVE | C.CAT_CORRECT | C.CAT_TP, C.CAT_VISIBLE | C.CAT_POSITIVE | C.CAT_FP,
                                      C.CAT_VISIBLE | C.CAT_FN, C.CAT_VISIBLE | C.CAT_POSITIVE | C.CAT_TN, 0, C.CAT_VISIBLE | C.CAT_CORRECT | C.CAT_TN]
    assert (st.first_bad_negative, st.first_bad_positive) == (2, 1)
    assert st.fn_mask.sum() == 5 and st.fp_mask.sum() == 2
    for bad in ([8.0, 0.0], [0.0, 6.0], [-9.0, 0.0], [7.5, 0.0]):          # 7.5 rounds to 8: off the frame
        with pytest.raises(IndexError):
            I.frame_state(logits, gt, torch.tensor([bad]), torch.ones(1), torch.ones(1, dtype=torch.int))
    for bad in ([float("nan"), 1.0], [1.0, float("inf")]):                 # not finite: off the frame, as the kernel has it
        with pytest.raises(IndexError):
            I.frame_state(logits, gt, torch.tensor([bad]), torch.ones(1), torch.ones(1, dtype=torch.int))
    I.frame_state(logits, gt, torch.tensor([[8.0, 0.0]]), torch.zeros(1), torch.ones(1, dtype=torch.int))     # invisible: ignored


# ---------------------------------------------------------------------------------------------------------------------- loop
@pytest.fixture(scope="module")
def our_runs():
    return {name: IR.run_our_loop(name) for name in IR.LOOP_CONFIGS}


def test_loop_equals_the_recorded_reference_forward(our_runs, golden):
    for name, (rows, logits, _) in our_runs.items():
        assert rows == IR.rows_of(golden, f"loop_{name}"), name
        assert (logits == golden[f"loop_{name}_logits"]).all(), name
    for name in IR.ALL_FOUR:                                                       # all four actions are exercised
        assert IR.actions_of(our_runs[name][0]) == set(IR.ACTIONS), name


@pytest.mark.skipif(not IR.available(), reason="the reference tree is not present")
def test_loop_equals_the_reference_forward_live(our_runs):
    pred, tracker = IR.cpu_predictor(), IR.ScriptedTracker()                       # the SAME objects for both sides
    for name in IR.LOOP_CONFIGS:
        ref_rows, ref_logits = IR.run_reference_loop(name, pred, tracker)
        rows, logits, _ = IR.run_our_loop(name, pred, tracker)
        assert rows == ref_rows and (logits == ref_logits).all(), name


def test_incremental_changes_nothing(our_runs):
    for name, (rows, logits, last) in our_runs.items():
        rows_all, logits_all, last_all = IR.run_our_loop(name, incremental=False)
        assert rows_all == rows and (logits_all == logits).all(), name
        assert last["decoder_calls"] < last_all["decoder_calls"], name


def test_contract_outputs_and_unbuilt_switches(tmp_path):
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    rows, logits, last = IR.run_our_loop("online", output_dir=str(tmp_path))
    assert logits.shape == (IR.T, IR.H, IR.W) and last["host_clicks"] > 0 and last["device_clicks"] == 0
    with open(os.path.join(tmp_path, "clip", "history.json")) as fh:
        hist = json.load(fh)
    assert [tuple(h[f] for f in IR.HISTORY_FIELDS) for h in hist] == rows
    with open(os.path.join(tmp_path, "clip", "overall_iou_history.json")) as fh:
        assert set(json.load(fh)) == {"threshold", "achieved_threshold", "before", "after"}
    base = dict(point_tracker=IR.ScriptedTracker(), sam_predictor=IR.cpu_predictor(), **IR.SAM_PT_KW)
    for kw in (dict(visualize_all_interactions_separately=True), dict(visualize_all_interactions_as_mp4=True), dict(font_path="x.ttf")):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            SamPtInteractive(**base, **kw)
    with pytest.raises(ValueError, match="decode_batch"):
        SamPtInteractive(**base, decode_batch=0)
    model = SamPtInteractive(**base, interactions_max=5).eval()
    images, gts = IR.clip()
    video = IR.video_of(images, gts)
    out = model({**video, "query_points": video["query_points"][:, :2], "target_hw": (IR.H, IR.W)})
    assert set(out) == {"logits", "scores", "scores_per_frame", "trajectories", "visibilities"}
    assert all(out[k] is None for k in out if k != "logits")
    with pytest.raises(NotImplementedError, match="track_decode"):                 # batched chains need a predictor that has them
        SamPtInteractive(**base, interactions_max=5, decode_batch=4).eval()(video)
    with pytest.raises(AssertionError, match="single mask"):
        model({**video, "query_points": video["query_points"].repeat(2, 1, 1)})
