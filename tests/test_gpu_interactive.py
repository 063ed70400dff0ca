"""Interactive point correction on the device (csrc/dbscan.hip, sam_pt_amd/interactive.py, sam_pt_amd/sam_pt_interactive.py): the
DBSCAN kernels against the NumPy restatement and the recorded scikit-learn labels, the frame state against its plain restatement,
the click selection and the whole loop against the same code with the device primitives switched off, all with ``==``; and batched
decoder chains against single ones within 8 x 1.9e-7."""
import numpy as np
import pytest
import torch

from sam_pt_amd import interactive as I
from tests import interactive_ref as IR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(IR.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return IR.dbscan_cases()


@pytest.fixture(scope="module")
def device_labels(cases, dev):
    return {name: I.dbscan_labels_device(X, eps, ms, dev) for name, (X, eps, ms) in cases.items()}


def test_dbscan_labels_device_equal_sklearn_golden_and_restatement(cases, device_labels, golden):
    for name, (X, eps, ms) in cases.items():
        got = device_labels[name]
        assert got.shape == (len(X),)
        assert (got == golden[f"dbscan_{name}"]).all(), name
        if name != "ref_18000":                                     # (tests/test_interactive_cpu.py holds the restatement to the same golden)
            assert (got == I.dbscan_labels(X, eps, ms)).all(), name


def test_dbscan_device_is_repeatable(cases, device_labels, dev):
    X, eps, ms = cases["n1000"]
    assert (I.dbscan_labels_device(X, eps, ms, dev) == device_labels["n1000"]).all()


def test_dbscan_largest_device_equals_host(device_labels, dev):
    for name, lab in device_labels.items():
        sizes = np.bincount(lab[lab >= 0]) if (lab >= 0).any() else np.zeros(1, int)
        for min_points in (1, int(sizes.max()), int(sizes.max()) + 1, 180):
            want, got = I.largest_cluster(lab, min_points), I.largest_cluster_device(lab, min_points, dev)
            assert got[:3] == want[:3], (name, min_points)
            assert got.members.tolist() == want.members.tolist(), (name, min_points)
    assert I.largest_cluster_device(device_labels["first_member_is_border"], 1, dev).cluster_id == 1
    assert I.largest_cluster_device(device_labels["tie_in_id_order"], 1, dev).cluster_id == 0


def test_dbscan_device_refuses_bad_input(dev):
    with pytest.raises(ValueError, match="integer pixel"):
        I.dbscan_labels_device(np.array([[0.5, 1.0], [2.0, 2.0]], dtype=np.float32), 1.5, 2, dev)
    with pytest.raises(ValueError, match="within 1e-6 of an integer"):
        I.dbscan_labels_device(np.array([[1.0, 1.0]], dtype=np.float32), 3.0, 2, dev)


# --------------------------------------------------------------------------------------------------------------- frame state
def _same_state(a, b):
    assert a[:5] == b[:5]
    assert a.categories.tolist() == b.categories.tolist()
    assert (a.fn_mask.cpu().bool() == b.fn_mask.cpu().bool()).all() and (a.fp_mask.cpu().bool() == b.fp_mask.cpu().bool()).all()


def test_frame_state_device_equals_restatement(dev):
    g = torch.Generator().manual_seed(3)
    Hh, Ww = 37, 70                                                   # more than one block of pixels, no multiple of the wave
    logits = torch.randn((Hh, Ww), generator=g)
    logits[5, 7] = 0.0                                                # exactly the threshold: not set
    gt = torch.rand((Hh, Ww), generator=g) < 0.4
    xy = torch.tensor([[69.0, 36.0], [69.4, 0.0], [0.0, 36.49], [2.5, 3.5], [3.5, 4.5], [-0.5, 0.5], [10.0, 10.0], [-1.0, -1.0],
                       [-70.0, -37.0], [68.5, 35.5], [20.2, 11.7], [33.0, 5.0]])
    n = len(xy)
    for seed in range(4):
        gg = torch.Generator().manual_seed(seed)
        vis = (torch.rand(n, generator=gg) < 0.8).float()
        vis[6] = 0.0                                                  # the invisible point is ignored wherever it sits
        vis[0] = vis[7] = 1.0
        lab = (torch.rand(n, generator=gg) < 0.5).int()
        _same_state(I.frame_state_device(logits.to(dev), gt.to(dev), xy, vis, lab), I.frame_state(logits, gt, xy, vis, lab))
    # an invisible point on an error pixel changes nothing; visible, it is the first incorrect one
    err = (((logits > 0) & ~gt).nonzero()[0]).flip(0).float()[None]   # a false positive pixel as (x, y)
    one = torch.ones(1)
    st = I.frame_state_device(logits.to(dev), gt.to(dev), err, 0 * one, one.int())
    assert (st.first_bad_positive, st.categories.tolist()) == (-1, [0])
    st = I.frame_state_device(logits.to(dev), gt.to(dev), err, one, one.int())
    assert st.first_bad_positive == 0 and st.categories.tolist() == [I.CAT_VISIBLE | I.CAT_POSITIVE | I.CAT_FP]
    # no points at all
    _same_state(I.frame_state_device(logits.to(dev), gt.to(dev), xy[:0], vis[:0], lab[:0]), I.frame_state(logits, gt, xy[:0], vis[:0], lab[:0]))
    for bad in ([70.0, 0.0], [69.5, 0.0], [0.0, 37.0], [-71.0, 0.0], [0.0, -37.6], [float("nan"), 1.0]):
        with pytest.raises(IndexError):
            I.frame_state_device(logits.to(dev), gt.to(dev), torch.tensor([bad]), one, one.int())
        I.frame_state_device(logits.to(dev), gt.to(dev), torch.tensor([bad]), 0 * one, one.int())          # invisible: ignored


# ----------------------------------------------------------------------------------------------------------- click selection
def test_extract_largest_cluster_points_device_equals_host(dev, golden):
    for name, (mask, n, seed) in IR.extract_cases().items():
        got = IR.our_extract(mask, n, seed, device=dev)
        assert (got == golden[f"extract_{name}"]).all(), name       # = the device=None path (tests/test_interactive_cpu.py) = the reference
        if name != "large_cluster":
            assert (got == IR.our_extract(mask, n, seed)).all(), name


# ---------------------------------------------------------------------------------------------------------------------- loop
# The clip of the loop tests is 5 frames of 128 x 256, not the 64 x 96 of the CPU pin.  The PIPS encoder (stride 4) runs residual
# layers at 1/2, 1/4, 1/8 and 1/16 of the frame: at 64 x 96 the last two maps are 8 x 12 and 4 x 6, smaller than ONE 16 x 16 output
# tile of the halo convolution (csrc/conv_halo_x3.hip) that computes them, and the coarsest of the four pyramid levels is 2 x 3,
# smaller than the 7 x 7 correlation window.  No kernel-level test of the tracker covers a map below one tile, and no GPU test of the
# suite runs the PIPS engine below 120 x 214; the loop test is not the place to be the first.  128 x 256 is the geometry smoke() and
# the tracker's own GPU tests use.
BAR = 8 * 1.9e-7      # batched against single chains: 8 x the figure DESIGN.md records for the ViT path


@pytest.fixture(scope="module")
def loop_setup(dev):
    return IR.gpu_loop_setup(dev)


@pytest.fixture(scope="module")
def loop_runs(loop_setup):
    """The loop with decode_batch=1, with the device primitives and with them switched off."""
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    video, tracker, predictor, kw = loop_setup
    runs = {}
    for device_primitives in (True, False):
        model = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, device_primitives=device_primitives, decode_batch=1, **kw).eval()
        torch.manual_seed(5)
        out = model(video)
        runs[device_primitives] = (IR.history_rows(model.last_run["interaction_history"]), out["logits"][0].cpu(), model.last_run, model)
    return runs


def test_loop_device_primitives_equal_host_primitives(loop_runs):
    """SamPtInteractive on a SamHip predictor with the PIPS tracker, against the same objects with the device primitives switched off
    (masks downloaded, host J&F, host frame state and clicks): both see the same device logits, so history and logits are equal."""
    (rows_d, logits_d, last_d, _), (rows_h, logits_h, last_h, _) = loop_runs[True], loop_runs[False]
    assert len(rows_d) == 9                                              # 12 minus the three query points
    assert rows_d == rows_h
    assert (logits_d == logits_h).all()
    assert any(r[0] == "add" for r in rows_d) and last_d["device_clicks"] > 0 and last_d["host_clicks"] == 0
    assert last_h["device_clicks"] == 0 and last_h["host_clicks"] == last_d["device_clicks"]


def test_decode_batch_4_against_1(loop_setup, loop_runs):
    """Batched chains (track_decode, positives first, frames with and without a visible negative point in separate chains) against the
    reference's call-by-call decode, on ONE point state — the final one of the decode_batch=1 run, since a history under another
    arithmetic may take other clicks.  Bar: 8 x 1.9e-7, DESIGN.md's figure for batched against single chains on the ViT path.
    Measured on the MI355X (profiles/interactive_bench.log): 2.4e-7 on the final state (two-pass chains only) and 1.6e-7 with the
    negatives hidden on frames 0 .. 2 (single-pass and two-pass chains side by side); largest |logit| 0.34."""
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    video, tracker, predictor, kw = loop_setup
    _, _, last, _ = loop_runs[True]
    results = IR.decode_batch_differences(loop_setup, last, batch=4)
    for name, diff, big, has_neg in results:
        print(f"decode_batch=4 against 1, {name}: largest logit difference {diff:.3e} (largest |logit| {big:.3e}; frames with a visible "
              f"negative {has_neg}), bar {BAR:.3e}")
    assert any(results[0][3])
    assert results[1][3][:3] == [False] * 3 and any(results[1][3][3:])      # single-pass and two-pass chains in one pass
    for name, diff, _, _ in results:
        assert diff <= BAR, name
    model4 = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, decode_batch=4, **kw).eval()
    # the whole loop runs batched too (its history may differ from the default's: nothing is asserted on it)
    torch.manual_seed(5)
    out = model4(video)
    assert out["logits"][0].shape == (5, 128, 256) and len(model4.last_run["interaction_history"]) == 9
    assert model4.last_run["decoder_chains"] < model4.last_run["decoder_calls"]
