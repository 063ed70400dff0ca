"""Prompt assembly for device-resident point tracks, without a GPU: the NumPy restatement that specifies the kernels
(sam_pt_amd/prompt_assembly.py) against ``SamPt._prepare_points`` + ``apply_coords``, the ``device_tracks`` keyword and its
fallbacks, and the trackers' ``results_on_device`` switch."""
import os

import numpy as np
import pytest
import torch

from sam_pt_amd import prompt_assembly as PA
from sam_pt_amd.point_tracker import PointTracker, _EngineTracker
from sam_pt_amd.sam_pt import PointVisibilityType, SamPt
from tests import prompt_assembly_cases as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("M,pp,P,negatives,add_others", CS.CASES)
def test_host_restatement_equals_prepare_points_loop(M, pp, P, negatives, add_others):
    traj, vis, xy, lab, k, npos = CS.reference(M, pp, P, negatives, add_others)
    sx, sy = CS.scales()
    got_xy, got_lab, got_k, got_npos = PA.assemble_prompts_host(traj, vis, pp, negatives, add_others, sx, sy)
    assert got_xy.dtype == np.float32 and got_lab.dtype == np.int32 and got_k.dtype == np.int32 and got_npos.dtype == np.int32
    assert got_xy.shape == xy.shape and (got_xy.view(np.int32) == xy.view(np.int32)).all()
    assert (got_lab == lab).all() and (got_k == k).all() and (got_npos == npos).all()
    ld = -(-xy.shape[1] // 8) * 8                                  # more slots than the longest prompt: zeros behind it
    wide_xy, wide_lab, _, _ = PA.assemble_prompts_host(traj, vis, pp, negatives, add_others, sx, sy, ld=ld)
    assert wide_xy.shape == (xy.shape[0], ld, 2) and (wide_xy[:, :xy.shape[1]] == xy).all() and (wide_lab[:, :xy.shape[1]] == lab).all()
    assert not wide_xy[:, xy.shape[1]:].any() and not wide_lab[:, xy.shape[1]:].any()


def test_cases_cover_what_they_claim():
    seen = set()
    for M, pp, P, negatives, add_others in CS.CASES:
        traj, vis, xy, lab, k, npos = CS.reference(M, pp, P, negatives, add_others)
        seen |= set(np.unique(vis).tolist())
        k2 = k.reshape(CS.T, M)
        assert (k2[1] == 0).all()                                  # a frame with nothing visible
        assert np.isfinite(traj).all()
        if negatives and P > pp:
            assert npos.reshape(CS.T, M)[2, 0] == 0 and k2[2, 0] > 0          # an item with only negatives visible
        assert not (vis[0, M - 1, :min(pp, P)] == 1).any()         # an object that contributes no negatives
    assert seen == {float(c.value) for c in PointVisibilityType}
    sx, sy = CS.scales()
    assert sx != sy and (sx, sy) == (1024 / 854, 576 / 480)
    # with pp = 8 the other objects contribute at most exactly 64 points at M = 9 and 72 at M = 10; M = 70 exceeds 256 candidates
    assert 8 * 8 == 64 and 9 * 8 == 72 and 70 * 8 > 256


class _StubPredictor:
    """The fused path's predictor as far as ``SamPt.__init__`` and ``_device_tracks_active`` look at it."""
    model = torch.nn.Identity()

    def encode_frames(self, *a, **k):
        raise AssertionError("not used")

    def track_decode(self, *a, **k):
        raise AssertionError("not used")


class _StubEngineTracker(torch.nn.Module):
    results_on_device = False


class _OnDevice:
    is_cuda = True


def _model(tracker=None, predictor=None, **kw):
    return SamPt(tracker if tracker is not None else _StubEngineTracker(), predictor if predictor is not None else _StubPredictor(),
                 sam_iou_threshold=0.0, **kw).eval()


def test_device_tracks_keyword_and_default():
    assert _model().device_tracks is False                        # a keyword with a default: the reference's contract holds
    assert _model(device_tracks=True).device_tracks is True
    assert not _model()._device_tracks_active(_OnDevice())         # off: the host path, whatever the clip
    assert _model(device_tracks=True)._device_tracks_active(_OnDevice())


def test_every_fallback_takes_the_host_path():
    on = _OnDevice()
    assert not _model(device_tracks=True, use_point_reinit=True)._device_tracks_active(on)
    assert not _model(device_tracks=True, max_other_objects_positive_points=5)._device_tracks_active(on)

    class WithMasks(_StubEngineTracker):                           # SuperGlue-style
        def set_masks(self, masks):
            pass

    assert not _model(WithMasks(), device_tracks=True)._device_tracks_active(on)
    assert not _model(torch.nn.Identity(), device_tracks=True)._device_tracks_active(on)      # a tracker without results_on_device

    class Stepwise:                                                # no encode_frames / track_decode
        model = torch.nn.Identity()

    assert not _model(predictor=Stepwise(), device_tracks=True)._device_tracks_active(on)
    assert not _model(device_tracks=True)._device_tracks_active(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))    # CPU tensors
    assert not _model(device_tracks=True)._device_tracks_active(on, frame_ids=[0, 1])


def test_cpu_clip_runs_the_host_path_unchanged():
    """``device_tracks=True`` on CPU tensors: the same calls and the same result as the default (no device call is attempted — there
    is no device here to attempt it on)."""
    from sam_pt_amd.synth import synthetic_clip
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    from tests.util import make_fake_device_predictor
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    Tn, M, P = 3, 2, 3
    frames, _ = synthetic_clip(T=Tn, H=128, W=256, seed=3)
    g = torch.Generator().manual_seed(7)
    traj = torch.rand(Tn, M * P, 2, generator=g) * torch.tensor([250.0, 120.0]) + 3.0
    vis = torch.ones(Tn, M * P, dtype=torch.bool)
    vis[1, :P] = False
    seen = []

    class Stub(_EngineTracker):
        _engines, _who = (), "Stub"

        def forward(self, rgbs, query_points):
            seen.append(self.results_on_device)
            return traj[None].clone(), vis[None].clone()

    q = torch.cat([torch.zeros(M, P, 1), traj[0].reshape(M, P, 2)], dim=2)
    video = {"image": frames, "target_hw": (128, 256), "query_points": q}
    kw = dict(sam_iou_threshold=0.0, positive_points_per_mask=3, negative_points_per_mask=0, iterative_refinement_iterations=1)
    outs = []
    for flag in (False, True):
        fake = make_fake_device_predictor(sd, cfg)
        outs.append((SamPt(Stub(), fake, device_tracks=flag, **kw).eval()(video), fake.calls))
    assert seen == [False, False]
    (a, ca), (b, cb) = outs
    assert ca == cb and a["scores_per_frame"] == b["scores_per_frame"]
    assert torch.equal(torch.stack(a["logits"]), torch.stack(b["logits"]))
    assert torch.equal(a["trajectories"], b["trajectories"]) and torch.equal(a["visibilities"], b["visibilities"])
    assert not a["trajectories"].is_cuda


def test_results_on_device_defaults_to_off_and_keeps_cpu_copies():
    from sam_pt_amd.point_tracker import CoTrackerPointTracker, PipsPointTracker
    assert _EngineTracker.results_on_device is False
    assert PipsPointTracker.results_on_device is False and CoTrackerPointTracker.results_on_device is False
    assert not hasattr(PointTracker, "results_on_device")          # the reference's abstract class is as it was

    class Stub(_EngineTracker):
        _engines, _who = (), "Stub"

        def forward(self, rgbs, query_points):
            self.out = (torch.rand(1, rgbs.shape[1], query_points.shape[1], 2), torch.ones(1, rgbs.shape[1], query_points.shape[1]))
            return self.out

    trk = Stub()
    rgbs, q = torch.zeros(1, 4, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 5, 3)
    gt = torch.rand(1, 4, 5, 2)
    out = trk.evaluate_batch(rgbs, q, trajectories_gt=gt)
    assert not out["trajectories_pred"].is_cuda and out["trajectories_pred"] is not trk.out[0]       # a CPU copy, as in the reference
    assert torch.equal(out["trajectories_pred"], trk.out[0]) and out["query_points"] is not q
    trk.results_on_device = True
    out = trk.evaluate_batch(rgbs, q, trajectories_gt=gt)
    assert out["trajectories_pred"] is trk.out[0] and out["visibilities_pred"] is trk.out[1] and out["query_points"] is q
    assert out["trajectories_gt"] is not gt and torch.equal(out["trajectories_gt"], gt) and out["visibilities_gt"] is None


def test_entry_points_are_declared_bound_and_built():
    from sam_pt_amd import _lib
    header = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    for name in ("sampt_prompt_count", "sampt_prompt_fill", "sampt_mark_outside_frame"):
        assert f"int {name}(" in header and name in _lib.exported_symbols()
    assert " prompt_assembly.hip " in open(os.path.join(ROOT, "sam_pt_amd", "csrc", "Makefile")).read()


def test_device_calls_refuse_cpu_tensors():
    from sam_pt_amd import _lib
    with pytest.raises(_lib.SamptError):
        PA.count_prompts(torch.ones(2, 2, 3), 2, False, True)
    with pytest.raises(_lib.SamptError):
        PA.mark_outside_frame(torch.zeros(2, 3, 2), torch.ones(2, 3), 8, 8)
    with pytest.raises(_lib.SamptError):
        z = torch.zeros(1, dtype=torch.int32)
        PA.fill_prompts(torch.zeros(2, 2, 3, 2), torch.ones(2, 2, 3), 2, False, True, 1.0, 1.0, z, torch.zeros(1, 4, 2),
                        torch.zeros(1, 4, dtype=torch.int32), z, z)
