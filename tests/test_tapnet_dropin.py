"""TapNet drop-in proof on the CPU, the way tests/test_tapir_dropin.py gives it for TAPIR: ``TapnetPointTracker`` over a recording fake
of its five C-ABI calls (tests/fake_hip_tapnet.py, which computes with the restatement of tests/tapnet_ref.py) as the tracker of

  * the UNCHANGED reference ``SamPt`` (sam_pt/modeling/sam_pt.py), built from the reference's own config tree with the overrides of
    INTEGRATION.md (``model/point_tracker=tapnet`` + the seam ``_target_``s) — where the reference tree exists;
  * ``sam_pt_amd.sam_pt.SamPt``, built directly — everywhere.

What the tracker hands to either model is what the reference's own adapter (tapnet/tracker.py:67-103) returns for the same restated
model, with ``==``.  PARITY UNPINNED for the model itself (no JAX, Haiku or checkpoint): see tests/tapnet_ref.py."""
import gc
import os

import pytest
import torch

from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict, init_tapnet_state_dict
from tests import fake_hip_tapnet
from tests import hydra_lite as H
from tests import tapnet_ref as R
from tests.util import disc_queries, max_abs, synthetic_clip

CONFIGS = os.path.join(R.REF, "configs")
needs_ref = pytest.mark.skipif(not R.available(), reason="reference tree not present (GPU box)")
T_CLIP, HW, N_POS = 3, (128, 256), 4


@pytest.fixture(scope="module")
def sd():
    return init_tapnet_state_dict(72)


@pytest.fixture(scope="module")
def sam():
    cfg = SAM_CONFIGS["vit_test"]
    return cfg, init_sam_state_dict(cfg, 72)


@pytest.fixture(scope="module")
def clip():
    """Three 128 x 256 frames, two objects of four positive points each, all queried on frame 0."""
    frames, centres = synthetic_clip(T=T_CLIP, H=HW[0], W=HW[1], seed=72)
    q = disc_queries(centres, n_pos=N_POS, r=9.0)
    q2 = q.clone()
    q2[:, 1:] += torch.tensor([-60.0, 25.0])
    return frames, torch.stack([q, q2])


@pytest.fixture(scope="module")
def restated_adapter(sd, clip):
    """(trajectories (T, 2, 4, 2), visibilities (T, 2, 4)) of the clip: our adapter's host code around the restated model."""
    from sam_pt_amd.point_tracker import TapnetPointTracker
    frames, qp = clip
    trk = TapnetPointTracker(state_dict={})
    model = R.model_fn(sd)
    trk._model = lambda f01, q: {k: torch.from_numpy(v) for k, v in model((f01.numpy() * 2 - 1).transpose(0, 1, 3, 4, 2), q.numpy()).items()}
    traj, vis = trk.forward(frames[None], qp.reshape(1, -1, 3))
    return traj[0].reshape(T_CLIP, 2, N_POS, 2), vis[0].reshape(T_CLIP, 2, N_POS)


def _check_tracker_calls(fake, n_clips):
    names = [c[0] for c in fake.tapnet_calls]
    assert names == ["create"] + ["workspace_bytes", "track_f32", "launches"] * n_clips
    assert fake.tapnet_calls[1:4] == [("workspace_bytes", T_CLIP, 2 * N_POS), ("track_f32", T_CLIP, 2 * N_POS), ("launches",)]
    assert fake.tapnet_names["tsm.stem.weight"].shape == (64, 7 * 7 * 4) and "tsm.u1.b0.conv0.weight_hl" in fake.tapnet_names     # pack_tapnet's


def test_tracker_over_the_recording_fake(monkeypatch, sd):
    """forward() on the golden's non-square clip through create / workspace_bytes / track_f32 / launches / destroy."""
    from sam_pt_amd.point_tracker import TapnetPointTracker
    gold = {k: torch.from_numpy(v) for k, v in R.golden().items()}
    fake = fake_hip_tapnet.install(monkeypatch, sd)
    trk = TapnetPointTracker(state_dict=sd)
    traj, vis = trk(gold["frames"][None], gold["query_points"][None])
    assert traj.shape == (1, 5, 6, 2) and traj.dtype == torch.float32 and vis.shape == (1, 5, 6) and vis.dtype == torch.bool
    Hc, Wc = gold["frames"].shape[-2:]
    bar = float(gold["bar_px"])
    assert max_abs(traj[0, ..., 0], gold["trajectories"][..., 0]) < bar * Wc / 256
    assert max_abs(traj[0, ..., 1], gold["trajectories"][..., 1]) < bar * Hc / 256
    assert torch.equal(vis[0], gold["visibilities"])
    assert fake.tapnet_calls == [("create", len(fake.tapnet_names)), ("workspace_bytes", 5, 6), ("track_f32", 5, 6), ("launches",)]
    assert trk.stats == {"clips": 1, "launches": 3 * 1 + 30}
    tracks, occ = trk.track(torch.zeros(1, 3, 256, 256), torch.tensor([[0.0, 100.0, 50.0]]))
    assert tracks.shape == (1, 1, 2) and occ.shape == (1, 1) and torch.equal(tracks[0, 0], torch.tensor([100.0, 50.0]))
    assert trk.stats == {"clips": 2, "launches": 3 * 1 + 30}
    assert fake.calls["tapnet_create"] == 1                    # the engine is built once and kept
    del trk
    gc.collect()
    assert fake.tapnet_calls[-1] == ("destroy",) and fake.calls["tapnet_destroy"] == 1


def _compose(extra=()):
    """The reference's model config with `model/point_tracker=tapnet model/sam@...=sam_vit_base` and INTEGRATION.md's overrides."""
    cfg = {"model": H.compose(CONFIGS, "model", "sam_pt", {"point_tracker": "tapnet", "sam@sam_predictor.sam_model": "sam_vit_base"})}
    assert cfg["model"]["point_tracker"]["_target_"] == "sam_pt.point_tracker.tapnet.TapnetPointTracker"
    H.apply_overrides(cfg, ["model.point_tracker._target_=sam_pt_amd.point_tracker.TapnetPointTracker",
                            "model.sam_predictor._target_=sam_pt_amd.sam_predictor.SamPredictor",
                            "model.sam_predictor.sam_model._target_=sam_pt_amd.sam_predictor.SamHip",
                            "+model.sam_predictor.sam_model._recursive_=false",
                            "model.point_tracker.checkpoint_path=null", "model.sam_predictor.sam_model.checkpoint=null",
                            # the reduced SAM geometry of tests/test_dropin_configs.py
                            "model.sam_predictor.sam_model.image_encoder.depth=2", "model.sam_predictor.sam_model.image_encoder.embed_dim=64",
                            "model.sam_predictor.sam_model.image_encoder.num_heads=2", "model.sam_predictor.sam_model.image_encoder.window_size=6",
                            "model.sam_predictor.sam_model.image_encoder.global_attn_indexes=[1]", "model.sam_predictor.sam_model.image_size=256",
                            "model.sam_predictor.sam_model.image_embedding_size=16",
                            "model.iterative_refinement_iterations=1", f"model.positive_points_per_mask={N_POS}",
                            "model.negative_points_per_mask=0", "model.sam_iou_threshold=-1.0e+9",
                            "+model.point_tracker.state_dict=null", "+model.sam_predictor.sam_model.precision=f32"] + list(extra))
    return H.resolve(cfg, cwd="/nonexistent")["model"]


@needs_ref
def test_unchanged_reference_sampt_runs_with_the_tapnet_tracker(monkeypatch, sd, sam, clip, restated_adapter):
    from oracle import reference_loader as RL
    from sam_pt_amd.point_tracker import TapnetPointTracker
    RefSamPt = RL.load_sam_pt()
    tcfg, ssd = sam
    frames, qp = clip
    fake = fake_hip_tapnet.install(monkeypatch, sd, ssd, tcfg)
    cfg = _compose()
    assert cfg["_target_"] == "sam_pt.modeling.sam_pt.SamPt"                 # untouched: the reference class itself
    assert cfg["point_tracker"]["visibility_threshold"] == 0.5               # tapnet.yaml's own keys reach our constructor
    cfg["point_tracker"]["state_dict"], cfg["sam_predictor"]["sam_model"]["state_dict"] = sd, ssd
    model = H.instantiate(cfg).eval()
    assert type(model) is RefSamPt and type(model.point_tracker) is TapnetPointTracker
    out = model({"image": [f for f in frames], "target_hw": HW, "query_points": qp})
    want_t, want_v = restated_adapter
    assert out["trajectories"].shape == (T_CLIP, 2, N_POS, 2) and torch.equal(out["trajectories"], want_t)
    assert torch.equal(out["visibilities"].bool(), want_v)
    # ... which is also what the reference's OWN adapter hands over for the same model
    ref_t, ref_v = R.reference_tracker(R.model_fn(sd), 0.5).forward(frames[None], qp.reshape(1, -1, 3))
    assert torch.equal(ref_t[0].reshape(T_CLIP, 2, N_POS, 2), out["trajectories"]) and torch.equal(ref_v[0].reshape(T_CLIP, 2, N_POS), want_v)
    assert len(out["logits"]) == 2 and torch.isfinite(torch.stack(list(out["logits"]))).all()
    _check_tracker_calls(fake, 1)                                            # both objects' points in ONE device call
    assert fake.calls["tapnet_track_frames"] == T_CLIP and fake.calls["vit_encode_frames"] >= T_CLIP


def test_our_sampt_runs_with_the_tapnet_tracker(monkeypatch, sd, sam, clip, restated_adapter):
    from sam_pt_amd.point_tracker import TapnetPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    tcfg, ssd = sam
    frames, qp = clip
    fake = fake_hip_tapnet.install(monkeypatch, sd, ssd, tcfg)
    model = SamPt(TapnetPointTracker(state_dict=sd), SamPredictor(SamHip(config=tcfg, state_dict=ssd, precision="f32")),
                  sam_iou_threshold=-1e9, positive_points_per_mask=N_POS, negative_points_per_mask=0,
                  iterative_refinement_iterations=1).eval()
    out = model({"image": [f for f in frames], "target_hw": HW, "query_points": qp})
    want_t, want_v = restated_adapter
    assert torch.equal(out["trajectories"], want_t) and torch.equal(out["visibilities"].bool(), want_v)
    assert len(out["logits"]) == 2 and torch.isfinite(torch.stack(list(out["logits"]))).all()
    _check_tracker_calls(fake, 1)
    assert model.point_tracker.stats == {"clips": 1, "launches": 3 * 1 + 30}
