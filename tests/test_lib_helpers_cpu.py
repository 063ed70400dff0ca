"""CPU tests of what the Python wrappers share in ``sam_pt_amd._lib``: the workspace query, the chunk plan of a bounded workspace
and the owner of the native engines — over the recording fake of tests/fake_hip.py (no GPU, no library)."""
import gc
import itertools

import pytest
import torch

from tests import fake_hip
from tests.util import disc_queries, synthetic_clip


def test_chunk_plan_equals_the_formulas_it_replaced():
    """``chunk_plan`` against the formulas as jf_counts_device, jf_pairs_counts_device and rle_encode_device spelled them out,
    over workspaces below / at / above one item and caps below / above the whole stack."""
    from sam_pt_amd import _lib
    for per, n in itertools.product((16, 1000, 1 << 20), (1, 2, 7, 4096)):
        for given, cap, mc in itertools.product((None, per - 1, per, 3 * per + 5, n * per), (per // 2, 5 * per, 1 << 28), (None, 1, 3)):
            workspace_bytes = given
            if workspace_bytes is None:
                workspace_bytes = max(per, min(n * per, cap))
            chunk = max(1, min(n, int(workspace_bytes) // per))
            if mc is not None:
                chunk = max(1, min(n, int(workspace_bytes) // per, mc))
            assert _lib.chunk_plan(per, n, given, cap, "who", 3, 5, max_chunk=mc) == (workspace_bytes, chunk), (per, n, given, cap, mc)
    assert _lib.chunk_plan(16, 7, 15, 1 << 28, "who", 3, 5) == (15, 1)      # less than one item: still planned, the call refuses it
    with pytest.raises(_lib.SamptError, match=r"who: h \* w must be below 2\^31; got 70000 x 40000$"):
        _lib.chunk_plan(0, 4, None, 1 << 28, "who", 70000, 40000)


def test_workspace_serves_both_forms_of_the_query(monkeypatch):
    from sam_pt_amd import _lib
    fake = fake_hip.install(monkeypatch)
    cpu = torch.device("cpu")
    ws = _lib.workspace("sampt_pips_fnet_workspace_bytes", cpu, None, 4, 64, 96)          # size through the out-parameter
    assert ws.dtype == torch.uint8 and ws.shape == (256,) and ws.device == cpu
    assert _lib.workspace_bytes("sampt_pips_fnet_workspace_bytes", None, 4, 64, 96) == 256
    ws = _lib.workspace("sampt_rle_decode_workspace_bytes", cpu, 100)                        # size as the result
    assert ws.dtype == torch.uint8 and ws.shape == (800,)
    assert _lib.workspace("sampt_rle_decode_workspace_bytes", cpu, 1).shape == (16,)         # the floor ...
    assert _lib.workspace("sampt_rle_decode_workspace_bytes", cpu, 1, min_bytes=256).shape == (256,)
    assert _lib.workspace("sampt_rle_decode_workspace_bytes", cpu, 100, min_bytes=256).shape == (800,)   # ... never a ceiling
    assert _lib.workspace_bytes("sampt_rle_decode_workspace_bytes", 0) == 0                  # the size alone has no floor
    fake.sampt_pips_fnet_workspace_bytes = lambda h, nf, H, W, out: -3
    with pytest.raises(_lib.SamptError, match="sampt_pips_fnet_workspace_bytes failed with code -3"):
        _lib.workspace("sampt_pips_fnet_workspace_bytes", cpu, None, 4, 64, 96)
    with pytest.raises(KeyError):
        _lib.workspace("sampt_no_such_workspace_bytes", cpu, 1)
    with pytest.raises(_lib.SamptError, match="not a workspace query"):
        _lib.workspace("sampt_pips_destroy", cpu, None)


def test_a_moved_tracker_destroys_its_old_engine(monkeypatch):
    from sam_pt_amd.point_tracker import CoTrackerPointTracker, PipsPointTracker
    from sam_pt_amd.weights import init_cotracker_state_dict, init_pips_state_dict
    fake = fake_hip.install(monkeypatch)
    cpu = torch.device("cpu")
    trk = PipsPointTracker(state_dict=init_pips_state_dict(1))
    trk._ensure(cpu)
    h = trk._h
    trk._ensure(cpu)
    assert fake.calls["pips_create"] == 1 and trk._h is h and trk._device == cpu and trk._lib is fake
    trk._device = torch.device("meta")                        # as if the engine had been built for another device
    trk._ensure(cpu)
    assert fake.calls["pips_create"] == 2 and fake.calls["pips_destroy"] == 1 and trk.engines_destroyed == 1
    assert trk._h.value != h.value and trk._device == cpu
    del trk
    gc.collect()
    assert fake.calls["pips_destroy"] == 2
    co = CoTrackerPointTracker(state_dict=init_cotracker_state_dict(1))
    co._ensure(cpu)
    co._pos[(1, 1)] = (torch.zeros(1), torch.zeros(1))
    co._ensure(cpu)
    assert len(co._pos) == 1                                  # nothing moved: the tables stay
    co.forget_engine_device()
    co._ensure(cpu)
    assert fake.calls["cotracker_create"] == 2 and fake.calls["cotracker_destroy"] == 1 and co._pos == {}


def test_a_moved_predictor_destroys_its_old_engines_and_caches(monkeypatch):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    fake = fake_hip.install(monkeypatch, sd, cfg)
    pred = SamPredictor(SamHip(config=cfg, state_dict=sd, precision="f32"))
    pred._ensure()
    vit, dec = pred._vit, pred._dec
    pred._ensure()
    assert (fake.calls["vit_create"], fake.calls["dec_create"]) == (1, 1) and pred._vit is vit and pred._dec is dec
    frames, _ = synthetic_clip(T=1, H=128, W=256, seed=3)
    pred.set_features(pred.encode_frames(frames)[0], (128, 256))
    pred._dec_ws(128, 256)
    pred._ws_hq = pred._ws_pts = pred._ws_score = (1, torch.zeros(16, dtype=torch.uint8))
    assert pred.is_image_set and pred._ws_vit and pred._ws_dec
    pred._dev = torch.device("meta")
    pred._ensure()
    assert (fake.calls["vit_create"], fake.calls["dec_create"]) == (2, 2)
    assert (fake.calls["vit_destroy"], fake.calls["dec_destroy"]) == (1, 1) and pred.engines_destroyed == 2
    assert pred._vit.value != vit.value and pred._dec.value != dec.value and pred._dev == torch.device("cpu")
    assert pred._ws_vit == {} and pred._ws_dec == {} and pred._ws_hq is None and pred._ws_pts is None and pred._ws_score is None
    assert not pred.is_image_set
    del pred
    gc.collect()
    assert (fake.calls["vit_destroy"], fake.calls["dec_destroy"]) == (2, 2)


def test_sampt_forward_makes_the_native_calls_it_made_before(monkeypatch):
    """The fake's call counter for one ``SamPt.forward`` (PIPS + SAM, fused device protocol) on a 4-frame clip.  The literal was
    recorded on the commit before the wrappers' shared helpers were introduced."""
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
    tcfg = SAM_CONFIGS["vit_test"]
    sd, psd = init_sam_state_dict(tcfg, 72), init_pips_state_dict(72)
    fake = fake_hip.install(monkeypatch, sd, tcfg, psd)
    frames, centres = synthetic_clip(T=4, H=128, W=256, seed=3)
    video = {"image": [f for f in frames], "target_hw": (128, 256), "query_points": disc_queries(centres, n_pos=4, r=9.0)[None]}
    model = SamPt(PipsPointTracker(state_dict=psd), SamPredictor(SamHip(config=tcfg, state_dict=sd, precision="f32")),
                  sam_iou_threshold=-1e9, positive_points_per_mask=4, negative_points_per_mask=0,
                  iterative_refinement_iterations=1).eval()
    model(video)
    assert dict(fake.calls) == {"dec_create": 1, "pips_create": 1, "pips_fnet_frames": 4, "pips_sample_feat": 1, "pips_update": 3,
                                "pips_update_points": 12, "sam_track_decode": 1, "sam_track_decode_items": 4, "vit_create": 1,
                                "vit_encode_frames": 4}


def test_a_predictor_whose_decoder_fails_to_build_still_gives_the_encoder_back(monkeypatch):
    from sam_pt_amd import _lib
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    fake = fake_hip.install(monkeypatch, sd, cfg)
    good = fake.sampt_dec_create
    fake.sampt_dec_create = lambda *a: -2
    pred = SamPredictor(SamHip(config=cfg, state_dict=sd, precision="f32"))
    with pytest.raises(_lib.SamptError, match="sampt_dec_create failed with code -2"):
        pred._ensure()
    assert pred._vit is not None and pred._dec is None and pred._dev is None
    fake.sampt_dec_create = good
    pred._ensure()                                            # the half-built predictor is replaced as a whole
    assert (fake.calls["vit_create"], fake.calls["vit_destroy"], fake.calls["dec_create"]) == (2, 1, 1) and pred._dec is not None
    fake.sampt_dec_create = lambda *a: -2
    other = SamPredictor(SamHip(config=cfg, state_dict=sd, precision="f32"))
    with pytest.raises(_lib.SamptError):
        other._ensure()
    del other
    gc.collect()
    assert fake.calls["vit_destroy"] == 2
