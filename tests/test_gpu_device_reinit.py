"""``SamPt(device_reinit=True)``: query points selected from masks that stay on the device (bit-planes, areas to the host, ranks to
``sampt_bits_select``) against the host loop — the same points, the same generator state, the same forward results with
``torch.equal`` — and against the reference's committed outputs with the existing golden test's tolerances."""
import os

import numpy as np
import pytest
import torch

from tests.util import synthetic_clip

pytestmark = pytest.mark.gpu

VARIANTS = ["reinit-on-horizon-and-sync-masks", "reinit-at-median-of-area-diff", "reinit-on-similar-mask-area",
            "reinit-on-similar-mask-area-and-sync-masks"]


@pytest.fixture(scope="module")
def pips_sd():
    from sam_pt_amd.weights import init_pips_state_dict
    return init_pips_state_dict(72)


@pytest.fixture(scope="module")
def clip():
    return synthetic_clip(T=12, H=128, W=256, seed=72)


# ---------------------------------------------------------------------------------------------- step level
def _segment_logits(H=128, W=256):
    """f32 logits of 3 objects x 6 frames of H x W (at least 121 x 215, which holds every shape below): discs of varying radius; blobs
    of at most 25 pixels, some of fewer pixels than points are asked for; an object that is empty from frame 2 on."""
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    masks = torch.zeros(3, 6, H, W, dtype=torch.bool)
    for f, r in enumerate([14, 9, 17, 12, 21, 11]):
        masks[0, f] = ((yy - 60 - f) ** 2 + (xx - 90 - 4 * f) ** 2) <= r * r
    for f, npx in enumerate([25, 2, 25, 9, 2, 3]):
        flat = torch.zeros(5 * 5, dtype=torch.bool)
        flat[torch.randperm(25, generator=g)[:npx]] = True
        masks[1, f, 20 + f:25 + f, 200:205] = flat.view(5, 5)
    masks[2, 0] = (yy > 100) & (xx < 30)
    masks[2, 1] = (yy > 104) & (xx < 26)
    noise = torch.rand(masks.shape, generator=g) + 0.25
    return torch.where(masks, noise, -noise)


def _stub_model(**kw):
    from sam_pt_amd.sam_pt import SamPt

    class Predictor:
        model = torch.nn.Identity()

    class Tracker(torch.nn.Module):
        pass

    return SamPt(Tracker(), Predictor(), sam_iou_threshold=0.0, use_point_reinit=True, reinit_horizon=6, reinit_point_tracker_horizon=6,
                 **kw).eval()


CONFIGS = [dict(positive_point_selection_method=p, positive_points_per_mask=4, negative_points_per_mask=neg) for p in ("random", "kmedoids")
           for neg in (0, 1)] + [dict(positive_point_selection_method="mixed", positive_points_per_mask=12, negative_points_per_mask=0)]


def test_device_step_equals_host_step(dev):
    """One segment's decision and new query points through both routes, four variants x five point settings (the negatives' method
    is the shipped ``mixed``; ``mixed`` at 12 points runs its Shi-Tomasi share with the k-medoid top-up)."""
    logits = _segment_logits().to(dev)
    pred = (logits > 0).cpu()
    frames = torch.randint(0, 256, (5, 3, 128, 256), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(dev)
    branches = {"draw": 0, "repeat": 0, "empty": 0}
    for variant in VARIANTS:
        for cfg in CONFIGS:
            model = _stub_model(reinit_variant=variant, negative_point_selection_method="mixed", **cfg)
            cur_t = torch.tensor([0, 0, 0, 3], dtype=torch.int32)            # a fourth object waits for frame 3
            torch.manual_seed(11)
            q_h, inv_h, upd_h = model._reinit_step(frames, logits, cur_t, 0, False)
            state_h = torch.get_rng_state()
            torch.manual_seed(11)
            q_d, inv_d, upd_d = model._reinit_step(frames, logits, cur_t, 0, True)
            state_d = torch.get_rng_state()
            what = f"{variant} {cfg}"
            assert torch.equal(q_h, q_d) and torch.equal(inv_h, inv_d), what
            assert upd_h is not None and upd_d is not None and upd_h.dtype == upd_d.dtype and upd_h.device == upd_d.device, what
            assert torch.equal(upd_h, upd_d), what
            assert torch.equal(state_h, state_d), what
            # which branches of the selectors the HOST path met on these inputs
            n = cfg["positive_points_per_mask"]
            for j in torch.nonzero(~inv_h).flatten().tolist():
                a = int(pred[j, 1 + int(q_h[j])].sum())
                branches["empty" if a == 0 else "repeat" if a < n else "draw"] += 1
    assert all(v > 0 for v in branches.values()), branches


def test_one_select_launch_per_call(dev):
    """Positives and negatives of every mask go to the device together."""
    from sam_pt_amd.mask_points import planes_of_masks
    from sam_pt_amd.query_points import select_query_points
    masks = (_segment_logits()[:, 0] > 0).float().to(dev)
    src = planes_of_masks(masks)
    frames = torch.zeros((1, 3, 128, 256), dtype=torch.uint8, device=dev)
    torch.manual_seed(1)
    out = select_query_points(src, frames, torch.zeros(3), "kmedoids", 4, "mixed", 1)
    assert src.select_launches == 1 and [tuple(o.shape) for o in out] == [(5, 2)] * 3 and not out[0].is_cuda


# ---------------------------------------------------------------------------------------------- end to end
def _model(dev, pips_sd, kw, **modes):
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import SAM_CONFIGS
    return SamPt(PipsPointTracker(state_dict=pips_sd), SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32").to(dev)),
                 **kw, **modes).eval()


def _run(model, video, dev, count_segments=False):
    segments = []
    if count_segments:
        inner, track = model._forward_w_reinit_inner, model._track_points
        model._forward_w_reinit_inner = lambda *a, **k: (segments.append(0), inner(*a, **k))[1]

        def counted(*a, **k):
            segments[-1] += 1
            return track(*a, **k)
        model._track_points = counted
    torch.manual_seed(5)
    out = model({**video, "image": [f.to(dev) for f in video["image"]]})
    return out, segments


def _assert_same(a, b, what):
    for x, y in zip(a["logits"], b["logits"]):
        assert torch.equal(x, y), what
    assert torch.equal(a["trajectories"], b["trajectories"]) and torch.equal(a["visibilities"], b["visibilities"]), what
    assert np.array_equal(np.array(a["scores"]), np.array(b["scores"]), equal_nan=True), what
    assert np.array_equal(np.array(a["scores_per_frame"]), np.array(b["scores_per_frame"]), equal_nan=True), what


def _compare_modes(dev, pips_sd, frames, kw, video, min_segments, what):
    want, segments = _run(_model(dev, pips_sd, kw), video, dev, count_segments=True)
    assert len(segments) == 2 and all(s >= m for s, m in zip(segments, min_segments)), segments      # re-initialisation happened
    for modes in (dict(device_reinit=True), dict(device_reinit=True, device_tracks=True)):
        model = _model(dev, pips_sd, kw, **modes)
        assert model._device_reinit_active(frames.to(dev)) and model._device_tracks_active(frames.to(dev)) == ("device_tracks" in modes)
        got, _ = _run(model, video, dev)
        _assert_same(got, want, f"{what} {modes}")
        assert not got["trajectories"].is_cuda and not got["visibilities"].is_cuda


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_equals_default_mode(dev, pips_sd, clip, variant):
    """The golden clip's re-initialisation video: four segments forwards.  Its queries sit on frames 0 and 2 of 12, so the flipped
    pass starts on frames 9 and 11 and each object ends inside one horizon of 5: one tracker call per object there, whatever the
    implementation (the test below re-initialises in both directions)."""
    from oracle.make_golden import reinit_kwargs, reinit_video
    frames, centres = clip
    kw, video = reinit_kwargs(variant, 1), reinit_video(frames, centres, 1)
    _compare_modes(dev, pips_sd, frames, kw, video, (3, 2), variant)


@pytest.mark.parametrize("variant", VARIANTS[1:3])
def test_forward_equals_default_mode_both_directions(dev, pips_sd, clip, variant):
    """Queries on frame 5 of 12 and a horizon of 3: a segment covers 3 frames and the next one starts at most 2 frames later
    (q_t <= H - 2), so the forward pass (frames 5 .. 11) and the flipped pass (frames 6 .. 11 of the flipped clip) take at least three
    segments each."""
    from oracle.make_golden import reinit_kwargs, reinit_video
    frames, centres = clip
    kw, video = reinit_kwargs(variant, 1), reinit_video(frames, centres, 1)
    kw.update(reinit_horizon=3, reinit_point_tracker_horizon=4)
    video["query_points"][:, :, 0] = 5
    _compare_modes(dev, pips_sd, frames, kw, video, (3, 3), variant)


@pytest.mark.parametrize("name", ["reinit_median", "reinit_sync"])
def test_device_reinit_vs_reference_golden(dev, pips_sd, clip, name):
    """The assertions of test_gpu_modules.py::test_reinit_and_query_masks_device_path_vs_reference_golden, with ``device_reinit``."""
    from oracle.make_golden import reinit_kwargs, reinit_video
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampt_reinit.npz"))
    frames, centres = clip
    if name == "reinit_median":
        kw, video = reinit_kwargs("reinit-at-median-of-area-diff", 0), reinit_video(frames, centres, 0)
    else:
        kw, video = reinit_kwargs("reinit-on-similar-mask-area-and-sync-masks", 1), reinit_video(frames, centres, 1)
    out, _ = _run(_model(dev, pips_sd, kw, device_reinit=True), video, dev)
    assert np.array_equal(out["visibilities"].numpy(), g[f"{name}_vis"])
    assert np.array_equal(np.round(out["trajectories"].numpy()), np.round(g[f"{name}_traj"]))
    masks = torch.stack([l > 0 for l in out["logits"]]).cpu().numpy()
    ref = np.unpackbits(g[f"{name}_masks"], axis=-1)[..., :masks.shape[-1]].astype(bool)
    inter, union = (masks & ref).sum(axis=(-1, -2)), (masks | ref).sum(axis=(-1, -2))
    assert np.where(union > 0, inter / np.maximum(union, 1), 1.0).min() >= 1 - 1e-3
    assert np.allclose(np.array(out["scores_per_frame"], dtype=np.float32), g[f"{name}_scores_per_frame"], atol=1e-3, equal_nan=True)


@pytest.mark.parametrize("methods", [("random", "random"), ("kmedoids", "mixed")])
def test_query_masks_mode_equals_default_mode(dev, pips_sd, clip, methods):
    from oracle.make_golden import query_mask_video, sampt_kwargs
    frames, centres = clip
    kw = dict(sampt_kwargs(4, 1), positive_point_selection_method=methods[0], negative_point_selection_method=methods[1],
              sam_iou_threshold=-1e9)
    video = query_mask_video(frames[:8], centres)
    video["query_masks"] = video["query_masks"].to(dev)                   # the masks uploaded
    want, _ = _run(_model(dev, pips_sd, kw), video, dev)
    states = []
    for modes in (dict(), dict(device_reinit=True)):                        # the generator ends where the default mode leaves it
        got, _ = _run(_model(dev, pips_sd, kw, **modes), video, dev)
        states.append(torch.get_rng_state())
        _assert_same(got, want, f"{methods} {modes}")
    assert torch.equal(states[0], states[1])
