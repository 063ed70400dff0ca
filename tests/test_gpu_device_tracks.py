"""``SamPt(device_tracks=True)`` end to end on the GPU: tracker results left on the device, border rule and prompt assembly there,
against the default mode of the same model — bitwise, since the chains get the same items, counts, slots and prompts.  The clip is the
smallest one the module tests run PIPS and CoTracker on (5 frames of 128 x 256)."""
import pytest
import torch

from tests.util import disc_queries, synthetic_clip

pytestmark = pytest.mark.gpu

T, HW = 5, (128, 256)


@pytest.fixture(scope="module")
def pred(dev):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.weights import SAM_CONFIGS
    return SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32", max_batch=4, max_decode_batch=4).to(dev))


@pytest.fixture(scope="module")
def trackers():
    from sam_pt_amd.point_tracker import CoTrackerPointTracker, PipsPointTracker
    return {"pips": PipsPointTracker(seed=72),
            "cotracker": CoTrackerPointTracker(seed=72, interp_shape=(96, 128), visibility_threshold=0.7, support_grid_size=2,
                                               support_grid_every_n_frames=12)}


def make_video(dev, n_objects, n_points, border_object=False):
    """Objects on and around the moving disc; ``border_object``: the last one sits on the left border, where the border rule marks
    its points OUTSIDE_FRAME on the query frame at least (x / W < 0.01)."""
    frames, centres = synthetic_clip(T=T, H=HW[0], W=HW[1], seed=72)
    offsets = [(0.0, 0.0), (-50.0, 20.0), (100.0, -30.0)]
    q = torch.stack([disc_queries(centres, n_pos=n_points, r=9.0 - 2 * i) + torch.tensor([0.0, *offsets[i]]) for i in range(n_objects)])
    if border_object:
        q[-1, :, 1] = 0.5 + 0.2 * torch.arange(n_points)
        q[-1, :, 2] = 30.0 + 8.0 * torch.arange(n_points)
    return {"image": [f.to(dev) for f in frames], "target_hw": HW, "query_points": q}


def both_modes(tracker, pred, **kw):
    from sam_pt_amd.sam_pt import SamPt
    base = dict(sam_iou_threshold=0.1, positive_points_per_mask=4, iterative_refinement_iterations=2)
    base.update(kw)
    return SamPt(tracker, pred, **base).eval(), SamPt(tracker, pred, device_tracks=True, **base).eval()


def assert_same(a, b):
    assert torch.equal(torch.stack(a["logits"]), torch.stack(b["logits"]))
    assert a["scores"] == b["scores"] and a["scores_per_frame"] == b["scores_per_frame"]
    assert not a["trajectories"].is_cuda and not a["visibilities"].is_cuda           # CPU tensors, as in the reference
    assert a["trajectories"].dtype == b["trajectories"].dtype and a["visibilities"].dtype == b["visibilities"].dtype
    assert torch.equal(a["trajectories"], b["trajectories"]) and torch.equal(a["visibilities"], b["visibilities"])


def spy_on_counts(model):
    """How many clips of ``model`` took their prompts' counts from the device."""
    seen = []
    inner = model._prompt_counts_on_device
    model._prompt_counts_on_device = lambda *a, **k: (seen.append(1), inner(*a, **k))[1]
    return seen


@pytest.mark.parametrize("neg", [0, 1])
@pytest.mark.parametrize("n_objects", [1, 3])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["pips", "cotracker"])
def test_device_tracks_equal_the_default_mode(dev, pred, trackers, name, use_graph, n_objects, neg):
    default, device = both_modes(trackers[name], pred, negative_points_per_mask=neg)
    video = make_video(dev, n_objects, 4 + neg)
    seen = spy_on_counts(device)
    keep = pred.use_graph
    pred.use_graph = use_graph
    try:
        want = default(video)
        for rep in range(3 if use_graph else 1):       # (a signature's first sight is eager, then captured, then replayed)
            assert_same(device(video), want)
        torch.cuda.synchronize()
    finally:
        pred.use_graph = keep
    assert len(seen) == (3 if use_graph else 1), "the mode fell back to the host path"
    assert trackers[name].results_on_device is False              # set around the mode's calls only


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["pips", "cotracker"])
def test_empty_prompts_keep_minus_inf(dev, pred, trackers, name, use_graph):
    """Other objects' positives are not appended and one object sits on the border: its items without a visible point are not
    decoded and keep -inf, in both modes alike."""
    default, device = both_modes(trackers[name], pred, negative_points_per_mask=0, add_other_objects_positive_points_as_negative_points=False,
                                 sam_iou_threshold=-1e9)
    video = make_video(dev, 3, 4, border_object=True)
    seen = spy_on_counts(device)
    keep = pred.use_graph
    pred.use_graph = use_graph
    try:
        want = default(video)
        got = device(video)
        torch.cuda.synchronize()
    finally:
        pred.use_graph = keep
    spf = torch.tensor(want["scores_per_frame"])
    assert (spf == -float("inf")).any() and torch.isfinite(spf).any(), "the clip was meant to have an empty and a non-empty prompt"
    empty = (spf == -float("inf")).T                                                 # (M, T)
    assert (torch.stack(got["logits"])[empty.to(dev)] == -float("inf")).all()
    assert_same(got, want)
    assert len(seen) == 1


@pytest.mark.parametrize("name", ["pips", "cotracker"])
def test_patch_filter_runs_on_the_device(dev, pred, trackers, name):
    """With the filter on, the mode's visibilities are ``patch_similarity_filter(..., border_rule=True)`` of the tracker's own
    ``forward`` output, and its logits are those of the host assembly fed exactly those tracks."""
    from sam_pt_amd.patch_filter import patch_similarity_filter
    from sam_pt_amd.sam_pt import SamPt
    from tests.patch_filter_ref import StubTracker
    trk = trackers[name]
    M, P = 3, 5
    kw = dict(negative_points_per_mask=1, patch_size=3, patch_similarity_threshold=0.3)
    _, device = both_modes(trk, pred, use_patch_matching_filtering=True, **kw)
    video = make_video(dev, M, P)
    device.encoder_gemm_workgroups_beside_tracker = 28             # (the default depends on the tracker's class: pin it for both runs)
    seen = spy_on_counts(device)
    got = device(video)
    assert len(seen) == 1
    frames = torch.stack(video["image"])
    q = video["query_points"].reshape(1, M * P, 3).to(dev)
    with torch.no_grad():
        traj, vis = trk(frames[None], q)
    codes = patch_similarity_filter(frames, q[0], traj[0], vis[0].float(), 3, 0.3, border_rule=True)
    assert torch.equal(got["visibilities"], codes.cpu().reshape(T, M, P))
    assert torch.equal(got["trajectories"], traj[0].cpu().reshape(T, M, P, 2))      # (target_hw is the frame size: factor 1)
    assert (codes == 1).any() and (codes != 1).any()
    # the host path of the same tree, handed those tracks (its border rule marks the same points again)
    host = SamPt(StubTracker(traj[0].cpu(), codes.cpu()), pred, sam_iou_threshold=0.1, positive_points_per_mask=4,
                 iterative_refinement_iterations=2, negative_points_per_mask=1).eval()
    host.encoder_gemm_workgroups_beside_tracker = 28
    want = host(video)
    torch.cuda.synchronize()
    assert torch.equal(want["visibilities"], got["visibilities"])
    assert torch.equal(torch.stack(got["logits"]), torch.stack(want["logits"])) and got["scores_per_frame"] == want["scores_per_frame"]


@pytest.mark.parametrize("name", ["pips", "cotracker"])
def test_forward_begin_and_end_equal_forward(dev, pred, trackers, name):
    default, device = both_modes(trackers[name], pred, negative_points_per_mask=1)
    videos = [make_video(dev, 3, 5), make_video(dev, 1, 5), make_video(dev, 3, 5, border_object=True)]
    want = [default(v) for v in videos]
    handle = device.forward_begin(videos[0])
    assert_same(device.forward_end(handle), want[0])
    for a, b in zip(device.stream(videos), want):                  # one clip in flight ahead of the one being collected
        assert_same(a, b)
    torch.cuda.synchronize()
