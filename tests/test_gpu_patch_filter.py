"""Patch-similarity filter on the HIP device (sam_pt_amd/patch_filter.py, csrc/patch_filter.hip) against the fixture
tests/golden/patch_filter.npz (the reference's own codes), against the host path run live, and against hand-made clips whose
similarities are exact.  Codes are compared with ==, similarities to bar_sim of the fixture: 8 x the host path's own
float32-against-float64 noise."""
import functools
import types

import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import patch_filter as PF
from sam_pt_amd.sam_pt import SamPt
from tests import patch_filter_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def flat_inputs(g):
    return g["frames"], g["query_points"].reshape(-1, 3), g["trajectories"], g["visibilities_raw"]


def on(dev, *xs):
    return [x.to(dev) for x in xs]


@functools.lru_cache(maxsize=None)
def host_similarities(ps):
    g = R.load_golden()
    frames, q, traj, _ = flat_inputs(g)
    return R.similarities(frames, q, traj, ps)


def test_fixture(dev, gold):
    frames, q, traj, vis = flat_inputs(gold)
    codes, sim = PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), gold["patch_size"], gold["threshold"], border_rule=True,
                                            return_similarities=True)
    worst = float((sim.cpu() - gold["similarities"]).abs().max())
    print(f"similarities: device against the stored host path, max |difference| {worst:.3e} (bar_sim {gold['bar_sim']:.3e})")
    assert torch.equal(codes.cpu(), gold["codes"].reshape(codes.shape))
    assert worst <= gold["bar_sim"]
    # without the similarities the raw-invisible items are skipped: same codes
    again = PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), gold["patch_size"], gold["threshold"], border_rule=True)
    assert torch.equal(again, codes)


@pytest.mark.parametrize("ps", [1, 2, 3, 5, 7, 9])
def test_patch_sizes_against_the_host_path(dev, gold, ps):
    """1, 2, 3 and 5 are the issue's; 7 fills one wave per frame, 9 makes a lane loop over taps.  The threshold goes to the middle of
    the widest gap among the middle half of the host's raw-visible similarities — a condition on the inputs, met by the host alone."""
    frames, q, traj, vis = flat_inputs(gold)
    s = host_similarities(ps)
    ordered = s[vis == 1].sort().values
    n = ordered.numel()
    mid = ordered[n // 4: n - n // 4]
    gaps = mid[1:] - mid[:-1]
    i = int(gaps.argmax())
    assert float(gaps[i]) > 8 * gold["bar_sim"], "the host's similarities leave no room for a threshold"
    thr = float(mid[i] + mid[i + 1]) / 2
    want = R.host_codes(frames, q, traj, vis, ps, thr)
    codes, sim = PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), ps, thr, border_rule=True, return_similarities=True)
    print(f"patch_size {ps}: threshold {thr:.4f} in a gap of {float(gaps[i]):.3e}; similarities max |difference| "
          f"{float((sim.cpu() - s).abs().max()):.3e}")
    assert torch.equal(codes.cpu(), want)
    assert float((sim.cpu() - s).abs().max()) <= gold["bar_sim"]


# ---- scan logic on clips whose similarities are exact: every frame one colour, A or B
COLOUR = {"A": (200, 40, 90), "B": (20, 180, 230)}
SCAN_CASES = {
    # name: (order of the frames' colours, query frame, frames with raw visibility 0, trajectory off the frame AT the query frame)
    "first_hit_forward": ("AAABABAAA", 0, (), False),
    "first_hit_backward": ("AABABAAAA", 8, (), False),
    "both_sides_of_a_middle_query": ("ABAAAABAB", 4, (), False),
    "hit_at_the_query_frame": ("AAAAAAAAA", 4, (), True),
    "hits_at_both_ends": ("BAAAAAAAB", 4, (), False),
    "raw_zero_on_a_b_frame": ("AAABAAAAA", 0, (3,), False),
    "raw_zero_hides_the_first_hit": ("AAABABAAA", 0, (3,), False),
    "single_frame": ("A", 0, (), False),
    "more_frames_than_threads_forward": ("A" * 270 + "B" + "A" * 29, 5, (), False),
    "more_frames_than_threads_backward": ("AAAB" + "A" * 296, 299, (), False),
}


def expected_scan(hit, raw, t0):
    """The loop of sam_pt.py:656-682 for one point: hit[t] = the patch is non-similar."""
    T = len(hit)
    v = [(-3.0 if raw[t] == 1 and hit[t] else float(raw[t])) for t in range(T)]
    for t in range(t0 + 1, T):
        if v[t] == -3:
            v[t + 1:] = [-4.0] * (T - t - 1)
            break
    for t in range(t0 - 1, -1, -1):
        if v[t] == -3:
            v[:t] = [-4.0] * t
            break
    return v


@pytest.mark.parametrize("case", list(SCAN_CASES))
def test_scan_logic_with_exact_similarities(dev, case):
    """Interior points on single-colour frames: a similarity is exactly 1 (same colour as the query frame: the two patches are the
    same arithmetic) or one known value far below the threshold.  A single-colour clip cannot be non-similar AT its query frame, so
    that case parks the trajectory at (-10, -10) on the query frame: every corner lies off the frame and the patch is exact zeros."""
    order, t0, zeros, off_at_query = SCAN_CASES[case]
    T, H, W = len(order), 9, 11
    frames = torch.tensor([COLOUR[c] for c in order], dtype=torch.uint8)[:, :, None, None].expand(T, 3, H, W).contiguous()
    xy = torch.tensor([[5.0, 4.0], [4.25, 3.5]])                                    # integer and fractional, both interior
    q = torch.cat([torch.full((2, 1), float(t0)), xy], dim=1)
    traj = xy[None].repeat(T, 1, 1)
    if off_at_query:
        traj[t0] = -10.0
    raw = torch.ones(T, 2)
    raw[list(zeros)] = 0
    hit = [order[t] != order[t0] or (off_at_query and t == t0) for t in range(T)]
    want = torch.tensor([expected_scan(hit, raw[:, 0].tolist(), t0)] * 2).t()
    codes, sim = PF.patch_similarity_filter(*on(dev, frames, q, traj, raw), 3, 0.01, return_similarities=True)
    assert torch.equal(codes.cpu(), want)
    same = torch.tensor([not h for h in hit])
    assert (sim.cpu()[same] == 1).all() and (sim.cpu()[~same] < 1e-3).all()


def test_border_rule_alone(dev):
    """Threshold -1: everything is similar and only the four comparisons speak.  Coordinates at and next to 0.01 w, 0.99 w, 0.01 h
    and 0.99 h in float32, for sizes where the products are and are not float32 numbers; the expectation is the torch lines on CPU
    tensors (an IEEE division), where the reference evaluates them."""
    for H, W in ((37, 53), (200, 100), (480, 854)):
        edges = []
        for size in (W, H):
            for f in (0.01, 0.99):
                c = torch.tensor(f * size, dtype=torch.float32)
                lo = torch.nextafter(c, torch.tensor(-1e9))
                hi = torch.nextafter(c, torch.tensor(1e9))
                edges += [torch.nextafter(lo, torch.tensor(-1e9)), lo, c, hi, torch.nextafter(hi, torch.tensor(1e9))]
        edges = torch.stack(edges)
        xs, ys = edges[:10], edges[10:]
        mid = torch.tensor([W / 2.0, H / 2.0])
        pts = [torch.stack([x, mid[1]]) for x in xs] + [torch.stack([mid[0], y]) for y in ys] + [mid, torch.tensor([-3.0, 5.0]),
                                                                                                  torch.tensor([W + 2.0, H + 2.0])]
        traj = torch.stack(pts)[None].repeat(2, 1, 1)                               # (2, N, 2)
        N = traj.shape[1]
        q = torch.cat([torch.zeros(N, 1), mid[None].repeat(N, 1)], dim=1)
        vis = torch.ones(2, N)
        frames = torch.full((2, 3, H, W), 128, dtype=torch.uint8)
        want = vis.clone()
        want[traj[:, :, 0] / W < 0.01] = -2
        want[traj[:, :, 1] / H < 0.01] = -2
        want[traj[:, :, 0] / W > 0.99] = -2
        want[traj[:, :, 1] / H > 0.99] = -2
        assert 2 < int((want == -2).sum()) < want.numel() - 2
        codes = PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), 3, -1.0, border_rule=True)
        assert torch.equal(codes.cpu(), want), (H, W)
        assert (PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), 3, -1.0) == 1).all()


def sam_pt_for(dev, gold, tracker, batch):
    pred = types.SimpleNamespace(model=types.SimpleNamespace(device=dev))
    return SamPt(tracker, pred, sam_iou_threshold=0.0, point_tracker_mask_batch_size=batch, use_patch_matching_filtering=True,
                 patch_size=gold["patch_size"], patch_similarity_threshold=gold["threshold"])


def test_track_points_device_and_host_paths(dev, gold, monkeypatch):
    frames, q, traj, vis = flat_inputs(gold)
    calls = []
    real = PF.patch_similarity_filter
    monkeypatch.setattr(PF, "patch_similarity_filter", lambda *a, **k: (calls.append(a[0].device), real(*a, **k))[1])
    results = {}
    for name, batch, on_device, fr in (("device", 5, True, frames), ("device_one_object", 1, True, frames),
                                       ("device_float_frames", 5, True, frames.float()), ("host", 5, False, frames),
                                       ("host_one_object", 1, False, frames)):
        m = sam_pt_for(dev, gold, R.StubTracker(traj, vis, dev), batch)
        m.patch_filter_on_device = on_device
        n_before = len(calls)
        tr, codes = m._track_points(fr, gold["query_points"])
        assert len(calls) - n_before == ((2 if batch == 1 else 1) if on_device else 0), "one launch per tracker call, none when forced to the host"
        assert codes.is_cuda and tr.is_cuda and torch.equal(tr.cpu().reshape(traj.shape), traj)
        results[name] = codes.cpu()
    assert all(d.type == "cuda" for d in calls), "a frame went back to the host"
    for name, codes in results.items():
        assert torch.equal(codes, gold["codes"]), name
    assert SamPt.patch_filter_on_device is True


def test_stream_and_repeat_give_the_same_bits(dev, gold):
    frames, q, traj, vis = on(dev, *flat_inputs(gold))
    args = (frames, q, traj, vis, gold["patch_size"], gold["threshold"])
    a = PF.patch_similarity_filter(*args, border_rule=True, return_similarities=True)
    b = PF.patch_similarity_filter(*args, border_rule=True, return_similarities=True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = PF.patch_similarity_filter(*args, border_rule=True, return_similarities=True)
    side.synchronize()
    for x in (b, c):
        assert torch.equal(x[0], a[0]) and torch.equal(x[1], a[1])
    # non-contiguous inputs are made contiguous; no points, no launch
    wide = torch.zeros(traj.shape[0], traj.shape[1], 4, device=dev)
    wide[..., :2] = traj
    d = PF.patch_similarity_filter(frames, q, wide[..., :2], vis, gold["patch_size"], gold["threshold"], border_rule=True)
    assert torch.equal(d, a[0])
    e, s = PF.patch_similarity_filter(frames, q[:0], traj[:, :0], vis[:, :0], 3, 0.01, return_similarities=True)
    assert e.shape == s.shape == (frames.shape[0], 0) and e.dtype == torch.float32


def test_non_finite_coordinates_are_non_similar(dev, gold):
    """The rule of this project for inputs the host path does not define: no fault, similarity 0, code -3 where raw-visible."""
    frames, q, traj, vis = flat_inputs(gold)
    traj = traj.clone()
    vis = torch.ones_like(vis)
    traj[2, 0, 0], traj[4, 0, 1], traj[5, 0, 0] = float("nan"), float("inf"), 3e38
    codes, sim = PF.patch_similarity_filter(*on(dev, frames, q, traj, vis), 3, 0.01, return_similarities=True)
    assert codes[2, 0] == -3 and sim[2, 0] == 0 and (codes[3:, 0] == -4).all() and (sim[4, 0] == 0) and not (sim[5, 0] > 0.01)
    bad_q = q.clone()
    bad_q[1, 0], bad_q[2, 1] = 99.0, float("nan")
    codes, sim = PF.patch_similarity_filter(*on(dev, frames, bad_q, gold["trajectories"], vis), 3, 0.01, return_similarities=True)
    assert (sim[:, 1:3] == 0).all() and torch.isfinite(sim).all()


def test_refusals_are_named(dev, gold):
    frames, q, traj, vis = on(dev, *flat_inputs(gold))
    f = PF.patch_similarity_filter
    with pytest.raises(_lib.SamptError, match=r"patch_size must be an integer in 1 \.\. 15; got 16"):
        f(frames, q, traj, vis, 16, 0.01)
    with pytest.raises(_lib.SamptError, match="mixed devices: rgbs on cuda:0, trajectories on cpu"):
        f(frames, q, traj.cpu(), vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"trajectories must be \(T, N, 2\) = \(7, 12, 2\)"):
        f(frames, q, traj[:, :5], vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"rgbs must be \(T, 3, H, W\)"):
        f(frames[:, 0], q, traj, vis, 3, 0.01)
    # ... and by the library itself
    lib = _lib.load()
    out = torch.empty_like(vis)
    tab = PF.companding_table().to(dev)

    def call(T=7, H=37, W=53, N=12, ps=3, rgb=frames, out=out):
        return lib.sampt_patch_filter(_lib.ptr(rgb), T, H, W, _lib.ptr(q), _lib.ptr(traj), _lib.ptr(vis), N, ps, 0.01, _lib.ptr(tab), 1,
                                      _lib.ptr(out), None, _lib.stream_ptr())

    assert call() == 0
    for kw, text in ((dict(ps=16), "patch_size must be in 1 .. 15; got 16"), (dict(ps=0), "patch_size"), (dict(T=0), "must be positive"),
                     (dict(N=-1), "must be positive"), (dict(H=0), "must be positive"), (dict(W=0), "must be positive"),
                     (dict(rgb=None), "null pointer"), (dict(out=None), "null pointer")):
        assert call(**kw) == -1
        assert text in lib.sampt_last_error().decode(), kw
    torch.cuda.synchronize()
