"""SuperGlue point tracker on the device (csrc/superglue.hip, csrc/engine_superglue.hip) against tests/golden/superglue_ref.npz —
recorded from the reference's own tracker — and against the restatement of tests/superglue_ref.py run live on the CPU (the
reference tree does not exist where these tests run; tests/test_superglue_cpu.py pins the restatement to it).

Tolerances: the ``bar_*`` entries of the golden file = 8 x the reference's own arithmetic noise at the test shape (f32 against
float64 and against a 1e-7 relative weight perturbation, whichever is larger; tools/make_superglue_golden.py), separately for the
score map, the sampled descriptors, the GNN output, the transport matrix and the matching scores.  Single kernels are held to
the fp32 grade of the project's kernel tests, 2e-5 x max |reference|; the non-maximum suppression is equality on f32 and is
compared with ==."""
import ctypes as C

import numpy as np
import pytest
import torch

from sam_pt_amd.weights import init_superglue_state_dict, init_superpoint_state_dict
from tests import superglue_ref as R
from tests.util import max_abs

pytestmark = pytest.mark.gpu
FP32_GRADE = 2e-5


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return {k: v for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def sds():
    return init_superpoint_state_dict(R.GOLDEN_WEIGHT_SEED), init_superglue_state_dict(R.GOLDEN_WEIGHT_SEED)


def make_tracker(sds, config=None, **kw):
    from sam_pt_amd.point_tracker import SuperGluePointTracker
    return SuperGluePointTracker(R.GOLDEN_POS, R.GOLDEN_NEG, [-1, -1], config or R.GOLDEN_CONFIG, state_dicts=sds, **kw)


@pytest.fixture(scope="module")
def tracker(sds):
    return make_tracker(sds)


@pytest.fixture(scope="module")
def restated(sds):
    """The restatement on the golden clip, computed once: (trajectories, visibilities, per-frame SuperPoint, per-pair SuperGlue)."""
    frames, masks, q = R.golden_clip()
    np.random.seed(R.GOLDEN_NP_SEED)
    return R.track(sds[0], sds[1], frames, masks, q, detail=True)


@pytest.fixture(scope="module")
def detected(dev, tracker):
    frames, _, _ = R.golden_clip()
    det = tracker.detect(frames.to(dev), return_dense=True)
    torch.cuda.synchronize()
    return det


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def S():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def check(rc, what):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


def device_nms(lib, dev, dense, radius, thr, border, cap):
    """dense (n, Hs, Ws) f32 -> (rc, counts list, kpts (n,cap,2), scores (n,cap)) through sampt_sg_nms."""
    n, Hs, Ws = dense.shape
    d = dense.contiguous().to(dev)
    kp = torch.full((n, cap, 2), -7.0, device=dev)
    sc = torch.full((n, cap), -7.0, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    host = (C.c_int * n)()
    ws = torch.empty(lib.sampt_sg_nms_workspace_bytes(n, Hs, Ws), dtype=torch.uint8, device=dev)
    rc = lib.sampt_sg_nms(P(d), n, Hs, Ws, radius, thr, border, cap, P(kp), P(sc), P(cnt), host, P(ws), ws.numel(), S())
    torch.cuda.synchronize()
    return rc, [int(c) for c in host], kp.cpu(), sc.cpu()


# ------------------------------------------------------------------------------------------ kernels
def test_nms_and_compaction_equal_the_restatement(dev, lib, restated):
    """Given the restatement's own f32 score maps, keypoints, their order and their scores are == (three frames in one call)."""
    sp = restated[2]
    cfg = R.GOLDEN_CONFIG["superpoint"]
    dense = torch.stack([s["dense"] for s in sp])
    rc, counts, kp, sc = device_nms(lib, dev, dense, cfg["nms_radius"], cfg["keypoint_threshold"], cfg["remove_borders"], 512)
    assert rc == 0
    for t, s in enumerate(sp):
        n = len(s["keypoints"])
        assert counts[t] == n
        assert torch.equal(kp[t, :n], s["keypoints"]) and torch.equal(sc[t, :n], s["scores"])
        assert (kp[t, n:] == -7).all() and (sc[t, n:] == -7).all()              # nothing beyond the count is written


@pytest.mark.parametrize("radius,border", [(2, 1), (1, 0), (4, 4), (0, 0)])
def test_nms_ties_on_a_hand_made_map(dev, lib, radius, border):
    """24 x 24 with equal neighbours: a plateau, two equal peaks closer than the window, equal peaks two windows apart (kept by the
    second suppression round), a peak on the border and a value exactly at the threshold (> is strict)."""
    s = torch.zeros(24, 24)
    s[3:6, 3:6] = 0.5                              # plateau: every pixel equals its window maximum
    s[10, 10] = s[10, 12] = 0.8                    # equal peaks inside one window
    s[18, 4] = 0.9
    s[18, 7] = 0.6                                 # suppressed by the 0.9 at radius >= 3, a survivor of round 2 otherwise
    s[18, 11] = 0.6
    s[0, 20] = 0.7                                 # on the border
    s[12, 20] = 0.25                               # exactly the threshold
    s[20, 20] = 0.25 + 2.0 ** -20
    s[14:17, 14] = torch.tensor([0.3, 0.31, 0.3])
    want_k, want_s = R.keypoints_from_scores(s, radius, 0.25, border)
    rc, counts, kp, sc = device_nms(lib, dev, s[None], radius, 0.25, border, 600)
    assert rc == 0 and counts[0] == len(want_k) > 3
    assert torch.equal(kp[0, :counts[0]], want_k) and torch.equal(sc[0, :counts[0]], want_s)


def test_capacity_overflow_returns_its_error_code(dev, lib, restated):
    """More keypoints than a deliberately small capacity: SAMPT_ERR_CAPACITY, the true count reported, nothing written beyond
    the capacity, nothing truncated silently."""
    from sam_pt_amd import _lib
    s = restated[2][0]
    cfg = R.GOLDEN_CONFIG["superpoint"]
    n = len(s["keypoints"])
    rc, counts, kp, sc = device_nms(lib, dev, s["dense"][None], cfg["nms_radius"], cfg["keypoint_threshold"], cfg["remove_borders"], 50)
    assert rc == _lib.ERR_CAPACITY and counts[0] == n > 50
    assert b"capacity" in lib.sampt_last_error()
    assert torch.equal(kp[0], s["keypoints"][:50])
    rc, counts, _, _ = device_nms(lib, dev, s["dense"][None], cfg["nms_radius"], cfg["keypoint_threshold"], cfg["remove_borders"], n)
    assert rc == 0 and counts[0] == n                                          # exactly full is not an overflow


def test_tracker_refuses_a_clip_beyond_its_capacity(dev, sds):
    from sam_pt_amd._lib import SamptError
    frames, masks, q = R.golden_clip()
    trk = make_tracker(sds, keypoint_capacity=64)
    trk.set_masks(masks)
    with pytest.raises(SamptError, match="capacity"):
        trk.forward(frames[None].to(dev), q.to(dev))
    torch.cuda.synchronize()


def test_descriptor_sampling_fp32_grade(dev, lib, gold, restated):
    """The golden keypoints of frame 1 plus points on the first and last valid row and column of the 72 x 104 score map."""
    s = restated[2][1]
    dmap = s["dmap"]                                                            # (256, 9, 13)
    _, h8, w8 = dmap.shape
    extra = torch.tensor([[0.0, 0.0], [103.0, 0.0], [0.0, 71.0], [103.0, 71.0], [103.0, 33.0], [51.0, 71.0], [100.0, 68.0], [3.0, 4.0]])
    kp = torch.cat([torch.from_numpy(gold["kpts1"]), extra])
    want = R.sample_descriptors(dmap, kp).t().contiguous()                      # (n, 256)
    out = torch.empty(len(kp), 256, device=dev)
    nhwc = dmap.permute(1, 2, 0).reshape(h8 * w8, 256).contiguous().to(dev)
    check(lib.sampt_sg_sample_descriptors(P(nhwc), h8, w8, P(kp.contiguous().to(dev)), len(kp), P(out), S()), "sample_descriptors")
    assert max_abs(out, want) <= FP32_GRADE * float(want.abs().max())
    assert max_abs(out.norm(dim=1), torch.ones(len(kp))) < 1e-5


@pytest.mark.parametrize("N,M", [(1, 130), (67, 64), (200, 131)])
def test_ragged_attention_fp32_grade(dev, lib, N, M):
    g = torch.Generator().manual_seed(100 * N + M)
    q, k, v = (torch.randn(4, n, 64, generator=g) * 1.5 for n in (N, M, M))
    want = R.attention(q, k, v).permute(1, 0, 2).reshape(N, 256)
    rows = [t.permute(1, 0, 2).reshape(-1, 256).contiguous().to(dev) for t in (q, k, v)]     # blocked heads: channel h * 64 + d
    out = torch.full((N, 256), float("nan"), device=dev)
    check(lib.sampt_sg_attention(P(rows[0]), P(rows[1]), P(rows[2]), P(out), N, M, 4, S()), "attention")
    assert max_abs(out, want) <= FP32_GRADE * float(want.abs().max())


def transport_from_uv(scores, alpha, u, v):
    """Z (N + 1, M + 1) from Sinkhorn's u and v in f32, term by term as the restatement forms it."""
    n, m = scores.shape
    Z = torch.full((n + 1, m + 1), float(alpha))
    Z[:n, :m] = scores
    norm = -(torch.tensor(float(n)) + torch.tensor(float(m))).log()
    return Z + u[:, None] + v[None, :] - norm


def device_sinkhorn(lib, dev, scores, alpha, iters):
    n, m = scores.shape
    u, v = torch.empty(n + 1, device=dev), torch.empty(m + 1, device=dev)
    sd, bd = scores.contiguous().to(dev), torch.tensor([float(alpha)], device=dev)
    check(lib.sampt_sg_sinkhorn(P(sd), n, m, P(bd), iters, P(u), P(v), S()), "sinkhorn")
    return sd, u, v


@pytest.mark.parametrize("iters", [20, 100])
@pytest.mark.parametrize("case", ["golden", "1x1", "3x70", "70x3"])
def test_sinkhorn_and_mutual_match(dev, lib, gold, restated, sds, case, iters):
    """u, v of the device loop rebuild the restatement's transport matrix within bar_sinkhorn; the mutual-match pass over the
    same S, u, v equals the restatement's rule applied to that matrix."""
    if case == "golden":
        scores, alpha = restated[3][0]["scores"], float(sds[1]["bin_score"])
    else:
        n, m = (int(x) for x in case.split("x"))
        scores, alpha = torch.randn(n, m, generator=torch.Generator().manual_seed(n * 100 + m)) * 3, 0.7
    want = R.log_optimal_transport(scores, torch.tensor(alpha), iters)
    sd, u, v = device_sinkhorn(lib, dev, scores, alpha, iters)
    Z = transport_from_uv(scores, alpha, u.cpu(), v.cpu())
    assert max_abs(Z, want) <= float(gold["bar_sinkhorn"])
    n, m = scores.shape
    m0 = torch.empty(n, dtype=torch.int32, device=dev)
    s0 = torch.empty(n, device=dev)
    ws = torch.empty((2 * n + m) * 4, dtype=torch.uint8, device=dev)
    check(lib.sampt_sg_mutual_match(P(sd), n, m, P(u), P(v), 0.2, P(m0), P(s0), P(ws), ws.numel(), S()), "mutual_match")
    want_m, want_s = R.matches_from_transport(Z, 0.2)
    near = (want_s - 0.2).abs() < 2e-6                                          # exp differs by an ulp between the two
    assert torch.equal(m0.cpu()[~near], want_m[~near])
    assert max_abs(s0, want_s) <= 2e-6            # one ulp of norm (|norm| < 8) and of exp on scores <= 1


def test_zero_keypoint_branch(dev, lib, tracker, detected):
    m0 = torch.full((5,), 3, dtype=torch.int32, device=dev)
    s0 = torch.full((5,), 3.0, device=dev)
    check(lib.sampt_sg_mutual_match(None, 5, 0, None, None, 0.2, P(m0), P(s0), None, 0, S()), "mutual_match")
    assert (m0.cpu() == -1).all() and (s0.cpu() == 0).all()
    check(lib.sampt_sg_mutual_match(None, 0, 5, None, None, 0.2, None, None, None, 0, S()), "mutual_match")
    det = dict(detected, counts=[detected["counts"][0], 0, detected["counts"][2]])        # frame 1 without keypoints
    m, s = tracker.match(det, 1)
    assert len(m) == det["counts"][0] and (m.cpu() == -1).all() and (s.cpu() == 0).all()


# ------------------------------------------------------------------------------------------ end to end, step by step
def test_score_map_keypoints_and_descriptors(dev, gold, restated, detected):
    sp = restated[2]
    dense = detected["dense"].cpu()
    assert dense.shape == (3, 72, 104)
    for t in range(3):
        assert max_abs(dense[t], sp[t]["dense"]) <= float(gold["bar_scores"])
        assert max_abs(dense[t][gold["dense_rows"]], torch.from_numpy(gold["dense"][t])) <= float(gold["bar_scores"])
        n = int(gold["counts"][t])
        assert detected["counts"][t] == n
        assert np.array_equal(detected["kpts"][t, :n].cpu().numpy(), gold[f"kpts{t}"])
        assert max_abs(detected["scores"][t, :n], torch.from_numpy(gold[f"kscores{t}"])) <= float(gold["bar_scores"])
        d = detected["desc"][t, :n].cpu()
        assert max_abs(d, sp[t]["descriptors"].t()) <= float(gold["bar_desc"])
        assert max_abs(d[gold[f"desc_cols{t}"]], torch.from_numpy(gold[f"desc{t}"]).t()) <= float(gold["bar_desc"])


@pytest.mark.parametrize("pair", [0, 1])
def test_matching_against_the_golden(dev, gold, tracker, detected, sds, pair):
    m0, s0, gnn, scores, uv = tracker.match(detected, pair + 1, debug=True)
    torch.cuda.synchronize()
    n0 = detected["counts"][0]
    assert max_abs(gnn.cpu()[gold[f"gnn_cols{pair}"]], torch.from_numpy(gold[f"gnn{pair}"]).t()) <= float(gold["bar_gnn"])
    Z = transport_from_uv(scores.cpu(), float(sds[1]["bin_score"]), uv[:n0 + 1].cpu(), uv[n0 + 1:].cpu())
    assert max_abs(Z[gold[f"z_rows{pair}"]], torch.from_numpy(gold[f"Z{pair}"])) <= float(gold["bar_sinkhorn"])
    marginal = gold[f"marginal{pair}"]
    assert len(marginal) <= 0.02 * n0
    keep = np.ones(n0, dtype=bool)
    keep[marginal] = False
    assert np.array_equal(m0.cpu().numpy()[keep], gold[f"matches{pair}"][keep])
    assert max_abs(s0.cpu()[keep], torch.from_numpy(gold[f"mscores{pair}"][keep])) <= float(gold["bar_mscores"])


def test_forward_equals_the_golden_trajectories(dev, gold, tracker, detected):
    """Under the golden NumPy seed, trajectories and visibilities are == the reference's wherever no marginal keypoint changed a
    match: every frame up to the first whose matches differ from the golden ones (later draws would consume the generator
    differently); that is the whole clip when none differs."""
    frames, masks, q = R.golden_clip()
    same = [np.array_equal(tracker.match(detected, p + 1)[0].cpu().numpy(), gold[f"matches{p}"]) for p in range(2)]
    tracker.set_masks(masks.to(dev))
    np.random.seed(int(gold["np_seed"]))
    before = tracker.stats["host_syncs"]
    out = tracker.evaluate_batch(frames[None].to(dev), q.to(dev))
    assert tracker.masks is None and tracker.stats["host_syncs"] - before == 2          # constant, whatever T is
    traj, vis = out["trajectories_pred"], out["visibilities_pred"]
    assert traj.shape == (1, 3, 12, 2) and vis.shape == (1, 3, 12) and vis.dtype == torch.float32
    upto = 1 + (2 if all(same) else (1 if same[0] else 0))
    assert np.array_equal(traj[:, :upto].numpy(), gold["trajectories"][:, :upto])
    assert np.array_equal(vis[:, :upto].numpy(), gold["visibilities"][:, :upto])
    if not all(same):
        for p in range(2):
            diff = np.nonzero(tracker.match(detected, p + 1)[0].cpu().numpy() != gold[f"matches{p}"])[0]
            assert set(diff.tolist()) <= set(gold[f"marginal{p}"].tolist())
    with pytest.raises(AssertionError, match="Masks must be set"):
        tracker.forward(frames[None].to(dev), q.to(dev))


def test_empty_case(dev, sds):
    """keypoint_threshold=0.5: no frame has a keypoint; every later frame is (-1, -1) with visibility 0, frame 0 the query points."""
    frames, masks, q = R.golden_clip()
    cfg = {"superpoint": dict(R.GOLDEN_CONFIG["superpoint"], keypoint_threshold=0.5), "superglue": R.GOLDEN_CONFIG["superglue"]}
    trk = make_tracker(sds, cfg)
    trk.set_masks(masks)
    traj, vis = trk.forward(frames[None].to(dev), q.to(dev))
    assert trk.stats["keypoints"] == [0, 0, 0]
    assert (traj[0, 1:].cpu() == -1).all() and (vis.cpu() == 0).all()
    assert torch.equal(traj[0, 0].cpu(), q[0, :, 1:])


# ------------------------------------------------------------------------------------------ through SamPt
@pytest.mark.parametrize("reinit", [False, True])
def test_through_sam_pt_in_query_points_mode(dev, sds, reinit):
    """The tracker inside sam_pt_amd.sam_pt.SamPt on the reduced SAM geometry the module tests use: set_masks is called with
    masks of the frames' size before every tracker call — once per clip, or once per window when points are re-initialised."""
    from oracle.make_golden import reinit_kwargs, sampt_kwargs, sampt_video
    from sam_pt_amd.point_tracker import SuperGluePointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import SAM_CONFIGS
    from tests.util import synthetic_clip
    frames, centres = synthetic_clip(T=8, H=128, W=256, seed=72)
    trk = SuperGluePointTracker(4, 0, [-1, -1], R.GOLDEN_CONFIG, state_dicts=sds)
    calls = []
    set_masks, forward = trk.set_masks, trk.forward

    def spy_set_masks(m):
        calls.append(("masks", tuple(m.shape)))
        return set_masks(m)

    def spy_forward(rgbs, q):
        calls.append(("forward", tuple(rgbs.shape)))
        return forward(rgbs, q)

    trk.set_masks, trk.forward = spy_set_masks, spy_forward
    kw = reinit_kwargs("reinit-at-median-of-area-diff", 0) if reinit else dict(sampt_kwargs(4, 0), sam_iou_threshold=-1e9)
    model = SamPt(trk, SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32").to(dev)), **kw).eval()
    video = sampt_video(frames, centres, 4, 0)
    np.random.seed(3)
    torch.manual_seed(5)
    out = model({**video, "image": [f.to(dev) for f in video["image"]]})
    kinds = [c[0] for c in calls]
    assert kinds[0::2] == ["masks"] * (len(calls) // 2) and kinds[1::2] == ["forward"] * (len(calls) // 2)    # strictly alternating
    for (_, m), (_, f) in zip(calls[0::2], calls[1::2]):
        assert m[1:] == (128, 256) and 1 <= m[0] <= 2 and f[-2:] == (128, 256)
    assert len(calls) // 2 == (1 if not reinit else len(calls) // 2) and (len(calls) >= 4 if reinit else len(calls) == 2)
    assert out["trajectories"].shape == (8, 2, 4, 2) and out["visibilities"].shape == (8, 2, 4)
    assert len(out["logits"]) == 2 and tuple(out["logits"][0].shape) == (8, 128, 256)
    assert trk.masks is None
