"""RAFT point tracker on the device (csrc/raft.hip, csrc/engine_raft.hip) against tests/golden/raft_ref.npz — recorded from the
reference's own RAFT — and against the restatement of tests/raft_ref.py run live on the CPU (the reference tree does not exist
where these tests run; tests/test_raft_cpu.py pins the restatement to it).

Flow tolerance: ``bar_px`` of the golden file = 8 x the reference's own arithmetic noise at the test shape (f32 against float64
and against a 1e-7 relative weight perturbation, whichever is larger; tools/make_raft_golden.py).  1/8-resolution flows count
cells of 8 px, so they get bar / 8; trajectories get bar x the number of chained frames.  Single kernels are held to the fp32
grade of the PIPS correlation test: 2e-5 x max |reference|."""
import ctypes as C

import pytest
import torch

from sam_pt_amd.weights import init_raft_state_dict
from tests import raft_ref as R
from tests.util import max_abs, synthetic_clip

pytestmark = pytest.mark.gpu
FP32_GRADE = 2e-5


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def sd():
    return init_raft_state_dict(72)


@pytest.fixture(scope="module")
def tracker(sd):
    from sam_pt_amd.point_tracker import RaftPointTracker
    return RaftPointTracker(state_dict=sd)


@pytest.fixture(scope="module")
def restated(gold, sd):
    """The restatement on the golden clip, computed once: (flows_forward, flows_backward, flow_low)."""
    return R.flows(sd, gold["frames"], int(gold["iters"]))


@pytest.fixture(scope="module")
def device_flows(dev, gold, tracker):
    fwd, bwd, low = tracker.flows(gold["frames"].to(dev), return_low=True)
    torch.cuda.synchronize()
    return fwd.cpu(), bwd.cpu(), low.cpu()


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def S():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


def _lookup(lib, dev, levels, coords):
    from sam_pt_amd import _lib
    lv = [l.reshape(l.shape[0], -1).contiguous().to(dev) for l in levels]
    h8, w8 = levels[0].shape[-2:]
    co = coords.contiguous().to(dev)
    out = torch.full((co.shape[0], 352), float("nan"), device=dev)
    ok(lib.sampt_raft_lookup(_lib.ptr_array(lv), h8, w8, P(co), co.shape[0], P(out), S()), "sampt_raft_lookup")
    torch.cuda.synchronize()
    return out.cpu()


def test_correlation_pyramid(lib, dev, gold, sd):
    """Four levels from one product each against the pooled second map == all-pairs product + avg_pool2d of the volume."""
    from sam_pt_amd import _lib
    p, rows = int(gold["pair"]), gold["rows"].long()
    with torch.no_grad():
        fmap, _, _ = R.features(sd, gold["frames"][p:p + 2])
        want = R.corr_pyramid(fmap[0], fmap[1])
    h8, w8 = fmap.shape[-2:]
    f1, f2 = (fmap[i].permute(1, 2, 0).contiguous().to(dev) for i in (0, 1))
    levels = [torch.full((h8 * w8, w.shape[1] * w.shape[2]), float("nan"), device=dev) for w in want]
    ws = torch.empty(lib.sampt_raft_corr_pyramid_workspace_bytes(h8, w8), dtype=torch.uint8, device=dev)
    ok(lib.sampt_raft_corr_pyramid(P(f1), P(f2), h8, w8, _lib.ptr_array(levels), P(ws), ws.numel(), S()), "sampt_raft_corr_pyramid")
    torch.cuda.synchronize()
    for l in range(4):
        got = levels[l].cpu().reshape(want[l].shape)
        assert max_abs(got, want[l]) < FP32_GRADE * float(want[l].abs().max()), f"level {l} vs the restatement"
        g = gold[f"pyr{l}"]
        assert max_abs(got[rows], g) < FP32_GRADE * float(g.abs().max()), f"level {l} vs the golden"


def test_lookup(lib, dev, gold):
    levels = [gold[f"pyr{l}"] for l in range(4)]
    got = _lookup(lib, dev, levels, gold["coords"])
    want = gold["lookup"]
    tol = FP32_GRADE * float(want.abs().max())
    assert max_abs(got[:, :324], want) < tol
    assert (got[:, 324:] == 0).all()
    # the window's first index moves x: a transposed window is far outside the tolerance
    assert max_abs(got[:, :324].reshape(-1, 4, 9, 9).transpose(2, 3).reshape(-1, 324), want) > 100 * tol
    # coordinates outside every level, exactly on the last row / column, on integers, just inside the border
    n = levels[0].shape[0]
    co = gold["coords"].clone()
    special = torch.tensor([[-50.0, -60.0], [1.0e4, 3.0], [17.0, 16.0], [17.0, 3.5], [2.25, 16.0], [0.0, 0.0], [-0.5, -0.5],
                            [-4.0, 8.0], [21.0, 20.0], [16.999, 15.999], [5.0, 7.0], [-1.0e9, 1.0e9]])
    co[:special.shape[0]] = special
    assert n >= special.shape[0]
    got = _lookup(lib, dev, levels, co)
    want = R.lookup(levels, co)
    assert max_abs(got[:, :324], want) < tol
    assert (got[0, :324] == 0).all() and (got[1, :324] == 0).all() and (got[11, :324] == 0).all()
    assert float(got[2, :81].abs().max()) > 0 and float(want[2, :81].abs().max()) > 0


def test_convex_upsampling(lib, dev, gold):
    h8, w8, H, W = 17, 18, 131, 140
    low = gold["mask_flow_low"]
    g = torch.Generator().manual_seed(11)
    mask = torch.randn(2, h8, w8, 576, generator=g) * 2
    mask[0] = 0
    mask[0, gold["mask_rows"].tolist()] = gold["mask"]
    lows = torch.stack([low, low.flip(-1) * 0.5])
    out = torch.full((2, 2, H, W), float("nan"), device=dev)
    ok(lib.sampt_raft_upsample(P(lows.permute(0, 2, 3, 1).contiguous().to(dev)), P(mask.contiguous().to(dev)), 1.0, 2, h8, w8, H, W,
                               P(out), S()), "sampt_raft_upsample")
    torch.cuda.synchronize()
    out = out.cpu()
    want = gold["flow_up"]
    tol = FP32_GRADE * float(want.abs().max())
    for r in gold["mask_rows"].tolist():                     # fine rows of coarse row r after removing the top padding of 2
        y0, y1 = max(8 * r - 2, 0), min(8 * r + 8 - 2, H)
        assert max_abs(out[0][:, y0:y1], want[:, y0:y1]) < tol
    for i in range(2):
        ref = R.unpad(R.upsample(lows[i], mask[i].permute(2, 0, 1)), H, W)
        assert max_abs(out[i], ref) < FP32_GRADE * float(ref.abs().max())


def test_chain_equals_the_restatement(dev, gold, restated, tracker):
    fwd, bwd, _ = restated
    H, W = fwd.shape[-2:]
    extra = torch.tensor([[3.0, 70.25, 60.5], [0.0, 12.0, 100.75], [3.0, 5.5, 120.0], [1.0, 138.9, 2.1], [2.0, 69.0, 64.0],
                          [0.0, -3.0, 50.0], [1.0, 150.0, 140.0]])          # last frame (backward only), frame 0, out of frame
    q = torch.cat([gold["query_points"], extra])
    traj, vis = tracker.chain(fwd.to(dev), bwd.to(dev), q.to(dev))
    want_t, want_v = R.chain(fwd, bwd, q)
    assert traj.dtype == torch.float32 and vis.dtype == torch.bool
    assert (traj.cpu() == want_t).all() and (vis.cpu() == want_v).all()
    assert not bool(want_v.all()) and bool(want_v[:, :12].all())            # both visibility outcomes occur


def test_engine_matches_the_golden(dev, gold, restated, device_flows, tracker):
    fwd, bwd, low = device_flows
    bar, p = float(gold["bar_px"]), int(gold["pair"])
    d_low, d_up = max_abs(low, gold["flow_low"]), max_abs(fwd[p], gold["flow_up"])
    rf, rb, _ = restated
    d_rest = max(max_abs(fwd, rf), max_abs(bwd, rb))
    print(f"flow_low vs golden {d_low:.3e} (bar {bar / 8:.3e}); flow_up vs golden {d_up:.3e}, all flows vs restatement {d_rest:.3e} (bar {bar:.3e})")
    assert d_low < bar / 8 and d_up < bar and d_rest < bar
    traj, vis = tracker(gold["frames"][None].to(dev), gold["query_points"][None].to(dev))
    assert traj.shape == (1, 4, 12, 2) and vis.shape == (1, 4, 12) and vis.dtype == torch.bool
    want = gold["trajectories"]
    d_traj = max_abs(traj[0], want)
    print(f"trajectories vs golden {d_traj:.3e} (bar {bar * 4:.3e})")
    assert d_traj < bar * 4
    assert (traj[0].cpu().round() == want.round()).all()
    assert (vis[0].cpu() == gold["visibilities"]).all()


def test_iterations(dev, gold, sd, tracker, device_flows):
    frames = gold["frames"][:2]
    bar = float(gold["bar_px"])
    fwd4, bwd4, low4 = tracker.flows(frames.to(dev), iters=4, return_low=True)
    rf, rb, rl = R.flows(sd, frames, 4)
    d = max(max_abs(fwd4, rf), max_abs(bwd4, rb))
    print(f"4 iterations vs restatement {d:.3e} (bar {bar:.3e})")
    assert d < bar and max_abs(low4, rl) < bar / 8
    fwd12, _ = tracker.flows(frames.to(dev), iters=12)
    assert max_abs(fwd12[0], device_flows[0][0]) > 1.0                       # 32 iterations are not 12


@pytest.mark.parametrize("H,W", [(128, 136), (133, 203)])
def test_geometry(dev, gold, sd, tracker, H, W):
    """No padding at all, and odd padding on both axes (3 -> 1 + 2 rows, 5 -> 2 + 3 columns)."""
    frames, _ = synthetic_clip(T=2, H=H, W=W, seed=5)
    bar = float(gold["bar_px"])
    fwd, bwd, low = tracker.flows(frames.to(dev), return_low=True)
    rf, rb, rl = R.flows(sd, frames, 32)
    assert fwd.shape == (1, 2, H, W) and low.shape == (2, 1, 2, (H + 7) // 8, (W + 7) // 8)
    d = max(max_abs(fwd, rf), max_abs(bwd, rb))
    print(f"{H} x {W}: flows vs restatement {d:.3e} (bar {bar:.3e})")
    assert d < bar and max_abs(low, rl) < bar / 8


def test_two_chunks_equal_one(lib, dev, gold, tracker, device_flows):
    frames = gold["frames"].to(dev)
    tracker._ensure(dev)
    n2, n3 = C.c_size_t(), C.c_size_t()
    ok(lib.sampt_raft_workspace_bytes(tracker._h, 4, 131, 140, 2, C.byref(n2)), "workspace")
    ok(lib.sampt_raft_workspace_bytes(tracker._h, 4, 131, 140, 3, C.byref(n3)), "workspace")
    assert n2.value < n3.value                               # a 2-pair workspace cannot hold the 3 pairs: chunks of 2 + 1
    fwd, bwd, low = tracker.flows(frames, return_low=True, workspace_pairs=2)
    assert torch.equal(fwd.cpu(), device_flows[0]) and torch.equal(bwd.cpu(), device_flows[1]) and torch.equal(low.cpu(), device_flows[2])
    one = tracker.flows(frames, workspace_pairs=1)
    assert torch.equal(one[0].cpu(), device_flows[0]) and torch.equal(one[1].cpu(), device_flows[1])


def test_sampt_runs_with_the_raft_tracker(dev, tracker):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import SAM_CONFIGS
    from tests.util import disc_queries
    frames, centres = synthetic_clip(T=3, H=128, W=256, seed=72)
    q = disc_queries(centres, n_pos=4, r=9.0)
    video = {"image": [f for f in frames], "target_hw": (128, 256), "query_points": q[None]}
    pred = SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32").to(dev))
    model = SamPt(tracker, pred, sam_iou_threshold=-1e9, positive_points_per_mask=4, negative_points_per_mask=0,
                  iterative_refinement_iterations=1).eval()
    out = model(video)
    tr, vi = tracker(frames[None].to(dev), q[None].to(dev))
    assert torch.equal(out["trajectories"][:, 0].cpu(), tr[0].cpu())
    assert torch.equal(out["visibilities"][:, 0].cpu().bool(), vi[0].cpu())
    assert torch.isfinite(torch.stack(out["logits"])).all()
