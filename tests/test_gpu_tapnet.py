"""TapNet point tracker on the device (csrc/tapnet.hip, csrc/engine_tapnet.hip, csrc/cost_volume_heads.h) against the restatement of
tests/tapnet_ref.py, run live on the CPU, and against tests/golden/tapnet_ref.npz recorded from it.  PARITY UNPINNED: the reference
model needs JAX, Haiku and a checkpoint, which do not exist where this project is built (tests/tapnet_ref.py says what is pinned on
the reference instead).

Bars.  The shift kernel's f32 output and the max-pool are exact (``==``).  The planes of the shift kernel sum back to the f32 value
within the split's rounding: hi = fp16(v) leaves |v - hi| <= 2^-11 |v|, lo = fp16(v - hi) leaves 2^-11 of that, and a lo below fp16's
smallest subnormal spacing is rounded by at most 2^-25: 2^-22 max|v| + 2^-25.  Single kernels with sums are held to the project's fp32
grade, 2e-5 x max |reference| (tests/test_gpu_raft.py).  A backbone stage has k convolutions between the frames and itself
(tapnet_ref.N_CONVS, shortcuts included), each held to that grade on its own by test_convolutions_of_the_backbone; BatchNorm keeps the
maps at unit scale, so the stage's bar is k x 2e-5 x max |reference|.  End to end and for the heads the bar is read from the golden
file: ``bar_px`` / ``bar_logit`` = 8 x the restatement's own arithmetic noise at the test shape (tools/make_tapnet_golden.py), whose
generator has asserted that no heat map's best cell is nearly tied and no occlusion logit lies within the bar's reach of the threshold."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import init_tapnet_state_dict
from tests import tapnet_ref as R
from tests.util import max_abs, synthetic_clip

pytestmark = pytest.mark.gpu
FP32_GRADE = 2e-5
HEAD_NAMES = ["heads.hid1.weight", "heads.hid1.bias", "heads.hid2.weight", "heads.hid2.bias", "heads.hid3.weight", "heads.hid3.bias",
              "heads.hid4.weight", "heads.hid4.bias", "heads.occ_out.weight", "heads.occ_out.bias"]


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def sd():
    return init_tapnet_state_dict(72)


@pytest.fixture(scope="module")
def packed(sd, dev):
    from sam_pt_amd.pack import pack_tapnet
    return pack_tapnet(sd, dev)


@pytest.fixture(scope="module")
def tracker(sd):
    from sam_pt_amd.point_tracker import TapnetPointTracker
    return TapnetPointTracker(state_dict=sd)


@pytest.fixture(scope="module")
def frames01(gold):
    """The adapter's resize on the CPU: (T,3,256,256) in [0, 1]."""
    return F.interpolate(gold["frames"] / 255, (R.SIZE, R.SIZE), mode="bilinear", align_corners=False, antialias=True)


@pytest.fixture(scope="module")
def restated(gold, sd, frames01):
    """The restatement on the golden clip, computed once, with its stages."""
    return R.forward(sd, (frames01 * 2 - 1).permute(0, 2, 3, 1), gold["video_q"], stages=True)


@pytest.fixture(scope="module")
def device_run(dev, gold, tracker, frames01):
    """(tracks, occlusion) of the engine on the golden clip, on the CPU."""
    out = tracker.track(frames01.to(dev), gold["video_q"][:, [0, 2, 1]].to(dev))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def S():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


def close(got, want, what, grade=FP32_GRADE):
    d, tol = max_abs(got, want), grade * float(want.abs().max())
    print(f"{what}: {d:.3e} (bar {tol:.3e})")
    assert d < tol, what


# ---------------------------------------------------------------------------------------------- the shift kernel
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("C_,n", [(64, 8), (128, 16), (64, 0)])
def test_bn_shift_kernel(lib, dev, T, C_, n, planes):
    """relu(a x + b) shifted by n channels each way over a 6 x 5 map, with and without the unshifted second output, as f32 (exact) and
    as planes (within the split's rounding of the exact f32 value)."""
    g = torch.Generator().manual_seed(T * 1000 + C_ + n)
    x = torch.randn(T, 6, 5, C_, generator=g) * 2
    sd = {"bn.scale": torch.randn(C_, generator=g) * 0.2 + 1, "bn.offset": torch.randn(C_, generator=g) * 0.2,
          "bn.mean": torch.randn(C_, generator=g) * 0.3, "bn.var": torch.rand(C_, generator=g) + 0.5}
    a, b = R.fold_batchnorm(sd, "bn")
    unshifted = R.preact(sd, "bn", x)
    shifted = R.temporal_shift(unshifted, n / C_)
    assert float(unshifted.min()) == 0.0 and (n == 0 or T == 1 or not torch.equal(shifted, unshifted))
    xd, ad, bd = x.to(dev), a.to(dev), b.to(dev)
    for second in (False, True):
        def buf():
            return (torch.full((2, T, 6, 5, C_), float("nan"), dtype=torch.float16, device=dev) if planes
                    else torch.full((T, 6, 5, C_), float("nan"), device=dev))
        ys, yu = buf(), (buf() if second else None)
        args = (None, P(ys), None, P(yu)) if planes else (P(ys), None, P(yu), None)
        ok(lib.sampt_tapnet_bn_shift_f32(P(xd), P(ad), P(bd), T, 30, C_, n, *args, S()), "sampt_tapnet_bn_shift_f32")
        torch.cuda.synchronize()
        for got, want, what in ((ys, shifted, "shifted"), (yu, unshifted, "unshifted")):
            if got is None:
                continue
            got = got.cpu()
            if planes:
                d, tol = max_abs(got[0].float() + got[1].float(), want), 2.0 ** -22 * float(want.abs().max()) + 2.0 ** -25
                print(f"{what} planes, T = {T}, C = {C_}, n = {n}: {d:.3e} (bar {tol:.3e})")
                assert d <= tol and torch.equal(got[0], want.half())
            else:
                assert torch.equal(got, want), f"{what}, T = {T}, C = {C_}, n = {n}"


@pytest.mark.parametrize("side", [12, 13])
def test_max_pool_kernel(lib, dev, side):
    """An even and an odd side, 3 images, all values negative (a padding read as zero would win every border maximum)."""
    g = torch.Generator().manual_seed(side)
    x = -torch.rand(3, side, side + 2, 8, generator=g) - 0.5
    want = R.max_pool_same(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
    assert float(want.max()) < 0
    xd = x.to(dev)
    y = torch.full(want.shape, float("nan"), device=dev)
    ok(lib.sampt_tapnet_maxpool_nhwc(P(xd), P(y), 3, side, side + 2, 8, S()), "sampt_tapnet_maxpool_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)


def test_query_features_kernel(lib, dev, restated):
    """The four corners of the frame, t = 0 and t = T - 1, a fractional t, t past both ends, an interior point."""
    grid = restated["grid"]
    T = grid.shape[0]
    q = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 256.0], [T - 1.0, 256.0, 0.0], [T - 1.0, 256.0, 256.0], [1.3, 100.25, 37.5],
                      [2.5, 3.0, 250.0], [-0.75, 60.0, 60.0], [T + 0.5, 200.0, 13.0], [3.0, 131.0, 77.7]])          # (t, y, x)
    want = R.query_features(grid, q)
    gd, qd = grid.contiguous().to(dev), q[:, [0, 2, 1]].contiguous().to(dev)
    qf = torch.full(want.shape, float("nan"), device=dev)
    ok(lib.sampt_tapnet_query_feats_f32(P(gd), T, P(qd), q.shape[0], P(qf), S()), "sampt_tapnet_query_feats_f32")
    torch.cuda.synchronize()
    close(qf.cpu(), want, "query features")
    assert torch.equal(qf[0].cpu(), grid[0, 0, 0]) and torch.equal(qf[3].cpu(), grid[T - 1, 31, 31])     # a clamped corner is the cell itself


# ---------------------------------------------------------------------------------------------- the heads
def _heads(lib, dev, packed, grid, qf, q_txy):
    from sam_pt_amd import _lib
    T, n = grid.shape[0], q_txy.shape[0]
    pts = torch.full((n, T, 2), float("nan"), device=dev)
    occ = torch.full((n, T), float("nan"), device=dev)
    gd, qd, qq = grid.contiguous().to(dev), qf.contiguous().to(dev), q_txy.contiguous().to(dev)        # (kept alive over the call)
    ok(lib.sampt_tapnet_heads_f32(P(gd), T, P(qd), P(qq), n, _lib.ptr_array([packed[k] for k in HEAD_NAMES]), P(pts), P(occ), S()),
       "sampt_tapnet_heads_f32")
    torch.cuda.synchronize()
    return pts.cpu(), occ.cpu()


def _within_bars(got, want, gold, what):
    bar_px, bar_logit = float(gold["bar_px"]), float(gold["bar_logit"])
    d_px, d_lg = max_abs(got[0], want[0]), max_abs(got[1], want[1])
    print(f"{what}: tracks {d_px:.3e} px (bar {bar_px:.3e}), occlusion {d_lg:.3e} (bar {bar_logit:.3e})")
    assert d_px < bar_px and d_lg < bar_logit, what


def test_heads_kernel_on_the_golden_items(lib, dev, sd, packed, gold, restated):
    q = gold["video_q"]
    got = _heads(lib, dev, packed, restated["grid"], restated["qf"], q[:, [0, 2, 1]])
    _within_bars(got, (restated["tracks"], restated["occlusion"]), gold, "heads vs restatement")
    _within_bars(got, (gold["tracks"], gold["occlusion"]), gold, "heads vs golden")
    for i in range(q.shape[0]):                                    # the query point comes back verbatim on its own frame
        assert torch.equal(got[0][i, int(q[i, 0])], q[i, [2, 1]])


def test_heads_kernel_corner_maximum_and_half_frames(lib, dev, sd, packed, gold):
    """Heat maps whose maximum sits in each of the four corners (the disk is clipped by two borders) and on an edge; query features
    e_0 and the cost map in channel 0, so that the cost volume is the map itself.  Queries at t = 0.5 and t = 1.5 round half-to-even
    to frames 0 and 2, where the query point comes back verbatim."""
    cells = [(0, 0), (0, 31), (31, 0), (31, 31), (0, 13), (17, 31)]
    T = len(cells)
    g = torch.Generator().manual_seed(5)
    grid = torch.zeros(T, 32, 32, 256)
    grid[..., 0] = torch.rand(T, 32, 32, generator=g) * 0.1
    for t, (y, x) in enumerate(cells):                                             # a low bump: the neighbours keep their weight
        grid[t, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3, 0] += 0.1
        grid[t, y, x, 0] = 0.3
    qf = torch.zeros(3, 256)
    qf[:, 0] = torch.tensor([1.0, 0.75, 0.9])
    q = torch.tensor([[-1.0, 10.0, 20.0], [0.5, 200.5, 31.25], [1.5, 7.75, 99.0]])      # (t, y, x): no query frame; frame 0; frame 2
    pts, occ, logits = R.heads(sd, qf, grid, q, return_logits=True)
    best = logits[0].reshape(T, -1).argmax(-1)
    assert [(int(b) // 32, int(b) % 32) for b in best] == cells                     # the case is what it claims to be
    got = _heads(lib, dev, packed, grid, qf, q[:, [0, 2, 1]])
    centres = torch.tensor([[8.0 * x + 4, 8.0 * y + 4] for y, x in cells])
    assert float((pts[0] - centres).abs().max(-1).values.min()) > 0.01                # every item is a real average, not the cell centre
    _within_bars(got, (pts, occ), gold, "corner maxima and half frames")
    assert torch.equal(got[0][1, 0], torch.tensor([31.25, 200.5])) and torch.equal(got[0][2, 2], torch.tensor([99.0, 7.75]))
    assert not torch.equal(got[0][1, 1], torch.tensor([31.25, 200.5])) and not torch.equal(got[0][2, 1], torch.tensor([99.0, 7.75]))


# ---------------------------------------------------------------------------------------------- convolutions
@pytest.mark.parametrize("side,k,stride,cin,cout,dtype", [(12, 3, 2, 64, 128, 0), (12, 3, 2, 64, 128, 3), (12, 3, 2, 64, 128, 4), (12, 1, 2, 64, 128, 3),
                                                         (12, 1, 2, 64, 128, 4), (16, 7, 2, 4, 64, 0)])
def test_convolutions_of_the_backbone(lib, dev, side, k, stride, cin, cout, dtype):
    """The backbone's three new situations with a batch of 3 images (TAPIR's convolutions run one image per launch): 3 x 3 stride 2 on
    an even side 64 -> 128, 1 x 1 stride 2, 7 x 7 stride 2 with Cin 4; on the exact-f32 path (0), the split-fp16 path (3) and the
    pre-split-planes path (4) where the layer can take them."""
    from sam_pt_amd.pack import _khwc, split_f16x3
    from tests.tapir_ref import conv_same
    g = torch.Generator().manual_seed(side * 100 + k + dtype)
    x = torch.randn(3, cin, side, side, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    want = conv_same(x, w, stride).permute(0, 2, 3, 1).contiguous()
    xh = x.permute(0, 2, 3, 1).contiguous()
    wk = _khwc(w)
    if dtype == 4:
        hi = xh.half()
        xd = torch.stack([hi, (xh - hi.float()).half()]).contiguous().to(dev)
    else:
        xd = xh.to(dev)
    wd = (wk if dtype == 0 else split_f16x3(wk)).to(dev)
    y = torch.full(want.shape, float("nan"), device=dev)
    ok(lib.sampt_conv2d_same_nhwc(dtype, P(xd), P(wd), P(y), 3, side, side, cin, cout, k, stride, S()), "sampt_conv2d_same_nhwc")
    torch.cuda.synchronize()
    close(y.cpu(), want, f"conv {k}x{k} stride {stride} on {side}, {cin} -> {cout}, 3 images, path {dtype}")


def test_null_pointers_are_refused(lib, dev):
    x = torch.zeros(64, device=dev)
    bad = -1                                                                          # SAMPT_ERR_ARG
    assert lib.sampt_tapnet_bn_shift_f32(None, P(x), P(x), 1, 1, 4, 0, P(x), None, None, None, S()) == bad
    assert lib.sampt_tapnet_bn_shift_f32(P(x), P(x), P(x), 1, 1, 4, 0, None, None, None, None, S()) == bad
    assert lib.sampt_tapnet_bn_shift_f32(P(x), P(x), P(x), 1, 1, 8, 6, P(x), None, None, None, S()) == bad       # n % 4, 2 n > C
    assert lib.sampt_tapnet_maxpool_nhwc(P(x), None, 1, 2, 2, 4, S()) == bad
    assert lib.sampt_tapnet_maxpool_nhwc(P(x), P(x), 1, 2, 2, 6, S()) == bad
    assert lib.sampt_tapnet_query_feats_f32(P(x), 1, None, 1, P(x), S()) == bad
    assert lib.sampt_tapnet_query_feats_f32(P(x), 0, P(x), 1, P(x), S()) == bad
    assert lib.sampt_tapnet_heads_f32(P(x), 1, P(x), P(x), 1, None, P(x), P(x), S()) == bad
    assert lib.sampt_tapnet_track_f32(None, P(x), 1, P(x), 1, P(x), P(x), P(x), 64, S()) == bad
    h = C.c_void_p()
    assert lib.sampt_tapnet_create(None, None, 0, C.byref(h)) == bad


# ---------------------------------------------------------------------------------------------- engine
def test_backbone_stages(lib, dev, gold, tracker, frames01, restated):
    from sam_pt_amd import _lib
    tracker._ensure(dev)
    T = frames01.shape[0]
    shapes = {"stem": (T, 64, 64, 64), "unit0": (T, 64, 64, 64), "unit1": (T, 32, 32, 128), "unit2": (T, 32, 32, 256)}
    st = {k: torch.full(s, float("nan"), device=dev) for k, s in shapes.items()}
    grid = torch.full((T, 32, 32, 256), float("nan"), device=dev)
    ws = _lib.workspace("sampt_tapnet_backbone_workspace_bytes", dev, tracker._h, T)
    fd = frames01.to(dev).contiguous()
    ok(lib.sampt_tapnet_backbone_f32(tracker._h, P(fd), T, P(grid), _lib.ptr_array([st[k] for k in ("stem", "unit0", "unit1", "unit2")]), P(ws),
                                     ws.numel(), S()), "sampt_tapnet_backbone_f32")
    torch.cuda.synchronize()
    assert lib.sampt_tapnet_launches(tracker._h) == 3 * 1 + 28
    rows = gold["map_rows"].long()
    for k, n in R.N_CONVS.items():
        close(st[k].cpu(), restated[k], "stage " + k, grade=n * FP32_GRADE)
        r = rows if k in ("stem", "unit0") else rows[rows < 1024]
        close(st[k].cpu().reshape(T, -1, shapes[k][-1])[:, r], gold[k + "_rows"], "stage " + k + ", golden rows", grade=n * FP32_GRADE)
    close(grid.cpu(), restated["grid"], "grid", grade=R.N_CONVS["unit2"] * FP32_GRADE)


def test_engine_matches_the_golden_and_the_restatement(gold, restated, device_run, tracker):
    tracks, occ = device_run
    assert tracks.shape == (6, 5, 2) and occ.shape == (6, 5)
    _within_bars((tracks, occ), (gold["tracks"], gold["occlusion"]), gold, "engine vs golden")
    _within_bars((tracks, occ), (restated["tracks"], restated["occlusion"]), gold, "engine vs restatement")
    vis = R.visibility_probability(occ).t() > float(gold["threshold"])
    assert torch.equal(vis, gold["visibilities"])                                    # every item
    assert tracker.stats["launches"] == 3 * 1 + 30


def test_forward_on_the_clip(dev, gold, tracker):
    """TapnetPointTracker.forward on the non-square 96 x 128 clip (its resize runs on the device): the bar scales with the clip's pixels."""
    frames, q = gold["frames"], gold["query_points"]
    traj, vis = tracker(frames[None].to(dev), q[None].to(dev))
    assert traj.shape == (1, 5, 6, 2) and vis.shape == (1, 5, 6) and vis.dtype == torch.bool
    H, W = frames.shape[-2:]
    bar = float(gold["bar_px"])
    dx, dy = max_abs(traj[0, ..., 0], gold["trajectories"][..., 0]), max_abs(traj[0, ..., 1], gold["trajectories"][..., 1])
    print(f"trajectories vs golden: x {dx:.3e} px (bar {bar * W / 256:.3e}), y {dy:.3e} px (bar {bar * H / 256:.3e})")
    assert dx < bar * W / 256 and dy < bar * H / 256
    assert torch.equal(vis[0].cpu(), gold["visibilities"])
    two = tracker(torch.stack([frames, frames.flip(0)]).to(dev), torch.stack([q, q]).to(dev))      # B = 2: one clip at a time
    assert torch.equal(two[0][0], traj[0]) and torch.equal(two[1][0], vis[0]) and not torch.equal(two[0][1], traj[0])


@pytest.mark.parametrize("T", [2, 1])
def test_short_clips(dev, gold, sd, tracker, frames01, T):
    """T = 2 and T = 1: the temporal shift reads nothing but zeros on one side or on both."""
    q = gold["video_q"].clone()
    q[:, 0] = q[:, 0].clamp(max=T - 1)
    want = R.forward(sd, (frames01[:T] * 2 - 1).permute(0, 2, 3, 1), q)
    got = [o.cpu() for o in tracker.track(frames01[:T].to(dev), q[:, [0, 2, 1]].to(dev))]
    assert got[0].shape == (6, T, 2)
    _within_bars(got, (want["tracks"], want["occlusion"]), gold, f"T = {T}")


def test_forty_queries_hold_the_six(dev, gold, tracker, frames01, device_run):
    g = torch.Generator().manual_seed(40)
    q = torch.stack([torch.randint(0, 5, (40,), generator=g).float(), torch.rand(40, generator=g) * 256, torch.rand(40, generator=g) * 256], 1)
    where = [0, 15, 16, 23, 32, 39]
    q[where] = gold["video_q"][:, [0, 2, 1]]
    out = [o.cpu() for o in tracker.track(frames01.to(dev), q.to(dev))]
    assert torch.equal(out[0][where], device_run[0]) and torch.equal(out[1][where], device_run[1])
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()


def test_two_runs_and_stem_chunks_are_bitwise_equal(dev, gold, tracker, frames01, device_run):
    f, q = frames01.to(dev), gold["video_q"][:, [0, 2, 1]].to(dev)
    out = tracker.track(f, q)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(out, device_run))
    assert tracker.stats["launches"] == 3 * 1 + 30
    from sam_pt_amd import _lib
    assert _lib.workspace_bytes("sampt_tapnet_workspace_bytes", tracker._h, 9, 3) > 0            # a sizing pass launches nothing ...
    assert tracker._lib.sampt_tapnet_launches(tracker._h) == 3 * 1 + 30                          # ... and leaves the last call's count
    assert tracker._lib.sampt_tapnet_launches(None) == 0
    ok(tracker._lib.sampt_tapnet_set_stem_chunk(tracker._h, 2), "sampt_tapnet_set_stem_chunk")   # 5 frames in chunks of 2, 2, 1
    try:
        part = tracker.track(f, q)
        assert tracker.stats["launches"] == 3 * 3 + 30                                           # the chunks really ran
        assert all(torch.equal(a.cpu(), b) for a, b in zip(part, device_run))
    finally:
        ok(tracker._lib.sampt_tapnet_set_stem_chunk(tracker._h, 8), "sampt_tapnet_set_stem_chunk")


def test_sampt_runs_with_the_tapnet_tracker(dev, tracker):
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
