"""TAPIR point tracker on the device (csrc/tapir.hip, csrc/engine_tapir.hip) against the restatement of tests/tapir_ref.py, run live on
the CPU, and against tests/golden/tapir_ref.npz recorded from it.  PARITY UNPINNED: the reference model needs JAX, Haiku and a
checkpoint, which do not exist where this project is built (tests/tapir_ref.py says what is pinned on the reference instead).

Single kernels are held to the project's fp32 grade, 2e-5 x max |reference| (tests/test_gpu_raft.py).  End to end the bar is read
from the golden file: ``bar_px`` / ``bar_logit`` = 8 x the restatement's own arithmetic noise at the test shape (f32 against float64
and against a 1e-7 relative weight perturbation, whichever is larger; tools/make_tapir_golden.py).  The generator has asserted that
no heat map's best cell is nearly tied and that no visibility probability lies within the bar's reach of the threshold, so no item is
excluded anywhere."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import init_tapir_state_dict
from tests import tapir_ref as R
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
    return init_tapir_state_dict(72)


@pytest.fixture(scope="module")
def packed(sd, dev):
    from sam_pt_amd.pack import pack_tapir
    return pack_tapir(sd, dev)


@pytest.fixture(scope="module")
def tracker(sd):
    from sam_pt_amd.point_tracker import TapirPointTracker
    return TapirPointTracker(state_dict=sd)


def resized(frames):
    """The adapter's resize on the CPU: (T,3,256,256) in [0, 1]."""
    return F.interpolate(frames / 255, (R.SIZE, R.SIZE), mode="bilinear", align_corners=False, antialias=True)


@pytest.fixture(scope="module")
def frames01(gold):
    return resized(gold["frames"])


@pytest.fixture(scope="module")
def restated(gold, sd, frames01):
    """The restatement on the golden clip, computed once, with its stages."""
    return R.forward(sd, (frames01 * 2 - 1).permute(0, 2, 3, 1), gold["video_q"], stages=True)


@pytest.fixture(scope="module")
def device_run(dev, gold, tracker, frames01):
    """(tracks, occlusion, expected_dist, per-iteration) of the engine on the golden clip, on the CPU."""
    q = gold["video_q"][:, [0, 2, 1]]
    out = tracker.track(frames01.to(dev), q.to(dev), return_iters=True)
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


def close(got, want, what):
    d, tol = max_abs(got, want), FP32_GRADE * float(want.abs().max())
    print(f"{what}: {d:.3e} (bar {tol:.3e})")
    assert d < tol, what


# ---------------------------------------------------------------------------------------------- single kernels
@pytest.mark.parametrize("side,k,stride,cin,cout,dtype,pad", [
    (12, 3, 2, 32, 8, 0, (0, 1)), (12, 3, 2, 32, 8, 3, (0, 1)), (12, 3, 2, 32, 8, 4, (0, 1)), (13, 3, 2, 32, 8, 3, (1, 1)), (13, 3, 2, 32, 8, 4, (1, 1)),
    (16, 7, 2, 4, 64, 0, (2, 3)), (15, 7, 2, 4, 64, 0, (3, 3)), (12, 1, 2, 64, 16, 3, (0, 0)), (9, 3, 1, 64, 12, 4, (1, 1))])
def test_conv_with_same_padding(lib, dev, side, k, stride, cin, cout, dtype, pad):
    """Asymmetric TensorFlow 'SAME' padding at stride 2 on an even side (nothing / 2 before, one more after) and on an odd side, on the
    exact-f32 path (0), the split-fp16 path (3) and the pre-split-planes path (4)."""
    from sam_pt_amd.pack import _khwc, split_f16x3
    g = torch.Generator().manual_seed(side * 100 + k)
    x = torch.randn(2, cin, side, side, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    want = R.conv_same(x, w, stride).permute(0, 2, 3, 1).contiguous()
    assert R.same_padding(side, k, stride) == pad
    xh = x.permute(0, 2, 3, 1).contiguous()
    wk = _khwc(w)
    if dtype == 4:
        hi = xh.half()
        xd = torch.stack([hi, (xh - hi.float()).half()]).contiguous().to(dev)
    else:
        xd = xh.to(dev)
    wd = (wk if dtype == 0 else split_f16x3(wk)).to(dev)
    y = torch.full(want.shape, float("nan"), device=dev)
    ok(lib.sampt_conv2d_same_nhwc(dtype, P(xd), P(wd), P(y), 2, side, side, cin, cout, k, stride, S()), "sampt_conv2d_same_nhwc")
    torch.cuda.synchronize()
    close(y.cpu(), want, f"conv {k}x{k} stride {stride} on {side}, path {dtype}")


@pytest.mark.parametrize("planes", [False, True])
def test_affine_instance_norm(lib, dev, planes):
    g = torch.Generator().manual_seed(3)
    n, h, w, c = 2, 7, 9, 64
    x = torch.randn(n, c, h, w, generator=g) * 3 + 1
    scale, offset = torch.randn(c, generator=g) * 0.2 + 1, torch.randn(c, generator=g) * 0.2
    want = F.relu(R.instance_norm(x, scale, offset)).permute(0, 2, 3, 1).contiguous()
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    ws = torch.empty(lib.sampt_instance_norm_workspace_bytes(n, h * w, c), dtype=torch.uint8, device=dev)
    y = torch.full(want.shape, float("nan"), device=dev)
    hl = torch.zeros((2,) + tuple(want.shape), dtype=torch.float16, device=dev) if planes else None
    sc, of = scale.to(dev), offset.to(dev)
    ok(lib.sampt_instance_norm_affine_nhwc(P(xd), P(sc), P(of), None if planes else P(y), P(hl), n, h * w, c, 1e-5, 1, P(ws), ws.numel(), S()),
       "sampt_instance_norm_affine_nhwc")
    torch.cuda.synchronize()
    got = (hl[0].float() + hl[1].float()).cpu() if planes else y.cpu()
    close(got, want, "affine InstanceNorm + ReLU" + (" (planes)" if planes else ""))
    assert float(want.min()) == 0.0 and float(got.min()) == 0.0


def _heads(lib, dev, packed, lowres, qf, ldq, qoff, q_txy):
    from sam_pt_amd import _lib
    T, n = lowres.shape[0], q_txy.shape[0]
    names = ["heads.hid1.weight", "heads.hid1.bias", "heads.hid2.weight", "heads.hid2.bias", "heads.hid3.weight", "heads.hid3.bias",
             "heads.hid4.weight", "heads.hid4.bias", "heads.occ_out.weight", "heads.occ_out.bias"]
    pts = torch.full((n, T, 2), float("nan"), device=dev)
    occ, expd = torch.full((n, T), float("nan"), device=dev), torch.full((n, T), float("nan"), device=dev)
    lo, qd, qq = lowres.contiguous().to(dev), qf.contiguous().to(dev), q_txy.contiguous().to(dev)      # (kept alive over the call)
    ok(lib.sampt_tapir_heads_f32(P(lo), T, P(qd), ldq, qoff, P(qq), n, _lib.ptr_array([packed[k] for k in names]), P(pts), P(occ), P(expd), S()),
       "sampt_tapir_heads_f32")
    torch.cuda.synchronize()
    return pts.cpu(), occ.cpu(), expd.cpu()


def test_heads_kernel(lib, dev, gold, restated):
    """Points, occlusion and expected_dist per (query, frame) item, the query-frame override included.  The occlusion head is taken
    without the golden clip's conditioning gain (weights.init_tapir_state_dict: occ_gain 1500 re-centres and magnifies a difference of
    nearly equal numbers, which belongs to the end-to-end bar, not to a kernel's fp32 grade)."""
    from sam_pt_amd.pack import pack_tapir
    sd1 = init_tapir_state_dict(72, occ_gain=1.0, occ_centre=(0.0, 0.0))
    q = gold["video_q"]
    want = R.heads(sd1, restated["qf"][:, 128:], restated["lowres"], q)
    got = _heads(lib, dev, pack_tapir(sd1, dev), restated["lowres"], restated["qf"], 384, 128, q[:, [0, 2, 1]])
    for g, w, what in zip(got, want, ("points", "occlusion", "expected_dist")):
        close(g, w, "heads: " + what)
    for i in range(q.shape[0]):                                    # the query point comes back verbatim on its own frame
        assert torch.equal(got[0][i, int(q[i, 0])], q[i, [2, 1]])


def test_heads_kernel_corner_maximum(lib, dev, sd, packed):
    """Heat maps whose maximum sits in each of the four corners (the disk is clipped by two borders) and on an edge; query features
    e_0 and the cost map in channel 0, so that the cost volume is the map itself."""
    cells = [(0, 0), (0, 31), (31, 0), (31, 31), (0, 13), (17, 31)]
    T = len(cells)
    g = torch.Generator().manual_seed(5)
    lowres = torch.zeros(T, 32, 32, 256)
    lowres[..., 0] = torch.rand(T, 32, 32, generator=g) * 0.1
    for t, (y, x) in enumerate(cells):                                             # a low bump: the neighbours keep their weight
        lowres[t, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3, 0] += 0.1
        lowres[t, y, x, 0] = 0.3
    qf = torch.zeros(2, 256)
    qf[:, 0] = torch.tensor([1.0, 0.75])
    q = torch.tensor([[-1.0, 10.0, 20.0], [2.0, 200.5, 31.25]])                    # (t, y, x): no query frame; frame 2
    pts, occ, expd, logits = R.heads(sd, qf, lowres, q, return_logits=True)
    best = logits[0].reshape(T, -1).argmax(-1)
    assert [(int(b) // 32, int(b) % 32) for b in best] == cells                     # the case is what it claims to be
    got = _heads(lib, dev, packed, lowres, qf, 256, 0, q[:, [0, 2, 1]])
    centres = torch.tensor([[8.0 * x + 4, 8.0 * y + 4] for y, x in cells])
    assert float((pts[0] - centres).abs().max(-1).values.min()) > 0.01                # every item is a real average, not the cell centre
    close(got[0], pts, "corner maxima: points")
    assert torch.equal(got[0][1, 2], torch.tensor([31.25, 200.5]))


def test_patch_correlation(lib, dev, gold, restated):
    """First-iteration form (query features) against the golden rows, later-iteration form (per-row features) with positions on
    both sides of every border and far outside."""
    hires, lowres, qf = restated["hires"], restated["lowres"], restated["qf"]
    T, n = hires.shape[0], qf.shape[0]

    def run(pos, occ, expd, feat, per_row, ldx):
        x = torch.full((n * T, ldx), float("nan"), device=dev)
        d = [t.contiguous().to(dev) for t in (hires, lowres, pos, occ, expd, feat)]                       # (kept alive over the call)
        ok(lib.sampt_tapir_patch_corr_f32(P(d[0]), P(d[1]), T, n, P(d[2]), P(d[3]), P(d[4]), P(d[5]), per_row, P(x), ldx, S()),
           "sampt_tapir_patch_corr_f32")
        torch.cuda.synchronize()
        return x.cpu().reshape(n, T, ldx)

    pos, occ, expd = restated["iter_tracks"][0], restated["iter_occlusion"][0], restated["iter_expected_dist"][0]
    got = run(pos, occ, expd, qf, 0, 496)
    want, _ = R.mixer_input(hires, lowres, qf, pos, occ, expd, None)
    assert torch.equal(got[..., :4], want[..., :4]) and torch.equal(got[..., 4:388], want[..., 4:388]) and (got[..., 486:] == 0).all()
    close(got[..., 388:486], want[..., 388:], "patch correlation, first iteration")
    close(got[..., 388:486], gold["x0"][..., 388:], "patch correlation, first iteration, golden")
    assert float(want[2, :, 388:].abs().min()) == 0.0 and float(want[2, :, 388:].abs().max()) > 0     # the corner query: some samples outside
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(n, T, 384, generator=g)
    pos2 = torch.rand(n, T, 2, generator=g) * 256
    pos2[0, :, 0], pos2[1, :, 1] = torch.tensor([-11.9, -12.1, 0.0, 2.0, 267.9]), torch.tensor([255.9, 256.0, 268.1, 1e9, -1e9])
    got = run(pos2, occ, expd, feats.reshape(n * T, 384), 1, 486)
    want, _ = R.mixer_input(hires, lowres, qf, pos2, occ, expd, feats)
    assert torch.equal(got[..., 4:388], feats)
    close(got[..., 388:], want[..., 388:], "patch correlation, later iteration")
    assert (got[1, 3:, 388:] == 0).all()


@pytest.mark.parametrize("T", [1, 2, 5, 11, 16])
def test_temporal_half_block(lib, dev, sd, packed, T):
    """T = 1 and 2 (the halo is all padding), 5 (one tile with a tail), 11 (a full tile and a tail), 16 (two full tiles)."""
    g = torch.Generator().manual_seed(T)
    n, p = 3, "mixer.blocks.4."
    x = torch.randn(n, T, 512, generator=g) * 2
    want = R.temporal_half(sd, p, x)
    xo, xd = torch.full(x.shape, float("nan"), device=dev), x.to(dev)
    ok(lib.sampt_tapir_temporal_mix_f32(P(xd), P(xo), P(packed[p + "ln1.scale"]), P(packed[p + "dw1.weight"]), P(packed[p + "dw1.bias"]),
                                        P(packed[p + "dw2.weight"]), P(packed[p + "dw2.bias"]), n, T, S()), "sampt_tapir_temporal_mix_f32")
    torch.cuda.synchronize()
    close(xo.cpu(), want, f"temporal half-block, T = {T}")
    close(xo.cpu() - x, want - x, f"temporal half-block without the skip, T = {T}")


@pytest.mark.parametrize("M,N,K,act,res", [(37, 2048, 512, 3, False), (70, 512, 2048, 0, True), (30, 388, 512, 0, False), (130, 512, 496, 0, False),
                                           (5, 64, 32, 1, True)])
def test_gemm_epilogues(lib, dev, M, N, K, act, res):
    """The mixer's four Linear shapes: tanh-GELU epilogue (act 3), residual, N = 388 (no multiple of the 32-column wave tile), K = 496;
    and the rows of a call do not depend on how many rows it has."""
    g = torch.Generator().manual_seed(M)
    a, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    y = a.double() @ w.double().t() + b.double()
    y = R.gelu_tanh(y) if act == 3 else (F.relu(y) if act == 1 else y)
    want = (y + r.double() if res else y).float()

    def run(m):
        c = torch.full((m, N), float("nan"), device=dev)
        ad, wd, bd, rd = a[:m].contiguous().to(dev), w.to(dev), b.to(dev), (r[:m].contiguous().to(dev) if res else None)
        ok(lib.sampt_tapir_gemm_f32(P(ad), P(wd), P(bd), P(rd), P(c), m, N, K, act, S()), "sampt_tapir_gemm_f32")
        torch.cuda.synchronize()
        return c.cpu()

    got = run(M)
    close(got, want, f"gemm {M} x {N} x {K}, act {act}")
    assert torch.equal(run(min(M, 3)), got[:min(M, 3)])


def test_null_pointers_are_refused(lib, dev):
    x = torch.zeros(64, device=dev)
    bad = -1                                                                          # SAMPT_ERR_ARG
    assert lib.sampt_tapir_gemm_f32(None, P(x), None, None, P(x), 1, 4, 16, 0, S()) == bad
    assert lib.sampt_tapir_gemm_f32(P(x), P(x), None, None, P(x), 0, 4, 16, 0, S()) == bad
    assert lib.sampt_tapir_temporal_mix_f32(P(x), None, P(x), P(x), P(x), P(x), P(x), 1, 1, S()) == bad
    assert lib.sampt_tapir_temporal_mix_f32(P(x), P(x), P(x), P(x), P(x), P(x), P(x), 1, 0, S()) == bad
    assert lib.sampt_tapir_patch_corr_f32(P(x), P(x), 1, 0, P(x), P(x), P(x), P(x), 0, P(x), 496, S()) == bad
    assert lib.sampt_tapir_heads_f32(P(x), 1, P(x), 384, 128, P(x), 1, None, P(x), P(x), P(x), S()) == bad
    assert lib.sampt_tapir_query_feats_f32(P(x), None, 1, P(x), 1, P(x), S()) == bad
    assert lib.sampt_conv2d_same_nhwc(0, None, P(x), P(x), 1, 4, 4, 4, 4, 3, 2, S()) == bad
    assert lib.sampt_instance_norm_affine_nhwc(P(x), P(x), P(x), None, None, 1, 4, 4, 1e-5, 1, P(x), 64, S()) == bad
    assert lib.sampt_tapir_track_f32(None, P(x), 1, P(x), 1, 4, P(x), P(x), P(x), None, P(x), 64, S()) == bad
    h = C.c_void_p()
    assert lib.sampt_tapir_create(None, None, 0, C.byref(h)) == bad


# ---------------------------------------------------------------------------------------------- end to end
def _check_iterations(its, want, bar_px, bar_logit, what):
    """its (iters + 1,N,T,4) of the device against lists / stacks of tracks, occlusion, expected_dist per iteration."""
    for i in range(its.shape[0]):
        d_px = max_abs(its[i, ..., :2], want[0][i])
        d_lg = max(max_abs(its[i, ..., 2], want[1][i]), max_abs(its[i, ..., 3], want[2][i]))
        print(f"{what}, iteration {i}: tracks {d_px:.3e} px (bar {bar_px:.3e}), logits {d_lg:.3e} (bar {bar_logit:.3e})")
        assert d_px < bar_px and d_lg < bar_logit, f"{what}, iteration {i}"


def test_engine_matches_the_golden_and_the_restatement(gold, restated, device_run):
    tracks, occ, expd, its = device_run
    bar_px, bar_logit = float(gold["bar_px"]), float(gold["bar_logit"])
    assert its.shape == (5, 6, 5, 4)
    _check_iterations(its, (gold["iter_tracks"], gold["iter_occlusion"], gold["iter_expected_dist"]), bar_px, bar_logit, "golden")
    _check_iterations(its, (restated["iter_tracks"], restated["iter_occlusion"], restated["iter_expected_dist"]), bar_px, bar_logit, "restatement")
    assert torch.equal(its[-1, ..., :2], tracks) and torch.equal(its[-1, ..., 2], occ) and torch.equal(its[-1, ..., 3], expd)
    vis = R.visibility_probability(occ, expd).t() > float(gold["threshold"])
    assert torch.equal(vis, gold["visibilities"])                                    # every item


def test_forward_on_the_clip(dev, gold, tracker):
    """TapirPointTracker.forward on the non-square 40 x 56 clip (its resize runs on the device): the bar scales with the clip's pixels."""
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
    """T = 2 and T = 1: the temporal convolutions see nothing but padding around one or two frames."""
    q = gold["video_q"].clone()
    q[:, 0] = q[:, 0].clamp(max=T - 1)
    want = R.forward(sd, (frames01[:T] * 2 - 1).permute(0, 2, 3, 1), q)
    out = tracker.track(frames01[:T].to(dev), q[:, [0, 2, 1]].to(dev), return_iters=True)
    its = out[3].cpu()
    assert its.shape == (5, 6, T, 4)
    _check_iterations(its, (want["iter_tracks"], want["iter_occlusion"], want["iter_expected_dist"]), float(gold["bar_px"]),
                      float(gold["bar_logit"]), f"T = {T}")


def test_seventy_queries_hold_the_six(dev, gold, tracker, frames01, device_run):
    """70 queries with the golden six among them, in one chunk, in chunks of 16 (4 full + a tail) and of 1: identical rows."""
    g = torch.Generator().manual_seed(70)
    q = torch.stack([torch.randint(0, 5, (70,), generator=g).float(), torch.rand(70, generator=g) * 256, torch.rand(70, generator=g) * 256], 1)
    where = [0, 15, 16, 33, 64, 69]
    q[where] = gold["video_q"][:, [0, 2, 1]]
    f = frames01.to(dev)
    one = [o.cpu() for o in tracker.track(f, q.to(dev), return_iters=True)]
    for a, b in zip(one, device_run):
        assert torch.equal(a[:, where] if a.dim() == 4 else a[where], b)
    # the engine's NOMINAL launch count (72 T + 2 + chunks x iterations x 53, added up per stage that ran): it proves how many chunks
    # ran, not how many kernels a stage launches
    assert tracker.stats["launches"] == 72 * 5 + 2 + 4 * 53
    for chunk in (16, 1):
        part = [o.cpu() for o in tracker.track(f, q.to(dev), return_iters=True, workspace_queries=chunk)]
        assert tracker.stats["launches"] == 72 * 5 + 2 + -(-70 // chunk) * 4 * 53           # the chunks really ran
        assert all(torch.equal(a, b) for a, b in zip(part, one)), f"chunks of {chunk}"
    assert torch.isfinite(one[3]).all()


def test_two_runs_are_bitwise_equal(dev, gold, tracker, frames01, device_run):
    out = tracker.track(frames01.to(dev), gold["video_q"][:, [0, 2, 1]].to(dev), return_iters=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(out, device_run))
    assert tracker.stats["launches"] == 72 * 5 + 2 + 4 * 53
    from sam_pt_amd import _lib
    assert _lib.workspace_bytes("sampt_tapir_workspace_bytes", tracker._h, 9, 3, 3) > 0          # a sizing pass launches nothing ...
    assert tracker._lib.sampt_tapir_launches(tracker._h) == 72 * 5 + 2 + 4 * 53                   # ... and leaves the last call's count
    assert tracker._lib.sampt_tapir_launches(None) == 0


def test_sampt_runs_with_the_tapir_tracker(dev, tracker):
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
