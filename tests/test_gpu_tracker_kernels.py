"""GPU parity tests, kernel level, of what turns GEMMs and convolutions into a point TRACKER: the window kernels of csrc/pips.hip,
pips2.hip and cotracker.hip one by one through the handle-free entry points of the C ABI, against the plain restatements of
tests/tracker_kernels_ref.py (pinned on the oracle by tests/test_tracker_kernels_cpu.py), at the smallest shapes where such a kernel
can go wrong: taps on the last row / column and off the map, the tail of a clip, carries between windows, a visibility exactly at
the linking threshold, pad columns, n = 67 and 300 around the block sizes.

Shared shapes: feature map 16 x 24 x 128 (levels 16x24, 8x12, 4x6, 2x3), S = 8, the coordinate set E of the restatements.  Every
output buffer is pre-filled with a sentinel (7.0) and carries a guard row behind it: what a kernel does not own must keep it.

Bars (each test prints its worst error; the value measured on an MI355X stands next to the bar):
  (a) moves, selects, one f32 rounding: torch.equal with the f32 restatement.
  (b) four-tap bilinear samples: |err| <= 8 * 2^-24 * max|v| against float64 (weights in [0, 1] summing to 1: at most 6 roundings
      of quantities <= max|v|).
  (c) sin / cos columns: |err| <= 4 * 2^-23 (the 4-ulp bound of the OpenCL profile the device library follows; |value| <= 1).
  (d) correlation sampler: 2e-5 * max|ref|, the bar of test_gpu_kernels.test_corr_sample_vs_oracle.
  (e) a 128-term dot product or a normalisation: error against float64 <= 2 x the error of the same formula evaluated by torch in
      f32 on the CPU, with the project's f32 bars as floors: 2e-6 * max|ref| (test_gemm_f32) for update / finalize / store,
      5e-6 (test_instance_norm) for instnorm1d_relu."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tracker_kernels_ref as K

pytestmark = pytest.mark.gpu

S = 8
H0, W0 = 16, 24
SENT = K.SENTINEL
BAR_B = 8 * 2.0 ** -24
BAR_C = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


_ALIVE = []


@pytest.fixture(autouse=True)
def _arguments_outlive_the_launch():
    """``P(x.to(dev))`` makes the device copy inside the call expression and only its address goes on: the tensor is kept until the
    test is over, so that no argument of a launch is freed memory.  A device error ends the session."""
    yield
    _ALIVE.clear()
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:            # a device fault poisons the process: nothing more is started on the card
            pytest.exit(f"device error after a kernel test, stopping the session: {e}", returncode=3)


def P(t):
    from sam_pt_amd import _lib
    _ALIVE.append(t)
    return _lib.ptr(t)


def St():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what=""):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


class Out:
    """A device buffer of ``shape`` filled with the sentinel, followed by a guard of 64 more sentinels."""

    def __init__(self, dev, *shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.raw = torch.full((self.n + 64,), int(SENT) if dtype != torch.float32 else SENT, dtype=dtype, device=dev)
        self.t = self.raw[:self.n].view(*shape)

    def cpu(self):
        torch.cuda.synchronize()
        assert bool((self.raw[self.n:] == SENT).all()), "the kernel wrote past the end of its output"
        return self.t.cpu()


def untouched(t: torch.Tensor) -> bool:
    return bool((t == SENT).all())


def report(what: str, err: float, bar: float):
    print(f"{what}: worst error {err:.3e}, bar {bar:.3e}")
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def err_of(got: torch.Tensor, ref: torch.Tensor) -> float:
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float((got.double() - ref.double()).abs().max())


@pytest.fixture(scope="module")
def world():
    """Feature maps of 3 frames with their pyramid, track features, E, non-monotone per-point window frames: computed once, never
    modified."""
    from oracle import pips_ref as PO
    g = torch.Generator().manual_seed(2024)
    fmap = torch.randn(3, H0, W0, 128, generator=g)
    pyr = [p.permute(0, 2, 3, 1).contiguous() for p in PO.build_pyramid(fmap.permute(0, 3, 1, 2))]
    ffeats = torch.randn(9, S, 128, generator=g)
    fidx = torch.tensor([[0, 2, 1, 1, 0, 2, 2, 0], [2, 1, 0, 0, 1, 2, 0, 1]] * 5)[:9].int().contiguous()
    coords = K.coords_E(S)
    drift = (torch.rand(9, 2, generator=g) * 17 - 8.5)                       # px per frame: flows up to +-60 px over the window
    fast = (coords + torch.arange(S, dtype=torch.float32)[:, None, None] * drift[None]).contiguous()
    return dict(fmap=fmap, pyr=pyr, ffeats=ffeats, fidx=fidx, coords=coords, fast=fast, times=torch.linspace(0, S, S))


def pyr_ptrs(pyr_d):
    from sam_pt_amd import _lib
    return _lib.ptr_array(pyr_d)


# ---------------------------------------------------------------------------------------------------------------- PIPS
@pytest.mark.parametrize("per_point_frames", [False, True])
def test_pips_sample_feat(lib, dev, world, per_point_frames):
    """bilinear_sample2d at E: integral positions, the last row and column, positions off the map on every side; frame 0 for every
    point, or a permuted frame per point."""
    xy = world["coords"][0].contiguous()
    fi = torch.tensor([2, 0, 1, 1, 2, 0, 0, 2, 1], dtype=torch.int32) if per_point_frames else None
    ref = K.sample_feat(world["fmap"], xy, fi)
    out = Out(dev, 9, 128)
    ok(lib.sampt_pips_sample_feat_f32(P(world["fmap"].to(dev)), H0, W0, P(fi.to(dev)) if fi is not None else None, P(xy.to(dev)), 9,
                                      P(out.t), St()), "sample_feat")
    report("pips_sample_feat (b)", err_of(out.cpu(), ref), BAR_B * float(world["fmap"].abs().max()))     # measured 2.4e-07


@pytest.mark.parametrize("ldx,xoff,fused", [(196, 0, False), (720, 196, False), (720, 392, False), (456, 130, False), (520, 128, True)])
def test_pips_corr_sample_layouts(lib, dev, world, ldx, xoff, fused):
    """The correlation sampler in the row layouts the three engines launch (PIPS with the fused mixer-input tail, PIPS++'s three
    templates, CoTracker), per-point window frames: the 196 columns against CorrBlock.corr + CorrBlock.sample, everything else
    untouched (with the tail the launch owns the whole PIPS row)."""
    ref = K.corr_sample(world["pyr"], world["fidx"], world["ffeats"], world["coords"])
    assert 0.2 < float((ref == 0).float().mean()) < 0.8
    x = Out(dev, 9, S, ldx)
    pyr_d = [p.to(dev) for p in world["pyr"]]
    ok(lib.sampt_pips_corr_sample_ex(pyr_ptrs(pyr_d), H0, W0, P(world["fidx"].to(dev)), S, 9, P(world["ffeats"].to(dev)),
                                     P(world["coords"].to(dev)), P(x.t), ldx, xoff, P(world["times"].to(dev)) if fused else None,
                                     St()), "corr_sample_ex")
    got = x.cpu()
    report(f"pips_corr_sample ldx {ldx} xoff {xoff} (d)", err_of(got[..., xoff:xoff + 196], ref), 2e-5 * float(ref.abs().max()))  # measured 2.1e-06
    if fused:
        assert not bool((got == SENT).any())
    else:
        assert untouched(got[..., :xoff]) and untouched(got[..., xoff + 196:])


@pytest.mark.parametrize("ldx", [519, 520, 580])
def test_pips_build_input_and_fused_tail(lib, dev, world, ldx):
    """k_pips_build_input and the tail fused into the correlation sampler repeat the same arithmetic: identical bits outside the
    correlation columns.  Flows up to +-60 px and times up to 8 put the sin / cos arguments at up to 6e4 rad.  Pad columns are
    exactly 0 and nothing is written past a row (ldx = 519 has no pad)."""
    ff, co, tm = world["ffeats"], world["fast"], world["times"]
    ref = K.pips_build_input(ff, co, tm, ldx)
    assert float(K.flows_from(co).abs().max()) > 50
    ff_d, co_d, tm_d = ff.to(dev), co.to(dev), tm.to(dev)
    a, b = Out(dev, 9, S, ldx), Out(dev, 9, S, ldx)
    ok(lib.sampt_pips_build_input_f32(P(ff_d), P(co_d), P(tm_d), S, 9, P(a.t), ldx, St()), "build_input")
    pyr_d = [p.to(dev) for p in world["pyr"]]
    ok(lib.sampt_pips_corr_sample_ex(pyr_ptrs(pyr_d), H0, W0, P(world["fidx"].to(dev)), S, 9, P(ff_d), P(co_d), P(b.t), ldx, 128,
                                     P(tm_d), St()), "corr_sample_ex")
    xa, xb = a.cpu(), b.cpu()
    assert untouched(xa[..., 128:324])
    assert torch.equal(xa[..., :128], xb[..., :128]) and torch.equal(xa[..., 324:], xb[..., 324:])
    assert torch.equal(xa[..., :128], ff)                                                        # (a)
    assert torch.equal(xa[..., 516:519], ref[..., 516:519].float())                              # (a): flow (one f32 subtraction), time
    assert float(xa[..., 519:].abs().max()) == 0.0 if ldx > 519 else xa.shape[-1] == 519         # pad columns
    report(f"pips_build_input ldx {ldx} sin/cos (c)", err_of(xa[..., 324:516], ref[..., 324:516]), BAR_C)   # measured 6.1e-08


@pytest.mark.parametrize("n", [1, 67])
def test_pips_init_state(lib, dev, n):
    g = torch.Generator().manual_seed(n)
    xys, fi = torch.rand(n, 2, generator=g) * 200 - 20, torch.randn(n, 128, generator=g)
    co, c0, ff = Out(dev, S, n, 2), Out(dev, n, 2), Out(dev, n, S, 128)
    ok(lib.sampt_pips_init_state_f32(P(xys.to(dev)), P(fi.to(dev)), 4.0, S, n, P(co.t), P(c0.t), P(ff.t), St()), "init_state")
    rc, r0, rf = K.pips_init_state(xys, fi, 4.0, S)
    assert torch.equal(co.cpu(), rc) and torch.equal(c0.cpu(), r0) and torch.equal(ff.cpu(), rf)           # (a)


def _update_inputs(n, seed):
    """GroupNorm input with a constant offset of 50 standard deviations on the 128 feature entries: a one-pass variance
    (E[x^2] - mean^2) loses (offset / sigma)^2 * 2^-24 ~ 1.5e-4 of the variance in f32, ten times the bar; the two-pass form keeps
    its error at that of the mean, ~3e-6 sigma."""
    g = torch.Generator().manual_seed(seed)
    delta = torch.randn(n, S, 130, generator=g)
    delta[..., 2:] += 50.0
    return dict(delta=delta, gn_w=1 + 0.1 * torch.randn(128, generator=g), gn_b=0.1 * torch.randn(128, generator=g),
                up_w=torch.randn(128, 128, generator=g) / 128 ** 0.5, up_b=0.1 * torch.randn(128, generator=g),
                ffeats=torch.randn(n, S, 128, generator=g), coords=torch.rand(S, n, 2, generator=g) * 30,
                coords0=torch.rand(n, 2, generator=g) * 30)


@pytest.mark.parametrize("locked", [True, False])
def test_pips_update(lib, dev, locked):
    """ffeats += gelu(Linear(GroupNorm(1, 128)(delta))) against float64; coords += delta[:2] bit for bit, frame 0 locked to coords0
    when given (PIPS) and updated like the rest when not (CoTracker)."""
    n = 5
    w = _update_inputs(n, 7)
    ref = K.feature_update(w["delta"], w["gn_w"], w["gn_b"], w["up_w"], w["up_b"], w["ffeats"])
    f32 = K.feature_update(w["delta"], w["gn_w"], w["gn_b"], w["up_w"], w["up_b"], w["ffeats"], dtype=torch.float32)
    ff, co = Out(dev, n, S, 128), Out(dev, S, n, 2)
    ff.t.copy_(w["ffeats"]), co.t.copy_(w["coords"])
    ok(lib.sampt_pips_apply_update_f32(P(w["delta"].to(dev)), P(w["gn_w"].to(dev)), P(w["gn_b"].to(dev)),
                                       P(w["up_w"].t().contiguous().to(dev)), P(w["up_b"].to(dev)), P(ff.t), P(co.t),
                                       P(w["coords0"].to(dev)) if locked else None, S, n, St()), "apply_update")
    assert torch.equal(co.cpu(), K.coords_update(w["delta"], w["coords"], w["coords0"] if locked else None))          # (a)
    yard = err_of(f32, ref)
    report(f"pips_update features (e), torch f32 on the CPU {yard:.3e}", err_of(ff.cpu(), ref),
           max(2 * yard, 2e-6 * float(ref.abs().max())))                                         # measured 1.3e-05 (yardstick 1.6e-05)


def _vis_head(n, seed):
    """Track features and a visibility head; rows 1 and n*S - 2 are built to give logits of +200 and -200."""
    g = torch.Generator().manual_seed(seed)
    ff = torch.randn(n, S, 128, generator=g)
    vw, vb = 0.3 * torch.randn(128, generator=g), torch.tensor([0.25])
    flat = ff.view(n * S, 128)
    unit = vw.double() / float(vw.double() @ vw.double())
    flat[1], flat[n * S - 2] = ((200.0 - 0.25) * unit).float(), ((-200.0 - 0.25) * unit).float()
    big = torch.zeros(n * S, dtype=torch.bool)
    big[1] = big[n * S - 2] = True
    return ff, vw, vb, big.view(n, S).t().contiguous()                # big [S][n]: where the +-200 logits sit


def test_pips_finalize(lib, dev):
    n = 5
    g = torch.Generator().manual_seed(3)
    ff, vw, vb, big = _vis_head(n, 3)
    co = torch.rand(S, n, 2, generator=g) * 60 - 5
    tr, vi = Out(dev, S, n, 2), Out(dev, S, n)
    ok(lib.sampt_pips_finalize_f32(P(ff.to(dev)), P(vw.to(dev)), P(vb.to(dev)), P(co.to(dev)), 4.0, S, n, P(tr.t), P(vi.t), St()),
       "finalize")
    assert torch.equal(tr.cpu(), co * 4.0)                                                         # (a)
    got = vi.cpu()
    lg = K.vis_logits(ff, vw, vb)
    assert abs(float(lg[big][0]) - 200) < 1e-3 and abs(float(lg[big][1]) + 200) < 1e-3
    assert got[big].tolist() == [1.0, 0.0]                                                         # saturated: exactly 1 / 0, no NaN
    ref, f32 = torch.sigmoid(lg), torch.sigmoid(K.vis_logits(ff, vw, vb, dtype=torch.float32))
    yard = err_of(f32[~big], ref[~big])
    report(f"pips_finalize visibility (e), torch f32 on the CPU {yard:.3e}", err_of(got[~big], ref[~big]),
           max(2 * yard, 2e-6 * float(ref[~big].abs().max())))                                    # measured 8.2e-08 (yardstick 1.5e-07)


def _chain_case(n, T):
    """Chains anchored on frame 0, mid-clip, T - 2 and T - 1 (finished from the start), mixed directions."""
    starts = [(0, T // 2, T - 2, T - 1, 0)[i % 5] if T > 2 else 0 for i in range(n)]
    q = torch.tensor([[starts[i], 100.0 * i + 0.5, 3.0 + i] for i in range(n)], dtype=torch.float32)
    flip = torch.tensor([(i // 2) % 2 for i in range(n)], dtype=torch.uint8)
    return q, flip


def _scripted_round(cur, T, n):
    tr, vi = torch.empty(S, n, 2), torch.empty(S, n)
    for i in range(n):
        xy, lg = K.scripted_window(i, min(int(cur[i]), T - 1))
        tr[:, i], vi[:, i] = xy, torch.sigmoid(lg)
    return tr, vi


@pytest.mark.parametrize("n,T", [(1, 5), (67, 9), (300, 20)])
def test_pips_chain_kernels(lib, dev, n, T):
    """chain_init, round_begin and round_end against their restatements, bit for bit (a), round after round until no chain is active:
    n = 67 crosses a 64-thread block, n = 300 makes round_end's single 256-thread block loop twice; T = 5 ends inside the first
    window; the scripted visibilities include one exactly at the threshold; one chain carries an anchor beyond T - 1."""
    q, flip = _chain_case(n, T)
    cur_d, traj_d, vis_d = Out(dev, n, dtype=torch.int32), Out(dev, T, n, 2), Out(dev, T, n)
    ok(lib.sampt_pips_chain_init(P(q.to(dev)), n, T, P(cur_d.t), P(traj_d.t), P(vis_d.t), St()), "chain_init")
    cur, traj, vis = K.chain_init(q, T)
    assert torch.equal(cur_d.cpu().long(), cur) and torch.equal(traj_d.cpu(), traj) and torch.equal(vis_d.cpu(), vis)
    if n > 3:
        cur[3] = T + 2                                           # a finished chain may sit beyond the clip
        cur_d.t.copy_(cur.int())
    flip_d = flip.to(dev)
    rounds = 0
    while True:
        first = rounds == 0
        fidx_d, xys_d = Out(dev, n, S, dtype=torch.int32), Out(dev, n, 2)
        xyf_d, f0_d = Out(dev, n, 2), Out(dev, n, dtype=torch.int32)
        ok(lib.sampt_pips_round_begin(P(cur_d.t), P(flip_d), P(traj_d.t), T, n, S, P(fidx_d.t), P(xys_d.t), P(xyf_d.t) if first else None,
                                      P(f0_d.t) if first else None, 4.0, St()), "round_begin")
        fidx, xys, xyf, f0 = K.round_begin(cur, flip, traj, T, S, 4.0)
        assert torch.equal(fidx_d.cpu().long(), fidx) and torch.equal(xys_d.cpu(), xys)
        assert int(fidx.min()) >= 0 and int(fidx.max()) <= T - 1
        if first:
            assert torch.equal(xyf_d.cpu(), xyf) and torch.equal(f0_d.cpu().long(), f0)
        else:
            assert untouched(xyf_d.cpu()) and untouched(f0_d.cpu())
        tr, vi = _scripted_round(cur, T, n)
        na_d = Out(dev, 1, dtype=torch.int32)
        ok(lib.sampt_pips_round_end(P(cur_d.t), P(tr.to(dev)), P(vi.to(dev)), T, n, S, 0.9, P(traj_d.t), P(vis_d.t), P(na_d.t), St()),
           "round_end")
        cur, traj, vis, n_active = K.round_end(cur, tr, vi, T, S, 0.9, traj, vis)
        assert torch.equal(cur_d.cpu().long(), cur) and torch.equal(traj_d.cpu(), traj) and torch.equal(vis_d.cpu(), vis)
        assert int(na_d.cpu()[0]) == n_active
        rounds += 1
        if n_active == 0:
            break
        assert rounds < T, "the chain does not advance"
    assert bool((cur >= T - 1).all())
    print(f"pips chain n {n} T {T}: {rounds} rounds, bit for bit")


def test_pips_round_end_thresholds(lib, dev):
    """The linking sweep at its edges: a visibility exactly AT the threshold in force is not taken, neither at 0.9 nor at the
    threshold of the fourth sweep (0.84000003 in the float32 arithmetic of the reference; 0.84 in exact arithmetic would take it),
    one ulp above it is; a window of zeros is swept until the threshold turns negative and then links to its last frame."""
    n, T = 4, 9
    thr3 = float(K.decayed_threshold(3))
    vi = torch.zeros(S, n)
    vi[1, 0], vi[5, 0] = thr3, 0.83
    vi[1, 1], vi[5, 1] = float(np.nextafter(np.float32(thr3), np.float32(1))), 0.83
    vi[2, 2], vi[3, 2] = 0.95, 0.9
    tr = torch.arange(S * n * 2, dtype=torch.float32).view(S, n, 2)
    q = torch.tensor([[0.0, 1.0 + i, 2.0] for i in range(n)])
    cur, traj, vis = K.chain_init(q, T)
    cur_d, traj_d, vis_d, na_d = Out(dev, n, dtype=torch.int32), Out(dev, T, n, 2), Out(dev, T, n), Out(dev, 1, dtype=torch.int32)
    cur_d.t.copy_(cur.int()), traj_d.t.copy_(traj), vis_d.t.copy_(vis)
    ok(lib.sampt_pips_round_end(P(cur_d.t), P(tr.to(dev)), P(vi.to(dev)), T, n, S, 0.9, P(traj_d.t), P(vis_d.t), P(na_d.t), St()), "round_end")
    cur, traj, vis, n_active = K.round_end(cur, tr, vi, T, S, 0.9, traj, vis)
    assert cur.tolist() == [5, 1, 2, 7] and n_active == 4
    assert torch.equal(cur_d.cpu().long(), cur) and torch.equal(traj_d.cpu(), traj) and torch.equal(vis_d.cpu(), vis)
    assert int(na_d.cpu()[0]) == n_active


# -------------------------------------------------------------------------------------------------------------- PIPS++
@pytest.mark.parametrize("have_init", [0, 1])
def test_pips2_init(lib, dev, world, have_init):
    """coords = trajs0 / 8 and the frame-0 backup (a); without feat_init the three templates are the feature of the point's first
    window frame at its frame-0 position on every row (b); with it they are left alone."""
    trajs0 = (world["coords"] * 8.0).contiguous()
    co, bak = Out(dev, S, 9, 2), Out(dev, 9, 2)
    f1, f2, f4 = Out(dev, 9, S, 128), Out(dev, 9, S, 128), Out(dev, 9, S, 128)
    ok(lib.sampt_pips2_init_f32(P(trajs0.to(dev)), P(world["fmap"].to(dev)), H0, W0, P(world["fidx"].to(dev)), 8.0, S, 9, have_init,
                                P(co.t), P(bak.t), P(f1.t), P(f2.t), P(f4.t), St()), "pips2_init")
    rc, rb = K.pips2_init(trajs0, 8.0)
    assert torch.equal(co.cpu(), rc) and torch.equal(bak.cpu(), rb) and torch.equal(rb, world["coords"][0])   # (a)
    g1, g2, g4 = f1.cpu(), f2.cpu(), f4.cpu()
    if have_init:
        assert untouched(g1) and untouched(g2) and untouched(g4)
        return
    assert torch.equal(g1, g2) and torch.equal(g1, g4)
    ref = K.sample_feat(world["fmap"], rb, world["fidx"][:, 0])[:, None, :].repeat(1, S, 1)
    report("pips2_init templates (b)", err_of(g1, ref), BAR_B * float(world["fmap"].abs().max()))     # measured 2.0e-07


@pytest.mark.parametrize("S_", [8, 3])
def test_pips2_templates(lib, dev, world, S_):
    """Row (pt, s) of f2 / f4 = the map of window frame max(s - 2, 0) / max(s - 4, 0) at the point's position on THAT frame, with
    shuffled window frames; at S = 3 every s - 4 clips to frame 0."""
    co = world["coords"][:S_].contiguous()
    fidx = world["fidx"][:, :S_].contiguous()
    r2, r4 = K.pips2_templates(world["fmap"], fidx, co, 2), K.pips2_templates(world["fmap"], fidx, co, 4)
    assert (S_ == 8) == (not torch.equal(r2, r4))                # the lags are told apart at S = 8 only
    f2, f4 = Out(dev, 9, S_, 128), Out(dev, 9, S_, 128)
    ok(lib.sampt_pips2_templates_f32(P(world["fmap"].to(dev)), H0, W0, P(fidx.to(dev)), P(co.to(dev)), S_, 9, P(f2.t), P(f4.t), St()),
       "pips2_templates")
    bar = BAR_B * float(world["fmap"].abs().max())
    report(f"pips2_templates S {S_} lag 2 (b)", err_of(f2.cpu(), r2), bar)                       # measured 2.7e-07
    report(f"pips2_templates S {S_} lag 4 (b)", err_of(f4.cpu(), r4), bar)                       # measured 2.4e-07


@pytest.mark.parametrize("S_", [8, 3, 2])
def test_pips2_build_input(lib, dev, world, S_):
    """Columns [588, 720) of the PIPS++ row: posemb_sincos_2d_xy of the frame-to-frame flow (the last frame repeats the previous
    one) with the frequency table the engine uploads, the flow itself, two zero pad columns; [0, 588) belongs to the sampler."""
    from sam_pt_amd.pack import pack_pips2
    omega = pack_pips2({}, "cpu")["__omega"]
    co = world["fast"][:S_].contiguous()
    ref = K.pips2_build_input(co, omega)
    assert torch.equal(ref[:, -1, 128:130], ref[:, -2, 128:130])
    x = Out(dev, 9, S_, 720)
    ok(lib.sampt_pips2_build_input_f32(P(co.to(dev)), P(omega.to(dev)), S_, 9, P(x.t), 720, St()), "pips2_build_input")
    got = x.cpu()
    assert untouched(got[..., :588])
    assert torch.equal(got[..., 716:718], ref[..., 128:130].float()) and float(got[..., 718:].abs().max()) == 0.0      # (a)
    report(f"pips2_build_input S {S_} sin/cos (c)", err_of(got[..., 588:716], ref[..., :128]), BAR_C)   # measured 5.8e-08


@pytest.mark.parametrize("n,S_,C_", [(5, 8, 128), (3, 5, 200), (2, 2, 96)])
@pytest.mark.parametrize("in_place", [False, True])
def test_instnorm1d_relu(lib, dev, n, S_, C_, in_place):
    """relu(InstanceNorm1d over the S frames) against float64, out of place and in place (as the engine calls it); a channel that
    is constant over time normalises to 0 (exactly: 2.5 * S is exact in f32)."""
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(n, S_, C_, generator=g) * 3 + 1
    x[:, :, 3] = 2.5
    ref, f32 = K.instnorm1d_relu(x), K.instnorm1d_relu(x, dtype=torch.float32)
    src, dst = Out(dev, n, S_, C_), Out(dev, n, S_, C_)
    src.t.copy_(x)
    ok(lib.sampt_instnorm1d_relu_f32(P(src.t), P(src.t if in_place else dst.t), n, S_, C_, St()), "instnorm1d_relu")
    got = (src if in_place else dst).cpu()
    if not in_place:
        assert torch.equal(src.cpu(), x)
    yard = err_of(f32, ref)
    bar = max(2 * yard, 5e-6)
    assert float(got[:, :, 3].abs().max()) == 0.0
    report(f"instnorm1d_relu {(n, S_, C_)} (e), torch f32 on the CPU {yard:.3e}", err_of(got, ref), bar)   # measured 3.9e-07, 3.8e-07, 4.1e-06 (yardsticks 3.0e-07, 2.9e-07, 5.3e-06)


@pytest.mark.parametrize("cin,cout", [(128, 128), (128, 256), (96, 131)])
@pytest.mark.parametrize("relu", [0, 1])
def test_add_chanpad(lib, dev, cin, cout, relu):
    """The residual of ResidualBlock1d with zero-padded channels: an odd difference (35) pads 17 on the left and 18 on the right."""
    g = torch.Generator().manual_seed(cout)
    out, ident = torch.randn(37, cout, generator=g), torch.randn(37, cin, generator=g)
    o = Out(dev, 37, cout)
    o.t.copy_(out)
    ok(lib.sampt_add_chanpad_f32(P(o.t), P(ident.to(dev)), 37, cin, cout, relu, St()), "add_chanpad")
    assert torch.equal(o.cpu(), K.add_chanpad(out, ident, bool(relu)))                            # (a)


@pytest.mark.parametrize("S_,n", [(8, 1), (8, 67), (2, 1), (2, 67)])
@pytest.mark.parametrize("last", [0, 1])
def test_pips2_apply_delta(lib, dev, S_, n, last):
    g = torch.Generator().manual_seed(S_ * n)
    delta, bak = torch.randn(n, S_, 2, generator=g), torch.rand(n, 2, generator=g) * 30
    coords = torch.rand(S_, n, 2, generator=g) * 30
    co, tr = Out(dev, S_, n, 2), Out(dev, S_, n, 2)
    co.t.copy_(coords)
    ok(lib.sampt_pips2_apply_delta_f32(P(delta.to(dev)), P(bak.to(dev)), 8.0, S_, n, last, P(co.t), P(tr.t), St()), "apply_delta")
    rc, rt = K.pips2_apply_delta(delta, bak, 8.0, coords)
    assert torch.equal(co.cpu(), rc)                                                               # (a)
    assert torch.equal(tr.cpu(), rt) if last else untouched(tr.cpu())


# ----------------------------------------------------------------------------------------------------------- CoTracker
@pytest.mark.parametrize("T,n", [(1, 300), (12, 5)])
def test_cot_prepare(lib, dev, T, n):
    g = torch.Generator().manual_seed(T)
    qxy = torch.rand(n, 2, generator=g) * 300 - 20
    qt = torch.randint(0, T, (n,), generator=g).int()
    fmap_ = torch.randperm(T + 3, generator=g)[:T].int()
    xy0, fp, tr, vi = Out(dev, n, 2), Out(dev, n, dtype=torch.int32), Out(dev, T, n, 2), Out(dev, T, n)
    ok(lib.sampt_cot_prepare(P(qxy.to(dev)), P(qt.to(dev)), P(fmap_.to(dev)), 4.0, n, T, P(xy0.t), P(fp.t), P(tr.t), P(vi.t), St()),
       "cot_prepare")
    r = K.cot_prepare(qxy, qt, fmap_, 4.0, T)
    assert torch.equal(xy0.cpu(), r[0]) and torch.equal(fp.cpu(), r[1]) and torch.equal(tr.cpu(), r[2]) and torch.equal(vi.cpu(), r[3])
    assert float(r[2].abs().max()) == 0.0 and bool((r[3] == 0.5).all())


@pytest.mark.parametrize("ind,S_local,prev,na,qt", [(0, 8, 0, 4, (0, 2, 3, 5, 9, 10, 11)), (4, 8, 4, 7, (0, 2, 3, 5, 8, 9, 11)),
                                                    (8, 5, 7, 7, (0, 2, 3, 5, 8, 9, 11)), (4, 8, 0, 3, (3, 4, 9))])
def test_cot_window_init(lib, dev, ind, S_local, prev, na, qt):
    """The state a CoTracker window starts from: carried points take the previous window's second half (coordinates and visibility
    logits), new ones their query position and logit 10; the track mask opens at the query frame (before, at or after ``ind``) or,
    for carried points, at the frames no window has written; the tail of a short window repeats its last frame and is masked."""
    T, n = 13, len(qt)
    g = torch.Generator().manual_seed(ind * 10 + na)
    qt_t = torch.tensor(qt, dtype=torch.int32)
    xy0 = torch.rand(n, 2, generator=g) * 30
    fmap_ = torch.randperm(T + 3, generator=g)[:T].int()
    cp, vp = torch.rand(S, max(prev, 1), 2, generator=g) * 30, torch.randn(S, max(prev, 1), generator=g) * 4
    fi = torch.randn(n, 128, generator=g)
    co, vs, mk = Out(dev, S, na, 2), Out(dev, S, na), Out(dev, S, na)
    fx, ff = Out(dev, na, S, dtype=torch.int32), Out(dev, na, S, 128)
    ok(lib.sampt_cot_window_init(ind, S_local, prev, na, S, P(qt_t.to(dev)), P(xy0.to(dev)), P(fmap_.to(dev)),
                                 P(cp.to(dev)) if prev else None, P(vp.to(dev)) if prev else None, P(fi.to(dev)), P(co.t), P(vs.t),
                                 P(mk.t), P(fx.t), P(ff.t), St()), "cot_window_init")
    r = K.cot_window_init(ind, S_local, prev, na, S, qt_t, xy0, fmap_, cp, vp, fi)
    assert torch.equal(co.cpu(), r[0]) and torch.equal(vs.cpu(), r[1]) and torch.equal(mk.cpu(), r[2])       # (a)
    assert torch.equal(fx.cpu(), r[3]) and torch.equal(ff.cpu(), r[4])
    assert 0 < float(r[2].sum()) < r[2].numel()


def test_cot_pos_embed(lib, dev, world):
    """sample_pos_embed at E on a 12 x 16 grid, from the two 1-D tables the engine uploads (the 2-D grid's column and row halves)."""
    from oracle import cotracker_ref as CO
    from sam_pt_amd.pack import cotracker_pos_tables
    grid = CO.sincos_2d_grid(456, 12, 16)
    px, py = grid[0, :, :228].contiguous(), grid[:, 0, 228:].contiguous()
    tx, ty = cotracker_pos_tables(12, 16)
    assert torch.equal(px, tx) and torch.equal(py, ty)
    xy = world["coords"][0].contiguous()
    pos = Out(dev, 9, 456)
    ok(lib.sampt_cot_pos_embed_f32(P(xy.to(dev)), P(px.to(dev)), P(py.to(dev)), 12, 16, 456, 9, P(pos.t), St()), "cot_pos_embed")
    report("cot_pos_embed (b)", err_of(pos.cpu(), K.cot_pos_embed(xy, grid)), BAR_B * float(grid.abs().max()))   # measured 8.3e-08


def test_cot_build_input(lib, dev, world):
    """The transformer's input row: (term + position embedding) + time embedding over [flow embedding | correlation, already in the
    row | track feature | mask, visibility logit].  Two f32 additions on top of bar (c): 6 * 2^-23 * max(1, B), B the largest
    partial sum of the row."""
    from sam_pt_amd.pack import sincos_1d
    g = torch.Generator().manual_seed(9)
    na = 9
    ff, co = world["ffeats"], world["fast"]
    visin, mask = torch.randn(S, na, generator=g) * 5, (torch.rand(S, na, generator=g) > 0.4).float()
    pos = torch.randn(na, 456, generator=g)
    times = sincos_1d(456, torch.linspace(0, S - 1, S).numpy())
    corr = torch.randn(na, S, 196, generator=g) * 3
    x = Out(dev, na, S, 456)
    x.t[..., 130:326] = corr.to(dev)
    ok(lib.sampt_cot_build_input_f32(P(ff.to(dev)), P(co.to(dev)), P(visin.to(dev)), P(mask.to(dev)), P(pos.to(dev)), P(times.to(dev)),
                                     S, na, P(x.t), St()), "cot_build_input")
    terms = K.cot_build_input_terms(ff, co, visin, mask, corr)
    ref = (terms + pos[:, None].double()) + times[None].double()
    B = torch.stack([terms.abs(), (terms + pos[:, None].double()).abs(), ref.abs()]).amax(dim=(0, 3)).clamp(min=1.0)      # [na][S]
    got = x.cpu()
    rel = float(((got.double() - ref).abs() / B[..., None]).max())
    report("cot_build_input (c + two additions), relative to max(1, B)", rel, 6 * 2.0 ** -23)        # measured 8.6e-08
    assert torch.equal(got[..., :2], K.flows_from(co) + pos[:, None, :2] + times[None, :, :2])     # flow columns: three f32 operations


@pytest.mark.parametrize("S_local,ind,na,n_total", [(8, 0, 4, 9), (5, 8, 7, 7)])
def test_cot_window_store(lib, dev, S_local, ind, na, n_total):
    """End of a window: the carries (coordinates bit for bit, visibility LOGITS against float64) and rows ind .. ind + S_local - 1,
    columns < na of the outputs; everything else keeps what it held.  Logits of +-200 give visibilities of exactly 1 and 0."""
    T = 13
    g = torch.Generator().manual_seed(na)
    ff, vw, vb, big = _vis_head(na, 10 + na)
    co = torch.rand(S, na, 2, generator=g) * 40 - 5
    cp, vp, tr, vi = Out(dev, S, na, 2), Out(dev, S, na), Out(dev, T, n_total, 2), Out(dev, T, n_total)
    ok(lib.sampt_cot_window_store_f32(P(ff.to(dev)), P(vw.to(dev)), P(vb.to(dev)), P(co.to(dev)), 4.0, S, na, ind, S_local, n_total,
                                      P(cp.t), P(vp.t), P(tr.t), P(vi.t), St()), "cot_window_store")
    lg, lg32 = K.vis_logits(ff, vw, vb), K.vis_logits(ff, vw, vb, dtype=torch.float32)
    got_lg, got_tr, got_vi = vp.cpu(), tr.cpu(), vi.cpu()
    assert torch.equal(cp.cpu(), co)                                                               # (a)
    yard = err_of(lg32[~big], lg[~big])
    report(f"cot_window_store logits (e), torch f32 on the CPU {yard:.3e}", err_of(got_lg[~big], lg[~big]),
           max(2 * yard, 2e-6 * float(lg[~big].abs().max())))                                     # measured 5.3e-07, 1.2e-06 (yardsticks 8.4e-07, 9.6e-07)
    assert float((got_lg[big].double() - lg[big]).abs().max()) <= 2e-6 * 200
    _, _, rt, rv = K.cot_window_store(got_lg, co, 4.0, ind, S_local, torch.full((T, n_total, 2), SENT), torch.full((T, n_total), SENT))
    assert torch.equal(got_tr, rt)                                                                 # (a), sentinel outside the window
    own = rv != SENT
    assert torch.equal(own, rt[..., 0] != SENT) and int(own.sum()) == S_local * na
    assert untouched(got_vi[~own])
    report("cot_window_store visibilities vs sigmoid of the stored logits", err_of(got_vi[own], rv[own]), 2e-6)   # measured 6.0e-08
    sat = big[:S_local]
    assert got_vi[ind:ind + S_local, :na][sat].tolist() == [1.0, 0.0][:int(sat.sum())]


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("sh,sw,dh,dw", [(9, 13, 21, 30), (40, 52, 20, 26), (16, 24, 16, 24)])
def test_resize_planes(lib, dev, u8, sh, sw, dh, dw):
    """F.interpolate(bilinear, align_corners=False) of uint8 and f32 planes: up (odd sizes, no common factor), down by 2, identity."""
    g = torch.Generator().manual_seed(sh)
    x = torch.randint(0, 256, (3, sh, sw), generator=g).to(torch.uint8) if u8 else torch.randn(3, sh, sw, generator=g) * 2
    ref = F.interpolate(x.double()[None], size=(dh, dw), mode="bilinear", align_corners=False)[0]
    out = Out(dev, 3, dh, dw)
    ok(lib.sampt_resize_frames_f32(P(x.to(dev)), int(u8), 3, sh, sw, P(out.t), dh, dw, St()), "resize_planes")
    report(f"resize_planes {'u8' if u8 else 'f32'} {(sh, sw)} -> {(dh, dw)} (b)", err_of(out.cpu(), ref),
           BAR_B * (255.0 if u8 else float(x.abs().max())))
    # measured (worst error / bar): 9x13 -> 21x30 u8 2.5e-05 / 1.2e-04, f32 4.4e-07 / 2.7e-06; 40x52 -> 20x26 u8 0 / 1.2e-04, f32 1.8e-07 /
    # 3.3e-06; 16x24 -> 16x24 u8 0, f32 0.  With the position formed as an f32 product (torch's operation order, the kernel before this
    # test) the first pair read 8.1e-05 and 2.75e-06: the f32 case was over its bar.


# ------------------------------------------------------------------------------------------- one window per learned tracker
def _floored_bar(what, floor, base):
    bar = max(base, 4 * floor)
    print(f"{what}: oracle noise floor (weights * (1 + 1e-7 N(0, 1))) {floor:.3e}, bar {bar:.3e}")
    return bar


def test_pips_window_at_the_edges(dev):
    """sampt_pips_update_f32 with E (scaled by the stride) as query positions — on the frame border, integral, off the frame on
    every side — against Pips.forward fed OUR feature maps, at the bars of test_update_window_vs_oracle (2e-3 px, 1e-4) or 4 x
    the oracle's own noise floor on these inputs if that is larger; past a floor of 0.05 px the window is cut to 2 iterations."""
    from oracle import noise_floor as NF
    from oracle import pips_ref as O
    from sam_pt_amd import _lib
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.weights import init_pips_state_dict
    from tests.util import synthetic_clip
    sd = init_pips_state_dict(72)
    frames, _ = synthetic_clip(T=12, H=128, W=256, seed=72)
    trk = PipsPointTracker(state_dict=sd)
    pyr = trk.compute_pyramid(frames[:8].to(dev))
    fm = pyr[0].permute(0, 3, 1, 2).cpu()
    xys = (K.coords_E(1)[0] * 4.0).contiguous()
    n = xys.shape[0]
    for iters in (6, 2):
        preds, vlog, ffeat = O.pips_forward(sd, xys, fm, None, iters=iters)
        p2, v2, _ = O.pips_forward(NF.perturbed(sd, 1e-7), xys, fm, None, iters=iters)
        floor_px, floor_vis = float((preds[-1] - p2[-1]).abs().max()), float((torch.sigmoid(vlog) - torch.sigmoid(v2)).abs().max())
        if floor_px <= 0.05:
            break
    lib = _lib.load()
    nb = C.c_size_t()
    _lib.check(lib.sampt_pips_update_workspace_bytes(trk._h, n, C.byref(nb)), "ws")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    fi = torch.empty(n, 128, device=dev)
    xy0 = (xys / 4.0).contiguous().to(dev)
    _lib.check(lib.sampt_pips_sample_feat_f32(P(pyr[0]), 32, 64, None, P(xy0), n, P(fi), St()), "feat")
    report("pips window: feat_init (b)", err_of(fi.cpu(), K.sample_feat(pyr[0].cpu(), xy0.cpu())), BAR_B * float(fm.abs().max()))   # measured 2.9e-07
    fidx = torch.arange(8, dtype=torch.int32, device=dev).repeat(n, 1).contiguous()
    tr, vi = torch.empty(8, n, 2, device=dev), torch.empty(8, n, device=dev)
    _lib.check(lib.sampt_pips_update_f32(trk._h, _lib.ptr_array(pyr), 32, 64, P(fidx), n, P(xys.to(dev)), P(fi), iters, P(tr), P(vi),
                                         P(ws), nb.value, St()), "update")
    print(f"pips window at E: {iters} iterations")
    # measured at 6 iterations: 3.1e-05 px against a floor of 3.1e-05 px; visibility 8.0e-06 against a floor of 8.5e-06
    report("pips window trajectory (px)", err_of(tr.cpu(), preds[-1]), _floored_bar("trajectory", floor_px, 2e-3))
    report("pips window visibility", err_of(vi.cpu(), torch.sigmoid(vlog)), _floored_bar("visibility", floor_vis, 1e-4))


def test_pips2_window_at_the_edges(dev):
    """The same for sampt_pips2_update_f32 (through PipsPlusPlusPointTracker._track, one chunk of 12 frames) against pips2_forward
    fed our stride-8 maps."""
    from oracle import noise_floor as NF
    from oracle import pips2_ref as O2
    from sam_pt_amd.point_tracker import PipsPlusPlusPointTracker
    from sam_pt_amd.weights import init_pips2_state_dict
    from tests.util import synthetic_clip
    sd = init_pips2_state_dict(72)
    frames, _ = synthetic_clip(T=12, H=128, W=256, seed=72)
    q = (K.coords_E(1)[0] * 8.0).contiguous()
    for iters in (16, 2):
        trk = PipsPlusPlusPointTracker(state_dict=sd, iters=iters)
        pyr = trk.compute_pyramid(frames.to(dev))
        fm = pyr[0].permute(0, 3, 1, 2).cpu()
        preds, _ = O2.pips2_forward(sd, q[None].repeat(12, 1, 1), fm, iters=iters)
        p2, _ = O2.pips2_forward(NF.perturbed(sd, 1e-7), q[None].repeat(12, 1, 1), fm, iters=iters)
        floor_px = float((preds[-1] - p2[-1]).abs().max())
        if floor_px <= 0.05:
            break
    got = trk._track(pyr, list(range(12)), q)
    print(f"pips2 window at E: {iters} iterations")
    # measured at 16 iterations: 1.4e-04 px against a floor of 1.2e-04 px
    report("pips2 window trajectory (px)", err_of(got.cpu(), preds[-1]), _floored_bar("trajectory", floor_px, 2e-3))
