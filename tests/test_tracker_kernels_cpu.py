"""CPU side of the trackers' kernel tests (no GPU needed): the restatements of tests/tracker_kernels_ref.py pinned on the oracle
— the PIPS chain kernels on ``PipsTrackerRef._one_direction``, CoTracker's prepare / window init / window store on
``cotracker_forward``, both with the network replaced by a scripted stub, and the sin/cos restatements on the oracle's embeddings —
and the C ABI surface of the kernel-level entry points with their refusals (which return before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import cotracker_ref as CO
from oracle import pips2_ref as P2
from oracle import pips_ref as PO
from tests import tracker_kernels_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_pips_corr_sample_ex", "sampt_pips_build_input_f32", "sampt_pips_init_state_f32", "sampt_pips_apply_update_f32",
               "sampt_pips_finalize_f32", "sampt_pips_chain_init", "sampt_pips_round_begin", "sampt_pips_round_end",
               "sampt_pips2_init_f32", "sampt_pips2_templates_f32", "sampt_pips2_build_input_f32", "sampt_instnorm1d_relu_f32",
               "sampt_add_chanpad_f32", "sampt_pips2_apply_delta_f32", "sampt_cot_prepare", "sampt_cot_window_init",
               "sampt_cot_pos_embed_f32", "sampt_cot_build_input_f32", "sampt_cot_window_store_f32")
S = 8


def run_restated_chain(q: torch.Tensor, flip: torch.Tensor, T: int, thr0: float = 0.9, max_rounds: int = 64):
    """chain_init, then rounds of round_begin -> scripted windows -> round_end until no chain is active.  -> traj, vis, cur,
    per-chain list of (anchor, window frames) of every round in which the chain was still active."""
    n = q.shape[0]
    cur, traj, vis = K.chain_init(q, T)
    hist = [[] for _ in range(n)]
    for _ in range(max_rounds):
        fidx, xys, _, _ = K.round_begin(cur, flip, traj, T, S, 4.0)
        tr, vi = torch.empty(S, n, 2), torch.empty(S, n)
        for i in range(n):
            f = min(int(cur[i]), T - 1)
            assert torch.equal(xys[i], traj[f, i])
            xy, lg = K.scripted_window(i, f, thr0)
            tr[:, i], vi[:, i] = xy, torch.sigmoid(lg)
            if int(cur[i]) < T - 1:
                hist[i].append((f, fidx[i].tolist()))
        cur, traj, vis, n_active = K.round_end(cur, tr, vi, T, S, thr0, traj, vis)
        assert n_active == int((cur < T - 1).sum())
        if n_active == 0:
            return traj, vis, cur, hist
    raise AssertionError("the restated chain did not finish")


@pytest.mark.parametrize("T", [5, 9, 20])
@pytest.mark.parametrize("flipped", [False, True])
def test_chain_restatement_equals_the_oracle_tracker(monkeypatch, T, flipped):
    """chain_init / round_begin / round_end == PipsTrackerRef._one_direction with Pips.forward replaced by the script: T < 8 (the
    window's tail repeats the last frame), T = 9, T = 20; queries on frame 0, mid-clip, T - 2 and the last frame; every script of
    ``scripted_window``; the time-flipped pass."""
    n = 10
    starts = [0, 0, 0, 0, 0, T // 2, T - 2, T - 1, 1, T // 2]
    q = torch.tensor([[t, 100.0 * i + 0.5, 3.0 + i] for i, t in enumerate(starts)], dtype=torch.float32)
    index_of = (lambda t: T - 1 - t) if flipped else (lambda t: t)
    rgbs = torch.arange(T, dtype=torch.uint8).reshape(T, 1, 1, 1).repeat(1, 3, 8, 8)
    seen, at_threshold = [[] for _ in range(n)], []

    def fake_fnet(sd, x, stride):          # a map that carries the ORIGINAL frame number
        t = torch.round((x[:, 0, 0, 0] + 1) / 2 * 255)
        return t.reshape(-1, 1, 1, 1).repeat(1, 128, 2, 2)

    def fake_forward(sd, xys, fm, feat_init, iters=6, stride=4, S=8, trace=None):
        frames = [int(v) for v in fm[:, 0, 0, 0].tolist()]
        f = index_of(frames[0])                                 # direction time of the anchor
        ids = [int(v) for v in torch.div(xys[:, 0], 100, rounding_mode="floor").tolist()]
        out = [K.scripted_window(i, f) for i in ids]
        for i in ids:
            seen[i].append((f, frames))
        vlog = torch.stack([o[1] for o in out], dim=1)
        at_threshold.append(bool((torch.sigmoid(vlog) == 0.9).any()))
        return [torch.stack([o[0] for o in out], dim=1)], vlog, None

    monkeypatch.setattr(PO, "fnet", fake_fnet)
    monkeypatch.setattr(PO, "pips_forward", fake_forward)
    traj_ref, vis_ref = PO.PipsTrackerRef({})._one_direction(rgbs, q, {}, index_of)
    traj, vis, cur, hist = run_restated_chain(q, torch.full((n,), int(flipped)), T)
    assert torch.equal(traj, traj_ref)
    assert torch.equal(vis > 0.5, vis_ref)
    assert (cur >= T - 1).all() and torch.equal(cur, torch.full((n,), T - 1))      # every chain ends anchored on the last frame
    assert any(at_threshold)                                                       # a visibility exactly AT 0.9 reached the sweep
    assert hist == seen                                                            # same anchors, same window frames, in order
    assert any(len(h) >= 2 for h in hist) and hist[7] == []                       # chains were linked; frame T - 1 never runs
    if T == 20 and not flipped:
        assert [f for f, _ in hist[2]][:2] == [0, 2]          # frame 3 sits exactly AT the threshold: not taken, frame 2 is


def test_chain_restatement_threshold_decay_is_float32():
    """0.9 - 3 * 0.02 is 0.84000003 in float32, one ulp above float32(0.84).  A visibility of exactly that value on frame 1 is AT
    the threshold of the fourth sweep, so that sweep fails too and the fifth (0.82000005) takes frame 5 (0.83), the later one; with
    the decay in double precision, or `<` for `<=`, frame 1 would be taken by the fourth sweep."""
    thr3 = K.decayed_threshold(3)
    assert thr3 > np.float32(0.84) and float(thr3) > 0.9 - 3 * 0.02
    cur, traj, vis = K.chain_init(torch.tensor([[0.0, 1.0, 1.0]]), 9)
    vi = torch.zeros(S, 1)
    vi[1, 0], vi[5, 0] = float(thr3), 0.83
    cur2, _, vis2, n_active = K.round_end(cur, torch.zeros(S, 1, 2), vi, 9, S, 0.9, traj, vis)
    assert int(cur2[0]) == 5 and n_active == 1 and torch.equal(vis2[1:8, 0], vi[1:, 0])
    vi[1, 0] = float(np.nextafter(thr3, np.float32(1)))                                # one ulp more: the fourth sweep takes it
    assert int(K.round_end(cur, torch.zeros(S, 1, 2), vi, 9, S, 0.9, traj, vis)[0][0]) == 1


# --------------------------------------------------------------------------------------------------------------------
def run_restated_cotracker(q: torch.Tensor, frame_map: torch.Tensor, T: int, script):
    """prepare, then per window: window_init -> scripted result -> window_store, as CotEngine::track chains them."""
    qt = q[:, 0].int()
    xy0, fidx_pt, traj_out, vis_out = K.cot_prepare(q[:, 1:].contiguous(), qt, frame_map, 4.0, T)
    feat_init = fidx_pt.float()[:, None].repeat(1, 128)          # the stubbed maps hold their frame number
    prev, coords_prev, vis_prev, wins = 0, None, None, []
    for ind in range(0, T - S // 2, S // 2):
        S_local = min(S, T - ind)
        na = int((qt < ind + S).sum())
        if na == 0:
            continue
        st = K.cot_window_init(ind, S_local, prev, na, S, qt, xy0, frame_map, coords_prev, vis_prev, feat_init)
        wins.append(dict(ind=ind, na=na, coords=st[0], visin=st[1], mask=st[2], fidx=st[3], ffeats=st[4]))
        coords, logits = script(ind, na)
        coords_prev, vis_prev, traj_out, vis_out = K.cot_window_store(logits, coords, 4.0, ind, S_local, traj_out, vis_out)
        prev = na
    return traj_out, vis_out, wins


@pytest.mark.parametrize("T", [5, 9, 14])
def test_cotracker_restatement_equals_the_oracle(monkeypatch, T):
    """prepare + window_init + window_store chained over the windows == cotracker_forward with forward_iteration scripted: T = 5
    (one window of 5 live frames), 9 (the second window has 5), 14 (three windows, the last with 6); points joining in the first,
    second and third window; a non-identity frame map."""
    starts = sorted(t for t in (0, 0, 3, 7, 8, 11, 12, 13) if t < T)
    if T == 5:
        starts = [0, 1, 3, 4]
    n = len(starts)
    g = torch.Generator().manual_seed(T)
    q = torch.cat([torch.tensor(starts, dtype=torch.float32)[:, None], torch.randint(0, 16, (n, 2), generator=g).float() * 4], dim=1)
    frame_map = (torch.arange(T) * 7 + 3) % 31

    def script(ind, na):                                   # -> coords (feature-map px) [S][na][2], logits [S][na]
        gg = torch.Generator().manual_seed(100 + ind)
        return torch.rand(S, na, 2, generator=gg) * 20 - 2, torch.randn(S, na, generator=gg) * 3

    def fake_iteration(sd, fm, coords_init, feat_init, vis_init, tm, iters, pos_grid, times_embed, trace=None):
        frames = fm[:, 0, 0, 0].long()
        ind = int((frame_map == frames[0]).nonzero()[0])
        trace.update(coords_init=coords_init.clone(), vis_init=vis_init.clone(), tm=tm.clone(), frames=frames, feat_init=feat_init.clone())
        c, lg = script(ind, coords_init.shape[1])
        return c * 4.0, lg

    monkeypatch.setattr(CO, "forward_iteration", fake_iteration)
    cache = {int(f): torch.full((128, 4, 4), float(f)) for f in frame_map}
    trace = []
    traj_ref, vis_ref = CO.cotracker_forward({}, torch.zeros(T, 3, 16, 16), q, fmap_cache=cache, frame_of=lambda t: int(frame_map[t]),
                                             trace=trace)
    traj, vis, wins = run_restated_cotracker(q, frame_map, T, script)
    assert len(wins) == len(trace) == {5: 1, 9: 2, 14: 3}[T]
    for w, tr in zip(wins, trace):
        assert (w["ind"], w["na"]) == (tr["ind"], tr["n_act"])
        assert torch.equal(w["coords"], tr["coords_init"]) and torch.equal(w["visin"], tr["vis_init"])
        assert torch.equal(w["mask"], tr["tm"])
        assert torch.equal(w["fidx"], tr["frames"][None].repeat(w["na"], 1))
        assert torch.equal(w["ffeats"], tr["feat_init"][:, None].repeat(1, S, 1))
    assert torch.equal(traj, traj_ref) and torch.equal(vis, vis_ref)
    if T == 14:
        assert [w["na"] for w in wins] == [4, 6, 8] and int(wins[1]["mask"][:, :4].sum()) == 16


# --------------------------------------------------------------------------------------------------------------------
def test_sincos_restatements_are_the_oracle_embeddings_in_f32():
    """The f32-argument restatements evaluated in f32 are bit for bit the oracle's embeddings (layout and argument formation), and
    in float64 they stay within f32 rounding of them — at arguments up to 6e4 rad, where a float64 ARGUMENT would not."""
    g = torch.Generator().manual_seed(5)
    xyz = torch.cat([torch.rand(9, S, 2, generator=g) * 120 - 60, torch.linspace(0, S, S).reshape(1, S, 1).repeat(9, 1, 1)], dim=-1)
    assert torch.equal(K.embed3d(xyz, torch.float32), PO.embed3d(xyz))
    assert float((K.embed3d(xyz) - PO.embed3d(xyz)).abs().max()) < 1e-6
    assert float((PO.embed3d(xyz.double()) - PO.embed3d(xyz)).abs().max()) > 1e-4      # what the f32 argument is for
    assert torch.equal(K.flow_embedding(xyz[..., :2], torch.float32), CO.flow_embedding(xyz[..., :2]))
    om = K.pips2_omega()
    from sam_pt_amd.pack import pack_pips2
    assert torch.equal(om, pack_pips2({}, "cpu")["__omega"])
    assert torch.equal(K.posemb_sincos_2d_xy(xyz[..., :2], om, torch.float32), P2.posemb_sincos_2d_xy(xyz[..., :2], 128))
    co = K.coords_E()
    assert co.shape == (S, 9, 2) and bool(torch.isfinite(co).all())
    x = K.pips_build_input(torch.zeros(9, S, 128), co, torch.linspace(0, S, S), 520)
    assert float((x[..., 324:519] - PO.embed3d(torch.cat([K.flows_from(co), xyz[..., 2:]], dim=-1))).abs().max()) < 1e-6
    assert bool(torch.isnan(x[..., 128:324]).all()) and float(x[..., 519].abs().max()) == 0.0


def test_sampler_restatements_accept_E_in_both_precisions():
    """The oracle samplers take the coordinate set E (on and off the 16 x 24 map) in f32 and f64; their own f32-vs-f64 distance is
    the yardstick the GPU bars were derived from (bars (b) and (d) of tests/test_gpu_tracker_kernels.py)."""
    g = torch.Generator().manual_seed(11)
    fm = torch.randn(3, 16, 24, 128, generator=g)
    co = K.coords_E()
    pyr = [p.permute(0, 2, 3, 1).contiguous() for p in PO.build_pyramid(fm.permute(0, 3, 1, 2))]
    assert [tuple(p.shape[1:3]) for p in pyr] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    f64, f32 = K.sample_feat(fm, co[0]), K.sample_feat(fm, co[0], dtype=torch.float32)
    assert float((f64 - f32).abs().max()) <= 8 * 2.0 ** -24 * float(fm.abs().max())
    fidx = torch.tensor([[0, 2, 1, 1, 0, 2, 2, 0]] * 9)
    ff = torch.randn(9, S, 128, generator=g)
    c64, c32 = K.corr_sample(pyr, fidx, ff, co), K.corr_sample(pyr, fidx, ff, co, dtype=torch.float32)
    assert float((c64 - c32).abs().max()) <= 2e-5 * float(c64.abs().max())
    zeros = float((c64 == 0).float().mean())
    assert 0.2 < zeros < 0.8, zeros                        # a good part of the taps is off the map, a good part on it


# --------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_and_binds_the_kernel_hooks():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
        res, args = _lib._SIGS[name]                                 # house style: int return code, stream last
        assert res is _lib.c_int and args[-1] is _lib._P
        assert len(args) == 1 + hdr.split(name + "(")[1].split(");")[0].count(","), name


def test_kernel_hooks_refuse_bad_arguments_before_any_launch():
    """A null pointer or a non-positive count is SAMPT_ERR_ARG for every hook, and so are the layouts the launchers cannot write.
    X is a host address standing in for device pointers: a call that got as far as a launch would fail differently (there is no
    device here), a call that dereferenced it on the device never happens."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    X = C.c_void_p(C.addressof(buf))
    pyr = (C.c_void_p * 4)(X, X, X, X)
    holed = (C.c_void_p * 4)(X, X, None, X)
    ARG = -1
    good = {
        "sampt_pips_corr_sample_ex": [pyr, 16, 24, X, 8, 9, X, X, X, 196, 0, None, None],
        "sampt_pips_build_input_f32": [X, X, X, 8, 9, X, 520, None],
        "sampt_pips_init_state_f32": [X, X, 4.0, 8, 9, X, X, X, None],
        "sampt_pips_apply_update_f32": [X, X, X, X, X, X, X, None, 8, 9, None],
        "sampt_pips_finalize_f32": [X, X, X, X, 4.0, 8, 9, X, X, None],
        "sampt_pips_chain_init": [X, 9, 5, X, X, X, None],
        "sampt_pips_round_begin": [X, X, X, 5, 9, 8, X, X, None, None, 4.0, None],
        "sampt_pips_round_end": [X, X, X, 5, 9, 8, 0.9, X, X, X, None],
        "sampt_pips2_init_f32": [X, X, 16, 24, X, 8.0, 8, 9, 0, X, X, X, X, X, None],
        "sampt_pips2_templates_f32": [X, 16, 24, X, X, 8, 9, X, X, None],
        "sampt_pips2_build_input_f32": [X, X, 8, 9, X, 720, None],
        "sampt_instnorm1d_relu_f32": [X, X, 9, 8, 128, None],
        "sampt_add_chanpad_f32": [X, X, 37, 96, 131, 0, None],
        "sampt_pips2_apply_delta_f32": [X, X, 8.0, 8, 9, 1, X, X, None],
        "sampt_cot_prepare": [X, X, X, 4.0, 9, 12, X, X, X, X, None],
        "sampt_cot_window_init": [4, 8, 4, 7, 8, X, X, X, X, X, X, X, X, X, X, X, None],
        "sampt_cot_pos_embed_f32": [X, X, X, 12, 16, 456, 9, X, None],
        "sampt_cot_build_input_f32": [X, X, X, X, X, X, 8, 9, X, None],
        "sampt_cot_window_store_f32": [X, X, X, X, 4.0, 8, 4, 0, 8, 9, X, X, X, X, None],
        "sampt_resize_frames_f32": [X, 1, 3, 9, 13, X, 21, 30, None],
    }
    assert set(good) == set(NEW_SYMBOLS) | {"sampt_resize_frames_f32"}        # the resize launcher already had its export
    optional = {("sampt_pips_corr_sample_ex", 11), ("sampt_pips_apply_update_f32", 7), ("sampt_pips_round_begin", 8),
                ("sampt_pips_round_begin", 9)}
    counts = {"sampt_pips_corr_sample_ex": (4, 5), "sampt_pips_build_input_f32": (3, 4), "sampt_pips_init_state_f32": (3, 4),
              "sampt_pips_apply_update_f32": (8, 9), "sampt_pips_finalize_f32": (5, 6), "sampt_pips_chain_init": (1, 2),
              "sampt_pips_round_begin": (3, 4, 5), "sampt_pips_round_end": (3, 4, 5), "sampt_pips2_init_f32": (6, 7),
              "sampt_pips2_templates_f32": (5, 6), "sampt_pips2_build_input_f32": (2, 3), "sampt_instnorm1d_relu_f32": (2, 3, 4),
              "sampt_add_chanpad_f32": (2, 3), "sampt_pips2_apply_delta_f32": (3, 4), "sampt_cot_prepare": (4, 5),
              "sampt_cot_window_init": (1, 3, 4), "sampt_cot_pos_embed_f32": (3, 4, 5, 6), "sampt_cot_build_input_f32": (6, 7),
              "sampt_cot_window_store_f32": (5, 6, 8), "sampt_resize_frames_f32": (2, 3, 4, 6, 7)}
    for name, args in good.items():
        fn = getattr(lib, name)
        for k, a in enumerate(args[:-1]):
            if a is X and (name, k) not in optional:                                   # every required pointer, one at a time
                bad = list(args)
                bad[k] = None
                assert fn(*bad) == ARG, f"{name}: null argument {k} accepted"
                assert name.encode() in lib.sampt_last_error()
        for k in counts[name]:                                                         # every count: zero and negative
            for v in (0, -3):
                bad = list(args)
                bad[k] = v
                assert fn(*bad) == ARG, f"{name}: argument {k} = {v} accepted"

    def call(name, **changes):
        a = list(good[name])
        for k, v in changes.items():
            a[int(k[1:])] = v
        return getattr(lib, name)(*a)

    assert call("sampt_pips_corr_sample_ex", _0=holed) == ARG                          # a missing pyramid level
    assert call("sampt_pips_corr_sample_ex", _0=None) == ARG
    assert call("sampt_pips_corr_sample_ex", _9=456, _10=130, _11=X) == ARG            # times outside the PIPS layout
    assert call("sampt_pips_corr_sample_ex", _9=720, _10=196, _11=X) == ARG
    assert call("sampt_pips_corr_sample_ex", _9=518, _10=128, _11=X) == ARG
    assert call("sampt_pips_corr_sample_ex", _9=581, _10=128, _11=X) == ARG
    assert b"xoff == 128" in lib.sampt_last_error()
    assert call("sampt_pips_corr_sample_ex", _9=300, _10=128) == ARG                   # the 196 columns do not fit the row
    assert call("sampt_pips_corr_sample_ex", _10=-1) == ARG
    assert call("sampt_pips_build_input_f32", _6=518) == ARG and call("sampt_pips_build_input_f32", _6=581) == ARG
    assert b"[519, 580]" in lib.sampt_last_error()
    assert call("sampt_pips2_build_input_f32", _5=719) == ARG and call("sampt_pips2_build_input_f32", _5=721) == ARG
    assert call("sampt_pips2_build_input_f32", _5=588) == ARG
    assert call("sampt_pips_round_begin", _8=X) == ARG and call("sampt_pips_round_begin", _9=X) == ARG   # xy_feat without f0, f0 without xy_feat
    assert call("sampt_pips2_init_f32", _8=1, _1=None, _4=None, _11=None, _12=None, _13=None, _9=None) == ARG   # coords still needed
    assert call("sampt_pips2_apply_delta_f32", _7=None) == ARG                         # last = 1 without trajs
    assert call("sampt_add_chanpad_f32", _3=131, _4=96) == ARG                         # cout < cin
    assert call("sampt_cot_window_init", _2=8) == ARG                                  # prev > na
    assert call("sampt_cot_window_init", _1=9) == ARG                                  # S_local > S
    assert call("sampt_cot_window_init", _0=-4) == ARG
    assert call("sampt_cot_window_init", _8=None) == ARG and call("sampt_cot_window_init", _9=None) == ARG   # carries with prev > 0
    assert call("sampt_cot_pos_embed_f32", _5=455) == ARG                              # odd embedding width
    assert call("sampt_cot_window_store_f32", _9=3) == ARG                             # n_total < na
    assert call("sampt_cot_window_store_f32", _8=9) == ARG
