"""Plain restatements of the point trackers' window kernels (csrc/pips.hip, pips2.hip, cotracker.hip), one function per kernel,
in the layouts of those files' headers: coords [S][n][2], rows pt * S + s, x rows of 519..580 / 720 / 456 columns.  Everything
runs on the CPU; tests/test_tracker_kernels_cpu.py pins the restatements on the oracle, tests/test_gpu_tracker_kernels.py holds
the kernels to them.

Arithmetic comes from the oracle wherever it has the operation (``bilinear_sample2d``, ``corr_volumes`` + ``sample_corr``, the
sin/cos tables) and is evaluated in ``dtype`` (float64 for the references).  Sin/cos columns take their ARGUMENT in f32 exactly as
the models form it (one f32 product) and only the sine / cosine of that f32 number in ``dtype``: a float64 argument would differ
by up to 4e-3 at the 6e4 rad these embeddings reach and the tests would measure argument rounding.  Bookkeeping (chain kernels,
CoTracker prepare / window init / window store) is f32 / int like the kernels."""
import functools
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pips_ref as PO

SENTINEL = 7.0
S = 8          # window length of the scripted chain windows
# coordinate set E of the kernel tests (x, y) on a 16 x 24 map: interior, exactly integral, the last column and row, just off
# the map, past the last column, far outside, half-way taps, negative integers, the origin
E_POINTS = ((5.3, 7.7), (10.0, 7.0), (23.0, 15.0), (-0.4, -0.6), (23.25, 3.2), (-7.5, 56.0), (4.5, 2.5), (-1.0, -3.0), (0.0, 0.0))


def coords_E(S: int = 8) -> torch.Tensor:
    """(S, 9, 2) f32: E shifted by 0.37 s per frame."""
    e = torch.tensor(E_POINTS, dtype=torch.float32)
    return torch.stack([e + torch.tensor(0.37, dtype=torch.float32) * s for s in range(S)]).contiguous()


# ------------------------------------------------------------------------------------------------------------ samplers
def sample_feat(fmap: torch.Tensor, xy: torch.Tensor, frame_idx: Optional[torch.Tensor] = None, dtype=torch.float64) -> torch.Tensor:
    """k_pips_sample_feat: fmap [frames][H][W][C] NHWC, xy [n][2], frame_idx [n] or None (frame 0) -> [n][C]."""
    out = []
    for i in range(xy.shape[0]):
        f = int(frame_idx[i]) if frame_idx is not None else 0
        p = xy[i:i + 1].to(dtype)
        out.append(PO.bilinear_sample2d(fmap[f].permute(2, 0, 1).to(dtype), p[:, 0], p[:, 1])[0])
    return torch.stack(out)


def corr_sample(pyr: List[torch.Tensor], frame_idx: torch.Tensor, ffeats: torch.Tensor, coords: torch.Tensor,
                dtype=torch.float64) -> torch.Tensor:
    """k_pips_corr_sample's 196 columns: pyr[l] [frames][H_l][W_l][128] NHWC, frame_idx [n][S], ffeats [n][S][128], coords
    [S][n][2] -> [n][S][196] (CorrBlock.corr + CorrBlock.sample of the oracle, one point at a time: every point has its own
    window frames)."""
    n, S = frame_idx.shape
    out = []
    for pt in range(n):
        fr = frame_idx[pt].long()
        lv = [p[fr].permute(0, 3, 1, 2).to(dtype) for p in pyr]
        vols = PO.corr_volumes(lv, ffeats[pt][:, None, :].to(dtype))
        out.append(PO.sample_corr(vols, coords[:, pt:pt + 1].to(dtype))[:, 0])
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------- sin / cos columns
def _sincos(arg32: torch.Tensor, dtype) -> (torch.Tensor, torch.Tensor):
    assert arg32.dtype == torch.float32
    a = arg32.to(dtype)
    return torch.sin(a), torch.cos(a)


def _interleaved(v32: torch.Tensor, C: int, dtype) -> torch.Tensor:
    """(...,) f32 -> (..., C): sin / cos interleaved at the frequencies arange(0, C, 2) * 1000 / C (utils/misc.py:30-55)."""
    div = torch.arange(0, C, 2, dtype=torch.float32) * (1000.0 / C)
    s, c = _sincos(v32[..., None] * div, dtype)
    return torch.stack([s, c], dim=-1).reshape(*v32.shape, C)


def embed3d(xyz32: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """oracle.pips_ref.embed3d with C = 64: (..., 3) f32 -> (..., 195) = [pe_x 64 | pe_y 64 | pe_t 64 | x, y, t]."""
    return torch.cat([_interleaved(xyz32[..., a], 64, dtype) for a in range(3)] + [xyz32.to(dtype)], dim=-1)


def flow_embedding(xy32: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """oracle.cotracker_ref.flow_embedding with C = 64: (..., 2) f32 -> (..., 130) = [x, y | pe_x 64 | pe_y 64]."""
    return torch.cat([xy32.to(dtype)] + [_interleaved(xy32[..., a], 64, dtype) for a in range(2)], dim=-1)


def pips2_omega() -> torch.Tensor:
    """The 32 frequencies of posemb_sincos_2d_xy(., 128) as oracle.pips2_ref forms them."""
    omega = torch.arange(32) / 31
    return (1.0 / (10000 ** omega)).float()


def posemb_sincos_2d_xy(xy32: torch.Tensor, omega32: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """oracle.pips2_ref.posemb_sincos_2d_xy with C = 128: (..., 2) f32 -> (..., 130) = [sin(x w) 32 | cos(x w) | sin(y w) | cos(y w)
    | x, y]."""
    sx, cx = _sincos(xy32[..., 0:1] * omega32, dtype)
    sy, cy = _sincos(xy32[..., 1:2] * omega32, dtype)
    return torch.cat([sx, cx, sy, cy, xy32.to(dtype)], dim=-1)


# ------------------------------------------------------------------------------------------------------------------ PIPS
def flows_from(coords: torch.Tensor) -> torch.Tensor:
    """[S][n][2] f32 -> [n][S][2] f32 = coords[s] - coords[0] (one f32 subtraction)."""
    return (coords - coords[0:1]).permute(1, 0, 2).contiguous()


def pips_build_input(ffeats: torch.Tensor, coords: torch.Tensor, times: torch.Tensor, ldx: int, dtype=torch.float64) -> torch.Tensor:
    """k_pips_build_input (and the fused tail of k_pips_corr_sample): [n][S][ldx] in ``dtype`` with NaN in the correlation columns
    [128, 324), which this kernel does not own."""
    n, S, _ = ffeats.shape
    x = torch.full((n, S, ldx), float("nan"), dtype=dtype)
    x[..., :128] = ffeats.to(dtype)
    xyz = torch.cat([flows_from(coords), times.reshape(1, S, 1).expand(n, S, 1)], dim=-1).contiguous()
    x[..., 324:519] = embed3d(xyz, dtype)
    x[..., 519:] = 0
    return x


def pips_init_state(xys: torch.Tensor, feat_init: torch.Tensor, stride: float, S: int):
    """k_pips_init_state -> coords [S][n][2], coords0 [n][2], ffeats [n][S][128] (f32)."""
    c0 = xys / torch.tensor(stride, dtype=torch.float32)
    return c0[None].repeat(S, 1, 1), c0.clone(), feat_init[:, None, :].repeat(1, S, 1)


def feature_update(delta: torch.Tensor, gn_w, gn_b, up_w, up_b, ffeats: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """ffeats + gelu(Linear(GroupNorm(1, 128)(delta[..., 2:]))) in ``dtype``; up_w [out][in] (pips.py:536-541)."""
    n, S, _ = delta.shape
    g = F.group_norm(delta[..., 2:].reshape(n * S, 128).to(dtype), 1, gn_w.to(dtype), gn_b.to(dtype), eps=1e-5)
    upd = F.gelu(F.linear(g, up_w.to(dtype), up_b.to(dtype)))
    return (upd + ffeats.reshape(n * S, 128).to(dtype)).reshape(n, S, 128)


def coords_update(delta: torch.Tensor, coords: torch.Tensor, coords0: Optional[torch.Tensor]) -> torch.Tensor:
    """coords [S][n][2] + delta[n][S][:2] (one f32 addition); frame 0 locked to coords0 when given (pips.py:542-544)."""
    out = coords + delta[..., :2].permute(1, 0, 2)
    if coords0 is not None:
        out[0] = coords0
    return out


def vis_logits(ffeats: torch.Tensor, vis_w: torch.Tensor, vis_b: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[n][S][128] -> logits [S][n] in ``dtype``."""
    return (F.linear(ffeats.to(dtype), vis_w.reshape(1, 128).to(dtype), vis_b.reshape(1).to(dtype))[..., 0]).t().contiguous()


# ---- chained windows (pips/tracker.py:42-153), one function per kernel, int64 / f32
def chain_init(q: torch.Tensor, T: int):
    """k_pips_chain_init: q [n][3] = (t, x, y) -> cur [n], traj [T][n][2], vis [T][n]."""
    n = q.shape[0]
    cur = q[:, 0].long().clone()
    traj, vis = torch.zeros(T, n, 2), torch.zeros(T, n)
    ar = torch.arange(n)
    traj[cur, ar], vis[cur, ar] = q[:, 1:], 1.0
    return cur, traj, vis


def round_begin(cur: torch.Tensor, flip: torch.Tensor, traj: torch.Tensor, T: int, S: int, stride: float):
    """k_pips_round_begin -> fidx [n][S], xys [n][2], xy_feat [n][2], f0 [n]; a finished chain (anchor >= T - 1, also beyond it)
    gets the dummy window of frame T - 1."""
    n = cur.shape[0]
    f = cur.clamp(max=T - 1)
    hi = torch.minimum(T - f, torch.tensor(S))
    w = torch.minimum(f[:, None] + torch.arange(S)[None], (f + hi - 1)[:, None])
    fl = flip.bool()
    fidx = torch.where(fl[:, None], T - 1 - w, w)
    xys = traj[f, torch.arange(n)].clone()
    return fidx, xys, xys / torch.tensor(stride, dtype=torch.float32), torch.where(fl, T - 1 - f, f)


def round_end(cur: torch.Tensor, tr: torch.Tensor, vi: torch.Tensor, T: int, S: int, thr0: float, traj: torch.Tensor,
              vis: torch.Tensor):
    """k_pips_round_end: tr [S][n][2], vi [S][n] -> (cur, traj, vis, n_active), all new tensors.  Frames 1 .. hi - 1 of every
    unfinished chain are written, then the anchor moves to the latest window frame whose visibility EXCEEDS the threshold, the
    threshold losing float32(0.02) per fruitless sweep."""
    cur, traj, vis = cur.clone(), traj.clone(), vis.clone()
    step = np.float32(0.02)
    n_active = 0
    for i in range(cur.shape[0]):
        f = int(cur[i])
        if f >= T - 1:
            continue
        hi = min(T - f, S)
        traj[f + 1:f + hi, i], vis[f + 1:f + hi, i] = tr[1:hi, i], vi[1:hi, i]
        thr = np.float32(thr0)
        earliest, last = f + 1, f + hi - 1
        nxt = last
        while np.float32(vis[nxt, i].item()) <= thr:
            nxt -= 1
            if nxt < earliest:
                thr, nxt = np.float32(thr - step), last
        cur[i] = nxt
        n_active += nxt < T - 1
    return cur, traj, vis, int(n_active)


# ---------------------------------------------------------------------------------------------------------------- PIPS++
def pips2_init(trajs0: torch.Tensor, stride: float):
    """k_pips2_init's bookkeeping: trajs0 [S][n][2] px -> coords [S][n][2], bak [n][2] (f32).  Without feat_init all three
    templates are ``sample_feat(fmap, bak, frame_idx[:, 0])`` on every frame."""
    coords = trajs0 / torch.tensor(stride, dtype=torch.float32)
    return coords, coords[0].clone()


def pips2_templates(fmap: torch.Tensor, frame_idx: torch.Tensor, coords: torch.Tensor, d: int, dtype=torch.float64) -> torch.Tensor:
    """k_pips2_templates for one lag d (2 -> f2, 4 -> f4): [n][S][128], row (pt, s) = the map of frame max(s - d, 0) of the point's
    window sampled at the point's position on that frame (pips_plus_plus.py:490-506)."""
    n, S = frame_idx.shape
    src = (torch.arange(S) - d).clip(min=0)
    return torch.stack([sample_feat(fmap, coords[src, pt], frame_idx[pt][src], dtype) for pt in range(n)])


def pips2_flows(coords: torch.Tensor) -> torch.Tensor:
    """[S][n][2] -> [n][S][2] f32: coords[s + 1] - coords[s], the last frame repeating the previous flow (zeros when S == 1)."""
    S = coords.shape[0]
    if S == 1:
        return torch.zeros(coords.shape[1], 1, 2)
    fl = (coords[1:] - coords[:-1]).permute(1, 0, 2)
    return torch.cat([fl, fl[:, -1:]], dim=1).contiguous()


def pips2_build_input(coords: torch.Tensor, omega32: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """k_pips2_build_input's columns [588, 720): [n][S][132] = [sin / cos 128 | flow 2 | 0 0]."""
    pe = posemb_sincos_2d_xy(pips2_flows(coords), omega32, dtype)
    return torch.cat([pe, torch.zeros(*pe.shape[:2], 2, dtype=dtype)], dim=-1)


def instnorm1d_relu(x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[n][S][C] -> relu(InstanceNorm1d over S) (no affine, eps 1e-5, biased variance), as the oracle's _res_block."""
    return F.relu(F.instance_norm(x.to(dtype).permute(0, 2, 1))).permute(0, 2, 1).contiguous()


def add_chanpad(out: torch.Tensor, identity: torch.Tensor, relu: bool) -> torch.Tensor:
    """out [rows][cout] + identity [rows][cin] zero-padded as the oracle's _res_block pads it; relu: DeltaBlock's final ReLU."""
    cin, cout = identity.shape[1], out.shape[1]
    ch1 = (cout - cin) // 2
    y = out + F.pad(identity, (ch1, cout - cin - ch1))
    return F.relu(y) if relu else y


def pips2_apply_delta(delta: torch.Tensor, bak: torch.Tensor, stride: float, coords: torch.Tensor):
    """k_pips2_apply_delta: delta [n][S][2] -> (coords, coords * stride) with frame 0 locked to bak (f32)."""
    c = coords + delta.permute(1, 0, 2)
    c[0] = bak
    return c, c * torch.tensor(stride, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------- CoTracker
def cot_prepare(qxy: torch.Tensor, qt: torch.Tensor, frame_map: torch.Tensor, stride: float, T: int):
    """k_cot_prepare -> xy0 [n][2], fidx_pt [n], traj_out [T][n][2] = 0, vis_out [T][n] = 0.5."""
    n = qxy.shape[0]
    return (qxy / torch.tensor(stride, dtype=torch.float32), frame_map[qt.long()].clone(), torch.zeros(T, n, 2),
            torch.full((T, n), 0.5))


def cot_window_init(ind: int, S_local: int, prev: int, na: int, S: int, qt, xy0, frame_map, coords_prev, vis_prev, feat_init):
    """k_cot_window_init -> coords [S][na][2], visin [S][na], mask [S][na], fidx [na][S], ffeats [na][S][128].  Points [0, prev)
    carry the second half of the previous window (frames 0 .. S/2 - 1 <- previous S/2 .., the rest <- its last frame); points
    [prev, na) start at their query position with visibility logit 10."""
    coords = xy0[None, :na].repeat(S, 1, 1)
    visin = torch.full((S, na), 10.0)
    mask = torch.zeros(S, na)
    s = torch.arange(S)
    if prev > 0:
        src = (s + S // 2).clamp(max=S - 1)
        coords[:, :prev] = coords_prev[src, :prev]
        visin[:, :prev] = vis_prev[src, :prev]
    live = s < S_local
    mask[:, :prev] = (live & (s >= S // 2)).float()[:, None]
    mask[:, prev:] = (live[:, None] & (ind + s[:, None] >= qt[None, prev:na])).float()
    fidx = frame_map[ind + s.clamp(max=S_local - 1)][None].repeat(na, 1)
    return coords, visin, mask, fidx, feat_init[:na, None, :].repeat(1, S, 1)


def cot_pos_embed(coords0: torch.Tensor, grid: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """k_cot_pos_embed: coords0 [na][2], grid (H, W, E) -> [na][E] (forward_iteration's sample_pos_embed)."""
    c = coords0.to(dtype)
    return PO.bilinear_sample2d(grid.permute(2, 0, 1).to(dtype), c[:, 0], c[:, 1])


def cot_build_input_terms(ffeats, coords, visin, mask, corr, dtype=torch.float64) -> torch.Tensor:
    """The first summand of k_cot_build_input: [na][S][456] = [flow embedding 130 | corr 196 | feature 128 | mask, visibility]."""
    fe = flow_embedding(flows_from(coords), dtype)
    return torch.cat([fe, corr.to(dtype), ffeats.to(dtype), mask.t()[..., None].to(dtype), visin.t()[..., None].to(dtype)], dim=-1)


def cot_window_store(logits: torch.Tensor, coords: torch.Tensor, stride: float, ind: int, S_local: int, traj_out: torch.Tensor,
                     vis_out: torch.Tensor):
    """k_cot_window_store given the window's visibility logits [S][na]: -> (coords_prev, vis_prev, traj_out, vis_out); the first
    S_local frames of EVERY active point go to rows ind .. of the outputs."""
    na = coords.shape[1]
    traj_out, vis_out = traj_out.clone(), vis_out.clone()
    traj_out[ind:ind + S_local, :na] = coords[:S_local] * torch.tensor(stride, dtype=torch.float32)
    vis_out[ind:ind + S_local, :na] = torch.sigmoid(logits[:S_local])
    return coords.clone(), logits.clone(), traj_out, vis_out


# --------------------------------------------------------------------------------------------------------------------
# scripted windows of the chain tests (CPU and GPU)
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logit_with_sigmoid(v: float) -> torch.Tensor:
    """An f32 logit whose f32 torch.sigmoid is EXACTLY float32(v) (the sigmoid is ~3 times coarser than f32 there, so one of the
    neighbours of logit(v) hits it)."""
    target = torch.tensor(v, dtype=torch.float32)
    x = torch.log(target.double() / (1 - target.double())).float()
    lo = hi = x
    for _ in range(64):
        for c in (lo, hi):
            if torch.sigmoid(c) == target:
                return c
        lo, hi = torch.nextafter(lo, torch.tensor(-1e9)), torch.nextafter(hi, torch.tensor(1e9))
    raise AssertionError(f"no f32 logit with sigmoid == {v}")


def scripted_window(i: int, f: int, thr0: float = 0.9):
    """Chain i anchored at (direction-time) frame f -> (positions (S, 2) px, visibility logits (S,)).  The x coordinate carries the
    chain number (hundreds), so a stub that only sees anchor positions knows whose window it is.  Scripts by i % 5:
    0 random; 1 every visibility at or below the threshold, so the sweep has to come back with a lower one (several times: the
    best value is 0.83); 2 frame 3 EXACTLY at the threshold (not above it: must not be taken) below a visible frame 2; 3 only the
    last frame visible; 4 only frame 1 visible."""
    g = torch.Generator().manual_seed(1000 * i + f)
    s = torch.arange(S, dtype=torch.float32)
    xy = torch.stack([100.0 * i + f + s + torch.rand(S, generator=g), 10.0 * f + s + torch.rand(S, generator=g)], dim=-1)
    kind = i % 5
    if kind == 0:
        lg = torch.randn(S, generator=g) * 2 + 1
    elif kind == 1:
        lg = torch.logit(torch.tensor([0.5, 0.83, 0.6, 0.81, 0.3, 0.82, 0.1, 0.7]))
    elif kind == 2:
        lg = torch.full((S,), -3.0)
        lg[2], lg[3] = 4.0, logit_with_sigmoid(thr0)
    elif kind == 3:
        lg = torch.full((S,), -2.0)
        lg[S - 1] = 5.0
    else:
        lg = torch.full((S,), -2.0)
        lg[1] = 5.0
    return xy, lg.float()


def decayed_threshold(k: int, thr0: float = 0.9) -> np.float32:
    """The linking threshold after k fruitless sweeps, in the float32 arithmetic of the reference's torch code."""
    thr = np.float32(thr0)
    for _ in range(k):
        thr = np.float32(thr - np.float32(0.02))
    return thr
