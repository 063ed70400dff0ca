"""Seam 1 of the drop-in boundary: the point-tracker API of the reference, backed by the HIP library.

``PointTracker`` mirrors ``sam_pt.point_tracker.tracker.PointTracker`` (sam_pt/point_tracker/tracker.py:13-118):
same method names, argument meaning and return conventions, so ``SamPt`` (the reference's or ours) can hold either.
``PipsPointTracker`` mirrors ``sam_pt.point_tracker.pips.PipsPointTracker`` (pips/tracker.py:9-201): same constructor
keywords as configs/model/point_tracker/pips.yaml, same window chaining / trajectory linking, but

  * ``fnet`` runs ONCE per distinct frame for the whole clip (InstanceNorm is per-sample, so the per-window
    recompute of the reference is redundant — SURVEY.md App. B-7) and its NHWC feature pyramid stays resident in HBM
    for both temporal directions;
  * every 8-frame window (correlation, MLP-Mixer, feature/coordinate update, visibility head) is one call into
    ``sampt_pips_update_f32``;
  * the redundant "init pass" of the reference (pips/tracker.py:81-90, App. B-6) is a 128-channel bilinear gather.

When the reference package itself is importable, subclass its ABC instead.
"""
from __future__ import annotations

import ctypes as C
import os
from abc import ABC, abstractmethod
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from .pack import pack_pips
from .weights import init_pips_state_dict


class PointTracker(ABC, nn.Module):
    """Abstract point tracker (interface of sam_pt/point_tracker/tracker.py:13-51)."""

    @abstractmethod
    def forward(self, rgbs, query_points) -> Tuple[torch.Tensor, torch.Tensor]:
        """rgbs (B,T,3,H,W) uint8; query_points (B,N,3)=(t,x,y) -> trajectories (B,T,N,2), visibilities (B,T,N)."""

    def evaluate_batch(self, rgbs, query_points, trajectories_gt=None, visibilities_gt=None):
        # contract of tracker.py:53-89: CPU copies, shape assert
        traj, vis = self.forward(rgbs, query_points)
        assert traj.shape == (rgbs.shape[0], rgbs.shape[1], query_points.shape[1], 2)

        def cpu(t):
            return t.detach().clone().cpu() if t is not None else None

        return {"trajectories_pred": cpu(traj), "visibilities_pred": cpu(vis), "query_points": cpu(query_points),
                "trajectories_gt": cpu(trajectories_gt), "visibilities_gt": cpu(visibilities_gt)}

    @classmethod
    def unpack_results(cls, packed_results, batch_idx):
        out = []
        for b in range(packed_results["trajectories_pred"].shape[0]):
            for n in range(packed_results["trajectories_pred"].shape[2]):
                r = {"idx": f"{batch_idx}_{b}_{n}", "iter": batch_idx, "video_idx": b, "point_idx_in_video": n,
                     "query_point": packed_results["query_points"][b, n, :],
                     "trajectory_pred": packed_results["trajectories_pred"][b, :, n, :],
                     "visibility_pred": packed_results["visibilities_pred"][b, :, n]}
                if packed_results["trajectories_gt"] is not None:
                    r["trajectory_gt"] = packed_results["trajectories_gt"][b, :, n, :]
                    r["visibility_gt"] = packed_results["visibilities_gt"][b, :, n]
                out.append(r)
        return out


def _prepared_entry(frames: torch.Tensor, pyr):
    """Cache entry of ``prepare``: holds the frames tensor itself (so its address cannot be recycled for another clip
    while the entry lives) and its version counter (in-place edits invalidate the entry)."""
    return (frames, frames.data_ptr(), tuple(frames.shape), frames._version, pyr)


def _clip_of(rgbs, batch_msg: str) -> torch.Tensor:
    """The one clip (T,3,H,W) of ``forward``'s rgbs (1,T,3,H,W), published for the unchanged-SamPt fast path (prefetch.py)."""
    from . import prefetch
    prefetch.publish(rgbs[0] if rgbs.dim() == 5 else rgbs)
    if rgbs.shape[0] != 1:
        raise NotImplementedError(batch_msg)
    return rgbs[0]


def _alloc_pyramid(T: int, H0: int, W0: int, device, shard=None):
    """The four NHWC f32 levels [T][H0 >> l][W0 >> l][128] of a clip; with ``shard`` padded to a whole number of frames per rank."""
    Tp = T if shard is None else shard.padded_frames(T)
    return [torch.empty((Tp, H0 >> l, W0 >> l, 128), dtype=torch.float32, device=device) for l in range(4)]


def _pyramid_chunks(pyr, lo: int, hi: int, chunk: int):
    """(first frame, frames, pointers of those frames' slices of every level) for frames [lo, hi) in encoder chunks."""
    for t0 in range(lo, hi, chunk):
        nf = min(chunk, hi - t0)
        yield t0, nf, _lib.ptr_array([p[t0:t0 + nf] for p in pyr])


def _sharded_encode(pyr, T: int, shard, encode):
    """Fill ``pyr`` through ``encode(lo, hi)``: the whole clip, or with ``shard`` (sam_pt_amd.dist.FnetShard) this rank's frames
    only, the rest arriving through ``shard.exchange`` (all_gather of the pyramid over RCCL).  -> the levels, T frames each."""
    if shard is None:
        encode(0, T)
        return pyr
    mine = shard.mine(T)
    encode(mine.start, mine.stop)
    shard.exchange(pyr, T, encode)
    return [p[:T] for p in pyr]


def load_pips_checkpoint(checkpoint_path: Optional[str]):
    """`saverloader.load` convention (utils/saverloader.py:30-73): newest model-*.pth in a directory, key
    'model_state_dict'.  None -> seeded random init (no checkpoints exist in this environment)."""
    if checkpoint_path is None:
        return None
    if os.path.isdir(checkpoint_path):
        names = sorted(f for f in os.listdir(checkpoint_path) if f.startswith("model-") and f.endswith(".pth"))
        if not names:
            raise FileNotFoundError(f"no model-*.pth under {checkpoint_path}")
        checkpoint_path = os.path.join(checkpoint_path, names[-1])
    ck = torch.load(checkpoint_path, map_location="cpu")
    return ck.get("model_state_dict", ck)


class _EngineTracker(PointTracker, _lib.EngineOwner):
    """A tracker over one native engine ``_h``: a subclass names ``_engines`` and itself (``_who``, for messages) and packs + creates in ``_build(lib, device)``."""
    _h = None
    _device = None
    # True: ``evaluate_batch`` leaves trajectories_pred / visibilities_pred / query_points where ``forward`` produced them (HIP
    # tensors) instead of the reference's CPU copies (tracker.py:82-83).  ``SamPt(device_tracks=True)`` sets it around its calls.
    results_on_device = False

    def _ensure(self, device: torch.device):
        self.ensure_engines(device, self._who, self._build)

    def evaluate_batch(self, rgbs, query_points, trajectories_gt=None, visibilities_gt=None):
        if not self.results_on_device:
            return super().evaluate_batch(rgbs, query_points, trajectories_gt, visibilities_gt)
        traj, vis = self.forward(rgbs, query_points)
        assert traj.shape == (rgbs.shape[0], rgbs.shape[1], query_points.shape[1], 2)

        def cpu(t):                                  # the ground-truth pass-throughs stay CPU copies, as in the reference
            return t.detach().clone().cpu() if t is not None else None

        return {"trajectories_pred": traj, "visibilities_pred": vis, "query_points": query_points,
                "trajectories_gt": cpu(trajectories_gt), "visibilities_gt": cpu(visibilities_gt)}


class _ClipTracker(_EngineTracker):
    """A tracker whose ``prepare`` can build a clip's feature pyramid ahead of ``forward``."""
    _prepared = None
    _prepared_events = None

    def _prepared_pyramid(self, frames: torch.Tensor):
        """The pyramid ``prepare`` cached for exactly this frames tensor (same storage, shape, version and device), or None."""
        e = self._prepared
        if e is not None and e[1] == frames.data_ptr() and e[2] == tuple(frames.shape) and \
                e[0]._version == e[3] and frames._version == e[3] and e[0].device == frames.device:
            return e[4]
        return None


class PipsPointTracker(_ClipTracker):
    _engines, _who = (("_h", "sampt_pips_destroy"),), "PipsPointTracker"

    def __init__(self, checkpoint_path=None, stride=4, s=8, initial_next_frame_visibility_threshold=0.9,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, seed: int = 72, fnet_chunk: int = 8):
        super().__init__()
        self.checkpoint_path, self.stride, self.s = checkpoint_path, stride, s
        self.initial_next_frame_visibility_threshold = initial_next_frame_visibility_threshold
        sd = state_dict if state_dict is not None else load_pips_checkpoint(checkpoint_path)
        self._sd = sd if sd is not None else init_pips_state_dict(seed)
        self.fnet_chunk = fnet_chunk
        self._w: Dict[str, torch.Tensor] = {}
        self.stats = {"windows": 0, "fnet_frames": 0}

    def _build(self, lib, device):
        self._w = pack_pips(self._sd, device, self.s)
        return [_lib.create_engine(lib, "sampt_pips_create", self._w, self.stride, self.s)]

    # -- fnet + pyramid for a whole clip -----------------------------------------------------------
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def compute_pyramid(self, frames: torch.Tensor, chunk_events: Optional[list] = None, shard=None):
        """frames (T,3,H,W) uint8 on device -> list of 4 NHWC f32 levels [T][H_l][W_l][128].  ``chunk_events``: a list that
        receives one ``(first_frame, end_frame, torch.cuda.Event)`` per encoder chunk, recorded on the current stream.
        ``shard`` (sam_pt_amd.dist.FnetShard): encode only this rank's share of the frames and fill in the rest through
        ``shard.exchange`` (all_gather of the pyramid over RCCL); one event for the whole pyramid."""
        self._ensure(frames.device)
        T, _, H, W = frames.shape
        pyr = _alloc_pyramid(T, H // self.stride, W // self.stride, frames.device, shard)
        chunk = min(self.fnet_chunk, T)
        ws = _lib.workspace("sampt_pips_fnet_workspace_bytes", frames.device, self._h, chunk, H, W)
        frames = frames.contiguous()
        events = chunk_events if frames.is_cuda else None

        def encode(lo, hi):
            for t0, nf, outs in _pyramid_chunks(pyr, lo, hi, chunk):
                _lib.check(self._lib.sampt_pips_fnet_f32(self._h, _lib.ptr(frames[t0:t0 + nf]), nf, H, W, outs, _lib.ptr(ws),
                                                         ws.numel(), _lib.stream_ptr()), "sampt_pips_fnet_f32")
                if events is not None and shard is None:      # (a sharded pyramid gets one event for all of it, below)
                    ev = torch.cuda.Event()
                    ev.record()
                    events.append((t0, t0 + nf, ev))
                self.stats["fnet_frames"] += nf

        pyr = _sharded_encode(pyr, T, shard, encode)
        if events is not None and shard is not None:
            ev = torch.cuda.Event()
            ev.record()
            events.append((0, T, ev))
        return pyr

    # -- chained windows for a set of independent point chains (pips/tracker.py:42-153) --------------------------
    def prepare(self, frames: torch.Tensor, shard=None):
        """Optional: build the feature pyramid of ``frames`` (T,3,H,W) now, on the current stream; the next ``forward``
        on the same frames tensor reuses it.  Lets a caller keep the compute-bound fnet on its main stream and run only
        the latency-bound window rounds on a second stream (sam_pt_amd.SamPt).  One event per encoder chunk is kept: a
        ``forward`` running on ANOTHER stream makes every window round wait only for the chunks that hold its frames
        (``chunk_events_on_other_stream``), so the first rounds start while later frames are still being encoded."""
        evs: list = []
        self._prepared = _prepared_entry(frames, self.compute_pyramid(frames, evs, shard=shard))
        self._prepared_events = evs

    chunk_events_on_other_stream = True      # SamPt: the side stream needs no event for the whole pyramid

    def _run_chains(self, pyr, T: int, query_points: torch.Tensor, flipped: torch.Tensor, chunk_events=None):
        """query_points (N,3) CPU float = (t, x, y) in each chain's OWN time axis; ``flipped[i]`` marks chains that run on
        the time-reversed clip (direction frame d = original frame T-1-d).  Returns CPU (T,N,2), (T,N) bool in each
        chain's own time axis.

        The reference walks ``current_frame`` upwards and runs one ``Pips.forward`` per distinct anchor frame with the
        points anchored there (tracker.py:67-109).  PIPS treats points independently (the mixer batch is per point,
        pips.py:525-532), so the same per-point window sequence is executed in ROUNDS: every unfinished chain advances by
        one window per round, all chains batched into one window call.  Results are identical per point; the number of
        window calls drops from one per distinct anchor to max-windows-per-chain.  The whole loop — window frames, write-back
        of frames 1..7, visibility-threshold linking (tracker.py:111-148) — runs on the device inside
        ``sampt_pips_track_f32``: no per-round download / upload, rounds are enqueued one ahead of the GPU."""
        import numpy as np
        dev = pyr[0].device
        N = query_points.shape[0]
        H0, W0 = pyr[0].shape[1:3]
        q_np = np.ascontiguousarray(query_points.numpy().astype(np.float32))
        f_np = np.ascontiguousarray(flipped.numpy().astype(np.uint8))
        q_d, f_d = torch.from_numpy(q_np).to(dev), torch.from_numpy(f_np).to(dev)
        traj = torch.empty((T, N, 2), dtype=torch.float32, device=dev)
        vis = torch.empty((T, N), dtype=torch.float32, device=dev)
        ws = _lib.workspace("sampt_pips_track_workspace_bytes", dev, self._h, N)
        evs = list(chunk_events) if chunk_events else []
        ev_arr = (C.c_void_p * max(len(evs), 1))(*[e[2].cuda_event for e in evs])
        lo_arr = (C.c_int * max(len(evs), 1))(*[int(e[0]) for e in evs])
        hi_arr = (C.c_int * max(len(evs), 1))(*[int(e[1]) for e in evs])
        rounds = C.c_int(0)
        _lib.check(self._lib.sampt_pips_track_f32(
            self._h, _lib.ptr_array(pyr), H0, W0, T, N, _lib.ptr(q_d), _lib.ptr(f_d), q_np.ctypes.data_as(C.c_void_p),
            f_np.ctypes.data_as(C.c_void_p), float(self.initial_next_frame_visibility_threshold), 6,
            ev_arr if evs else None, lo_arr if evs else None, hi_arr if evs else None, len(evs), _lib.ptr(traj), _lib.ptr(vis),
            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), C.byref(rounds)), "sampt_pips_track_f32")
        self.stats["windows"] += rounds.value
        self.stats["launches_per_round"] = int(self._lib.sampt_pips_round_launches(self._h))
        return traj.cpu(), vis.cpu() > 0.5

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        frames = _clip_of(rgbs, "Batch size > 1 is not supported for PIPS yet")  # tracker.py:50-51
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        dev = rgbs.device
        self._ensure(dev)
        T = frames.shape[0]
        q = query_points[0].detach().float().cpu()
        N = q.shape[0]
        pyr = self._prepared_pyramid(frames)
        chunk_events = self._prepared_events if pyr is not None else None
        if pyr is None:
            pyr = self.compute_pyramid(frames)
        # both temporal directions are independent chains too: run them in the same rounds (tracker.py:159-167)
        qf = q.clone()
        qf[:, 0] = T - qf[:, 0] - 1
        flipped = torch.cat([torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool)])
        # (a direction whose query sits on its last frame never runs a window, tracker.py:67: those chains are left out)
        q_all = torch.cat([q, qf])
        live = (q_all[:, 0] < T - 1).nonzero().flatten()
        tr_all = torch.zeros(T, 2 * N, 2)
        vi_all = torch.zeros(T, 2 * N, dtype=torch.bool)
        tr_all[q_all[:, 0].long(), torch.arange(2 * N)] = q_all[:, 1:]
        vi_all[q_all[:, 0].long(), torch.arange(2 * N)] = True
        if live.numel():
            tr_l, vi_l = self._run_chains(pyr, T, q_all[live], flipped[live], chunk_events)
            tr_all[:, live], vi_all[:, live] = tr_l, vi_l
        for c in (chunk_events or []):                          # chunks no round touched: still order this stream after them
            torch.cuda.current_stream().wait_event(c[2])
        tr_r, vi_r = tr_all[:, :N], vi_all[:, :N]
        tr_l, vi_l = tr_all[:, N:].flip(0), vi_all[:, N:].flip(0)
        traj, vis = tr_r.clone(), vi_r.clone()
        for n in range(N):                                                       # tracker.py:173-199
            s = int(q[n, 0].item())
            traj[:s, n] = tr_l[:s, n]
            vis[:s, n] = vi_l[:s, n]
            assert torch.allclose(traj[s, n], q[n, 1:]) and bool(vis[s, n])
        return traj.unsqueeze(0).to(dev), vis.unsqueeze(0).to(dev)


class PipsPlusPlusPointTracker(_ClipTracker):
    """PIPS++ behind the reference constructor of
    ``sam_pt.point_tracker.pips_plus_plus.PipsPlusPlusPointTracker`` (tracker.py:11-24; configs/model/point_tracker/
    pips_plus_plus.yaml).  Differences from the reference, on purpose:

    * the encoder runs ONCE per clip; the reference re-runs it for every (query frame, direction, chunk) although its
      per-frame InstanceNorm makes the maps identical, and sub-clips / time-reversed clips become frame-index maps;
    * queries on several frames and on the last frame work (the reference raises IndexError at tracker.py:121 for the
      former and returns T-1 frames for the latter — see oracle/pips2_ref.py);
    * ``image_size`` (off in the shipped config): the bilinear pre-resize runs on the device with torch (plumbing) and
      the float video feeds the encoder directly; the reference's coordinate scaling is kept verbatim, including its
      x <-> height / y <-> width mix-up (tracker.py:77-78, 126-128), which cancels on the way back.
    """
    _engines, _who = (("_h", "sampt_pips2_destroy"),), "PipsPlusPlusPointTracker"

    def __init__(self, checkpoint_path=None, stride=8, max_sequence_length=128, iters=16, image_size=None,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, seed: int = 72, fnet_chunk: int = 8):
        super().__init__()
        from .weights import init_pips2_state_dict
        self.checkpoint_path, self.stride = checkpoint_path, stride
        self.max_sequence_length, self.iters = max_sequence_length, iters
        self.image_size = tuple(image_size) if image_size is not None else None
        sd = state_dict if state_dict is not None else load_pips_checkpoint(checkpoint_path)
        self._sd = sd if sd is not None else init_pips2_state_dict(seed)
        self.fnet_chunk = fnet_chunk
        self.stats = {"chunks": 0, "fnet_frames": 0}

    def _build(self, lib, device):
        from .pack import pack_pips2
        self._w = pack_pips2(self._sd, device)
        return [_lib.create_engine(lib, "sampt_pips2_create", self._w, self.stride)]

    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def compute_pyramid(self, frames: torch.Tensor):
        """frames (T,3,H,W) uint8 (or float32 in [0,255]) on device -> 4 NHWC f32 levels [T][H/8 >> l][W/8 >> l][128]."""
        self._ensure(frames.device)
        is_f32 = 1 if frames.dtype == torch.float32 else 0
        T, _, H, W = frames.shape
        pyr = _alloc_pyramid(T, H // self.stride, W // self.stride, frames.device)
        chunk = min(self.fnet_chunk, T)
        ws = _lib.workspace("sampt_pips2_fnet_workspace_bytes", frames.device, self._h, chunk, H, W)
        frames = frames.contiguous()
        for t0, nf, outs in _pyramid_chunks(pyr, 0, T, chunk):
            _lib.check(self._lib.sampt_pips2_fnet_f32(self._h, _lib.ptr(frames[t0:t0 + nf]), is_f32, nf, H, W, outs, _lib.ptr(ws),
                                                      ws.numel(), _lib.stream_ptr()), "sampt_pips2_fnet_f32")
        self.stats["fnet_frames"] += T
        return pyr

    def prepare(self, frames: torch.Tensor, shard=None):
        """``shard`` is accepted for interface parity and ignored: PIPS++ encodes the whole clip on every rank."""
        if self.image_size is not None:        # forward() encodes the RESIZED float video: a pyramid of `frames` is unused
            return
        self._prepared = _prepared_entry(frames, self.compute_pyramid(frames))

    def _track(self, pyr, frame_ids: List[int], query_xy: torch.Tensor) -> torch.Tensor:
        """One direction (tracker.py:26-62): the clip is ``frame_ids`` (pyramid frame of every time step); chunks of
        ``max_sequence_length`` frames overlapping by one, templates carried from chunk to chunk.  -> (S,N,2) on device."""
        dev = pyr[0].device
        S_all, N = len(frame_ids), query_xy.shape[0]
        H0, W0 = pyr[0].shape[1:3]
        trajs = query_xy.to(dev)[None].repeat(S_all, 1, 1).contiguous()          # zero-velocity init
        pyr_ptrs = _lib.ptr_array(pyr)
        cur, done, have_init = 0, False, 0
        feats = None
        while not done:
            end = cur + self.max_sequence_length
            if end > S_all:
                diff = end - S_all
                end -= diff
                cur = max(cur - diff, 0)
            S = end - cur
            fidx = torch.tensor(frame_ids[cur:end], dtype=torch.int32)[None].repeat(N, 1).contiguous().to(dev)
            if feats is None:
                feats = [torch.empty((N, S, 128), dtype=torch.float32, device=dev) for _ in range(3)]
            else:                                                                # feat_init[:, :S_local] (tracker.py:52-54)
                feats = [f[:, :S].contiguous() for f in feats]
            ws = _lib.workspace("sampt_pips2_update_workspace_bytes", dev, self._h, N, S)
            t0 = trajs[cur:end].contiguous()
            out = torch.empty_like(t0)
            _lib.check(self._lib.sampt_pips2_update_f32(self._h, pyr_ptrs, H0, W0, _lib.ptr(fidx), N, S, _lib.ptr(t0),
                                                        have_init, _lib.ptr_array(feats), self.iters, _lib.ptr(out),
                                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sampt_pips2_update_f32")
            trajs[cur:end] = out
            trajs[end:] = trajs[end - 1:end]                                     # zero-velocity for the future
            have_init = 1
            self.stats["chunks"] += 1
            if end >= S_all:
                done = True
            else:
                cur = cur + self.max_sequence_length - 1
        return trajs

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        frames = _clip_of(rgbs, "Only batch size 1 is supported.")               # tracker.py:83
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        dev = rgbs.device
        self._ensure(dev)
        T, _, H, W = frames.shape
        q = query_points[0].detach().float().cpu()
        prepared = self._prepared_pyramid(frames)
        if self.image_size is not None:                                          # tracker.py:69-78
            fr = torch.nn.functional.interpolate(frames.float() / 255.0, size=self.image_size, mode="bilinear") * 255.0
            pyr = self.compute_pyramid(fr.contiguous())
            q[:, 1] *= self.image_size[0] / H
            q[:, 2] *= self.image_size[1] / W
        elif prepared is not None:
            pyr = prepared
        else:
            pyr = self.compute_pyramid(frames)
        N = q.shape[0]
        groups: Dict[int, List[int]] = {}
        for i in range(N):
            groups.setdefault(int(q[i, 0].item()), []).append(i)
        traj = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        for t, idxs in groups.items():                                           # tracker.py:84-122
            xy = q[idxs, 1:].contiguous()
            if t != T - 1:
                traj[t:, idxs] = self._track(pyr, list(range(t, T)), xy)
            if t != 0:
                right = self._track(pyr, list(range(t, -1, -1)), xy).flip(0)     # frames 0..t
                traj[:t + 1 if t == T - 1 else t, idxs] = right if t == T - 1 else right[:-1]
        if self.image_size is not None:                                          # tracker.py:126-128
            traj[:, :, 0] *= H / self.image_size[0]
            traj[:, :, 1] *= W / self.image_size[1]
        vis = torch.ones((1, T, N), dtype=torch.float32, device=dev)             # PIPS++ predicts no visibility (:64)
        return traj.unsqueeze(0), vis


_COTRACKER_MODELS = {"cotracker_stride_4_wind_8": (8, 4), "cotracker_stride_4_wind_12": (12, 4),
                     "cotracker_stride_8_wind_16": (16, 8)}


def cotracker_model_from_checkpoint_name(checkpoint_path: str) -> Tuple[int, int]:
    """(window length S, stride) of a CoTracker checkpoint, chosen from the FILE NAME as upstream's ``build_cotracker`` does
    (co-tracker @ 4f297a9, cotracker/models/build_cotracker.py: ``model_name = checkpoint.split("/")[-1].split(".")[0]``,
    unknown names raise ValueError).  The three checkpoints of configs/model/point_tracker/cotracker.yaml:2-4 share every
    weight SHAPE (UpdateFormer and fnet do not depend on S or the stride), so loading one into the wrong model would run
    silently with the wrong window — the name is the only thing that tells them apart."""
    import os
    name = os.path.basename(str(checkpoint_path)).split(".")[0]
    if name not in _COTRACKER_MODELS:
        raise ValueError(f"Unknown model name {name}")
    return _COTRACKER_MODELS[name]


def load_cotracker_checkpoint(checkpoint_path: Optional[str]):
    """``build_cotracker`` convention (co-tracker @ 4f297a9): a ``.pth`` state dict, optionally under the key 'model'."""
    if checkpoint_path is None:
        return None
    with open(checkpoint_path, "rb") as f:
        sd = torch.load(f, map_location="cpu")
    return sd["model"] if "model" in sd else sd


def get_points_on_a_grid(grid_size: int, interp_shape) -> torch.Tensor:
    """Upstream's support grid (cotracker.py ``get_points_on_a_grid``): (grid_size^2, 2) = (x, y), a regular grid with a
    margin of ``interp_shape[1] // 64`` pixels, rows first."""
    if grid_size == 1:
        return torch.tensor([[interp_shape[1] / 2, interp_shape[0] / 2]])
    step = interp_shape[1] // 64
    lin = torch.linspace(0, grid_size - 1, grid_size)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    gy = step + gy.reshape(-1) / float(grid_size - 1) * (interp_shape[0] - step * 2)
    gx = step + gx.reshape(-1) / float(grid_size - 1) * (interp_shape[1] - step * 2)
    return torch.stack([gx, gy], dim=-1)


class CoTrackerPointTracker(_ClipTracker):
    """CoTracker behind the constructor of ``sam_pt.point_tracker.cotracker.CoTrackerPointTracker``
    (cotracker/tracker.py:32-66; configs/model/point_tracker/cotracker.yaml) — the reference's default tracker.

    The adapter logic is the reference's: float video resized bilinearly to ``interp_shape`` and queries rescaled
    (tracker.py:87-96), a ``support_grid_size``^2 grid of support queries every ``support_grid_every_n_frames`` frames
    (:98-102), the model with 6 iterations (:104), the time-flipped pass filling entries that are exactly 0 (:154-170),
    support points dropped, visibility > threshold, trajectories scaled back (:144-150); clips shorter than the window
    are padded with their last frame (:12-24).  Different on purpose:

    * the encoder runs ONCE per frame for both temporal directions (upstream re-encodes 4 new frames per window and the
      whole clip again for the flipped pass; InstanceNorm is per-sample, so the maps are identical);
    * a whole direction is ONE device call (``sampt_cotracker_track_f32``): window membership depends only on the query
      frames, the window-to-window carry stays on the device, nothing synchronises with the host;
    * the debug visualisation branch (cv2 / imageio, :107-142) is control plane and not built.
    """
    _engines, _who = (("_h", "sampt_cotracker_destroy"),), "CoTrackerPointTracker"

    def __init__(self, checkpoint_path=None, interp_shape=(384, 512), visibility_threshold=0.7, support_grid_size=2,
                 support_grid_every_n_frames=12, add_debug_visualisations=False,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, seed: int = 72, fnet_chunk: int = 8, iters: int = 6):
        super().__init__()
        self.checkpoint_path = checkpoint_path
        self.interp_shape = tuple(interp_shape) if interp_shape is not None else None
        self.visibility_threshold = visibility_threshold
        self.support_grid_size = support_grid_size
        self.support_grid_every_n_frames = support_grid_every_n_frames
        self.add_debug_visualisations = add_debug_visualisations
        if add_debug_visualisations:
            raise NotImplementedError("add_debug_visualisations (cv2 / imageio gif dump, tracker.py:107-142) is not built")
        from .weights import init_cotracker_state_dict
        self.s, self.stride = 8, 4            # the HIP engine is built for cotracker_stride_4_wind_8 (the YAML's default)
        if state_dict is None and checkpoint_path is not None:
            s_ckpt, stride_ckpt = cotracker_model_from_checkpoint_name(checkpoint_path)
            if (s_ckpt, stride_ckpt) != (self.s, self.stride):
                raise NotImplementedError(
                    f"{checkpoint_path}: CoTracker with window {s_ckpt} / stride {stride_ckpt} is not built; the HIP engine "
                    f"implements cotracker_stride_4_wind_8 (window {self.s}, stride {self.stride}) only")
        sd = state_dict if state_dict is not None else load_cotracker_checkpoint(checkpoint_path)
        self._sd = sd if sd is not None else init_cotracker_state_dict(seed)
        self.fnet_chunk, self.iters = fnet_chunk, iters
        self._pos: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self.stats = {"windows": 0, "fnet_frames": 0, "calls": 0}

    def _build(self, lib, device):
        from .pack import pack_cotracker
        self._w = pack_cotracker(self._sd, device, self.s)
        return [_lib.create_engine(lib, "sampt_cotracker_create", self._w, self.stride, self.s)]

    def on_replace(self):
        self._pos = {}                                         # position tables of the old device

    # -- resize + encoder for a whole clip ---------------------------------------------------------------------
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def compute_pyramid(self, frames: torch.Tensor, shard=None):
        """frames (T,3,H,W) uint8 / float32 on device -> 4 NHWC f32 levels [T][h/4 >> l][w/4 >> l][128] of the video resized
        to ``interp_shape`` (h, w).  ``shard`` (sam_pt_amd.dist.FnetShard): resize + encode this rank's frames only, the rest
        arrives through ``shard.exchange`` (see PipsPointTracker.compute_pyramid)."""
        self._ensure(frames.device)
        dev = frames.device
        T, _, H, W = frames.shape
        h, w = self.interp_shape if self.interp_shape is not None else (H, W)
        frames = frames.contiguous()
        if frames.dtype != torch.uint8:
            frames = frames.float()
        pyr = _alloc_pyramid(T, h // self.stride, w // self.stride, dev, shard)
        chunk = min(self.fnet_chunk, T)
        ws = _lib.workspace("sampt_cotracker_fnet_workspace_bytes", dev, self._h, chunk, h, w)

        def encode(lo, hi):
            if hi <= lo:
                return
            small = torch.empty((hi - lo, 3, h, w), dtype=torch.float32, device=dev)
            _lib.check(self._lib.sampt_resize_frames_f32(_lib.ptr(frames[lo:hi]), 1 if frames.dtype == torch.uint8 else 0,
                                                         (hi - lo) * 3, H, W, _lib.ptr(small), h, w, _lib.stream_ptr()),
                       "sampt_resize_frames_f32")
            for t0, nf, outs in _pyramid_chunks(pyr, lo, hi, chunk):
                _lib.check(self._lib.sampt_cotracker_fnet_f32(self._h, _lib.ptr(small[t0 - lo:t0 - lo + nf]), nf, h, w, outs,
                                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sampt_cotracker_fnet_f32")
            self.stats["fnet_frames"] += hi - lo

        return _sharded_encode(pyr, T, shard, encode)

    def prepare(self, frames: torch.Tensor, shard=None):
        """Build the (resized) clip's feature pyramid now, on the current stream; the next ``forward`` on the same frames
        tensor reuses it (see PipsPointTracker.prepare)."""
        self._prepared = _prepared_entry(frames, self.compute_pyramid(frames, shard=shard))

    def _pos_tables(self, H0: int, W0: int, dev):
        if (H0, W0) not in self._pos:
            from .pack import cotracker_pos_tables
            px, py = cotracker_pos_tables(H0, W0)
            self._pos[(H0, W0)] = (px.to(dev), py.to(dev))
        return self._pos[(H0, W0)]

    def _model(self, pyr, T: int, q: torch.Tensor, flipped: bool):
        """One ``CoTrackerForShortVideosWrapper.__call__`` (tracker.py:17-24): q (n,3) CPU = (t, x, y) in the model's own
        time axis and frame size; ``flipped`` = the clip is time-reversed (model frame t = pyramid frame T-1-t).
        -> traj (T,n,2), vis (T,n) on the device, in the order of q."""
        dev = pyr[0].device
        n = q.shape[0]
        Tm = max(T, self.s)                                            # short clips: last frame repeated
        t = torch.arange(Tm).clamp(max=T - 1)
        fmap = ((T - 1 - t) if flipped else t).to(torch.int32)
        qt = q[:, 0].long()
        order = torch.sort(qt, stable=True).indices                    # CoTracker.forward sorts the points by query frame
        inv = torch.argsort(order)
        qt_s = qt[order].to(torch.int32).contiguous()
        H0, W0 = pyr[0].shape[1:3]
        px, py = self._pos_tables(H0, W0, dev)
        ws = _lib.workspace("sampt_cotracker_track_workspace_bytes", dev, self._h, n)
        traj = torch.empty((Tm, n, 2), dtype=torch.float32, device=dev)
        vis = torch.empty((Tm, n), dtype=torch.float32, device=dev)
        fmap_d, qt_d = fmap.to(dev).contiguous(), qt_s.to(dev)
        qxy_d = q[order, 1:].float().contiguous().to(dev)
        _lib.check(self._lib.sampt_cotracker_track_f32(self._h, _lib.ptr_array(pyr), H0, W0, Tm, _lib.ptr(fmap_d), n,
                                                       C.c_void_p(qt_s.data_ptr()), _lib.ptr(qt_d), _lib.ptr(qxy_d),
                                                       _lib.ptr(px), _lib.ptr(py), self.iters, _lib.ptr(traj), _lib.ptr(vis),
                                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "sampt_cotracker_track_f32")
        self.stats["calls"] += 1
        inv_d = inv.to(dev)
        return traj[:T].index_select(1, inv_d), vis[:T].index_select(1, inv_d)

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        frames = _clip_of(rgbs, "Batch size > 1 is not supported for CoTracker")   # the model asserts B == 1
        dev = rgbs.device
        self._ensure(dev)
        T, _, H, W = frames.shape
        if self.interp_shape is None:                                   # tracker.py:87-88 (kept on the object)
            self.interp_shape = (H, W)
        h, w = self.interp_shape
        q = query_points[0].detach().float().cpu().clone()
        assert q.shape[1] == 3
        n_points = q.shape[0]
        q[:, 1] *= w / W                                                # tracker.py:95-96
        q[:, 2] *= h / H
        if self.support_grid_size > 0:                                  # tracker.py:98-102
            for i in range(0, T, self.support_grid_every_n_frames):
                g = get_points_on_a_grid(self.support_grid_size, (h, w))
                q = torch.cat([q, torch.cat([torch.full((g.shape[0], 1), float(i)), g], dim=1)], dim=0)
        pyr = self._prepared_pyramid(frames)
        if pyr is None:
            pyr = self.compute_pyramid(frames)
        traj, vis = self._model(pyr, T, q, False)                       # tracker.py:104
        qf = q.clone()                                                  # _compute_backward_tracks, tracker.py:154-170
        qf[:, 0] = T - qf[:, 0] - 1
        traj_f, vis_f = self._model(pyr, T, qf, True)
        traj_f, vis_f = traj_f.flip(0), vis_f.flip(0)
        mask = traj == 0
        traj = torch.where(mask, traj_f, traj)
        vis = torch.where(mask[:, :, 0], vis_f, vis)
        traj, vis = traj[:, :n_points].clone(), vis[:, :n_points].clone()     # tracker.py:144-150
        visb = vis > self.visibility_threshold
        traj[:, :, 0] *= W / float(w)
        traj[:, :, 1] *= H / float(h)
        return traj.unsqueeze(0), visb.unsqueeze(0)


# ------------------------------------------------------------------------------------------------------------------
# RAFT
# ------------------------------------------------------------------------------------------------------------------
RAFT_MIN_SIDE = 128      # padded frame side below which the coarsest correlation level is a single cell


def raft_padded_size(H: int, W: int) -> Tuple[int, int]:
    """Frame size after InputPadder (raft_core/util.py:9-22): the next multiples of 8."""
    return (H + 7) // 8 * 8, (W + 7) // 8 * 8


def load_raft_checkpoint(checkpoint_path: Optional[str]):
    """``Raftnet.__init__`` (raftnet.py:20-27): the checkpoint was saved from nn.DataParallel, so ``module.`` is removed
    from every key.  None -> seeded random init."""
    if checkpoint_path is None:
        return None
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Raft checkpoint not found at {checkpoint_path}")          # raft/tracker.py:24-25
    sd = torch.load(checkpoint_path, map_location="cpu")
    return {k.replace("module.", ""): v for k, v in sd.items() if k != "module"}


class RaftPointTracker(_EngineTracker):
    """RAFT optical flow chained into point tracks, behind the constructor of
    ``sam_pt.point_tracker.raft.RaftPointTracker`` (raft/tracker.py:17-27; configs/model/point_tracker/raft.yaml).
    ``iters`` is an extra keyword; its default is the reference's hard-coded 32 (tracker.py:40-41).

    Differences from the reference, on purpose:

    * both encoders run ONCE per frame (the reference runs ``fnet`` four times and ``cnet`` twice on every inner frame);
      the mask head and the convex upsampling run after the last iteration only;
    * frames whose size padded to multiples of 8 is below 128 on either side are refused by name.  There the coarsest of
      the four correlation levels is a single cell, ``bilinear_sampler`` divides by ``W - 1 = 0`` and the reference returns
      NaN everywhere.
    """
    _engines, _who = (("_h", "sampt_raft_destroy"),), "RaftPointTracker"

    def __init__(self, checkpoint_path=None, iters: int = 32, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 72, max_pairs_in_flight: int = 8):
        super().__init__()
        from .weights import init_raft_state_dict
        self.checkpoint_path, self.iters = checkpoint_path, int(iters)
        if self.iters < 1:
            raise ValueError("RaftPointTracker: iters must be at least 1")
        sd = state_dict if state_dict is not None else load_raft_checkpoint(checkpoint_path)
        self._sd = sd if sd is not None else init_raft_state_dict(seed)
        self.max_pairs_in_flight = max(1, int(max_pairs_in_flight))
        self.stats = {"pair_directions": 0, "encoded_frames": 0}

    def _build(self, lib, device):
        from .pack import pack_raft
        self._w = pack_raft(self._sd, device)
        return [_lib.create_engine(lib, "sampt_raft_create", self._w)]

    @staticmethod
    def check_frame_size(H: int, W: int):
        Hp, Wp = raft_padded_size(H, W)
        if Hp < RAFT_MIN_SIDE or Wp < RAFT_MIN_SIDE:
            raise ValueError(f"RaftPointTracker: frames of {H} x {W} pixels (padded to {Hp} x {Wp}) are too small: RAFT needs at "
                             f"least {RAFT_MIN_SIDE} pixels on both sides, or the coarsest of its 4 correlation levels is a "
                             "single cell (the reference returns NaN there)")

    @torch.no_grad()
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def flows(self, frames: torch.Tensor, iters: Optional[int] = None, return_low: bool = False,
              workspace_pairs: Optional[int] = None):
        """frames (T,3,H,W) uint8 on the device -> (flows_forward, flows_backward), each (T-1,2,H,W) f32: pair t holds the
        flow from frame t to t+1 and from t+1 to t.  ``return_low`` adds the 1/8-resolution flows (2,T-1,2,Hp/8,Wp/8).
        ``workspace_pairs`` sizes the workspace for that many pairs per chunk (default: ``max_pairs_in_flight``)."""
        if frames.dim() == 5:
            if frames.shape[0] != 1:
                raise ValueError("RaftPointTracker.flows takes one clip (T,3,H,W)")
            frames = frames[0]
        assert frames.dtype == torch.uint8, "frames must be uint8 (PointTracker.forward contract)"
        T, _, H, W = frames.shape
        self.check_frame_size(H, W)
        dev = frames.device
        self._ensure(dev)
        Hp, Wp = raft_padded_size(H, W)
        fwd = torch.empty((max(T - 1, 0), 2, H, W), dtype=torch.float32, device=dev)
        bwd = torch.empty_like(fwd)
        low = torch.empty((2, max(T - 1, 0), 2, Hp // 8, Wp // 8), dtype=torch.float32, device=dev) if return_low else None
        if T > 1:
            pairs = min(T - 1, workspace_pairs if workspace_pairs is not None else self.max_pairs_in_flight)
            ws = _lib.workspace("sampt_raft_workspace_bytes", dev, self._h, T, H, W, pairs)
            _lib.check(self._lib.sampt_raft_flows_f32(self._h, _lib.ptr(frames.contiguous()), T, H, W,
                                                      self.iters if iters is None else int(iters), _lib.ptr(fwd), _lib.ptr(bwd),
                                                      _lib.ptr(low), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "sampt_raft_flows_f32")
            self.stats["pair_directions"] += 2 * (T - 1)
            self.stats["encoded_frames"] += T
        return (fwd, bwd, low) if return_low else (fwd, bwd)

    @torch.no_grad()
    @_lib.on_device(lambda self, fwd, *a, **k: fwd.device)
    def chain(self, fwd: torch.Tensor, bwd: torch.Tensor, query_points: torch.Tensor):
        """tracker.py:46-88 on the device: flows (T-1,2,H,W), query_points (N,3) = (t, x, y) -> trajectories (T,N,2) f32,
        visibilities (T,N) bool."""
        _lib.require_hip(fwd.device, "RaftPointTracker")
        lib = _lib.load()
        T, H, W = fwd.shape[0] + 1, fwd.shape[2], fwd.shape[3]
        q = query_points.detach().to(device=fwd.device, dtype=torch.float32).contiguous()
        N = q.shape[0]
        traj = torch.empty((T, N, 2), dtype=torch.float32, device=fwd.device)
        vis = torch.empty((T, N), dtype=torch.uint8, device=fwd.device)
        if N > 0:
            _lib.check(lib.sampt_raft_chain(_lib.ptr(fwd.contiguous()) if T > 1 else None, _lib.ptr(bwd.contiguous()) if T > 1 else None,
                                            T, H, W, _lib.ptr(q), N, _lib.ptr(traj), _lib.ptr(vis), _lib.stream_ptr()),
                       "sampt_raft_chain")
        return traj, vis.bool()

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        B, T, _, H, W = rgbs.shape
        self.check_frame_size(H, W)
        _lib.require_hip(rgbs.device, "RaftPointTracker")
        trajs, viss = [], []
        for b in range(B):                                       # any batch size: one clip at a time
            fwd, bwd = self.flows(rgbs[b])
            t, v = self.chain(fwd, bwd, query_points[b])
            trajs.append(t)
            viss.append(v)
        return torch.stack(trajs), torch.stack(viss)


# ------------------------------------------------------------------------------------------------------------------
# TAPIR (sam_pt/point_tracker/tapir/)
# ------------------------------------------------------------------------------------------------------------------
TAPIR_SIZE = 256          # configs/tapir_config.py: inference.resize_height / resize_width


class TapirPointTracker(_EngineTracker):
    """TAPIR behind the constructor of ``sam_pt.point_tracker.tapir.TapirPointTracker`` (tapir/tracker.py:14-37;
    configs/model/point_tracker/tapir.yaml: ``checkpoint_path``, ``visibility_threshold``).  PARITY UNPINNED: the reference model
    needs JAX, Haiku and a checkpoint, none of which exists where this project is built; the device path is held to the
    restatement of tests/tapir_ref.py, and ``load_tapir_checkpoint``'s key map is unverified against a real checkpoint.

    ``forward`` is tracker.py:72-108: the clip / 255 goes through the same antialiased ``F.interpolate`` to 256 x 256 (on the
    device tensor), the queries are scaled and flipped, the model runs — ONE device call per clip: the ResNet once per frame, the
    cost-volume heads and the four refinements for all queries of the clip, any number of frames, no window chaining —, and
    ``visibilities = (1 - sigmoid(occlusion)) * (1 - sigmoid(expected_dist)) > visibility_threshold``.  The reference's random
    query permutation and its chunks of 64 change no value (queries are independent), so they are not reproduced."""
    _engines, _who = (("_h", "sampt_tapir_destroy"),), "TapirPointTracker"

    def __init__(self, checkpoint_path=None, visibility_threshold: float = 0.1, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 72, max_queries_in_flight: int = 256):
        super().__init__()
        from .weights import init_tapir_state_dict, load_tapir_checkpoint
        self.checkpoint_path, self.visibility_threshold = checkpoint_path, visibility_threshold
        sd = state_dict if state_dict is not None else (load_tapir_checkpoint(checkpoint_path) if checkpoint_path is not None else None)
        self._sd = sd if sd is not None else init_tapir_state_dict(seed)
        self.max_queries_in_flight = max(1, int(max_queries_in_flight))
        self.iters = 4                                          # num_pips_iter (tapir_model.py:267)
        self.stats = {"clips": 0, "launches": 0}

    def _build(self, lib, device):
        from .pack import pack_tapir
        self._w = pack_tapir(self._sd, device)
        return [_lib.create_engine(lib, "sampt_tapir_create", self._w)]

    @torch.no_grad()
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def track(self, frames: torch.Tensor, queries: torch.Tensor, iters: Optional[int] = None, return_iters: bool = False,
              workspace_queries: Optional[int] = None):
        """The model on one clip: frames (T,3,256,256) f32 in [0, 1] on the device, queries (N,3) = (t, x, y) in 256 x 256 pixels
        -> tracks (N,T,2), occlusion (N,T), expected_dist (N,T) [, per-iteration (iters + 1,N,T,4) = x, y, occlusion,
        expected_dist].  ``workspace_queries``: queries per refinement chunk (default ``max_queries_in_flight``); the workspace is sized
        for it and the values do not depend on it."""
        _lib.require_hip(frames.device, self._who)
        assert frames.dtype == torch.float32 and tuple(frames.shape[1:]) == (3, TAPIR_SIZE, TAPIR_SIZE), "frames must be (T,3,256,256) f32"
        dev = frames.device
        self._ensure(dev)
        T, N = frames.shape[0], queries.shape[0]
        iters = self.iters if iters is None else int(iters)
        q = queries.detach().to(device=dev, dtype=torch.float32).contiguous()
        tracks = torch.empty((N, T, 2), dtype=torch.float32, device=dev)
        occ = torch.empty((N, T), dtype=torch.float32, device=dev)
        expd = torch.empty_like(occ)
        its = torch.empty((iters + 1, N, T, 4), dtype=torch.float32, device=dev) if return_iters else None
        if N > 0:
            qc = min(N, workspace_queries if workspace_queries is not None else self.max_queries_in_flight)
            ws = _lib.workspace("sampt_tapir_workspace_bytes", dev, self._h, T, N, qc)
            _lib.check(self._lib.sampt_tapir_set_max_queries(self._h, qc), "sampt_tapir_set_max_queries")
            _lib.check(self._lib.sampt_tapir_track_f32(self._h, _lib.ptr(frames.contiguous()), T, _lib.ptr(q), N, iters, _lib.ptr(tracks),
                                                       _lib.ptr(occ), _lib.ptr(expd), _lib.ptr(its), _lib.ptr(ws), ws.numel(),
                                                       _lib.stream_ptr()), "sampt_tapir_track_f32")
            self.stats["clips"] += 1
            self.stats["launches"] = int(self._lib.sampt_tapir_launches(self._h))
        return (tracks, occ, expd, its) if return_iters else (tracks, occ, expd)

    def _model(self, frames01: torch.Tensor, q_tyx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """What the reference calls ``jitted_forward``, on our inputs: frames01 (B,T,3,256,256) in [0, 1] (the model's ``* 2 - 1``
        happens on the device), q_tyx (B,N,3) = (t, y, x) -> tracks (B,N,T,2), occlusion, expected_dist (B,N,T)."""
        outs = [self.track(frames01[b], q_tyx[b][:, [0, 2, 1]]) for b in range(frames01.shape[0])]      # any batch size: one clip at a time
        return {k: torch.stack([o[i] for o in outs]) for i, k in enumerate(("tracks", "occlusion", "expected_dist"))}

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        B, T, _, H, W = rgbs.shape
        size = (TAPIR_SIZE, TAPIR_SIZE)
        rescale_hw = torch.tensor(size) / torch.tensor((H, W))
        frames01 = torch.nn.functional.interpolate(rgbs.flatten(0, 1) / 255, size, mode="bilinear", align_corners=False,
                                                   antialias=True).unflatten(0, (B, T))
        q = query_points.detach().cpu().clone()
        q[:, :, 1:] *= rescale_hw.flip(0)
        q[:, :, 1:] = q[:, :, 1:].flip(-1)                        # (t, x, y) -> (t, y, x)
        out = self._model(frames01, q)
        dev = out["tracks"].device
        expected_dist = out["expected_dist"].permute(0, 2, 1)
        occlusion = out["occlusion"].permute(0, 2, 1)
        visibilities = (1 - torch.sigmoid(occlusion)) * (1 - torch.sigmoid(expected_dist)) > self.visibility_threshold
        trajectories = out["tracks"].permute(0, 2, 1, 3) / rescale_hw.flip(-1).to(dev)
        return trajectories, visibilities


# ------------------------------------------------------------------------------------------------------------------
# TapNet (sam_pt/point_tracker/tapnet/)
# ------------------------------------------------------------------------------------------------------------------
TAPNET_SIZE = 256         # configs/tapnet_config.py: inference.resize_height / resize_width


class TapnetPointTracker(_EngineTracker):
    """TapNet behind the constructor of ``sam_pt.point_tracker.tapnet.TapnetPointTracker`` (tapnet/tracker.py:13-36;
    configs/model/point_tracker/tapnet.yaml: ``checkpoint_path``, ``visibility_threshold``).  PARITY UNPINNED: the reference model
    needs JAX, Haiku and a checkpoint, none of which exists where this project is built; the device path is held to the
    restatement of tests/tapnet_ref.py, and ``load_tapnet_checkpoint``'s key map is unverified against a real checkpoint.

    Only the adapter's configuration is built: TSM-ResNet-18 up to unit 2 at output stride 8 on a 5-D input (``tsm_mode='gpu'``,
    ``num_frames`` = the clip's length), one head, 256 x 256 frames.

    ``forward`` is tracker.py:67-103: the clip / 255 goes through the same antialiased ``F.interpolate`` to 256 x 256 (on the
    device tensor), the queries are scaled and flipped, the model runs — ONE device call per clip, every block of the backbone over
    all frames at once —, and ``visibilities = (1 - sigmoid(occlusion)) > visibility_threshold``.  The reference's chunks of 16
    queries change no value (queries are independent), so they are not reproduced."""
    _engines, _who = (("_h", "sampt_tapnet_destroy"),), "TapnetPointTracker"

    def __init__(self, checkpoint_path=None, visibility_threshold: float = 0.5, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 72):
        super().__init__()
        from .weights import init_tapnet_state_dict, load_tapnet_checkpoint
        self.checkpoint_path, self.visibility_threshold = checkpoint_path, visibility_threshold
        sd = state_dict if state_dict is not None else (load_tapnet_checkpoint(checkpoint_path) if checkpoint_path is not None else None)
        self._sd = sd if sd is not None else init_tapnet_state_dict(seed)
        self.stats = {"clips": 0, "launches": 0}

    def _build(self, lib, device):
        from .pack import pack_tapnet
        self._w = pack_tapnet(self._sd, device)
        return [_lib.create_engine(lib, "sampt_tapnet_create", self._w)]

    @torch.no_grad()
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def track(self, frames: torch.Tensor, queries: torch.Tensor):
        """The model on one clip: frames (T,3,256,256) f32 in [0, 1] on the device, queries (N,3) = (t, x, y) in 256 x 256 pixels
        -> tracks (N,T,2), occlusion (N,T) logits."""
        _lib.require_hip(frames.device, self._who)
        assert frames.dtype == torch.float32 and tuple(frames.shape[1:]) == (3, TAPNET_SIZE, TAPNET_SIZE), "frames must be (T,3,256,256) f32"
        dev = frames.device
        self._ensure(dev)
        T, N = frames.shape[0], queries.shape[0]
        q = queries.detach().to(device=dev, dtype=torch.float32).contiguous()
        tracks = torch.empty((N, T, 2), dtype=torch.float32, device=dev)
        occ = torch.empty((N, T), dtype=torch.float32, device=dev)
        if N > 0:
            ws = _lib.workspace("sampt_tapnet_workspace_bytes", dev, self._h, T, N)
            _lib.check(self._lib.sampt_tapnet_track_f32(self._h, _lib.ptr(frames.contiguous()), T, _lib.ptr(q), N, _lib.ptr(tracks),
                                                        _lib.ptr(occ), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sampt_tapnet_track_f32")
            self.stats["clips"] += 1
            self.stats["launches"] = int(self._lib.sampt_tapnet_launches(self._h))
        return tracks, occ

    def _model(self, frames01: torch.Tensor, q_tyx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """What the reference calls ``jitted_forward``, on our inputs: frames01 (B,T,3,256,256) in [0, 1] (the model's ``* 2 - 1``
        happens on the device), q_tyx (B,N,3) = (t, y, x) -> tracks (B,N,T,2), occlusion (B,N,T)."""
        outs = [self.track(frames01[b], q_tyx[b][:, [0, 2, 1]]) for b in range(frames01.shape[0])]      # any batch size: one clip at a time
        return {k: torch.stack([o[i] for o in outs]) for i, k in enumerate(("tracks", "occlusion"))}

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        B, T, _, H, W = rgbs.shape
        size = (TAPNET_SIZE, TAPNET_SIZE)
        rescale_hw = torch.tensor(size) / torch.tensor((H, W))
        frames01 = torch.nn.functional.interpolate(rgbs.flatten(0, 1) / 255, size, mode="bilinear", align_corners=False,
                                                   antialias=True).unflatten(0, (B, T))
        q = query_points.detach().cpu().clone()
        q[:, :, 1:] *= rescale_hw.flip(0)
        q[:, :, 1:] = q[:, :, 1:].flip(-1)                        # (t, x, y) -> (t, y, x)
        out = self._model(frames01, q)
        dev = out["tracks"].device
        occlusion = out["occlusion"].permute(0, 2, 1)
        visibilities = (1 - torch.sigmoid(occlusion)) > self.visibility_threshold
        trajectories = out["tracks"].permute(0, 2, 1, 3) / rescale_hw.flip(-1).to(dev)
        return trajectories, visibilities


# ------------------------------------------------------------------------------------------------------------------
# SuperGlue (sam_pt/point_tracker/superglue/)
# ------------------------------------------------------------------------------------------------------------------
SUPERPOINT_DEFAULTS = {"descriptor_dim": 256, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": -1,
                       "remove_borders": 4}                                                  # superpoint.py:107-113
SUPERGLUE_DEFAULTS = {"descriptor_dim": 256, "weights": "indoor", "keypoint_encoder": [32, 64, 128, 256],
                      "GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.2}   # superglue.py:199-206


def superglue_keypoint_capacity(H: int, W: int, nms_radius: int) -> int:
    """Keypoints a frame can hold at most: survivors of simple_nms are at least ``nms_radius + 1`` pixels apart."""
    s = int(nms_radius) + 1
    return max(1, ((H + s - 1) // s) * ((W + s - 1) // s))


def register_with_reference() -> bool:
    """The reference's ``SamPt`` recognises the mask-consuming tracker by ``isinstance(self.point_tracker,
    SuperGluePointTracker)`` against ITS class (sam_pt/modeling/sam_pt.py:189, :437).  That class is an ABC (``PointTracker``
    is one), so ours is registered as a virtual subclass of it and passes that test.  Returns False where the reference
    package is not importable (nothing to register with)."""
    try:
        from sam_pt.point_tracker.superglue.tracker import SuperGluePointTracker as Ref
    except Exception:
        return False
    Ref.register(SuperGluePointTracker)
    return True


class SuperGluePointTracker(_EngineTracker):
    """SuperPoint keypoints of frame 0 matched by SuperGlue to every later frame, independently per frame, behind the
    constructor of ``sam_pt.point_tracker.superglue.SuperGluePointTracker`` (superglue/tracker.py:24-61;
    configs/model/point_tracker/superglue.yaml).  The only tracker that needs ``set_masks`` before ``forward``.

    The whole clip runs on the device (csrc/engine_superglue.hip, csrc/superglue.hip): SuperPoint once per frame, SuperGlue
    per pair, and the tracker's per-mask split of the matched points.  The random draws stay on the host, in the
    reference's order and with its arguments (``np.random.choice(a=len, size=min(len, k))``, per frame, per mask,
    positives then negatives), so a seeded run consumes NumPy's global generator identically.  Host synchronisations per
    clip: the keypoint counts and the selection counts — two, whatever T is.

    ``matching_config[...]['checkpoint']`` absent or None: seeded random weights (``seed``).  Refused by name:
    ``resize`` other than "no resize" (the reference raises on it as well), ``max_keypoints`` other than -1, and network
    shapes other than the shipped ones."""
    _engines, _who = (("_h", "sampt_sg_destroy"),), "SuperGluePointTracker"

    def __init__(self, positive_points_per_mask: int, negative_points_per_mask: int, resize, matching_config,
                 seed: int = 72, keypoint_capacity: Optional[int] = None,
                 state_dicts: Optional[Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]] = None):
        super().__init__()
        self.positive_points_per_mask = int(positive_points_per_mask)
        self.negative_points_per_mask = int(negative_points_per_mask)
        if self.positive_points_per_mask < 0 or self.negative_points_per_mask < 0 or \
                self.positive_points_per_mask + self.negative_points_per_mask < 1:
            raise ValueError("SuperGluePointTracker: needs at least one point per mask")
        resize = [int(v) for v in resize]
        if len(resize) == 2 and resize[1] == -1:
            resize = resize[0:1]
        if len(resize) > 2 or len(resize) == 0:
            raise ValueError("SuperGluePointTracker: Cannot specify more than two integers for `resize`")
        if len(resize) == 2 or resize[0] > 0:
            raise NotImplementedError(f"SuperGluePointTracker: resize={resize} is not supported: the reference's resize path "
                                      "raises NotImplementedError as well (superglue/tracker.py:91-97); use resize=[-1, -1]")
        self.resize = resize
        cfg = {k: dict(v) for k, v in dict(matching_config).items()}
        self.matching_config = cfg
        sp = {**SUPERPOINT_DEFAULTS, **cfg.get("superpoint", {})}
        sg = {**SUPERGLUE_DEFAULTS, **cfg.get("superglue", {})}
        if int(sp["max_keypoints"]) != -1:
            raise NotImplementedError(f"SuperGluePointTracker: max_keypoints={sp['max_keypoints']} is not supported (top-k "
                                      "selection is not built); the shipped value is -1")
        if int(sp["descriptor_dim"]) != 256 or int(sg["descriptor_dim"]) != 256:
            raise NotImplementedError("SuperGluePointTracker: descriptor_dim must be 256")
        if list(sg["keypoint_encoder"]) != SUPERGLUE_DEFAULTS["keypoint_encoder"] or list(sg["GNN_layers"]) != SUPERGLUE_DEFAULTS["GNN_layers"]:
            raise NotImplementedError("SuperGluePointTracker: keypoint_encoder / GNN_layers other than the shipped networks")
        if int(sp["nms_radius"]) < 0 or int(sp["nms_radius"]) > 16:
            raise NotImplementedError("SuperGluePointTracker: nms_radius must be within 0..16")
        if int(sg["sinkhorn_iterations"]) < 0:
            raise ValueError("SuperGluePointTracker: sinkhorn_iterations must not be negative")
        self.sp_cfg, self.sg_cfg = sp, sg
        from .weights import init_superglue_state_dict, init_superpoint_state_dict
        if state_dicts is not None:
            self._sp_sd, self._sg_sd = state_dicts
        else:
            a, b = sp.get("checkpoint"), sg.get("checkpoint")
            self._sp_sd = torch.load(a, map_location="cpu") if a is not None else init_superpoint_state_dict(seed)
            self._sg_sd = torch.load(b, map_location="cpu") if b is not None else init_superglue_state_dict(seed)
        self.keypoint_capacity = keypoint_capacity
        self.masks = None
        self.stats = {"frames": 0, "pairs": 0, "host_syncs": 0, "keypoints": []}

    def _build(self, lib, device):
        from .pack import pack_superglue
        self._w = pack_superglue(self._sp_sd, self._sg_sd, device)
        return [_lib.create_engine(lib, "sampt_sg_create", self._w)]

    def set_masks(self, masks):
        """masks (n_masks, H, W) with values in {0, 1}: the query masks of the clip's first frame, at the frames' own size."""
        masks = torch.as_tensor(masks)
        if masks.dim() != 3:
            raise ValueError("SuperGluePointTracker.set_masks: masks must be (n_masks, height, width)")
        self.masks = masks

    @torch.no_grad()
    @_lib.on_device(lambda self, frames, *a, **k: frames.device)
    def detect(self, frames: torch.Tensor, return_dense: bool = False):
        """frames (T,3,H,W) uint8 on the device -> dict(kpts (T,cap,2), scores (T,cap), desc (T,cap,256), counts list[int],
        [dense (T,Hs,Ws)]); one host synchronisation.  More keypoints than the capacity raise (nothing is truncated)."""
        assert frames.dtype == torch.uint8 and frames.dim() == 4, "frames must be uint8 (T,3,H,W)"
        T, _, H, W = frames.shape
        if H < 8 or W < 8:
            raise ValueError("SuperGluePointTracker: frames must be at least 8 x 8 pixels")
        dev = frames.device
        self._ensure(dev)
        r = int(self.sp_cfg["nms_radius"])
        cap = int(self.keypoint_capacity) if self.keypoint_capacity else superglue_keypoint_capacity(H, W, r)
        kpts = torch.empty((T, cap, 2), dtype=torch.float32, device=dev)
        scores = torch.empty((T, cap), dtype=torch.float32, device=dev)
        desc = torch.empty((T, cap, 256), dtype=torch.float32, device=dev)
        counts = torch.empty((T,), dtype=torch.int32, device=dev)
        dense = torch.empty((T, H // 8 * 8, W // 8 * 8), dtype=torch.float32, device=dev) if return_dense else None
        host = (C.c_int * T)()
        nbytes = C.c_size_t()
        _lib.check(self._lib.sampt_sg_workspace_bytes(self._h, T, H, W, 0, 0, C.byref(nbytes), None), "sampt_sg_workspace_bytes")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        _lib.check(self._lib.sampt_sg_detect(self._h, _lib.ptr(frames.contiguous()), T, H, W, r, float(self.sp_cfg["keypoint_threshold"]),
                                             int(self.sp_cfg["remove_borders"]), cap, _lib.ptr(kpts), _lib.ptr(scores), _lib.ptr(desc),
                                             _lib.ptr(counts), host, _lib.ptr(dense), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "sampt_sg_detect")
        self.stats["frames"] += T
        self.stats["host_syncs"] += 1
        out = {"kpts": kpts, "scores": scores, "desc": desc, "counts": [int(c) for c in host], "counts_dev": counts, "cap": cap,
               "hw": (H, W)}
        self.stats["keypoints"] = out["counts"]
        if return_dense:
            out["dense"] = dense
        return out

    def match_workspace(self, det):
        n0, n1 = det["counts"][0], max(det["counts"][1:], default=0)
        # (the query's first size, detect's, is not asked for; the helper appends the out-parameter of the second, match's)
        return _lib.workspace("sampt_sg_workspace_bytes", det["kpts"].device, self._h, 1, det["hw"][0], det["hw"][1], n0, n1, None,
                              min_bytes=256)

    @torch.no_grad()
    @_lib.on_device(lambda self, det, *a, **k: det["kpts"].device)
    def match(self, det, i: int, ws: Optional[torch.Tensor] = None, debug: bool = False):
        """SuperGlue between frame 0 and frame i of ``detect``'s result -> (matches0 int32 (n0,), matching_scores0 (n0,)) on the
        device, no host synchronisation.  ``debug`` adds the GNN output descriptors (n0 + n1, 256), the score matrix (n0, n1)
        and Sinkhorn's u | v."""
        dev = det["kpts"].device
        n0, n1 = det["counts"][0], det["counts"][i]
        H, W = det["hw"]
        ws = ws if ws is not None else self.match_workspace(det)
        m0 = torch.empty((n0,), dtype=torch.int32, device=dev)
        s0 = torch.empty((n0,), dtype=torch.float32, device=dev)
        both = n0 > 0 and n1 > 0
        gnn = torch.empty((n0 + n1, 256), dtype=torch.float32, device=dev) if debug and both else None
        sm = torch.empty((n0, n1), dtype=torch.float32, device=dev) if debug and both else None
        uv = torch.empty((n0 + n1 + 2,), dtype=torch.float32, device=dev) if debug and both else None
        _lib.check(self._lib.sampt_sg_match(self._h, _lib.ptr(det["kpts"][0]), _lib.ptr(det["scores"][0]), _lib.ptr(det["desc"][0]), n0,
                                            _lib.ptr(det["kpts"][i]), _lib.ptr(det["scores"][i]), _lib.ptr(det["desc"][i]), n1, H, W,
                                            int(self.sg_cfg["sinkhorn_iterations"]), float(self.sg_cfg["match_threshold"]),
                                            _lib.ptr(m0) if n0 else None, _lib.ptr(s0) if n0 else None, _lib.ptr(gnn), _lib.ptr(sm),
                                            _lib.ptr(uv), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sampt_sg_match")
        self.stats["pairs"] += 1
        return (m0, s0, gnn, sm, uv) if debug else (m0, s0)

    @torch.no_grad()
    @_lib.on_device(lambda self, rgbs, query_points: rgbs.device)
    def forward(self, rgbs, query_points):
        assert self.masks is not None, "Masks must be set before calling forward() for SuperGluePointTracker"
        assert rgbs.dtype == torch.uint8, "rgbs must be uint8 (PointTracker.forward contract)"
        import numpy as np
        B, T, _, H, W = rgbs.shape
        if B != 1:
            raise NotImplementedError("Batch size > 1 is not supported for SuperGluePointTracker yet")
        dev = rgbs.device
        _lib.require_hip(dev, "SuperGluePointTracker")
        n_pos, n_neg = self.positive_points_per_mask, self.negative_points_per_mask
        P = n_pos + n_neg
        nm = self.masks.shape[0]
        assert P * nm == query_points.shape[1]
        if tuple(self.masks.shape[1:]) != (H, W):
            raise ValueError(f"SuperGluePointTracker: masks of {tuple(self.masks.shape[1:])} for frames of {(H, W)}")
        masks = self.masks.to(device=dev, dtype=torch.float32).contiguous()
        det = self.detect(rgbs[0])
        n0 = det["counts"][0]
        lcap = max(1, n0)
        traj = torch.empty((T, nm * P, 2), dtype=torch.float32, device=dev)
        vis = torch.empty((T, nm * P), dtype=torch.float32, device=dev)
        qxy = query_points[0, :, 1:].to(device=dev, dtype=torch.float32).contiguous()
        lists = counts = draw = None
        if T > 1:
            lists = torch.empty((T - 1, nm, 2, lcap), dtype=torch.int32, device=dev)
            counts = torch.zeros((T - 1, nm, 2), dtype=torch.int32, device=dev)
            ws = self.match_workspace(det)
            for i in range(1, T):
                m0, _ = self.match(det, i, ws)
                if n0 > 0 and det["counts"][i] > 0:
                    _lib.check(self._lib.sampt_sg_select(_lib.ptr(m0), n0, _lib.ptr(det["kpts"][i]), _lib.ptr(masks), nm, H, W, lcap,
                                                         _lib.ptr(lists[i - 1]), _lib.ptr(counts[i - 1]), _lib.stream_ptr()),
                               "sampt_sg_select")
            host = counts.cpu().numpy()                         # the clip's second (and last) host synchronisation
            self.stats["host_syncs"] += 1
            pick = np.full((T - 1, nm, P), -1, dtype=np.int32)
            for i in range(T - 1):                              # tracker.py:137-162: per frame, per mask, positives then negatives
                for mi in range(nm):
                    for which, want, off in ((0, n_pos, 0), (1, n_neg, n_pos)):
                        have = int(host[i, mi, which])
                        idx = np.random.choice(a=have, size=min(have, want))
                        pick[i, mi, off:off + len(idx)] = idx
            draw = torch.from_numpy(pick).to(dev)
        _lib.check(self._lib.sampt_sg_gather(_lib.ptr(qxy), _lib.ptr(det["kpts"]), det["cap"], _lib.ptr(lists), lcap, _lib.ptr(counts),
                                             _lib.ptr(draw), T, nm, n_pos, n_neg, _lib.ptr(traj), _lib.ptr(vis), _lib.stream_ptr()),
                   "sampt_sg_gather")
        self.masks = None                                       # tracker.py:188-189: used up
        return traj[None], vis[None]
