"""Prompt assembly of ``SamPt`` for point tracks that stay on the HIP device (csrc/prompt_assembly.hip).

``assemble_prompts_host`` is the specification: a vectorised NumPy restatement of ``SamPt._prepare_points`` followed by
``ResizeLongestSide.apply_coords`` (reference sam_pt/modeling/sam_pt.py:726-758) for every (frame, object) item of a clip at once,
without ``max_other_objects_positive_points`` (its ``np.random.choice`` is host RNG and stays on the host path).  It is held to that
loop with ``==`` on the CPU (tests/test_prompt_assembly_cpu.py), and the kernels are held to it with ``==`` on every word
(tests/test_gpu_prompt_assembly.py).

Per item ``t * M + m``:

  * its own visible points (visibility code ``== 1``) in index order: label 1 for index < ``pp``, label 0 for index >= ``pp`` when
    ``negatives`` (``negative_points_per_mask > 0``), label 1 throughout otherwise;
  * then, when ``M > 1`` and ``add_others``, the visible points among the first ``pp`` of every other object, object-major, label 0;
  * a coordinate is ``float32(float64(x) * sx)``: ``apply_coords`` multiplies in float64 and the prompt block is float32;
  * ``k`` is the prompt's length, ``npos`` its number of label-1 entries; slots past ``k`` hold zeros.

The device side is two stream-ordered calls — ``count_prompts`` (every item's ``k`` / ``npos``: all the host needs for its decisions)
and ``fill_prompts`` (a chunk's prompts, straight into the decoder's input buffers) — plus ``mark_outside_frame``, the border rule of
``SamPt._track_points`` for tracks that are not going through the patch-similarity filter's launch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch


def assemble_prompts_host(traj, vis, pp: int, negatives: bool, add_others: bool, sx: float, sy: float,
                          ld: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """traj (T,M,P,2) float32, vis (T,M,P) visibility codes -> (xy (T*M,ld,2) float32, lab (T*M,ld) int32, k (T*M,) int32,
    npos (T*M,) int32).  ``ld``: point slots per item, default ``max(1, k.max())`` (what ``SamPt._enqueue_sam_fused`` calls kmax)."""
    traj = np.asarray(traj, dtype=np.float32)
    v = np.asarray(vis) == 1
    T, M, P = v.shape
    assert traj.shape == (T, M, P, 2)
    pp = int(pp)
    ppe = min(max(pp, 0), P)
    others = bool(add_others) and M > 1
    own_k = v.sum(-1)                                              # (T,M)
    lead = v[:, :, :ppe].sum(-1)                                   # (T,M) visible among the points other objects receive
    k = own_k + ((lead.sum(1, keepdims=True) - lead) if others else 0)
    npos = lead if negatives else own_k
    if ld is None:
        ld = max(1, int(k.max()) if k.size else 1)
    assert k.size == 0 or int(k.max()) <= ld, "ld is smaller than the longest prompt"
    scaled = np.stack([traj[..., 0].astype(np.float64) * sx, traj[..., 1].astype(np.float64) * sy], axis=-1).astype(np.float32)
    xy = np.zeros((T * M, ld, 2), dtype=np.float32)
    lab = np.zeros((T * M, ld), dtype=np.int32)
    # own points: the slot is the number of visible points in front
    t_i, m_i, p_i = np.nonzero(v)
    slot = (np.cumsum(v, axis=-1) - 1)[t_i, m_i, p_i]
    xy[t_i * M + m_i, slot] = scaled[t_i, m_i, p_i]
    lab[t_i * M + m_i, slot] = 1 if not negatives else (p_i < pp)
    if others and ppe > 0:
        # the frame's candidate list is the same for its M items, each minus its own segment: a candidate's slot in item m is its rank
        # in the frame's list, less the length of m's own segment when the candidate lies behind it
        vp = v[:, :, :ppe].reshape(T, M * ppe)
        t_j, j = np.nonzero(vp)
        rank = (np.cumsum(vp, axis=1) - 1)[t_j, j]
        obj = j // ppe
        m_t = np.arange(M)[None, :]                                # every target item of the candidate's frame
        keep = obj[:, None] != m_t
        dst = own_k[t_j] + rank[:, None] - np.where(obj[:, None] > m_t, lead[t_j], 0)
        src = scaled[:, :, :ppe].reshape(T, M * ppe, 2)[t_j, j]
        item = t_j[:, None] * M + m_t
        xy[item[keep], dst[keep]] = np.broadcast_to(src[:, None, :], keep.shape + (2,))[keep]
    return xy, lab, k.reshape(-1).astype(np.int32), npos.reshape(-1).astype(np.int32)


def _check_tracks(who: str, traj: torch.Tensor, vis: torch.Tensor):
    from . import _lib
    for name, x in (("trajectories", traj), ("visibilities", vis)):
        if not isinstance(x, torch.Tensor):
            raise _lib.SamptError(f"{who}: {name} must be a tensor; got {type(x).__name__}")
    if vis.dim() != 3 or min(vis.shape) == 0:
        raise _lib.SamptError(f"{who}: visibilities must be (T, M, P) with T, M, P > 0; got {tuple(vis.shape)}")
    if tuple(traj.shape) != tuple(vis.shape) + (2,):
        raise _lib.SamptError(f"{who}: trajectories must be {tuple(vis.shape) + (2,)}; got {tuple(traj.shape)}")
    _lib.require_hip(vis.device, who)
    if traj.device != vis.device:
        raise _lib.SamptError(f"{who}: mixed devices: trajectories on {traj.device}, visibilities on {vis.device}")
    return traj.float().contiguous(), vis.float().contiguous()


def count_prompts(vis: torch.Tensor, pp: int, negatives: bool, add_others: bool) -> torch.Tensor:
    """vis (T,M,P) codes on a HIP device -> int32 (2, T*M) on that device: row 0 every item's ``k``, row 1 its ``npos``.  One launch on
    the current stream, no synchronisation."""
    from . import _lib
    who = "count_prompts"
    if not isinstance(vis, torch.Tensor) or vis.dim() != 3 or min(vis.shape) == 0:
        raise _lib.SamptError(f"{who}: visibilities must be a (T, M, P) tensor with T, M, P > 0")
    _lib.require_hip(vis.device, who)
    T, M, P = vis.shape
    with _lib.device_guard(vis.device):
        v = vis.float().contiguous()
        out = torch.empty((2, T * M), dtype=torch.int32, device=vis.device)
        _lib.check(_lib.load().sampt_prompt_count(_lib.ptr(v), T, M, P, int(pp), int(bool(negatives)), int(bool(add_others)),
                                                  _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr()), "sampt_prompt_count")
    return out


def fill_prompts(traj: torch.Tensor, vis: torch.Tensor, pp: int, negatives: bool, add_others: bool, sx: float, sy: float,
                 items: torch.Tensor, pts: torch.Tensor, labels: torch.Tensor, k_item: torch.Tensor, npos_item: torch.Tensor):
    """The prompts of the items named by ``items`` (int32 (F,) on the device, item = t * M + m, any subset in any order) written into
    ``pts`` (F,ld,2) float32, ``labels`` (F,ld) int32 (zeros past an item's k), ``k_item`` / ``npos_item`` (F,) int32 — contiguous
    views of a ``SamPredictor.decode_staging`` block, or plain tensors.  ``ld`` must hold the chunk's longest prompt.  One launch on the
    current stream, no synchronisation; the inputs are read as they stand when the launch runs."""
    from . import _lib
    who = "fill_prompts"
    tr, vi = _check_tracks(who, traj, vis)
    T, M, P = vi.shape
    F = int(items.shape[0])
    if F == 0:
        return
    ld = int(pts.shape[1])
    if tuple(pts.shape) != (F, ld, 2) or tuple(labels.shape) != (F, ld) or tuple(k_item.shape) != (F,) or tuple(npos_item.shape) != (F,):
        raise _lib.SamptError(f"{who}: outputs must be pts (F, ld, 2), labels (F, ld), k_item (F,), npos_item (F,) with F = {F}; got "
                              f"{tuple(pts.shape)}, {tuple(labels.shape)}, {tuple(k_item.shape)}, {tuple(npos_item.shape)}")
    if pts.dtype != torch.float32 or any(x.dtype != torch.int32 for x in (items, labels, k_item, npos_item)):
        raise _lib.SamptError(f"{who}: pts must be float32; items, labels, k_item and npos_item int32")
    if any(x.device != vi.device for x in (items, pts, labels, k_item, npos_item)):
        raise _lib.SamptError(f"{who}: every tensor must live on {vi.device}")
    with _lib.device_guard(vi.device):
        _lib.check(_lib.load().sampt_prompt_fill(_lib.ptr(tr), _lib.ptr(vi), T, M, P, int(pp), int(bool(negatives)), int(bool(add_others)),
                                                 float(sx), float(sy), _lib.ptr(items), F, ld, _lib.ptr(pts), _lib.ptr(labels),
                                                 _lib.ptr(k_item), _lib.ptr(npos_item), _lib.stream_ptr()), "sampt_prompt_fill")


def mark_outside_frame(traj: torch.Tensor, vis: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """``SamPt._mark_outside_frame`` for tracks on a HIP device: traj (...,2), vis (...) -> new float32 codes, OUTSIDE_FRAME (-2) where
    one of the four border comparisons holds.  One launch on the current stream, no synchronisation."""
    from . import _lib
    who = "mark_outside_frame"
    if not isinstance(traj, torch.Tensor) or not isinstance(vis, torch.Tensor) or tuple(traj.shape) != tuple(vis.shape) + (2,):
        raise _lib.SamptError(f"{who}: trajectories must be visibilities' shape + (2,)")
    _lib.require_hip(vis.device, who)
    if traj.device != vis.device:
        raise _lib.SamptError(f"{who}: mixed devices: trajectories on {traj.device}, visibilities on {vis.device}")
    with _lib.device_guard(vis.device):
        tr, vi = traj.float().contiguous(), vis.float().contiguous()
        out = torch.empty_like(vi)
        if vi.numel():
            _lib.check(_lib.load().sampt_mark_outside_frame(_lib.ptr(tr), _lib.ptr(vi), vi.numel(), int(height), int(width), _lib.ptr(out),
                                                            _lib.stream_ptr()), "sampt_mark_outside_frame")
    return out
