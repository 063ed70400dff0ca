"""Patch-similarity filter of ``SamPt._track_points`` on the HIP device (csrc/patch_filter.hip, ``sampt_patch_filter``).

The definitions are those of the host restatement, ``sam_pt_amd/sam_pt.py``: ``rgb2lab`` and ``SamPt._patch_similarity_filter``
(reference sam_pt/modeling/sam_pt.py:597-682) followed by the four border comparisons of ``_track_points`` (:684-690).  The host
path copies the clip to the host, converts every pixel of every frame to CIELAB in float64 and samples a few hundred thousand
of them; the kernel converts only the four bilinear corners under each tap, from the bytes, in one launch per call.

What equals the host bit for bit, and what does not:

  * the sRGB companding: a 256-entry float64 table computed here by ``rgb2lab``'s own two torch lines and uploaded once per device;
  * a tap's source index, weights and weighted sum: torch's CPU ``grid_sample`` arithmetic, fused multiply-adds included;
  * the border rule: f32 IEEE divisions and comparisons, as the torch lines give on CPU tensors;
  * NOT pinned bit for bit: the float64 matrix product and cube root of a pixel (the host's run through BLAS and ``pow``; the
    results are rounded to f32, which hides a last-place float64 difference all but never) and the order of the f32 sum under the
    norm.  The similarities are held to ``bar_sim`` of tests/golden/patch_filter.npz — 8 x the host path's own f32-against-float64
    noise — and the codes to equality wherever the host's similarity is further than that from the threshold.

``rgb2lab`` itself restates ``skimage.color.rgb2lab``; skimage is absent where this project is built, so that one function is
parity unpinned, and so is everything here that follows it (table, matrix, white point, cube root).

Even ``patch_size``: the taps are ``-(ps // 2) .. ps // 2`` on both axes, ``ps + 1`` per side, while the divisor stays
``2 * ps ** 2`` — the reference's behaviour, kept.

Non-finite trajectory coordinates: the item is non-similar (similarity 0).  The same holds for every item of a point whose query is
non-finite or names a frame outside the clip.  The host path's result for such inputs is not defined and is not tested against.
"""
from __future__ import annotations

from typing import Any, Dict

import torch

MAX_PATCH_SIZE = 15        # SAMPT_PATCH_FILTER_MAX_PATCH_SIZE of include/sampt_hip.h: what the kernel sizes its LDS for

_TABLE_ON: Dict[Any, torch.Tensor] = {}


def companding_table() -> torch.Tensor:
    """float64 (256,): linear sRGB of byte / 255 — the first two lines of ``sam_pt.rgb2lab`` on every byte value (same torch
    operations on the same float64 inputs, hence the same bits)."""
    rgb = torch.arange(256, dtype=torch.uint8).double() / 255.0
    return torch.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)


def _table_on(dev) -> torch.Tensor:
    if dev not in _TABLE_ON:
        _TABLE_ON[dev] = companding_table().to(dev)
    return _TABLE_ON[dev]


def patch_similarity_filter(rgbs: torch.Tensor, query_points: torch.Tensor, trajectories: torch.Tensor, visibilities: torch.Tensor,
                            patch_size: int, threshold: float, *, border_rule: bool = False, return_similarities: bool = False):
    """rgbs (T,3,H,W) uint8 (another dtype goes through ``.byte()``), query_points (N,3) = (t, x, y), trajectories (T,N,2),
    visibilities (T,N), all on one HIP device -> the visibility codes (T,N) float32 of ``SamPt._patch_similarity_filter``; with
    ``border_rule`` also OUTSIDE_FRAME of ``_track_points``' four border comparisons; with ``return_similarities`` the pair
    (codes, similarities (T,N) float32 of every item, whatever its visibility).  One launch on the current stream, no
    synchronisation; ``N == 0`` launches nothing.  Items with a non-finite coordinate are non-similar (module docstring)."""
    from . import _lib
    who = "patch_similarity_filter"
    for name, x in (("rgbs", rgbs), ("query_points", query_points), ("trajectories", trajectories), ("visibilities", visibilities)):
        if not isinstance(x, torch.Tensor):
            raise _lib.SamptError(f"{who}: {name} must be a tensor; got {type(x).__name__}")
    if int(patch_size) != patch_size or not 1 <= int(patch_size) <= MAX_PATCH_SIZE:
        raise _lib.SamptError(f"{who}: patch_size must be an integer in 1 .. {MAX_PATCH_SIZE}; got {patch_size}")
    if rgbs.dim() != 4 or rgbs.shape[1] != 3 or min(rgbs.shape) == 0:
        raise _lib.SamptError(f"{who}: rgbs must be (T, 3, H, W) with T, H, W > 0; got {tuple(rgbs.shape)}")
    T, _, H, W = rgbs.shape
    if query_points.dim() != 2 or query_points.shape[1] != 3:
        raise _lib.SamptError(f"{who}: query_points must be (N, 3); got {tuple(query_points.shape)}")
    N = query_points.shape[0]
    if tuple(trajectories.shape) != (T, N, 2):
        raise _lib.SamptError(f"{who}: trajectories must be (T, N, 2) = ({T}, {N}, 2); got {tuple(trajectories.shape)}")
    if tuple(visibilities.shape) != (T, N):
        raise _lib.SamptError(f"{who}: visibilities must be (T, N) = ({T}, {N}); got {tuple(visibilities.shape)}")
    dev = rgbs.device
    _lib.require_hip(dev, who)
    for name, x in (("query_points", query_points), ("trajectories", trajectories), ("visibilities", visibilities)):
        if x.device != dev:
            raise _lib.SamptError(f"{who}: mixed devices: rgbs on {dev}, {name} on {x.device}")
    with _lib.device_guard(dev):
        rgb = (rgbs if rgbs.dtype == torch.uint8 else rgbs.byte()).contiguous()
        q, tr, vi = query_points.float().contiguous(), trajectories.float().contiguous(), visibilities.float().contiguous()
        out = torch.empty((T, N), dtype=torch.float32, device=dev)
        sim = torch.empty((T, N), dtype=torch.float32, device=dev) if return_similarities else None
        if N:
            _lib.check(_lib.load().sampt_patch_filter(_lib.ptr(rgb), T, H, W, _lib.ptr(q), _lib.ptr(tr), _lib.ptr(vi), N, int(patch_size),
                                                      float(threshold), _lib.ptr(_table_on(dev)), int(bool(border_rule)), _lib.ptr(out),
                                                      _lib.ptr(sim), _lib.stream_ptr()), "sampt_patch_filter")
    return (out, sim) if return_similarities else out
