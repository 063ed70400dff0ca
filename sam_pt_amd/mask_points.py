"""Rank -> pixel on bit-planes: "the r-th set pixel of this mask, in ``nonzero()`` order" (csrc/mask_points.hip).

Query-point selection from a mask (``sam_pt_amd/query_points.py``) draws pixel RANKS on the host — it needs the mask's area for
that, one int — and turns ranks into pixels here, so masks that live on the device (the logits of a re-initialisation segment,
uploaded query masks) never come to the host.  Planes are in the ``sampt_bits_pack`` format (``vis_metrics.pack_bits``): uint64
(n, ceil(h / 64), w), bit j of word (band b, column x) = pixel (64 b + j, x), the bits of rows >= h are 0.

* ``row_prefix`` / ``select_ranks`` — the NumPy restatement of the two entry points: the specification of the kernels.
* ``row_prefix_device`` / ``select_device`` / ``unpack_plane_device`` — the HIP calls.
* ``HostMasks`` / ``DevicePlanes`` — the two sources of pixels that ``query_points.select_query_points`` reads through.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch


# --------------------------------------------------------------------------------------------------------------------
# host restatement
# --------------------------------------------------------------------------------------------------------------------
def _row_counts(bits, h: int) -> np.ndarray:
    """Bit-planes (n, nb, w) -> int64 (n, h): set pixels per row."""
    b = np.ascontiguousarray(np.asarray(bits).astype("<u8"))
    n, nb, w = b.shape
    px = np.unpackbits(b.view(np.uint8).reshape(n, nb, w, 8), axis=-1, bitorder="little")           # (n, nb, w, 64)
    return px.sum(axis=2, dtype=np.int64).reshape(n, nb * 64)[:, :h]


def row_prefix(bits, h: int) -> np.ndarray:
    """``sampt_bits_row_prefix``: int32 (n, h + 1), prefix[i][y] = set pixels of plane i in rows < y (prefix[i][h] = the area)."""
    rc = _row_counts(bits, h)
    out = np.zeros((rc.shape[0], h + 1), dtype=np.int32)
    out[:, 1:] = np.cumsum(rc, axis=1)
    return out


def select_ranks(bits, prefix, h: int, queries) -> np.ndarray:
    """``sampt_bits_select``: queries int (nq, 3) = (plane, invert, rank) -> float32 (nq, 2) = (y, x) of the rank-th set pixel — with
    invert != 0 the rank-th clear pixel inside the image — in row-major order; (-1, -1) for a plane or rank out of range."""
    b = np.ascontiguousarray(np.asarray(bits).astype("<u8"))
    n, _, w = b.shape
    prefix = np.asarray(prefix, dtype=np.int64)
    out = np.full((len(queries), 2), -1.0, dtype=np.float32)
    for qi, (plane, invert, rank) in enumerate(np.asarray(queries, dtype=np.int64).reshape(-1, 3)):
        if not 0 <= plane < n:
            continue
        pf = prefix[plane]
        cnt = np.arange(h + 1, dtype=np.int64) * w - pf if invert else pf
        if not 0 <= rank < cnt[h]:
            continue
        y = int(np.searchsorted(cnt, rank, side="right")) - 1            # the last row with cnt[y] <= rank
        row = ((b[plane, y >> 6] >> np.uint64(y & 63)) & np.uint64(1)).astype(np.int64) ^ (1 if invert else 0)
        x = int(np.nonzero(row)[0][rank - cnt[y]])
        out[qi] = (y, x)
    return out


# --------------------------------------------------------------------------------------------------------------------
# device path (csrc/mask_points.hip)
# --------------------------------------------------------------------------------------------------------------------
def _check_bits(who: str, bits: torch.Tensor, h: int):
    from . import _lib
    _lib.require_hip(getattr(bits, "device", None), who)
    if bits.dtype != torch.int64 or bits.dim() != 3 or bits.shape[1] != (h + 63) // 64 or bits.shape[2] == 0 or h <= 0:
        raise _lib.SamptError(f"{who}: bit-planes int64 (n, ceil(h / 64), w) are required; got {tuple(bits.shape)} {bits.dtype} for h = {h}")
    if h * int(bits.shape[2]) >= 1 << 31:
        raise _lib.SamptError(f"{who}: h * w must be below 2^31")
    return bits if bits.is_contiguous() else bits.contiguous()


def row_prefix_device(bits: torch.Tensor, h: int) -> torch.Tensor:
    """``row_prefix`` on the HIP device: bit-planes int64 (n, nb, w) (``vis_metrics.bits_pack_device``) -> int32 (n, h + 1) there."""
    from . import _lib
    bits = _check_bits("row_prefix_device", bits, h)
    n, _, w = bits.shape
    lib = _lib.load()
    with _lib.device_guard(bits.device):
        prefix = torch.empty((n, h + 1), dtype=torch.int32, device=bits.device)
        if n:
            _lib.check(lib.sampt_bits_row_prefix(_lib.ptr(bits), n, h, w, _lib.ptr(prefix), _lib.stream_ptr()), "sampt_bits_row_prefix")
    return prefix


def select_device(bits: torch.Tensor, prefix: torch.Tensor, h: int, queries) -> torch.Tensor:
    """``select_ranks`` on the HIP device in ONE launch: queries (nq, 3) = (plane, invert, rank), an int array on the host (uploaded in
    one copy) or an int32 tensor on the device -> float32 (nq, 2) = (y, x) on the device."""
    from . import _lib
    bits = _check_bits("select_device", bits, h)
    n, _, w = bits.shape
    dev = bits.device
    if prefix.device != dev or prefix.dtype != torch.int32 or tuple(prefix.shape) != (n, h + 1):
        raise _lib.SamptError(f"select_device: prefix must be int32 ({n}, {h + 1}) on {dev}; got {tuple(prefix.shape)} {prefix.dtype}")
    if isinstance(queries, torch.Tensor):
        q = queries.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    else:
        q = torch.from_numpy(np.ascontiguousarray(np.asarray(queries, dtype=np.int32).reshape(-1, 3))).to(dev)
    nq = int(q.shape[0])
    lib = _lib.load()
    with _lib.device_guard(dev):
        out = torch.empty((nq, 2), dtype=torch.float32, device=dev)
        if n == 0:
            out.fill_(-1.0)
        _lib.check(lib.sampt_bits_select(_lib.ptr(bits), _lib.ptr(prefix.contiguous()), n, h, w, _lib.ptr(q), nq, _lib.ptr(out),
                                         _lib.stream_ptr()), "sampt_bits_select")
    return out


def unpack_plane_device(bits: torch.Tensor, plane: int, h: int) -> torch.Tensor:
    """Plane ``plane`` of bit-planes int64 (n, nb, w) as a uint8 (h, w) mask of 0 / 1 on the device (``sampt_bits_unpack``)."""
    from . import _lib
    bits = _check_bits("unpack_plane_device", bits, h)
    one = bits[plane]
    w = int(one.shape[1])
    lib = _lib.load()
    with _lib.device_guard(bits.device):
        out = torch.empty((h, w), dtype=torch.uint8, device=bits.device)
        _lib.check(lib.sampt_bits_unpack(_lib.ptr(one), 1, h, w, _lib.ptr(out), _lib.stream_ptr()), "sampt_bits_unpack")
    return out


# --------------------------------------------------------------------------------------------------------------------
# the two sources of pixels of query_points.select_query_points
# --------------------------------------------------------------------------------------------------------------------
class HostMasks:
    """Masks (M, H, W) on the host: ``nonzero()`` of the mask or of its complement, as the selectors of query_points.py read them."""

    def __init__(self, masks: torch.Tensor):
        self.masks = masks
        self.n_masks, self.h, self.w = (int(s) for s in masks.shape)
        self._area = [int((m != 0).sum()) for m in masks]
        self._px = {}

    def area(self, i: int, invert: bool) -> int:
        return self.h * self.w - self._area[i] if invert else self._area[i]

    def mask(self, i: int, invert: bool) -> torch.Tensor:
        return 1 - self.masks[i] if invert else self.masks[i]

    def select(self, queries: np.ndarray) -> torch.Tensor:
        out = torch.empty((len(queries), 2), dtype=torch.float32)
        for qi, (i, inv, rank) in enumerate(queries.tolist()):
            if (i, inv) not in self._px:
                self._px[(i, inv)] = self.mask(i, bool(inv)).nonzero().float()
            out[qi] = self._px[(i, inv)][rank]
        return out

    def kmedoids(self, px: torch.Tensor, n_clusters: int) -> np.ndarray:
        from .query_points import kmedoids_alternate
        return kmedoids_alternate(px.numpy(), n_clusters)

    def corners(self, image: torch.Tensor, i: int, invert: bool, n_points: int) -> torch.Tensor:
        from .query_points import shi_tomasi_host
        return shi_tomasi_host(image, self.mask(i, invert), n_points)

    def take(self, yx: torch.Tensor, rows: Sequence[int]) -> torch.Tensor:
        return yx[torch.as_tensor(rows, dtype=torch.long)]


class DevicePlanes:
    """Masks as bit-planes on the HIP device, with their areas on the host (all the rank step needs) and their row prefixes beside
    them: every rank of a call becomes a pixel in one ``sampt_bits_select`` launch, clustering and corner selection read the device
    copies, and ``take`` downloads only the chosen points."""

    def __init__(self, bits: torch.Tensor, areas: Sequence[int], h: int, prefix: Optional[torch.Tensor] = None):
        self.bits, self.h = bits, int(h)
        self.n_masks, self.w = int(bits.shape[0]), int(bits.shape[2])
        self._area = [int(a) for a in areas]
        assert len(self._area) == self.n_masks
        self.prefix = prefix if prefix is not None else row_prefix_device(bits, self.h)
        self.device = bits.device
        self.select_launches = 0

    def area(self, i: int, invert: bool) -> int:
        return self.h * self.w - self._area[i] if invert else self._area[i]

    def mask(self, i: int, invert: bool) -> torch.Tensor:
        m = unpack_plane_device(self.bits, i, self.h)
        return 1 - m if invert else m

    def select(self, queries: np.ndarray) -> torch.Tensor:
        self.select_launches += 1
        return select_device(self.bits, self.prefix, self.h, queries)

    def kmedoids(self, px: torch.Tensor, n_clusters: int) -> np.ndarray:
        from .query_points import kmedoids_alternate, kmedoids_alternate_device
        if len(px) <= 2048 and n_clusters <= 64:               # (the kernel's limits, as in extract_kmedoid_points)
            return kmedoids_alternate_device(px, n_clusters, self.device)
        return kmedoids_alternate(px.cpu().numpy(), n_clusters)

    def corners(self, image: torch.Tensor, i: int, invert: bool, n_points: int) -> torch.Tensor:
        from .query_points import shi_tomasi_device, shi_tomasi_host
        m = self.mask(i, invert)
        if 1 <= n_points <= 64 and min(self.h, self.w) >= 3:   # (the kernel's limits, as in extract_corner_points)
            return shi_tomasi_device(image, m, n_points, self.device)[0]
        return shi_tomasi_host(image.cpu(), m.cpu().float(), n_points)

    def take(self, yx: torch.Tensor, rows: Sequence[int]) -> torch.Tensor:
        idx = torch.as_tensor(rows, dtype=torch.long).to(self.device)
        return yx[idx].cpu()


def planes_of_masks(masks: torch.Tensor) -> DevicePlanes:
    """Masks (M, H, W) on the HIP device -> ``DevicePlanes`` of ``mask != 0`` (one pack, one download of M areas)."""
    from .vis_metrics import bits_pack_device
    bits, area = bits_pack_device((masks != 0).to(torch.uint8))
    return DevicePlanes(bits, area.cpu().tolist(), int(masks.shape[-2]))


def device_reinit_areas(logits: torch.Tensor):
    """f32 logits (n, F, H, W) on the HIP device -> (bit-planes of ``logits > 0`` (NaN clear), plane j * F + f; areas int64 (n, F) on
    the host): one pack, one download of n * F ints."""
    from .vis_metrics import bits_pack_device
    n, f, h, w = logits.shape
    bits, area = bits_pack_device(logits.reshape(n * f, h, w), threshold=0.0)
    return bits, area.cpu().view(n, f).long()


__all__: List[str] = ["row_prefix", "select_ranks", "row_prefix_device", "select_device", "unpack_plane_device", "HostMasks",
                      "DevicePlanes", "planes_of_masks", "device_reinit_areas"]
