"""DAVIS J&F: region similarity J and boundary F-measure per object and frame, the semi-supervised sequence protocol and its
statistics.  The definitions are restated from the published DAVIS 2017 evaluation (the reference calls the third-party
``davis2017`` package, vos_eval/davis2017eval.py); that package is absent here, so this restatement is **parity unpinned**
against it.

An item is a pair of binary images: ``seg`` (the prediction) and ``ann`` (the ground truth), both ANDed with ``~void`` first.
Everything reduces to six integer counts per item (``COUNT_NAMES``); J, precision, recall and F are float64 formulas of them.
The host functions (numpy) and the device functions (csrc/vos_metrics.hip) produce the same integers, hence the same floats.

    seg2bmap(m)   b = (m ^ e) | (m ^ s) | (m ^ se) with the east, south and south-east neighbours (0 outside the image);
                  the last row is m ^ e, the last column m ^ s, the bottom-right pixel 0
    radius        bound_th if bound_th >= 1, else ceil(bound_th * sqrt(h * h + w * w))
    disk(r)       offsets dy * dy + dx * dx <= r * r; dilation takes everything outside the image as 0

Around the counts: the DAVIS semi-supervised protocol (``evaluate_semisupervised``), the DAVIS unsupervised protocol on the counts of
every (proposal, object) pair (``jf_pairs_counts``, csrc/vos_pairs.hip; ``evaluate_unsupervised``, parity unpinned as well), and the
BDD100K protocol of the reference's vos_eval/bdd100keval.py (``evaluate_bdd100k_sequence``, ``BDD100KEval``), which is pinned on the
reference's own evaluator (tests/bdd100k_ref.py, tests/golden/bdd100k_ref.npz).
"""
import math
import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

COUNT_NAMES = ("inter", "union", "n_seg", "n_ann", "seg_match", "ann_match")
MAX_DEVICE_RADIUS = 64
_KIND_BYTES, _KIND_F32, _KIND_INDEX = 0, 1, 2
_WS_CAP = 256 << 20


# --------------------------------------------------------------------------------------------------------------------
# host restatement
# --------------------------------------------------------------------------------------------------------------------
def _as_bool(x, threshold: Optional[float] = None) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype.kind == "f":
        if threshold is None:
            raise ValueError("a float image needs a threshold")
        with np.errstate(invalid="ignore"):
            return x > threshold                                       # NaN and equality are clear
    return x != 0


def boundary_radius(h: int, w: int, bound_th: float = 0.008) -> int:
    """The disk radius of the boundary measure for an (h, w) image."""
    if bound_th >= 1:
        return int(bound_th)
    return int(math.ceil(float(bound_th) * math.sqrt(float(h) * h + float(w) * w)))


def seg2bmap(m) -> np.ndarray:
    """Boundary map of a binary image (H, W) or stack (..., H, W)."""
    m = _as_bool(m)
    e, s, se = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    e[..., :, :-1] = m[..., :, 1:]
    s[..., :-1, :] = m[..., 1:, :]
    se[..., :-1, :-1] = m[..., 1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[..., -1, :] = m[..., -1, :] ^ e[..., -1, :]
    b[..., :, -1] = m[..., :, -1] ^ s[..., :, -1]
    b[..., -1, -1] = False
    return b


def disk(r: int) -> np.ndarray:
    """The structuring element (2 r + 1, 2 r + 1): dy * dy + dx * dx <= r * r."""
    d = np.arange(-r, r + 1)
    return d[:, None] ** 2 + d[None, :] ** 2 <= r * r


def dilate_disk(b, r: int) -> np.ndarray:
    """Binary dilation of (..., H, W) with ``disk(r)`` as the union of the disk's spans, the way the kernel forms it: the
    vertical dilations V_k of the map grow by one row up and down per step, and the span of the column at distance dx has the
    half-height isqrt(r * r - dx * dx), so out(x) |= V_k(x - dx) | V_k(x + dx) for every dx of that half-height."""
    b = _as_bool(b)
    h, w = b.shape[-2:]
    out = np.zeros_like(b)
    v = b.copy()
    for k in range(0, r + 1):
        if 0 < k < h:
            v[..., k:, :] |= b[..., :h - k, :]
            v[..., :h - k, :] |= b[..., k:, :]
        lo = 0 if k == r else math.isqrt(r * r - (k + 1) * (k + 1)) + 1      # isqrt(r * r - dx * dx) == k  <=>  lo <= dx <= hi
        hi = math.isqrt(r * r - k * k)
        for dx in range(lo, min(hi, w - 1) + 1):
            out[..., :, dx:] |= v[..., :, :w - dx]
            out[..., :, :w - dx] |= v[..., :, dx:]
    return out


def jf_counts(seg, ann, void=None, radius: Optional[int] = None, bound_th: float = 0.008, seg_threshold: Optional[float] = None,
              ann_threshold: Optional[float] = None) -> np.ndarray:
    """The six counts (``COUNT_NAMES``) of every item of two stacks (..., H, W) on the host: int64 (n, 6), n = the product of the
    leading dimensions.  ``radius`` overrides the one that ``bound_th`` gives."""
    seg, ann = _as_bool(seg, seg_threshold), _as_bool(ann, ann_threshold)
    if seg.shape != ann.shape or seg.ndim < 2:
        raise ValueError(f"seg {seg.shape} and ann {ann.shape} must be (..., H, W) of one shape")
    h, w = seg.shape[-2:]
    if void is not None:
        keep = ~np.broadcast_to(_as_bool(void), seg.shape)
        seg, ann = seg & keep, ann & keep
    seg, ann = seg.reshape(-1, h, w), ann.reshape(-1, h, w)
    r = boundary_radius(h, w, bound_th) if radius is None else int(radius)
    bs, ba = seg2bmap(seg), seg2bmap(ann)
    out = np.empty((seg.shape[0], 6), dtype=np.int64)
    out[:, 0] = (seg & ann).sum(axis=(1, 2))
    out[:, 1] = (seg | ann).sum(axis=(1, 2))
    out[:, 2] = bs.sum(axis=(1, 2))
    out[:, 3] = ba.sum(axis=(1, 2))
    out[:, 4] = (bs & dilate_disk(ba, r)).sum(axis=(1, 2))
    out[:, 5] = (ba & dilate_disk(bs, r)).sum(axis=(1, 2))
    return out


def jaccard_from_counts(counts) -> np.ndarray:
    """J = inter / union, 1 for an empty union; counts (..., 6) -> float64 (...)."""
    c = np.asarray(counts).astype(np.float64)
    inter, union = c[..., 0], c[..., 1]
    return np.where(union == 0, 1.0, inter / np.where(union == 0, 1.0, union))


def f_measure(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(F, precision, recall) from counts (..., 6), float64.  An empty predicted boundary against a non-empty one is P = 1,
    R = 0; the reverse P = 0, R = 1; both empty P = R = 1.  F = 2 P R / (P + R), 0 when P + R = 0."""
    c = np.asarray(counts).astype(np.float64)
    n_seg, n_ann, sm, am = c[..., 2], c[..., 3], c[..., 4], c[..., 5]
    p = np.where(n_seg == 0, 1.0, sm / np.where(n_seg == 0, 1.0, n_seg))
    r = np.where(n_ann == 0, 1.0, am / np.where(n_ann == 0, 1.0, n_ann))
    p = np.where((n_seg > 0) & (n_ann == 0), 0.0, p)
    r = np.where((n_seg == 0) & (n_ann > 0), 0.0, r)
    f = np.where(p + r == 0, 0.0, 2 * p * r / np.where(p + r == 0, 1.0, p + r))
    return f, p, r


def _lead_shape(x) -> Tuple[int, ...]:
    return tuple(x.shape[:-2])


def db_eval_iou(annotation, segmentation, void_pixels=None):
    """Region similarity J of (H, W) images (a float) or of (..., H, W) stacks (float64 (...))."""
    c = jf_counts(segmentation, annotation, void_pixels, radius=0)
    j = jaccard_from_counts(c).reshape(_lead_shape(np.asarray(annotation)))
    return float(j) if j.ndim == 0 else j


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th: float = 0.008):
    """Boundary F-measure of (H, W) images (a float) or of (..., H, W) stacks (float64 (...))."""
    c = jf_counts(segmentation, annotation, void_pixels, bound_th=bound_th)
    f = f_measure(c)[0].reshape(_lead_shape(np.asarray(annotation)))
    return float(f) if f.ndim == 0 else f


def _nanmean(v) -> float:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return float(np.nanmean(v))


def db_statistics(per_frame_values) -> Tuple[float, float, float]:
    """(mean, recall, decay) of one object's per-frame values: nanmean(v), nanmean(v > 0.5), and the nanmean of the first
    minus that of the last of four bins v[ids[i] : ids[i + 1] + 1], ids = round(linspace(1, len(v), 5) + 1e-10) - 1."""
    v = np.asarray(per_frame_values, dtype=np.float64)
    mean = _nanmean(v)
    with np.errstate(invalid="ignore"):
        recall = _nanmean(v > 0.5)
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    decay = _nanmean(bins[0]) - _nanmean(bins[3])
    return mean, recall, decay


# --------------------------------------------------------------------------------------------------------------------
# device path (csrc/vos_metrics.hip)
# --------------------------------------------------------------------------------------------------------------------
class _Source:
    """One stack of planes on the device, with what the kernel needs to read item i from it."""

    def __init__(self, who: str, x: torch.Tensor, threshold, values, planes, dev):
        from . import _lib
        if not isinstance(x, torch.Tensor) or x.device != dev:
            raise _lib.SamptError(f"{who}: every input must be a tensor on {dev}")
        if x.dim() < 2:
            raise _lib.SamptError(f"{who}: a (..., H, W) tensor is required; got {tuple(x.shape)}")
        self.h, self.w = int(x.shape[-2]), int(x.shape[-1])
        if self.h == 0 or self.w == 0:
            raise _lib.SamptError(f"{who}: empty images {tuple(x.shape)}")
        self.n_planes = int(np.prod(x.shape[:-2], dtype=np.int64))
        self.thr = 0.0
        if values is not None:
            if x.dtype != torch.uint8:
                raise _lib.SamptError(f"{who}: an index map must be uint8; got {x.dtype}")
            if threshold is not None:
                raise _lib.SamptError(f"{who}: threshold applies to float input only")
            self.kind = _KIND_INDEX
        elif x.dtype.is_floating_point:
            if x.dtype != torch.float32:
                raise _lib.SamptError(f"{who}: float input must be float32; got {x.dtype}")
            if threshold is None:
                raise _lib.SamptError(f"{who}: a float tensor needs a threshold")
            self.kind, self.thr = _KIND_F32, float(threshold)
        elif x.dtype in (torch.bool, torch.uint8):
            if threshold is not None:
                raise _lib.SamptError(f"{who}: threshold applies to float input only")
            self.kind = _KIND_BYTES
        else:
            raise _lib.SamptError(f"{who}: bool, uint8 or float32 input is required; got {x.dtype}")
        x = x.reshape(self.n_planes, self.h, self.w)                   # (a view when x is contiguous)
        if not x.is_contiguous():
            x = x.contiguous()
        self.x = x.view(torch.uint8) if x.dtype == torch.bool else x
        self.itemsize = self.x.element_size()
        self.values = self._ints(who, "values", values, 0, 255)
        self.planes = self._ints(who, "planes", planes, 0, self.n_planes - 1)
        if self.values is not None and self.planes is not None and len(self.values) != len(self.planes):
            raise _lib.SamptError(f"{who}: {len(self.values)} values for {len(self.planes)} planes")
        self.n = len(self.planes) if self.planes is not None else (len(self.values) if self.values is not None else self.n_planes)
        if self.planes is None and self.n != self.n_planes:
            raise _lib.SamptError(f"{who}: {self.n} values for {self.n_planes} planes and no plane numbers")
        self.values_dev = None if self.values is None else torch.from_numpy(self.values).to(dev)
        self.planes_dev = None if self.planes is None else torch.from_numpy(self.planes).to(dev)

    @staticmethod
    def _ints(who, what, v, lo, hi):
        """Validated on the host, before anything is uploaded: the device does not check them."""
        from . import _lib
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if v.ndim != 1 or v.dtype.kind not in "iu":
            raise _lib.SamptError(f"{who}: {what} must be a 1-D integer sequence")
        if v.size and (int(v.min()) < lo or int(v.max()) > hi):
            raise _lib.SamptError(f"{who}: {what} outside {lo} .. {hi}")
        return np.ascontiguousarray(v, dtype=np.int32)

    def args(self, c0: int):
        """(base, kind, thr, values, planes) pointers for the items from c0 on."""
        from . import _lib
        base = self.x.data_ptr() + (0 if self.planes is not None else c0 * self.h * self.w * self.itemsize)
        values = None if self.values_dev is None else _lib.c_void_p(self.values_dev.data_ptr() + 4 * c0)
        planes = None if self.planes_dev is None else _lib.c_void_p(self.planes_dev.data_ptr() + 4 * c0)
        return _lib.c_void_p(base), self.kind, self.thr, values, planes


def jf_counts_device(seg: torch.Tensor, ann: torch.Tensor, void: Optional[torch.Tensor] = None, radius: Optional[int] = None,
                     seg_threshold: Optional[float] = None, seg_values: Optional[Sequence[int]] = None,
                     seg_planes: Optional[Sequence[int]] = None, ann_threshold: Optional[float] = None,
                     ann_values: Optional[Sequence[int]] = None, ann_planes: Optional[Sequence[int]] = None,
                     void_planes: Optional[Sequence[int]] = None, bound_th: float = 0.008,
                     workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """The six counts (``COUNT_NAMES``) of n items on the HIP device: int64 (n, 6) on that device.  ``seg`` / ``ann`` / ``void``
    are stacks (..., H, W) of planes: bool / uint8 (set iff non-zero), float32 with ``*_threshold`` (set iff above it; NaN and
    equality are clear), or a uint8 index map with ``*_values`` (item i is set where the map equals ``values[i]``).  ``*_planes``
    names the plane of every item, so that the objects of a frame share its plane; without it item i reads plane i.  ``radius``
    (0 .. 64) overrides the one that ``bound_th`` gives.  ``workspace_bytes`` bounds the scratch memory (default: the whole stack,
    at most 256 MiB); a stack that needs more is processed in chunks of items, less than one item's worth is an error."""
    from . import _lib
    who = "jf_counts_device"
    dev = getattr(seg, "device", None)
    _lib.require_hip(dev, who)
    S = _Source(who + " seg", seg, seg_threshold, seg_values, seg_planes, dev)
    A = _Source(who + " ann", ann, ann_threshold, ann_values, ann_planes, dev)
    V = None if void is None else _Source(who + " void", void, None, None, void_planes, dev)
    h, w, n = S.h, S.w, S.n
    for o in (A, V):
        if o is not None and ((o.h, o.w) != (h, w) or o.n != n):
            raise _lib.SamptError(f"{who}: {n} items of {h} x {w} against {o.n} of {o.h} x {o.w}")
    if V is not None and V.kind != _KIND_BYTES:
        raise _lib.SamptError(f"{who}: void must be bool or uint8")
    r = boundary_radius(h, w, bound_th) if radius is None else int(radius)
    if not 0 <= r <= MAX_DEVICE_RADIUS:
        raise _lib.SamptError(f"{who}: radius {r} outside 0 .. {MAX_DEVICE_RADIUS}")
    if n == 0:
        return torch.zeros((0, 6), dtype=torch.int64, device=dev)
    lib = _lib.load()
    per = _lib.workspace_bytes("sampt_jf_workspace_bytes", 1, h, w, r)
    workspace_bytes, chunk = _lib.chunk_plan(per, n, workspace_bytes, _WS_CAP, who, h, w)
    with _lib.device_guard(dev):
        stream = _lib.stream_ptr()
        ws = torch.empty(max(16, workspace_bytes), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, 6), dtype=torch.int32, device=dev)
        for c0 in range(0, n, chunk):
            c = min(chunk, n - c0)
            va = (None, None) if V is None else (V.args(c0)[0], V.args(c0)[4])
            _lib.check(lib.sampt_jf_counts(*S.args(c0), *A.args(c0), *va, c, h, w, r, _lib.c_void_p(counts.data_ptr() + 24 * c0),
                                           _lib.ptr(ws), workspace_bytes, stream), "sampt_jf_counts")
        return counts.to(torch.int64)


def jf_device(annotation: torch.Tensor, segmentation: torch.Tensor, void_pixels: Optional[torch.Tensor] = None,
              bound_th: float = 0.008, threshold: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(J, F) of (..., H, W) stacks on the HIP device, float64 numpy arrays (...); ``threshold`` binarises a float32
    ``segmentation``.  Only the 6 counts per item reach the host."""
    if tuple(annotation.shape) != tuple(segmentation.shape):
        raise ValueError(f"annotation {tuple(annotation.shape)} and segmentation {tuple(segmentation.shape)} differ")
    void = None
    if void_pixels is not None:
        void = void_pixels.expand(annotation.shape) if tuple(void_pixels.shape) != tuple(annotation.shape) else void_pixels
    c = jf_counts_device(segmentation, annotation, void, seg_threshold=threshold, bound_th=bound_th).cpu().numpy()
    lead = tuple(annotation.shape[:-2])
    return jaccard_from_counts(c).reshape(lead), f_measure(c)[0].reshape(lead)


# --------------------------------------------------------------------------------------------------------------------
# the semi-supervised sequence protocol
# --------------------------------------------------------------------------------------------------------------------
def _is_hip(x) -> bool:
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def evaluate_semisupervised(pred_index, gt_index, n_objects: Optional[int] = None, bound_th: float = 0.008) -> Dict[str, object]:
    """DAVIS semi-supervised evaluation of one sequence.  ``pred_index`` and ``gt_index`` are object index maps (T, H, W) uint8
    (background 0, object m is ``map == m + 1``; 255 in the ground truth is void).  The number of objects is ``max(gt[0])`` unless
    given; a prediction with fewer objects contributes empty masks; the first and the last frame are dropped.  Returns ``J`` and
    ``F`` float64 (M, T - 2), and ``J-Mean`` / ``J-Recall`` / ``J-Decay`` / ``F-Mean`` / ``F-Recall`` / ``F-Decay`` — the means
    over the objects of ``db_statistics`` of each object's frames — and ``J&F-Mean``.  HIP tensors (the output of
    ``dist.index_masks`` as it is) take the device path, anything else the host path, with identical results."""
    if tuple(pred_index.shape) != tuple(gt_index.shape) or len(pred_index.shape) != 3:
        raise ValueError(f"index maps (T, H, W) of one shape are required; got {tuple(pred_index.shape)} and {tuple(gt_index.shape)}")
    T = int(pred_index.shape[0])
    if T < 3:
        raise ValueError(f"the protocol drops the first and the last frame: at least 3 frames are required; got {T}")
    if _is_hip(pred_index) or _is_hip(gt_index):
        counts, M = _sequence_counts_device(pred_index, gt_index, n_objects, bound_th)
    else:
        counts, M = _sequence_counts_host(pred_index, gt_index, n_objects, bound_th)
    counts = counts.reshape(M, T - 2, 6)
    out: Dict[str, object] = {"J": jaccard_from_counts(counts), "F": f_measure(counts)[0]}
    for k in ("J", "F"):
        stats = np.array([db_statistics(out[k][m]) for m in range(M)], dtype=np.float64).reshape(M, 3)
        for i, name in enumerate(("Mean", "Recall", "Decay")):
            out[f"{k}-{name}"] = _nanmean(stats[:, i]) if M else float("nan")
    out["J&F-Mean"] = (out["J-Mean"] + out["F-Mean"]) / 2
    return out


def _index_dtype_check(x, what):
    dt = x.dtype
    if dt not in (torch.uint8, np.dtype(np.uint8)):
        raise ValueError(f"{what} must be uint8; got {dt}")


def _sequence_counts_host(pred, gt, n_objects, bound_th):
    pred = pred.detach().cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
    gt = gt.detach().cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
    _index_dtype_check(pred, "pred_index"), _index_dtype_check(gt, "gt_index")
    void = gt == 255
    gt = np.where(void, 0, gt).astype(np.uint8)
    M = int(gt[0].max()) if n_objects is None else int(n_objects)
    ids = np.arange(1, M + 1, dtype=np.uint8)[:, None, None, None]
    seg, ann = pred[None, 1:-1] == ids, gt[None, 1:-1] == ids          # (M, T - 2, H, W)
    return jf_counts(seg, ann, void[None, 1:-1], bound_th=bound_th), M


def _sequence_counts_device(pred, gt, n_objects, bound_th):
    dev = pred.device if _is_hip(pred) else gt.device
    pred = pred if _is_hip(pred) else torch.as_tensor(pred).to(dev)
    gt = gt if _is_hip(gt) else torch.as_tensor(gt).to(dev)
    _index_dtype_check(pred, "pred_index"), _index_dtype_check(gt, "gt_index")
    T = int(gt.shape[0])
    void = gt == 255                                                   # (255 never equals an object's value: gt is read as it is)
    if n_objects is None:
        M = int(gt[0].masked_fill(void[0], 0).max().item())
    else:
        M = int(n_objects)
    if M > 254:
        raise ValueError(f"at most 254 objects; got {M}")
    values = np.repeat(np.arange(1, M + 1, dtype=np.int32), T - 2)     # item (m, t): value m + 1, plane t + 1
    planes = np.tile(np.arange(1, T - 1, dtype=np.int32), M)
    if M == 0:
        return np.zeros((0, 6), dtype=np.int64), 0
    c = jf_counts_device(pred, gt, void, seg_values=values, seg_planes=planes, ann_values=values, ann_planes=planes,
                         void_planes=planes, bound_th=bound_th)
    return c.cpu().numpy(), M


# --------------------------------------------------------------------------------------------------------------------
# all pairs of P seg masks and K ann masks per frame (csrc/vos_pairs.hip)
# --------------------------------------------------------------------------------------------------------------------
def _values_of(who, values) -> np.ndarray:
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    v = np.asarray(values)
    if v.ndim != 1 or v.dtype.kind not in "iu" or (v.size and (int(v.min()) < 0 or int(v.max()) > 255)):
        raise ValueError(f"{who}: values must be a 1-D integer sequence inside 0 .. 255")
    return v.astype(np.int32)


def _pair_masks(who, x, values, threshold) -> np.ndarray:
    """One side of ``jf_pairs_counts`` as bool (n, T, H, W)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if values is not None:
        if x.ndim != 3 or x.dtype != np.uint8:
            raise ValueError(f"{who}: an index map must be uint8 (T, H, W); got {x.dtype} {x.shape}")
        return x[None] == _values_of(who, values).astype(np.uint8)[:, None, None, None]
    if x.ndim != 4:
        raise ValueError(f"{who}: planes (n, T, H, W) are required; got {x.shape}")
    return _as_bool(x, threshold)


def _pairs_assemble(inter, seg_match, ann_match, seg_stat, ann_stat, xp):
    """(P, K, T, 6) in ``COUNT_NAMES`` order from inter / seg_match / ann_match (P, K, T) and the stats (P, T, 2), (K, T, 2) = area,
    boundary count; ``xp`` is numpy or torch."""
    P, K = seg_stat.shape[0], ann_stat.shape[0]
    sa, sb = seg_stat[:, None, :, 0], seg_stat[:, None, :, 1]
    aa, ab = ann_stat[None, :, :, 0], ann_stat[None, :, :, 1]
    shape = inter.shape
    if xp is np:
        return np.stack([inter, sa + aa - inter, np.broadcast_to(sb, shape), np.broadcast_to(ab, shape), seg_match, ann_match], axis=-1)
    return torch.stack([inter, sa + aa - inter, sb.expand(shape), ab.expand(shape), seg_match, ann_match], dim=-1)


def jf_pairs_counts(seg, ann, void=None, radius: Optional[int] = None, bound_th: float = 0.008, seg_threshold: Optional[float] = None,
                    ann_threshold: Optional[float] = None, seg_values: Optional[Sequence[int]] = None,
                    ann_values: Optional[Sequence[int]] = None, return_stats: bool = False):
    """The six counts (``COUNT_NAMES``) of every (seg mask p, ann mask k) pair of every frame on the host: int64 (P, K, T, 6), with
    ``union = area_p + area_k - inter``; slice ``[p, k]`` equals ``jf_counts(seg[p], ann[k], void)``.  A side is planes (n, T, H, W)
    (bool / uint8, or float with ``*_threshold``) or a uint8 index map (T, H, W) with ``*_values`` (mask i is ``map == values[i]``);
    ``void`` (T, H, W) is cleared from both.  Every boundary is dilated once.  ``return_stats`` adds the per-mask (area, boundary
    count) arrays int64 (P, T, 2) and (K, T, 2)."""
    S, A = _pair_masks("seg", seg, seg_values, seg_threshold), _pair_masks("ann", ann, ann_values, ann_threshold)
    if S.shape[1:] != A.shape[1:]:
        raise ValueError(f"seg frames {S.shape[1:]} and ann frames {A.shape[1:]} differ")
    (P, T, h, w), K = S.shape, A.shape[0]
    if void is not None:
        keep = ~_as_bool(void)
        if keep.shape != (T, h, w):
            raise ValueError(f"void must be (T, H, W) = {(T, h, w)}; got {keep.shape}")
        S, A = S & keep[None], A & keep[None]
    r = boundary_radius(h, w, bound_th) if radius is None else int(radius)
    bs, ba = seg2bmap(S), seg2bmap(A)
    ds, da = dilate_disk(bs, r), dilate_disk(ba, r)
    seg_stat = np.stack([S.sum(axis=(2, 3)), bs.sum(axis=(2, 3))], axis=-1).astype(np.int64)
    ann_stat = np.stack([A.sum(axis=(2, 3)), ba.sum(axis=(2, 3))], axis=-1).astype(np.int64)
    inter, sm, am = (np.zeros((P, K, T), dtype=np.int64) for _ in range(3))
    for p in range(P):
        for k in range(K):
            inter[p, k] = (S[p] & A[k]).sum(axis=(1, 2))
            sm[p, k] = (bs[p] & da[k]).sum(axis=(1, 2))
            am[p, k] = (ba[k] & ds[p]).sum(axis=(1, 2))
    out = _pairs_assemble(inter, sm, am, seg_stat, ann_stat, np)
    return (out, seg_stat, ann_stat) if return_stats else out


def _pair_source(who, x, threshold, values, dev):
    """(source, n): the items of one side in the kernel's order, item t * n + i = mask i of frame t."""
    from . import _lib
    if not isinstance(x, torch.Tensor):
        raise _lib.SamptError(f"{who}: every input must be a tensor on {dev}")
    if values is not None:
        if x.dim() != 3:
            raise _lib.SamptError(f"{who}: an index map must be (T, H, W); got {tuple(x.shape)}")
        v = _values_of(who, values)
        n, T = len(v), int(x.shape[0])
        return _Source(who, x, threshold, np.tile(v, T), np.repeat(np.arange(T, dtype=np.int32), n), dev), n, T
    if x.dim() != 4:
        raise _lib.SamptError(f"{who}: planes (n, T, H, W) are required; got {tuple(x.shape)}")
    n, T = int(x.shape[0]), int(x.shape[1])
    planes = (np.arange(n, dtype=np.int32)[None, :] * T + np.arange(T, dtype=np.int32)[:, None]).reshape(-1)
    return _Source(who, x, threshold, None, planes, dev), n, T


def jf_pairs_counts_device(seg: torch.Tensor, ann: torch.Tensor, void: Optional[torch.Tensor] = None, radius: Optional[int] = None,
                           bound_th: float = 0.008, seg_threshold: Optional[float] = None, ann_threshold: Optional[float] = None,
                           seg_values: Optional[Sequence[int]] = None, ann_values: Optional[Sequence[int]] = None,
                           return_stats: bool = False, workspace_bytes: Optional[int] = None):
    """``jf_pairs_counts`` on the HIP device (csrc/vos_pairs.hip): int64 (P, K, T, 6) on that device, the same integers.  Every mask
    is read once and its boundary dilated once; the pairs are a popcount GEMM over bit-planes.  ``workspace_bytes`` bounds the scratch
    memory (default: all frames, at most 256 MiB); more frames than fit are processed in chunks of frames, less than one frame's worth
    is an error."""
    from . import _lib
    who = "jf_pairs_counts_device"
    dev = getattr(seg, "device", None)
    _lib.require_hip(dev, who)
    S, P, T = _pair_source(who + " seg", seg, seg_threshold, seg_values, dev)
    A, K, Ta = _pair_source(who + " ann", ann, ann_threshold, ann_values, dev)
    h, w = S.h, S.w
    if (A.h, A.w, Ta) != (h, w, T):
        raise _lib.SamptError(f"{who}: {T} frames of {h} x {w} against {Ta} of {A.h} x {A.w}")
    V = None
    if void is not None:
        V = _Source(who + " void", void, None, None, None, dev)
        if V.kind != _KIND_BYTES or void.dim() != 3 or (V.n, V.h, V.w) != (T, h, w):
            raise _lib.SamptError(f"{who}: void must be bool or uint8 (T, H, W) = {(T, h, w)}; got {void.dtype} {tuple(void.shape)}")
    r = boundary_radius(h, w, bound_th) if radius is None else int(radius)
    if not 0 <= r <= MAX_DEVICE_RADIUS:
        raise _lib.SamptError(f"{who}: radius {r} outside 0 .. {MAX_DEVICE_RADIUS}")
    if P == 0 or K == 0 or T == 0:
        z = torch.zeros((P, K, T, 6), dtype=torch.int64, device=dev)
        return (z, torch.zeros((P, T, 2), dtype=torch.int64, device=dev), torch.zeros((K, T, 2), dtype=torch.int64, device=dev)) \
            if return_stats else z
    lib = _lib.load()
    per = _lib.workspace_bytes("sampt_jf_pairs_workspace_bytes", P, K, 1, h, w, r)
    if per == 0:                                          # (this query has a second way to refuse: its own words)
        raise _lib.SamptError(f"{who}: h * w and 3 * P * K must be below 2^31; got {h} x {w}, P = {P}, K = {K}")
    workspace_bytes, chunk = _lib.chunk_plan(per, T, workspace_bytes, _WS_CAP, who, h, w, max_chunk=((1 << 31) - 1) // (3 * P * K))
    with _lib.device_guard(dev):
        stream = _lib.stream_ptr()
        ws = torch.empty(max(16, workspace_bytes), dtype=torch.uint8, device=dev)
        pair = torch.empty((T, P, K, 3), dtype=torch.int32, device=dev)
        sstat = torch.empty((T, P, 2), dtype=torch.int32, device=dev)
        astat = torch.empty((T, K, 2), dtype=torch.int32, device=dev)
        for t0 in range(0, T, chunk):
            c = min(chunk, T - t0)
            va = (None, None) if V is None else (V.args(t0)[0], V.args(t0)[4])
            _lib.check(lib.sampt_jf_pairs_counts(*S.args(t0 * P), P, *A.args(t0 * K), K, *va, c, h, w, r,
                                                 _lib.c_void_p(pair.data_ptr() + 12 * P * K * t0), _lib.c_void_p(sstat.data_ptr() + 8 * P * t0),
                                                 _lib.c_void_p(astat.data_ptr() + 8 * K * t0), _lib.ptr(ws), workspace_bytes, stream),
                       "sampt_jf_pairs_counts")
        pair = pair.to(torch.int64).permute(1, 2, 0, 3)                   # (P, K, T, 3)
        sstat, astat = sstat.to(torch.int64).permute(1, 0, 2), astat.to(torch.int64).permute(1, 0, 2)
        out = _pairs_assemble(pair[..., 0], pair[..., 1], pair[..., 2], sstat, astat, torch)
        return (out, sstat.contiguous(), astat.contiguous()) if return_stats else out


# --------------------------------------------------------------------------------------------------------------------
# the unsupervised sequence protocol
# --------------------------------------------------------------------------------------------------------------------
def evaluate_unsupervised(pred, gt_index, max_n_proposals: int = 20, bound_th: float = 0.008,
                          n_objects: Optional[int] = None) -> Dict[str, object]:
    """DAVIS unsupervised evaluation of one sequence, restated from the published DAVIS 2017 toolkit (``Davis2017Evaluator`` with
    ``task="unsupervised"``, which the reference calls): **parity unpinned**, as the rest of this J&F restatement.  ``pred`` is an
    index map (T, H, W) uint8 with the proposals 1 .. P = ``max(pred)``, or boolean planes (P, T, H, W); ``gt_index`` is as in
    ``evaluate_semisupervised`` (255 is void; the objects are 1 .. ``max(gt[0])`` unless ``n_objects`` is given).  The first and the
    last frame are dropped; more than ``max_n_proposals`` proposals is a ``ValueError``; fewer proposals than objects are padded with
    empty masks.  With ``J_all`` / ``F_all`` float64 (P, K, T - 2) of every pair, the score is (J.mean(2) + F.mean(2)) / 2, the
    assignment ``scipy.optimize.linear_sum_assignment(-score)``; the matched pairs give ``J`` and ``F`` (K, T - 2), and from them the
    seven figures of ``evaluate_semisupervised``.  ``assignment`` is (proposal rows, object columns).  HIP tensors take the device
    path (``jf_pairs_counts_device``), anything else the host path, with identical results."""
    from scipy.optimize import linear_sum_assignment
    if len(gt_index.shape) != 3:
        raise ValueError(f"gt_index must be (T, H, W); got {tuple(gt_index.shape)}")
    T = int(gt_index.shape[0])
    planes = len(pred.shape) == 4
    if tuple(pred.shape[-3:]) != tuple(gt_index.shape) or len(pred.shape) not in (3, 4):
        raise ValueError(f"pred (T, H, W) or (P, T, H, W) must match gt_index {tuple(gt_index.shape)}; got {tuple(pred.shape)}")
    if T < 3:
        raise ValueError(f"the protocol drops the first and the last frame: at least 3 frames are required; got {T}")
    device = _is_hip(pred) or _is_hip(gt_index)
    if device:
        dev = pred.device if _is_hip(pred) else gt_index.device
        pred = pred if _is_hip(pred) else torch.as_tensor(pred).to(dev)
        gt = gt_index if _is_hip(gt_index) else torch.as_tensor(gt_index).to(dev)
    else:
        pred = pred.detach().cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
        gt = gt_index.detach().cpu().numpy() if isinstance(gt_index, torch.Tensor) else np.asarray(gt_index)
    _index_dtype_check(gt, "gt_index")
    if planes:
        if pred.dtype not in (torch.bool, np.dtype(bool)):
            raise ValueError(f"proposal planes must be bool; got {pred.dtype}")
        P = int(pred.shape[0])
    else:
        _index_dtype_check(pred, "pred")
        P = int(pred.max())
    void = gt == 255
    if n_objects is not None:
        K = int(n_objects)
    elif device:
        K = int(gt[0].masked_fill(void[0], 0).max().item())
    else:
        K = int(np.where(void[0], 0, gt[0]).max())
    if P > max_n_proposals:
        raise ValueError(f"{P} proposals: at most max_n_proposals = {max_n_proposals} are allowed")
    if max(P, K) > 254:
        raise ValueError(f"at most 254 proposals and objects; got {P} and {K}")
    Pp = max(P, K)                                                     # (padded with empty proposals)
    out: Dict[str, object] = {}
    if K == 0:
        J_all = F_all = np.zeros((Pp, 0, T - 2))
        rows = cols = np.zeros(0, dtype=np.int64)
    else:
        if planes and P < Pp:
            pad = (Pp - P,) + tuple(pred.shape[1:])
            pred = torch.cat([pred, pred.new_zeros(pad)]) if device else np.concatenate([pred, np.zeros(pad, dtype=bool)])
        seg = pred[:, 1:-1] if planes else pred[1:-1]
        kw = dict(bound_th=bound_th, ann_values=np.arange(1, K + 1), seg_values=None if planes else np.arange(1, Pp + 1))
        if device:                                                     # (255 never equals an object's value: gt is read as it is)
            counts = jf_pairs_counts_device(seg, gt[1:-1], void[1:-1], **kw).cpu().numpy()
        else:
            counts = jf_pairs_counts(seg, gt[1:-1], void[1:-1], **kw)
        J_all, F_all = jaccard_from_counts(counts), f_measure(counts)[0]
        rows, cols = linear_sum_assignment(-((J_all.mean(axis=2) + F_all.mean(axis=2)) / 2))
    out["J_all"], out["F_all"], out["assignment"] = J_all, F_all, (rows, cols)
    out["J"], out["F"] = J_all[rows, cols], F_all[rows, cols]
    for k in ("J", "F"):
        stats = np.array([db_statistics(v) for v in out[k]], dtype=np.float64).reshape(K, 3)
        for i, name in enumerate(("Mean", "Recall", "Decay")):
            out[f"{k}-{name}"] = _nanmean(stats[:, i]) if K else float("nan")
    out["J&F-Mean"] = (out["J-Mean"] + out["F-Mean"]) / 2
    return out


# --------------------------------------------------------------------------------------------------------------------
# the BDD100K protocol (the reference's vos_eval/bdd100keval.py)
# --------------------------------------------------------------------------------------------------------------------
BDD100K_GLOBAL_NAMES = ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay", "J&F-Mean-Vis", "J-Mean-Vis",
                        "F-Mean-Vis", "J&F-Mean-NonVis", "J-Mean-NonVis", "F-Mean-NonVis", "J&F-Mean-Short", "J-Mean-Short", "F-Mean-Short",
                        "J&F-Mean-Medium", "J-Mean-Medium", "F-Mean-Medium", "J&F-Mean-Long", "J-Mean-Long", "F-Mean-Long")
_BDD_KINDS = ("J", "F", "J_vis", "F_vis", "J_nonvis", "F_nonvis")


def _bdd100k_counts_host(pred, gt, overlap, bound_th):
    pred = pred.detach().cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
    gt = gt.detach().cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
    _index_dtype_check(gt, "gt_index")
    K = _bdd100k_check(int(gt.max()), None if overlap else int(pred.max()), pred, gt, overlap)
    ids = np.arange(1, K + 1, dtype=np.uint8)[:, None, None, None]
    ann = gt[None] == ids                                              # (K, T, H, W)
    seg = np.ascontiguousarray(pred[:, 1:].transpose(1, 0, 2, 3)) if overlap else pred[None] == ids
    counts = jf_counts(seg, ann, None, bound_th=bound_th).reshape(K, -1, 6)
    return counts, ann.sum(axis=(2, 3)).astype(np.int64)


def _bdd100k_check(max_gt, max_pred, pred, gt, overlap) -> int:
    T, h, w = (int(v) for v in gt.shape)
    if max_gt == 255:
        raise ValueError("gt_index holds 255: BDD100K has no void label")
    if max_gt == 0:
        raise ValueError("there are no objects in the ground truth")
    if overlap:
        if pred.dtype not in (torch.bool, np.dtype(bool)) or tuple(pred.shape) != (T, max_gt + 1, h, w):
            raise ValueError(f"with object_overlapping_allowed pred must be bool (T, K + 1, H, W) = {(T, max_gt + 1, h, w)} with plane 0 the "
                             f"background; got {pred.dtype} {tuple(pred.shape)}")
    else:
        _index_dtype_check(pred, "pred")
        if tuple(pred.shape) != (T, h, w):
            raise ValueError(f"pred {tuple(pred.shape)} and gt_index {(T, h, w)} differ")
        if max_pred > max_gt:
            raise ValueError(f"pred holds the index {max_pred}, above the {max_gt} objects of the sequence")
    return max_gt


def _bdd100k_counts_device(pred, gt, overlap, bound_th):
    from .vis_metrics import bits_pack_device
    dev = pred.device if _is_hip(pred) else gt.device
    pred = pred if _is_hip(pred) else torch.as_tensor(pred).to(dev)
    gt = gt if _is_hip(gt) else torch.as_tensor(gt).to(dev)
    _index_dtype_check(gt, "gt_index")
    T = int(gt.shape[0])
    if overlap:
        max_gt, max_pred = int(gt.max().item()), None
    else:
        max_gt, max_pred = (int(v) for v in torch.stack([gt.max(), pred.max().to(gt.dtype)]).cpu().tolist())
    K = _bdd100k_check(max_gt, max_pred, pred, gt, overlap)
    if K > 254:
        raise ValueError(f"at most 254 objects; got {K}")
    values = np.repeat(np.arange(1, K + 1, dtype=np.int32), T)         # item (k, t): value k + 1, plane t
    planes = np.tile(np.arange(T, dtype=np.int32), K)
    if overlap:                                                        # plane (t, k + 1) of (T, K + 1, H, W)
        seg_kw = dict(seg_planes=planes * (K + 1) + values)
    else:
        seg_kw = dict(seg_values=values, seg_planes=planes)
    c = jf_counts_device(pred, gt, None, ann_values=values, ann_planes=planes, bound_th=bound_th, **seg_kw)
    area = bits_pack_device(gt, values=values, planes=planes)[1]
    both = torch.cat([c, area.to(torch.int64)[:, None]], dim=1).cpu().numpy()      # the one download of the sequence's counts
    return both[:, :6].reshape(K, T, 6), both[:, 6].reshape(K, T)


def evaluate_bdd100k_sequence(pred, gt_index, object_overlapping_allowed: bool = False, bound_th: float = 0.008) -> Dict[str, object]:
    """The BDD100K protocol of the reference's ``BDD100KEvaluation`` (vos_eval/bdd100keval.py) for one sequence.  ``gt_index`` is an
    index map (T, H, W) uint8 without a void label (a 255 is refused); the objects are 1 .. ``max(gt_index)`` over the whole sequence.
    ``pred`` is an index map of that shape (an index above the number of objects is an error) or, with
    ``object_overlapping_allowed``, boolean planes (T, K + 1, H, W) with plane 0 the background.  An object is visible on a frame when
    its ground-truth area is positive; it is scored on the frames after the first visible one, no end frame is dropped, and those
    frames split into visible and non-visible ones.  ``n_frames`` = scored frames + 1 and ``visible_frames`` = visible scored frames
    + 1; an object that first appears on the last frame gets the record of all ones (a one-frame ``J`` = ``F`` = [1.], the visible and
    the non-visible subsets included).  An object that is never visible is a ``ValueError``.

    Returns, per object (lists of K float64 arrays): ``J``, ``F``, ``J_vis``, ``F_vis``, ``J_nonvis``, ``F_nonvis``; int64 arrays (K,)
    ``n_frames``, ``visible_frames``, ``nonvisible_frames``; and ``stats``: for each of the six names the (K, 3) array of
    ``db_statistics`` (mean, recall, decay), NaN where a subset is empty.  HIP tensors take the device path: every (object, frame) item
    goes through ``sampt_jf_counts``, the ground-truth areas come from ``sampt_bits_pack``, and only these integers reach the host;
    frame selection and statistics are the float64 host code that the host path runs too, so the results are identical."""
    if len(gt_index.shape) != 3:
        raise ValueError(f"gt_index must be (T, H, W); got {tuple(gt_index.shape)}")
    overlap = bool(object_overlapping_allowed)
    if _is_hip(pred) or _is_hip(gt_index):
        counts, areas = _bdd100k_counts_device(pred, gt_index, overlap, bound_th)
    else:
        counts, areas = _bdd100k_counts_host(pred, gt_index, overlap, bound_th)
    K, T = areas.shape
    out: Dict[str, object] = {k: [] for k in _BDD_KINDS}
    frames = np.zeros((K, 3), dtype=np.int64)
    one = np.array([1.0])
    for k in range(K):
        visible = areas[k] > 0
        if not visible.any():
            raise ValueError(f"object id {k + 1} is never visible in the ground truth")
        first = int(np.argmax(visible))
        if first == T - 1:
            rec, n, nv = (one.copy() for _ in range(6)), 1, 1
        else:
            vis = visible[first + 1:]
            J, F = jaccard_from_counts(counts[k, first + 1:]), f_measure(counts[k, first + 1:])[0]
            rec, n, nv = (J, F, J[vis], F[vis], J[~vis], F[~vis]), len(vis) + 1, int(vis.sum()) + 1
        for name, v in zip(_BDD_KINDS, rec):
            out[name].append(v)
        frames[k] = n, nv, n - nv
    out["n_frames"], out["visible_frames"], out["nonvisible_frames"] = frames[:, 0], frames[:, 1], frames[:, 2]
    out["stats"] = {name: np.array([db_statistics(v) for v in out[name]], dtype=np.float64).reshape(K, 3) for name in _BDD_KINDS}
    return out


class BDD100KEval:
    """Accumulates ``evaluate_bdd100k_sequence`` over the sequences of a data set and forms the tables of the reference's
    ``BDD100KEvaluator.evaluate``: ``add(name, pred, gt_index)`` per sequence, then ``summarize()``.  Objects with fewer visible
    frames than ``short_object_threshold`` are short, those with at least ``long_object_threshold`` long, the rest medium."""

    def __init__(self, short_object_threshold: int = 5, long_object_threshold: int = 30, object_overlapping_allowed: bool = False,
                 bound_th: float = 0.008):
        self.sot, self.lot = short_object_threshold, long_object_threshold
        self.object_overlapping_allowed, self.bound_th = object_overlapping_allowed, bound_th
        self.names = []
        self.stats = {k: [] for k in _BDD_KINDS}                       # per object: (mean, recall, decay)
        self.frames = []                                               # per object: (n_frames, visible, non-visible)
        self.sequences: Dict[str, Dict[str, object]] = {}

    def add(self, name: str, pred, gt_index) -> Dict[str, object]:
        if name in self.sequences:
            raise ValueError(f"sequence {name!r} was added before")
        res = evaluate_bdd100k_sequence(pred, gt_index, self.object_overlapping_allowed, self.bound_th)
        self.sequences[name] = res
        for k in range(len(res["n_frames"])):
            self.names.append(f"{name}_{k + 1}")
            for kind in _BDD_KINDS:
                self.stats[kind].append(res["stats"][kind][k])
            self.frames.append((int(res["n_frames"][k]), int(res["visible_frames"][k]), int(res["nonvisible_frames"][k])))
        return res

    def _label(self, v: int) -> str:
        return "short" if v < self.sot else "medium" if v < self.lot else "long"

    def summarize(self) -> Tuple[Dict[str, float], Dict[str, list]]:
        """(the 22 global figures under the reference's names, the per-object table as a dict of columns).  The plain figures are
        means over all objects, ``-Vis`` / ``-NonVis`` nanmeans (an object without such frames does not count), and the three length
        bins means over the objects of the bin (NaN for an empty bin)."""
        if not self.names:
            raise ValueError("no sequence was added")
        st = {k: np.ascontiguousarray(np.array(v, dtype=np.float64).reshape(-1, 3).T) for k, v in self.stats.items()}   # (3, objects)
        fr = np.array(self.frames, dtype=np.int64).reshape(-1, 3)
        vis = fr[:, 1]
        Jm, Fm = st["J"][0], st["F"][0]
        g: Dict[str, float] = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            g["J&F-Mean"] = (np.mean(Jm) + np.mean(Fm)) / 2.
            for i, what in enumerate(("Mean", "Recall", "Decay")):
                g[f"J-{what}"], g[f"F-{what}"] = np.mean(st["J"][i]), np.mean(st["F"][i])
            for tag, kind in (("Vis", "vis"), ("NonVis", "nonvis")):
                j, f = np.nanmean(st[f"J_{kind}"][0]), np.nanmean(st[f"F_{kind}"][0])
                g[f"J&F-Mean-{tag}"], g[f"J-Mean-{tag}"], g[f"F-Mean-{tag}"] = (j + f) / 2., j, f
            for tag, sel in (("Short", vis < self.sot), ("Medium", (vis >= self.sot) & (vis < self.lot)), ("Long", vis >= self.lot)):
                j, f = Jm[sel].mean(), Fm[sel].mean()
                g[f"J&F-Mean-{tag}"], g[f"J-Mean-{tag}"], g[f"F-Mean-{tag}"] = j / 2. + f / 2., j, f
        g = {k: float(g[k]) for k in BDD100K_GLOBAL_NAMES}
        table = {"Sequence": list(self.names), "J-Mean": Jm.tolist(), "F-Mean": Fm.tolist(),
                 "J-Mean-Vis": st["J_vis"][0].tolist(), "F-Mean-Vis": st["F_vis"][0].tolist(),
                 "J-Mean-NonVis": st["J_nonvis"][0].tolist(), "F-Mean-NonVis": st["F_nonvis"][0].tolist(),
                 "n_frames": fr[:, 0].tolist(), "visible_frames": fr[:, 1].tolist(), "nonvisible_frames": fr[:, 2].tolist(),
                 "short-medium-long": [self._label(int(v)) for v in vis]}
        return g, table
