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
    per = int(lib.sampt_jf_workspace_bytes(1, h, w, r))
    if per == 0:
        raise _lib.SamptError(f"{who}: h * w must be below 2^31; got {h} x {w}")
    if workspace_bytes is None:
        workspace_bytes = max(per, min(n * per, _WS_CAP))
    chunk = max(1, min(n, int(workspace_bytes) // per))              # (0 items' worth: the call itself refuses the workspace)
    with _lib.device_guard(dev):
        stream = _lib.stream_ptr()
        ws = torch.empty(max(16, int(workspace_bytes)), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, 6), dtype=torch.int32, device=dev)
        for c0 in range(0, n, chunk):
            c = min(chunk, n - c0)
            va = (None, None) if V is None else (V.args(c0)[0], V.args(c0)[4])
            _lib.check(lib.sampt_jf_counts(*S.args(c0), *A.args(c0), *va, c, h, w, r, _lib.c_void_p(counts.data_ptr() + 24 * c0),
                                           _lib.ptr(ws), int(workspace_bytes), stream), "sampt_jf_counts")
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
