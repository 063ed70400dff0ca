"""YouTube-VIS / UVO AP and AR: the evaluator behind the reference's ``YTVISEvaluator`` (vis_eval/mask2former_video/data_video/
ytvis_eval.py), which calls ``YTVOSeval`` (.../datasets/ytvis_api/ytvoseval.py) on top of pycocotools.  pycocotools is absent here;
this module restates the protocol — the IoU over a sequence, crowd / ignore handling, the greedy matching, the accumulation and the
12 summary figures — on the host in NumPy, and runs its two expensive parts on the HIP device (csrc/vis_eval.hip): all-pairs
spatio-temporal intersection / union as popcounts of ANDed 64-bit column words, and the matching.  The protocol is pinned on the
reference's own evaluator run in place (tests/ytvis_ref.py, tests/golden/vis_eval_ref.npz); only the pixel primitives are ours.

Everything on the device is integer work or one correctly rounded float64 division, so the device functions return exactly what
their host twins return.

    bit-planes    a stack (n, h, w) as words (n, ceil(h / 64), w): bit j of word (band b, column x) is pixel (64 b + j, x); the bits
                  of rows >= h are 0.  On the device the words live in an int64 tensor (torch has no uint64 arithmetic).
    plane tables  int (items, frames): the plane of every item on every frame, -1 = no mask on that frame.  An absent and an empty
                  mask behave alike in the sequence IoU (the reference's ``iou_seq``: both add the other side's area to the union).
    positions     the matching works on positions: ``dt_match`` is 1 + the ground truth's index in the group (0 = unmatched),
                  ``gt_match`` 1 + the detection's position in score order, per column of the area range's ground-truth order.
"""
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .automatic_mask_generator import coco_rle_counts

METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
MAX_DEVICE_GT = 960
MAX_DEVICE_THRS = 64


class Params:
    """The evaluation parameters with the reference's defaults for segmentation (``useCats = 1`` is the only mode)."""

    def __init__(self):
        self.iouThrs = np.linspace(0.5, 0.95, 10, endpoint=True)
        self.recThrs = np.linspace(0.0, 1.0, 101, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0.0, 1e10], [0.0, 128.0 ** 2], [128.0 ** 2, 256.0 ** 2], [256.0 ** 2, 1e10]]     # inclusive bounds
        self.areaRngLbl = ["all", "small", "medium", "large"]


# --------------------------------------------------------------------------------------------------------------------
# host restatement
# --------------------------------------------------------------------------------------------------------------------
def pack_bits(masks) -> np.ndarray:
    """bool (n, h, w) -> bit-planes uint64 (n, ceil(h / 64), w)."""
    m = np.asarray(masks).astype(bool)
    n, h, w = m.shape
    nb = (h + 63) // 64
    pad = np.zeros((n, nb * 64, w), dtype=bool)
    pad[:, :h] = m
    by = np.packbits(pad.reshape(n, nb, 64, w).transpose(0, 1, 3, 2), axis=-1, bitorder="little")     # (n, nb, w, 8)
    return np.ascontiguousarray(by).view("<u8").reshape(n, nb, w).astype(np.uint64)


def unpack_bits(bits, h: int) -> np.ndarray:
    """Bit-planes (n, nb, w) -> bool (n, h, w)."""
    b = np.ascontiguousarray(np.asarray(bits).astype("<u8"))
    n, nb, w = b.shape
    px = np.unpackbits(b.view(np.uint8).reshape(n, nb, w, 8), axis=-1, bitorder="little")           # (n, nb, w, 64)
    return px.transpose(0, 1, 3, 2).reshape(n, nb * 64, w)[:, :h].astype(bool)


def bits_pack(x, threshold: Optional[float] = None, values: Optional[Sequence[int]] = None,
              planes: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(bit-planes uint64 (n, nb, w), areas int32 (n,)) of a stack (..., H, W) on the host: bool / uint8 (set iff non-zero), float
    with ``threshold`` (set iff above it; NaN and equality are clear), or a uint8 index map with ``values`` (item i is set where the
    map equals ``values[i]``); ``planes`` names the plane of every item."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    x = x.reshape((-1,) + x.shape[-2:])
    if planes is not None:
        x = x[np.asarray(planes, dtype=np.int64)]
    if values is not None:
        if planes is None and len(values) != x.shape[0]:
            raise ValueError(f"{len(values)} values for {x.shape[0]} planes and no plane numbers")
        m = x == np.asarray(values).reshape(-1, 1, 1)
    elif x.dtype.kind == "f":
        if threshold is None:
            raise ValueError("a float stack needs a threshold")
        with np.errstate(invalid="ignore"):
            m = x > np.float32(threshold)
    else:
        m = x != 0
    return pack_bits(m), m.sum(axis=(1, 2)).astype(np.int32)


def _counts_of(rle: Dict[str, Any]) -> List[int]:
    c = rle["counts"]
    if isinstance(c, (str, bytes, bytearray)):
        return coco_rle_counts(c)
    return [int(v) for v in c]


def rle_decode(counts_list: Sequence[Sequence[int]], h: int, w: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Column-major runs (the first run counts zeros) of n masks -> (bit-planes uint64 (n, nb, w), areas int32, status int32).
    A mask whose runs do not sum to h * w has status 1, an all-zero plane and area 0."""
    n = len(counts_list)
    masks = np.zeros((n, h, w), dtype=bool)
    area, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i, c in enumerate(counts_list):
        c = np.asarray(c, dtype=np.int64).reshape(-1)
        if c.size == 0 or (c < 0).any() or int(c.sum()) != h * w:
            status[i] = 1
            continue
        masks[i] = np.repeat((np.arange(c.size) % 2).astype(bool), c).reshape(w, h).T
        area[i] = int(c[1::2].sum())
    return pack_bits(masks), area, status


def seq_iou_counts(dt_masks, dt_planes, gt_masks, gt_planes) -> np.ndarray:
    """int64 (D, G, 2) = (inter, union) of every pair over the frames.  ``dt_masks`` / ``gt_masks``: bool stacks (planes, h, w);
    ``dt_planes`` (D, T) / ``gt_planes`` (G, T): plane tables.  inter = sum_t |d_t & g_t|, union = sum_t (|d_t| + |g_t|) - inter
    with an absent frame contributing nothing of its own."""
    dm, gm = np.asarray(dt_masks).astype(bool), np.asarray(gt_masks).astype(bool)
    dp, gp = np.asarray(dt_planes, dtype=np.int64), np.asarray(gt_planes, dtype=np.int64)
    D, G = dp.shape[0], gp.shape[0]
    if dp.ndim != 2 or gp.ndim != 2 or (D and G and dp.shape[1] != gp.shape[1]):
        raise ValueError(f"plane tables (items, frames) with one frame count are required; got {dp.shape} and {gp.shape}")
    T = dp.shape[1] if D else (gp.shape[1] if G else 0)
    df = dm.reshape(dm.shape[0], int(np.prod(dm.shape[1:])))           # (an explicit size: a stack may have no plane)
    gf = gm.reshape(gm.shape[0], int(np.prod(gm.shape[1:])))
    ft = np.float32 if df.shape[1] < (1 << 24) else np.float64        # 0 / 1 products: every per-frame sum is exact
    da, ga = df.sum(axis=1).astype(np.int64), gf.sum(axis=1).astype(np.int64)
    inter = np.zeros((D, G), dtype=np.int64)
    for t in range(T if D and G else 0):
        di, gi = np.flatnonzero(dp[:, t] >= 0), np.flatnonzero(gp[:, t] >= 0)
        if di.size and gi.size:
            inter[np.ix_(di, gi)] += np.rint(df[dp[di, t]].astype(ft) @ gf[gp[gi, t]].astype(ft).T).astype(np.int64)
    ad = np.where(dp >= 0, da[np.maximum(dp, 0)] if da.size else 0, 0).sum(axis=1) if D else np.zeros(0, dtype=np.int64)
    ag = np.where(gp >= 0, ga[np.maximum(gp, 0)] if ga.size else 0, 0).sum(axis=1) if G else np.zeros(0, dtype=np.int64)
    union = ad[:, None] + ag[None, :] - inter
    return np.stack([inter, union], axis=-1).astype(np.int64)


def seq_iou(counts) -> np.ndarray:
    """float64 (D, G): inter / union, 0 for an empty union."""
    c = np.asarray(counts)
    inter, union = c[..., 0].astype(np.float64), c[..., 1].astype(np.float64)
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def _match_inputs(counts, gt_ignore, iscrowd, dt_out, thrs):
    gt_ignore = np.asarray(gt_ignore).astype(bool)
    dt_out = np.asarray(dt_out).astype(bool)
    iscrowd = np.asarray(iscrowd).astype(bool).reshape(-1)
    thrs = np.asarray(thrs, dtype=np.float64).reshape(-1)
    if gt_ignore.ndim != 2 or dt_out.ndim != 2 or gt_ignore.shape[0] != dt_out.shape[0]:
        raise ValueError(f"gt_ignore (ranges, G) and dt_out (ranges, D) are required; got {gt_ignore.shape} and {dt_out.shape}")
    A, G = gt_ignore.shape
    D = dt_out.shape[1]
    if tuple(counts.shape) != (D, G, 2) or iscrowd.shape[0] != G:
        raise ValueError(f"counts {tuple(counts.shape)} / iscrowd {iscrowd.shape} do not fit D = {D}, G = {G}")
    order = np.stack([np.argsort(gt_ignore[a].astype(np.int64), kind="mergesort") for a in range(A)]).astype(np.int32).reshape(A, G)
    ig_sorted = np.take_along_axis(gt_ignore, order.astype(np.int64), axis=1)
    return gt_ignore, dt_out, iscrowd, thrs, order, ig_sorted, A, D, G


def match_video(counts, gt_ignore, iscrowd, dt_out, thrs) -> Dict[str, np.ndarray]:
    """The greedy matching of one (video, category) group for every area range and IoU threshold.  ``counts`` int64 (D, G, 2) with
    the detections in score order, already cut to the last ``maxDets``; ``gt_ignore`` (ranges, G): the ground truth is a crowd or
    its average area is outside the range; ``iscrowd`` (G,); ``dt_out`` (ranges, D): the detection's average area is outside the
    range.  Returns ``gt_order`` int32 (ranges, G) (the stable sort by the ignore flag), ``gt_ignore`` bool in that order, and the
    position tables ``dt_match`` int32 (ranges, thrs, D), ``gt_match`` int32 (ranges, thrs, G), ``dt_ignore`` bool (ranges, thrs, D).

    Per threshold t and detection, in score order: the best IoU so far starts at min(t, 1 - 1e-10); a ground truth that is already
    matched and no crowd is passed over; the scan stops when a regular match exists and the ignored ground truths begin; a
    candidate must not be below the best so far, so among equal IoUs the last one wins; a crowd can be matched again.  A detection
    takes its match's ignore flag; an unmatched one is ignored iff it is outside the area range."""
    counts = np.asarray(counts)
    gt_ignore, dt_out, iscrowd, thrs, order, ig_sorted, A, D, G = _match_inputs(counts, gt_ignore, iscrowd, dt_out, thrs)
    ious = seq_iou(counts)
    n = thrs.shape[0]
    dtm, gtm = np.zeros((A, n, D), dtype=np.int32), np.zeros((A, n, G), dtype=np.int32)
    dtig = np.zeros((A, n, D), dtype=bool)
    for a in range(A):
        o, ig = order[a].tolist(), ig_sorted[a].tolist()
        crowd = iscrowd[order[a]].tolist()
        iou_a = ious[:, order[a]].tolist() if G else [[] for _ in range(D)]
        for ti, t in enumerate(thrs.tolist()):
            taken = [False] * G
            for d in range(D):
                best, m = min(t, 1 - 1e-10), -1
                row = iou_a[d]
                for gi in range(G):
                    if taken[gi] and not crowd[gi]:
                        continue
                    if m > -1 and not ig[m] and ig[gi]:
                        break
                    if row[gi] < best:
                        continue
                    best, m = row[gi], gi
                if m == -1:
                    continue
                dtig[a, ti, d] = ig[m]
                dtm[a, ti, d] = o[m] + 1
                gtm[a, ti, m] = d + 1
                taken[m] = True
        dtig[a] |= (dtm[a] == 0) & dt_out[a][None, :]
    return {"gt_order": order, "gt_ignore": ig_sorted, "dt_match": dtm, "gt_match": gtm, "dt_ignore": dtig}


def accumulate(eval_imgs: Sequence[Optional[Dict[str, Any]]], params: Params, n_cats: int, n_vids: int) -> Dict[str, np.ndarray]:
    """Precision (thrs, recThrs, cats, ranges, maxDets), recall (thrs, cats, ranges, maxDets) and the scores at the recall
    thresholds from the per-group results, ordered category-major, then area range, then video.  -1 marks a setting without a
    regular ground truth."""
    thrs, rec = np.asarray(params.iouThrs), np.asarray(params.recThrs)
    T, R, K, A, M = len(thrs), len(rec), n_cats, len(params.areaRng), len(params.maxDets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            base = (k * A + a) * n_vids
            E = [e for e in eval_imgs[base:base + n_vids] if e is not None]
            if not E:
                continue
            gt_ig = np.concatenate([np.asarray(e["gtIgnore"]) for e in E])
            npig = int(np.count_nonzero(gt_ig == 0))
            if npig == 0:
                continue
            for m, max_det in enumerate(params.maxDets):
                sc = np.concatenate([np.asarray(e["dtScores"][:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                sc_sorted = sc[inds]
                dtm = np.concatenate([e["dtMatches"][:, :max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, :max_det] for e in E], axis=1)[:, inds]
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    q, ss = [0.0] * R, np.zeros(R)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):                     # the precision envelope, right to left
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, rec, side="left")):
                        if pi >= nd:                                   # recall never gets here: the rest stays 0
                            break
                        q[ri], ss[ri] = pr[pi], sc_sorted[pi]
                    precision[t, :, k, a, m], scores[t, :, k, a, m] = np.array(q), ss
    return {"precision": precision, "recall": recall, "scores": scores, "counts": [T, R, K, A, M]}


def summarize(ev: Dict[str, np.ndarray], params: Params) -> np.ndarray:
    """The 12 figures (``METRICS``) in [0, 1]: the mean over the entries > -1, or -1 when there is none."""
    thrs = np.asarray(params.iouThrs)

    def one(ap, thr=None, rng="all", max_det=None):
        a = [i for i, l in enumerate(params.areaRngLbl) if l == rng]
        m = [i for i, v in enumerate(params.maxDets) if v == (params.maxDets[-1] if max_det is None else max_det)]
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    md = params.maxDets
    return np.array([one(1, max_det=100), one(1, 0.5, max_det=md[2]), one(1, 0.75, max_det=md[2]), one(1, rng="small", max_det=md[2]),
                     one(1, rng="medium", max_det=md[2]), one(1, rng="large", max_det=md[2]), one(0, max_det=md[0]),
                     one(0, max_det=md[1]), one(0, max_det=md[2]), one(0, rng="small", max_det=md[2]),
                     one(0, rng="medium", max_det=md[2]), one(0, rng="large", max_det=md[2])], dtype=np.float64)


# --------------------------------------------------------------------------------------------------------------------
# device path (csrc/vis_eval.hip)
# --------------------------------------------------------------------------------------------------------------------
def _is_hip(x) -> bool:
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def bits_pack_device(x: torch.Tensor, threshold: Optional[float] = None, values: Optional[Sequence[int]] = None,
                     planes: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``bits_pack`` on the HIP device: (bit-planes int64 (n, nb, w) holding the 64-bit words, areas int32 (n,)), both on the device.
    ``x``: bool / uint8 / float32 with ``threshold`` / uint8 index map with ``values``, as for ``vos_metrics.jf_counts_device``."""
    from . import _lib
    from .vos_metrics import _Source
    who = "bits_pack_device"
    dev = getattr(x, "device", None)
    _lib.require_hip(dev, who)
    if x.dim() >= 2 and x.numel() == 0 and x.shape[-1] > 0 and x.shape[-2] > 0:
        h, w = int(x.shape[-2]), int(x.shape[-1])
        return torch.zeros((0, (h + 63) // 64, w), dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    S = _Source(who, x, threshold, values, planes, dev)
    h, w, n = S.h, S.w, S.n
    if h * w >= 1 << 31:
        raise _lib.SamptError(f"{who}: h * w must be below 2^31; got {h} x {w}")
    nb = (h + 63) // 64
    lib = _lib.load()
    with _lib.device_guard(dev):
        bits = torch.empty((n, nb, w), dtype=torch.int64, device=dev)
        area = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            _lib.check(lib.sampt_bits_pack(*S.args(0), n, h, w, _lib.ptr(bits), _lib.ptr(area), _lib.stream_ptr()), "sampt_bits_pack")
    return bits, area


def rle_decode_device(counts_list: Sequence[Sequence[int]], h: int, w: int, device, as_bytes: bool = False):
    """``rle_decode`` on the HIP device: the runs are uploaded as one array, the planes are built there.  Returns (bit-planes int64
    (n, nb, w), areas int32, status int32) on the device, and with ``as_bytes`` a fourth tensor: the masks as uint8 (n, h, w)."""
    from . import _lib
    who = "rle_decode_device"
    dev = torch.device(device)
    _lib.require_hip(dev, who)
    if h <= 0 or w <= 0 or h * w >= 1 << 31:
        raise _lib.SamptError(f"{who}: 0 < h * w < 2^31 is required; got {h} x {w}")
    n, nb = len(counts_list), (h + 63) // 64
    arrs = [np.asarray(c, dtype=np.int64).reshape(-1) for c in counts_list]
    for i, c in enumerate(arrs):
        if c.size and (int(c.min()) < 0 or int(c.max()) >= 1 << 32):
            raise _lib.SamptError(f"{who}: mask {i} has a run outside 0 .. 2^32 - 1")
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([c.size for c in arrs]) if n else []
    total = int(offsets[n])
    flat = (np.concatenate(arrs) if total else np.zeros(0, dtype=np.int64)).astype(np.uint32)
    lib = _lib.load()
    with _lib.device_guard(dev):
        bits = torch.empty((n, nb, w), dtype=torch.int64, device=dev)
        area = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        out = [bits, area, status]
        if n:
            counts_d = torch.from_numpy(np.ascontiguousarray(flat).view(np.int32)).to(dev) if total else \
                torch.zeros(1, dtype=torch.int32, device=dev)
            offsets_d = torch.from_numpy(offsets).to(dev)
            ws = _lib.workspace("sampt_rle_decode_workspace_bytes", dev, total)
            _lib.check(lib.sampt_rle_decode_bits(_lib.ptr(counts_d), _lib.ptr(offsets_d), n, total, h, w, _lib.ptr(bits), _lib.ptr(area),
                                                 _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "sampt_rle_decode_bits")
        if as_bytes:
            by = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
            if n:
                _lib.check(lib.sampt_bits_unpack(_lib.ptr(bits), n, h, w, _lib.ptr(by), _lib.stream_ptr()), "sampt_bits_unpack")
            out.append(by)
    return tuple(out)


def _plane_table(who, what, planes, n_planes) -> np.ndarray:
    from . import _lib
    p = planes.detach().cpu().numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    if p.ndim != 2 or (p.size and p.dtype.kind not in "iu"):
        raise _lib.SamptError(f"{who}: {what} must be an integer table (items, frames)")
    if p.size and (int(p.min()) < -1 or int(p.max()) >= n_planes):
        raise _lib.SamptError(f"{who}: {what} outside -1 .. {n_planes - 1}")
    return np.ascontiguousarray(p, dtype=np.int32)


def seq_iou_counts_device(dt_bits: torch.Tensor, dt_area: torch.Tensor, dt_planes, gt_bits: torch.Tensor, gt_area: torch.Tensor,
                          gt_planes, h: int, w: int) -> torch.Tensor:
    """``seq_iou_counts`` on the HIP device from bit-planes (``bits_pack_device`` / ``rle_decode_device``): int64 (D, G, 2) there."""
    from . import _lib
    who = "seq_iou_counts_device"
    dev = dt_bits.device
    _lib.require_hip(dev, who)
    nb = (h + 63) // 64
    for b, a, name in ((dt_bits, dt_area, "dt"), (gt_bits, gt_area, "gt")):
        if b.device != dev or a.device != dev or b.dtype != torch.int64 or a.dtype != torch.int32 or b.dim() != 3 or \
                tuple(b.shape[1:]) != (nb, w) or a.shape != (b.shape[0],):
            raise _lib.SamptError(f"{who}: {name} bit-planes int64 (n, {nb}, {w}) with areas int32 (n,) on {dev} are required")
    dp = _plane_table(who, "dt_planes", dt_planes, int(dt_bits.shape[0]))
    gp = _plane_table(who, "gt_planes", gt_planes, int(gt_bits.shape[0]))
    D, G = dp.shape[0], gp.shape[0]
    if D == 0 or G == 0:
        return torch.zeros((D, G, 2), dtype=torch.int64, device=dev)
    T = dp.shape[1]
    if gp.shape[1] != T or T == 0:
        raise _lib.SamptError(f"{who}: plane tables of one positive frame count are required; got {dp.shape} and {gp.shape}")
    lib = _lib.load()
    ws_bytes = _lib.workspace_bytes("sampt_seq_iou_workspace_bytes", D, G, T, h, w)
    if ws_bytes == 0:
        raise _lib.SamptError(f"{who}: bad shape D = {D}, G = {G}, T = {T}, {h} x {w}")
    with _lib.device_guard(dev):
        dpd, gpd = torch.from_numpy(dp).to(dev), torch.from_numpy(gp).to(dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((D, G, 2), dtype=torch.int64, device=dev)
        _lib.check(lib.sampt_seq_iou_counts(_lib.ptr(dt_bits.contiguous()), _lib.ptr(dt_area.contiguous()), _lib.ptr(dpd), D,
                                            int(dt_bits.shape[0]), _lib.ptr(gt_bits.contiguous()), _lib.ptr(gt_area.contiguous()),
                                            _lib.ptr(gpd), G, int(gt_bits.shape[0]), T, h, w, _lib.ptr(out), _lib.ptr(ws), ws_bytes,
                                            _lib.stream_ptr()), "sampt_seq_iou_counts")
    return out


def match_video_device(counts: torch.Tensor, gt_ignore, iscrowd, dt_out, thrs) -> Dict[str, np.ndarray]:
    """``match_video`` on the HIP device; ``counts`` is the tensor ``seq_iou_counts_device`` returns.  Only the tables reach the host."""
    from . import _lib
    who = "match_video_device"
    dev = counts.device
    _lib.require_hip(dev, who)
    if counts.dtype != torch.int64:
        raise _lib.SamptError(f"{who}: counts must be int64; got {counts.dtype}")
    gt_ignore, dt_out, iscrowd, thrs, order, ig_sorted, A, D, G = _match_inputs(counts, gt_ignore, iscrowd, dt_out, thrs)
    n = thrs.shape[0]
    if not 1 <= n <= MAX_DEVICE_THRS or G > MAX_DEVICE_GT or A < 1:
        raise _lib.SamptError(f"{who}: 1 .. {MAX_DEVICE_THRS} thresholds, at most {MAX_DEVICE_GT} ground truths and at least one "
                              f"area range are required; got {n}, {G}, {A}")
    if D == 0 or G == 0:                                               # nothing to match: an unmatched detection is ignored iff out of range
        return {"gt_order": order, "gt_ignore": ig_sorted, "dt_match": np.zeros((A, n, D), dtype=np.int32),
                "gt_match": np.zeros((A, n, G), dtype=np.int32), "dt_ignore": np.repeat(dt_out[:, None, :], n, axis=1)}
    lib = _lib.load()
    with _lib.device_guard(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        thr_d, ord_d = up(thrs), up(order)
        ig_d, cr_d, out_d = up(ig_sorted.astype(np.uint8)), up(iscrowd.astype(np.uint8)), up(dt_out.astype(np.uint8))
        dtm = torch.empty((A, n, D), dtype=torch.int32, device=dev)
        gtm = torch.empty((A, n, G), dtype=torch.int32, device=dev)
        dtig = torch.empty((A, n, D), dtype=torch.uint8, device=dev)
        _lib.check(lib.sampt_vis_match(_lib.ptr(counts.contiguous()), D, G, A, n, _lib.ptr(thr_d), _lib.ptr(ord_d), _lib.ptr(ig_d),
                                       _lib.ptr(cr_d), _lib.ptr(out_d), _lib.ptr(dtm), _lib.ptr(gtm), _lib.ptr(dtig), _lib.stream_ptr()),
                   "sampt_vis_match")
        return {"gt_order": order, "gt_ignore": ig_sorted, "dt_match": dtm.cpu().numpy(), "gt_match": gtm.cpu().numpy(),
                "dt_ignore": dtig.cpu().numpy().astype(bool)}


# --------------------------------------------------------------------------------------------------------------------
# the evaluator
# --------------------------------------------------------------------------------------------------------------------
class _Stack:
    """A stack of mask sequences of one video, (N, T, H, W): a tensor or array (bool / uint8, or float with a threshold)."""

    def __init__(self, data, threshold):
        self.data, self.threshold = data, threshold


def _avg_area(areas) -> float:
    nz = [a for a in areas if a]                                       # (None and 0 are both left out)
    return float(np.array(nz).mean()) if nz else 0.0


class YTVISEval:
    """AP / AR of video instance segmentation results against YouTube-VIS style annotations.

    ``dataset``: an annotation dict (``videos`` with ``id`` / ``height`` / ``width``, ``categories`` with ``id``, ``annotations``
    with ``id`` >= 1, ``video_id``, ``category_id``, ``iscrowd``, ``segmentations`` — per frame an uncompressed or compressed RLE
    record or ``None`` — and ``areas``); videos can also be added one by one with ``add_video``.  Detections arrive through
    ``process`` (what the reference's ``YTVISEvaluator.process`` receives), ``add_results`` (the list ``instances_to_ytvis_json``
    returns) or ``add_video``.  ``evaluate()``, ``accumulate()``, ``summarize()`` and ``results()`` follow the reference.

    With ``device`` a HIP device, or with any mask tensor on one, the masks are packed / decoded, intersected and matched there
    (csrc/vis_eval.hip) and no mask is downloaded; otherwise everything runs on the host.  Both give identical results."""

    def __init__(self, dataset: Optional[Dict[str, Any]] = None, device=None, params: Optional[Params] = None,
                 categories: Optional[Sequence[int]] = None):
        self.params = params or Params()
        self.device = None if device is None else torch.device(device)
        self.videos: Dict[Any, Tuple[int, int]] = {}
        self._cats = set(categories or [])
        self._gts: Dict[Any, List[Dict[str, Any]]] = defaultdict(list)
        self._dts: Dict[Any, List[Dict[str, Any]]] = defaultdict(list)
        self._n_dt = 0
        self.evalImgs: List[Optional[Dict[str, Any]]] = []
        self.ious: Dict[Tuple[Any, Any], Any] = {}
        self.eval: Dict[str, Any] = {}
        self.stats = None
        if dataset is not None:
            for v in dataset["videos"]:
                self.videos[v["id"]] = (int(v["height"]), int(v["width"]))
            self._cats |= {c["id"] for c in dataset.get("categories", [])}
            for ann in dataset.get("annotations", []):
                self._add_gt(ann["video_id"], ann)

    # ------------------------------------------------------------------------------------------------------ input
    def _add_gt(self, vid, ann):
        if vid not in self.videos:
            raise ValueError(f"annotation {ann.get('id')} names the unknown video {vid}")
        if not isinstance(ann.get("id"), (int, np.integer)) or ann["id"] < 1:
            raise ValueError(f"ground-truth ids must be integers >= 1 (0 means unmatched); got {ann.get('id')!r}")
        g = {"id": int(ann["id"]), "category_id": ann["category_id"], "iscrowd": int(ann.get("iscrowd", 0))}
        if "masks" in ann:
            g["stack"], g["index"] = _Stack(ann["masks"][None], ann.get("threshold")), 0
        else:
            g["segmentations"] = self._check_segs(vid, ann["segmentations"], f"annotation {ann['id']}")
        g["areas"] = None if ann.get("areas") is None else list(ann["areas"])
        self._gts[vid].append(g)

    def _check_segs(self, vid, segs, what):
        h, w = self.videos[vid]
        out = []
        for s in segs:
            if not s:
                out.append(None)
                continue
            if isinstance(s, (list, tuple)):
                raise ValueError(f"{what}: polygon segmentations are not supported; convert them to RLE first")
            if [int(v) for v in s["size"]] != [h, w]:
                raise ValueError(f"{what}: RLE size {list(s['size'])} does not fit the video's {h} x {w}")
            out.append(s)
        return out

    def _new_dt(self, vid, score, cat, **src):
        self._n_dt += 1
        self._dts[vid].append(dict(id=self._n_dt, score=float(score), category_id=cat, **src))

    def add_video(self, video: Dict[str, Any], gts: Sequence[Dict[str, Any]], dts: Sequence[Dict[str, Any]]):
        """One video with its ground truths and detections.  ``video``: ``id``, ``height``, ``width``.  A ground truth has ``id``,
        ``category_id``, ``iscrowd`` and ``segmentations`` + ``areas``, or ``masks`` (T, H, W) (the areas are then taken from the
        masks).  A detection has ``score``, ``category_id`` and ``segmentations``, ``masks`` (T, H, W) or ``logits`` (T, H, W) with
        ``threshold`` (default 0)."""
        vid = video["id"]
        self.videos[vid] = (int(video["height"]), int(video["width"]))
        for g in gts:
            self._add_gt(vid, g)
        for d in dts:
            if "segmentations" in d:
                self._new_dt(vid, d["score"], d["category_id"], segmentations=self._check_segs(vid, d["segmentations"], "a detection"))
            elif "masks" in d:
                self._new_dt(vid, d["score"], d["category_id"], stack=_Stack(d["masks"][None], None), index=0)
            else:
                self._new_dt(vid, d["score"], d["category_id"], stack=_Stack(d["logits"][None], float(d.get("threshold", 0.0))), index=0)

    def add_results(self, results: Sequence[Dict[str, Any]]):
        """Entries ``{"video_id", "score", "category_id", "segmentations"}``: the list ``instances_to_ytvis_json`` returns."""
        for r in results:
            if r["video_id"] not in self.videos:
                raise ValueError(f"a result names the unknown video {r['video_id']}")
            self._new_dt(r["video_id"], r["score"], r["category_id"],
                         segmentations=self._check_segs(r["video_id"], r["segmentations"], "a result"))

    def process(self, inputs: Sequence[Dict[str, Any]], outputs: Dict[str, Any], use_logits: bool = False):
        """The detections of one video as ``SamBasedVisToVosAdapter`` returns them: ``pred_scores``, ``pred_labels`` and
        ``pred_rles``, or ``pred_masks`` (or, with ``use_logits``, ``pred_logits`` thresholded at 0) as a list of (T, H, W)
        tensors or one (N, T, H, W) tensor, on the device or the host."""
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        vid = inputs[0]["video_id"]
        if vid not in self.videos:
            raise ValueError(f"process: the unknown video {vid}")
        scores, labels = outputs["pred_scores"], outputs["pred_labels"]
        if "pred_rles" in outputs:
            for s, l, rles in zip(scores, labels, outputs["pred_rles"]):
                self._new_dt(vid, s, l, segmentations=self._check_segs(vid, rles, "a prediction"))
            return
        key, thr = ("pred_logits", 0.0) if use_logits else ("pred_masks", None)
        data = outputs[key]
        if not isinstance(data, (torch.Tensor, np.ndarray)):
            data = torch.stack([torch.as_tensor(m) for m in data]) if len(data) else torch.zeros((0, 0) + self.videos[vid])
        stack = _Stack(data, thr)
        for i, (s, l) in enumerate(zip(scores, labels)):
            self._new_dt(vid, s, l, stack=stack, index=i)

    # ------------------------------------------------------------------------------------------------- per video
    def _device_of(self, items):
        if self.device is not None:
            return self.device
        for it in items:
            if "stack" in it and _is_hip(it["stack"].data):
                return it["stack"].data.device
        return None

    def _planes(self, vid, items, dev):
        """The masks of ``items`` as planes: (planes, areas, table) — on the device bit-planes and an int32 tensor, on the host a
        bool stack and an int64 array; ``table`` int32 (items, T) with -1 for an absent frame."""
        h, w = self.videos[vid]
        chunks, areas, base, T = [], [], 0, None
        table: List[Optional[np.ndarray]] = [None] * len(items)
        stacks: Dict[int, Tuple[_Stack, int]] = {}
        for i, it in enumerate(items):
            if "stack" not in it:
                continue
            st = it["stack"]
            if tuple(st.data.shape[-2:]) != (h, w) or len(st.data.shape) != 4:
                raise ValueError(f"video {vid}: masks {tuple(st.data.shape)} do not fit (N, T, {h}, {w})")
            n, t = int(st.data.shape[0]), int(st.data.shape[1])
            if id(st) not in stacks:
                stacks[id(st)] = (st, base)
                if dev is not None:
                    x = st.data if isinstance(st.data, torch.Tensor) else torch.as_tensor(st.data)
                    x = x.to(dev)
                    if x.dtype.is_floating_point and x.dtype != torch.float32:
                        x = x.float()
                    b, a = bits_pack_device(x.reshape(n * t, h, w), threshold=st.threshold)
                else:
                    x = st.data.detach().cpu().numpy() if isinstance(st.data, torch.Tensor) else np.asarray(st.data)
                    x = x.reshape(n * t, h, w)
                    if x.dtype.kind == "f":
                        with np.errstate(invalid="ignore"):
                            b = x.astype(np.float32) > np.float32(st.threshold)
                    else:
                        b = x != 0
                    a = b.sum(axis=(1, 2)).astype(np.int64)
                chunks.append(b), areas.append(a)
                base += n * t
            table[i] = stacks[id(st)][1] + it["index"] * t + np.arange(t, dtype=np.int32)
        recs, where = [], []
        for i, it in enumerate(items):
            if "stack" in it:
                continue
            row = np.full(len(it["segmentations"]), -1, dtype=np.int32)
            for f, s in enumerate(it["segmentations"]):
                if s is not None:
                    row[f] = base + len(recs)
                    recs.append(_counts_of(s))
                    where.append(f"{it.get('id')} frame {f}")
            table[i] = row
        if recs:
            if dev is not None:
                b, a, status = rle_decode_device(recs, h, w, dev)
                status = status.cpu().numpy()
            else:
                b, a, status = rle_decode(recs, h, w)
                b, a = unpack_bits(b, h), a.astype(np.int64)
            if status.any():
                raise ValueError(f"video {vid}: the RLE of item {where[int(np.flatnonzero(status)[0])]} does not cover {h} x {w}")
            chunks.append(b), areas.append(a)
        for row in table:
            T = len(row) if T is None else T
            if len(row) != T:
                raise ValueError(f"video {vid}: the items have {T} and {len(row)} frames")
        tab = np.stack(table).astype(np.int32) if table else np.zeros((0, 0), dtype=np.int32)
        if dev is not None:
            nb = (h + 63) // 64
            planes = torch.cat(chunks) if len(chunks) > 1 else (chunks[0] if chunks else torch.zeros((0, nb, w), dtype=torch.int64, device=dev))
            area = torch.cat(areas) if len(areas) > 1 else (areas[0] if areas else torch.zeros(0, dtype=torch.int32, device=dev))
        else:
            planes = np.concatenate(chunks) if chunks else np.zeros((0, h, w), dtype=bool)
            area = np.concatenate(areas) if areas else np.zeros(0, dtype=np.int64)
        return planes, area, tab

    def _evaluate_video(self, vid, cat_ids):
        p = self.params
        gts, dts = self._gts.get(vid, []), self._dts.get(vid, [])
        dev = self._device_of(list(gts) + list(dts))
        h, w = self.videos[vid]
        gpl, garea, gtab = self._planes(vid, gts, dev)
        dpl, darea, dtab = self._planes(vid, dts, dev)
        garea_h = garea.cpu().numpy() if dev is not None else garea
        darea_h = darea.cpu().numpy() if dev is not None else darea
        for items, tab, ar in ((gts, gtab, garea_h), (dts, dtab, darea_h)):
            for it, row in zip(items, tab):
                own = it.get("areas") if items is gts else None            # detections always take their areas from their masks
                it["avg_area"] = _avg_area(own if own is not None else [int(ar[q]) if q >= 0 else None for q in row])
        out = {}
        for cat in cat_ids:
            gi = [i for i, g in enumerate(gts) if g["category_id"] == cat]
            di = [i for i, d in enumerate(dts) if d["category_id"] == cat]
            if not gi and not di:
                out[cat] = None
                continue
            di = [di[i] for i in np.argsort([-dts[i]["score"] for i in di], kind="mergesort")][:p.maxDets[-1]]
            G, D = len(gi), len(di)
            T = gtab.shape[1] if len(gts) else dtab.shape[1]
            gt_tab, dt_tab = gtab[gi].reshape(G, T), dtab[di].reshape(D, T)
            if dev is not None:
                counts = seq_iou_counts_device(dpl, darea, dt_tab, gpl, garea, gt_tab, h, w)
                counts_h = counts.cpu().numpy()
            else:
                counts = counts_h = seq_iou_counts(dpl, dt_tab, gpl, gt_tab)
            g_avg, d_avg = np.array([gts[i]["avg_area"] for i in gi]), np.array([dts[i]["avg_area"] for i in di])
            crowd = np.array([bool(gts[i]["iscrowd"]) for i in gi], dtype=bool)
            rng = np.asarray(p.areaRng, dtype=np.float64)
            g_ig = crowd[None, :] | (g_avg[None, :] < rng[:, :1]) | (g_avg[None, :] > rng[:, 1:]) if G else np.zeros((len(rng), 0), dtype=bool)
            d_out = (d_avg[None, :] < rng[:, :1]) | (d_avg[None, :] > rng[:, 1:]) if D else np.zeros((len(rng), 0), dtype=bool)
            m = (match_video_device if dev is not None else match_video)(counts, g_ig, crowd, d_out, p.iouThrs)
            out[cat] = dict(ious=seq_iou(counts_h) if D else [], gi=gi, di=di, match=m)
        return out

    # -------------------------------------------------------------------------------------------------- protocol
    def evaluate(self):
        """Per (category, area range, video) results in ``evalImgs`` (category-major, as the reference orders them) and the IoU
        matrices in ``ious``."""
        p = self.params
        p.maxDets = sorted(p.maxDets)
        self.vidIds = sorted(set(self.videos))
        self.catIds = sorted(self._cats | {g["category_id"] for gs in self._gts.values() for g in gs})
        per_vid = {v: self._evaluate_video(v, self.catIds) for v in self.vidIds}
        self.ious = {(v, c): ([] if per_vid[v][c] is None else per_vid[v][c]["ious"]) for v in self.vidIds for c in self.catIds}
        self.evalImgs = []
        for c in self.catIds:
            for a, rng in enumerate(p.areaRng):
                for v in self.vidIds:
                    r = per_vid[v][c]
                    if r is None:
                        self.evalImgs.append(None)
                        continue
                    gts, dts, m = [self._gts[v][i] for i in r["gi"]], [self._dts[v][i] for i in r["di"]], r["match"]
                    gt_ids = np.array([g["id"] for g in gts], dtype=np.float64)
                    dt_ids = np.array([d["id"] for d in dts], dtype=np.float64)
                    order = m["gt_order"][a]
                    dtm, gtm = m["dt_match"][a], m["gt_match"][a]
                    self.evalImgs.append({
                        "video_id": v, "category_id": c, "aRng": list(rng), "maxDet": p.maxDets[-1],
                        "dtIds": [d["id"] for d in dts], "gtIds": [gts[i]["id"] for i in order],
                        "dtMatches": np.where(dtm > 0, gt_ids[np.maximum(dtm - 1, 0)] if len(gts) else 0.0, 0.0),
                        "gtMatches": np.where(gtm > 0, dt_ids[np.maximum(gtm - 1, 0)] if len(dts) else 0.0, 0.0),
                        "dtScores": [d["score"] for d in dts], "gtIgnore": m["gt_ignore"][a].astype(np.int64),
                        "dtIgnore": m["dt_ignore"][a]})
        return self.evalImgs

    def accumulate(self):
        if not self.evalImgs:
            raise RuntimeError("run evaluate() first")
        self.eval = accumulate(self.evalImgs, self.params, len(self.catIds), len(self.vidIds))
        return self.eval

    def summarize(self) -> np.ndarray:
        if not self.eval:
            raise RuntimeError("run accumulate() first")
        self.stats = summarize(self.eval, self.params)
        return self.stats

    def results(self) -> Dict[str, float]:
        """``{"AP": .., "AP50": .., ...}`` in percent, ``nan`` where a figure is undefined (-1); runs the missing steps."""
        if self.stats is None:
            if not self.eval:
                if not self.evalImgs:
                    self.evaluate()
                self.accumulate()
            self.summarize()
        return {k: float(self.stats[i] * 100) if self.stats[i] >= 0 else float("nan") for i, k in enumerate(METRICS)}


def evaluate_ytvis(dataset_dict: Dict[str, Any], results_list: Sequence[Dict[str, Any]], device=None,
                   params: Optional[Params] = None) -> Dict[str, float]:
    """The 12 figures of a YTVIS annotation dict and the results list ``instances_to_ytvis_json`` returns; with ``device`` a HIP
    device the masks are decoded, intersected and matched there."""
    ev = YTVISEval(dataset_dict, device=device, params=params)
    ev.add_results(results_list)
    return ev.results()
