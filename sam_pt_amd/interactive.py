"""Click selection of the interactive point-correction simulator (reference: sam_pt/modeling/sam_pt_interactive.py:330-395 the
click rule, :678-729 ``extract_largest_cluster_points``), on the host and on the HIP device (csrc/dbscan.hip).

The reference picks every added point with ``sklearn.cluster.DBSCAN(eps = 2.4 H W / 18000, min_samples = 10)`` over up to 18 000
error pixels, takes the largest cluster (the whole mask if that has fewer than 180 points) and runs
``sklearn_extra.cluster.KMedoids`` on up to 720 of its points.

**DBSCAN, order-free.**  scikit-learn expands clusters sequentially, but its labels have a restatement without any order:

* a point is core iff its neighbour count, itself included, is at least ``min_samples``;
* clusters are the connected components of the core points under the neighbour relation;
* a cluster's id is the rank of its smallest core index among all clusters' smallest core indices;
* a non-core point with at least one core neighbour takes the smallest cluster id among its core neighbours;
* everything else is -1.

``dbscan_labels`` is that restatement in NumPy (pinned with ``==`` on scikit-learn's labels, tests/test_interactive_cpu.py) and
the oracle of ``dbscan_labels_device``.  Pixel coordinates are integers, so a pair is a neighbour iff its exact integer squared
distance is ``<= r2 = floor(eps * eps)`` (float64, computed once).  That equals scikit-learn's ``dist <= eps`` unless ``eps^2``
lies within rounding distance of an integer; ``eps_to_r2`` refuses such an ``eps`` (fractional part of ``eps^2`` below 1e-6 or
above 1 - 1e-6) instead of guessing.

**k-medoids** is ``query_points.kmedoids_alternate`` / ``kmedoids_alternate_device`` (scikit-learn-extra is absent: parity
unpinned, as for the query points).

**RNG.**  ``extract_largest_cluster_points`` consumes the global generator exactly as the reference does: two ``torch.randperm``
draws on the host, each of the length of the pixel list it permutes, whatever device does the rest.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .query_points import kmedoids_alternate, kmedoids_alternate_device

_BIG = np.iinfo(np.int32).max

# category bits of ``frame_state`` (one byte per point; an invisible point is 0)
CAT_VISIBLE, CAT_POSITIVE, CAT_CORRECT, CAT_TP, CAT_TN, CAT_FP, CAT_FN = 1, 2, 4, 8, 16, 32, 64


def eps_to_r2(eps: float) -> int:
    """floor(eps^2) in float64: the integer bound on squared pixel distances that ``dist <= eps`` amounts to.  Refuses an ``eps``
    whose square is within 1e-6 of an integer, where one rounding could move a pair across the bound."""
    e2 = float(eps) * float(eps)
    if not math.isfinite(e2) or e2 < 0:
        raise ValueError(f"eps must be finite; got {eps}")
    frac = e2 - math.floor(e2)
    if frac < 1e-6 or frac > 1 - 1e-6:
        raise ValueError(f"eps = {eps!r}: eps^2 = {e2!r} is within 1e-6 of an integer, so 'd^2 <= floor(eps^2)' and 'd <= eps' may differ "
                         "by one rounding; nudge eps")
    return int(min(math.floor(e2), _BIG))


def _int_pixels(X) -> np.ndarray:
    X = np.asarray(X)
    Xi = X.astype(np.int64)
    if X.ndim != 2 or X.shape[1] != 2 or len(X) == 0 or not (Xi == X).all() or Xi.min() < 0 or Xi.max() > 32767:
        raise ValueError("points must be a non-empty (n, 2) array of integer pixel coordinates in 0 .. 32767")
    return Xi.astype(np.int32)


def dbscan_labels(X, eps: float, min_samples: int) -> np.ndarray:
    """Labels of ``sklearn.cluster.DBSCAN(eps, min_samples).fit(X).labels_`` for integer pixel coordinates X (n, 2), by the
    order-free restatement of the module docstring.  Exact, with the points bucketed into square cells so that n = 18 000 takes
    a fraction of a second: a cell's side s satisfies 2 (s - 1)^2 <= r2, so all points of one cell are mutual neighbours (its core
    points share a component), and only cells at most ``reach`` apart can hold a neighbouring pair."""
    P = _int_pixels(X).astype(np.int64)
    n, r2 = len(P), eps_to_r2(eps)
    s = math.isqrt(r2 // 2) + 1
    reach = 0 if r2 == 0 else (math.isqrt(r2) - 1) // s + 1          # k cells apart: coordinates differ by >= (k - 1) s + 1
    ci, cj = P[:, 0] // s, P[:, 1] // s
    ncj = int(cj.max()) + 1
    key = ci * ncj + cj
    order = np.argsort(key, kind="stable")
    ukeys, start = np.unique(key[order], return_index=True)
    cells = {int(k): order[a:b] for k, a, b in zip(ukeys, start, list(start[1:]) + [n])}
    # every (cell, nearby cell) pair with its neighbour matrix; neighbour counts on the way
    count = np.zeros(n, dtype=np.int64)
    pairs = []
    for ka, ia in cells.items():
        ai, aj = divmod(ka, ncj)
        for di in range(-reach, reach + 1):
            for dj in range(-reach, reach + 1):
                if not 0 <= aj + dj < ncj:
                    continue
                ib = cells.get((ai + di) * ncj + aj + dj)
                if ib is None:
                    continue
                d = P[ia][:, None, :] - P[ib][None, :, :]
                near = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] <= r2
                count[ia] += near.sum(axis=1)
                pairs.append((ia, ib, near))
    core = count >= min_samples
    # components of the core points: one node per cell that holds a core point (its smallest core index), joined when any core
    # pair across the two cells is a neighbour pair; roots are kept at the smaller index
    parent = {}
    rep = {}
    for k, ia in cells.items():
        c = ia[core[ia]]
        if len(c):
            rep[k] = int(c.min())
            parent[rep[k]] = rep[k]

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    cell_of = {int(ia[0]): k for k, ia in cells.items()}
    for ia, ib, near in pairs:
        ka, kb = cell_of[int(ia[0])], cell_of[int(ib[0])]
        if ka < kb and ka in rep and kb in rep and near[np.ix_(core[ia], core[ib])].any():
            ra, rb = find(rep[ka]), find(rep[kb])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.full(n, -1, dtype=np.int64)
    for k, ia in cells.items():
        if k in rep:
            root[ia[core[ia]]] = find(rep[k])
    roots = np.unique(root[core])                                    # ascending smallest core indices = cluster ids in order
    out = np.full(n, -1, dtype=np.int64)
    out[core] = np.searchsorted(roots, root[core])
    # border points: the smallest cluster id among the core neighbours
    bmin = np.full(n, _BIG, dtype=np.int64)
    for ia, ib, near in pairs:
        rows, cols = ~core[ia], core[ib]
        if rows.any() and cols.any():
            m = np.where(near[np.ix_(rows, cols)], out[ib[cols]][None, :], _BIG).min(axis=1)
            bmin[ia[rows]] = np.minimum(bmin[ia[rows]], m)
    border = ~core & (bmin != _BIG)
    out[border] = bmin[border]
    return out


class LargestCluster(NamedTuple):
    cluster_id: int          # the chosen cluster, or -1: "use the whole mask" (no cluster, or the largest is below min_points)
    size: int                # size of the largest cluster (0 without one)
    n_clusters: int
    members: np.ndarray      # ascending indices of the chosen cluster (empty with cluster_id == -1)


def largest_cluster(labels, min_points: int) -> LargestCluster:
    """``Counter(labels).most_common(1)`` after -1 is removed: the largest cluster, on equal size the one that appears first (whose
    first member has the smallest index); below ``min_points`` (or without a cluster) the answer is "use the whole mask"."""
    labels = np.asarray(labels).astype(np.int64)
    ids, first, sizes = np.unique(labels[labels >= 0], return_index=True, return_counts=True)
    if len(ids) == 0:
        return LargestCluster(-1, 0, 0, np.empty(0, np.int64))
    first = np.array([int(np.argmax(labels == c)) for c in ids])
    best = int(np.lexsort((first, -sizes))[0])
    n_clusters = int(ids.max()) + 1
    if sizes[best] < min_points:
        return LargestCluster(-1, int(sizes[best]), n_clusters, np.empty(0, np.int64))
    return LargestCluster(int(ids[best]), int(sizes[best]), n_clusters, np.nonzero(labels == ids[best])[0])


# ---- device twins ----------------------------------------------------------------------------------------------------------------
def _dbscan_device_raw(xy: torch.Tensor, r2: int, min_samples: int):
    """xy: (n, 2) f32 on the HIP device -> (labels int32 [n] on the device, workspace).  No synchronisation."""
    from . import _lib
    lib = _lib.load()
    n = int(xy.shape[0])
    ws = _lib.workspace("sampt_dbscan_workspace_bytes", xy.device, n)
    labels = torch.empty(n, dtype=torch.int32, device=xy.device)
    _lib.check(lib.sampt_dbscan_labels(_lib.ptr(xy), n, int(r2), int(min_samples), _lib.ptr(labels), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr()), "sampt_dbscan_labels")
    return labels, ws


def _check_status(ws: torch.Tensor, who: str):
    from . import _lib
    status = int(ws[:4].view(torch.int32)[0].item())
    if status & 2:
        raise ValueError(f"{who}: points must be integer pixel coordinates in 0 .. 32767")
    if status:
        raise _lib.SamptError(f"{who}: the union-find hit its hard step cap (status {status}); the labels are not valid")


def dbscan_labels_device(X, eps: float, min_samples: int, device) -> np.ndarray:
    """``dbscan_labels`` on the HIP device (csrc/dbscan.hip): the same array, element for element."""
    from . import _lib
    device = torch.device(device)
    _lib.require_hip(device, "dbscan_labels_device")
    r2 = eps_to_r2(eps)
    with _lib.device_guard(device):
        xy = torch.as_tensor(X).detach().to(torch.float32).contiguous().to(device)
        if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] == 0:
            raise ValueError("points must be a non-empty (n, 2) array")
        labels, ws = _dbscan_device_raw(xy, r2, min_samples)
        out = labels.cpu().numpy().astype(np.int64)
        _check_status(ws, "dbscan_labels_device")
        return out


def _largest_device_raw(labels: torch.Tensor, min_points: int, ws: Optional[torch.Tensor] = None):
    from . import _lib
    lib = _lib.load()
    n = int(labels.shape[0])
    if ws is None:
        ws = _lib.workspace("sampt_dbscan_workspace_bytes", labels.device, n)
    members = torch.empty(n, dtype=torch.int32, device=labels.device)
    info = torch.empty(4, dtype=torch.int32, device=labels.device)
    _lib.check(lib.sampt_dbscan_largest(_lib.ptr(labels), n, int(min_points), _lib.ptr(members), _lib.ptr(info), _lib.ptr(ws), ws.numel(),
                                        _lib.stream_ptr()), "sampt_dbscan_largest")
    return members, info


def largest_cluster_device(labels, min_points: int, device) -> LargestCluster:
    """``largest_cluster`` on the HIP device (csrc/dbscan.hip: k_db_largest)."""
    from . import _lib
    device = torch.device(device)
    _lib.require_hip(device, "largest_cluster_device")
    with _lib.device_guard(device):
        lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(torch.int32).contiguous().to(device)
        members, info = _largest_device_raw(lab, min_points)
        cid, size, ncl, _ = info.cpu().tolist()
        mem = members[:size].cpu().numpy().astype(np.int64) if cid >= 0 else np.empty(0, np.int64)
        return LargestCluster(cid, size, ncl, mem)


def _is_hip(device) -> bool:
    return device is not None and torch.device(device).type == "cuda"


def extract_largest_cluster_points(mask: torch.Tensor, n_points_to_select: int, dbscan_points: int = 18000,
                                   db_largest_cluster_min_points: int = 180, kmedian_points: int = 720, device=None) -> torch.Tensor:
    """``n_points_to_select`` k-medoid centres, as (x, y) float32, of (720 random points of) the largest DBSCAN cluster of (18 000
    random points of) the mask, or of the whole mask if that cluster has fewer than 180 points (sam_pt_interactive.py:678-729).
    The two ``torch.randperm`` draws are the reference's (global generator, host, lengths of the lists they permute).  ``device``: a
    HIP device keeps the pixel list, the DBSCAN, the cluster choice and the k-medoids there (the mask may already live there); only
    the list lengths and the final points reach the host.  ``kmedian_points`` above 2048 or more than 64 points to select are beyond the
    device k-medoids and refused by name there.  The result equals the ``device=None`` path bit for bit."""
    H, W = int(mask.shape[0]), int(mask.shape[1])
    dbscan_eps = 2.4 * (H * W) / dbscan_points
    if _is_hip(device):
        from . import _lib
        device = torch.device(device)
        with _lib.device_guard(device):
            all_px = (mask.to(device) != 0).nonzero().float()                          # (row, col), row-major: torch's order
            n_all = int(all_px.shape[0])                                               # (the length: first figure the host needs)
            assert n_all > 0
            px = all_px[torch.randperm(n_all)[:dbscan_points].to(device)].contiguous()
            labels, ws = _dbscan_device_raw(px, eps_to_r2(dbscan_eps), 10)
            members, info = _largest_device_raw(labels, db_largest_cluster_min_points, ws)
            cid, size, _, _ = info.cpu().tolist()
            _check_status(ws, "extract_largest_cluster_points")
            pts = px[members[:size].long()] if cid >= 0 else all_px
            pts = pts[torch.randperm(int(pts.shape[0]))[:kmedian_points].to(device)].contiguous()
            if len(pts) > 2048 or n_points_to_select > 64:
                raise ValueError(f"extract_largest_cluster_points(device=...): the device k-medoids take at most 2048 points and 64 "
                                 f"clusters; got kmedian_points = {kmedian_points}, n_points_to_select = {n_points_to_select}")
            idx = kmedoids_alternate_device(pts, n_points_to_select, device)
            return pts[torch.as_tensor(idx, dtype=torch.long, device=device)].cpu().type(torch.float32).flip(1)
    mask = mask.cpu()
    px = (mask != 0).nonzero().float()
    px = px[torch.randperm(len(px))[:dbscan_points]]
    assert len(px) > 0
    best = largest_cluster(dbscan_labels(px.numpy(), dbscan_eps, 10), db_largest_cluster_min_points)
    pts = px[torch.from_numpy(best.members)] if best.cluster_id >= 0 else (mask != 0).nonzero().float()
    pts = pts[torch.randperm(len(pts))[:kmedian_points]]
    idx = kmedoids_alternate(pts.numpy(), n_points_to_select)
    return pts[torch.as_tensor(idx, dtype=torch.long)].type(torch.float32).flip(1)


# ---- frame state of the click rule ------------------------------------------------------------------------------------------------
class FrameState(NamedTuple):
    tp: int
    fn: int
    fp: int
    first_bad_negative: int      # index of the first incorrect visible negative point, -1 without one
    first_bad_positive: int
    categories: np.ndarray       # uint8 [n_points]: CAT_* bits at the rounded coordinate
    fn_mask: torch.Tensor        # bool / uint8 (H, W), on the device for the device twin
    fp_mask: torch.Tensor


def frame_state(logits: torch.Tensor, gt: torch.Tensor, xy: torch.Tensor, vis: torch.Tensor, labels: torch.Tensor) -> FrameState:
    """What the click rule reads of one frame (sam_pt_interactive.py:330-361), restated plainly: mask = logits > 0 against the
    ground truth, and per visible point the category at ``round().int()`` coordinates (half to even; -1 .. -size wraps as Python's
    indexing does; beyond that ``IndexError``, as ``tp_mask[y, x]`` raises)."""
    m, g = (logits > 0).cpu(), (gt != 0).cpu()
    H, W = m.shape
    tp_mask, tn_mask, fp_mask, fn_mask = m & g, ~m & ~g, m & ~g, ~m & g
    cats = np.zeros(len(labels), dtype=np.uint8)
    bad_neg = bad_pos = -1
    for p in range(len(labels)):
        if vis[p].item() != 1:
            continue
        positive = labels[p].item() == 1
        if not bool(torch.isfinite(xy[p]).all()):                  # (round().int() of a NaN is undefined; the kernel calls it off-frame)
            raise IndexError(f"point {p} has a coordinate that is not finite")
        x, y = xy[p].cpu().round().int().tolist()
        if not (-W <= x < W and -H <= y < H):
            raise IndexError(f"point {p} at ({x}, {y}) is off the {H} x {W} frame")
        tp, tn, fp, fn = (bool(a[y, x].item()) for a in (tp_mask, tn_mask, fp_mask, fn_mask))
        correct = (tp or fn) if positive else (tn or fp)
        cats[p] = (CAT_VISIBLE | CAT_POSITIVE * positive | CAT_CORRECT * correct | CAT_TP * tp | CAT_TN * tn | CAT_FP * fp | CAT_FN * fn)
        if not correct and positive and bad_pos < 0:
            bad_pos = p
        if not correct and not positive and bad_neg < 0:
            bad_neg = p
    return FrameState(int(tp_mask.sum()), int(fn_mask.sum()), int(fp_mask.sum()), bad_neg, bad_pos, cats, fn_mask, fp_mask)


def frame_state_device(logits: torch.Tensor, gt: torch.Tensor, xy: torch.Tensor, vis: torch.Tensor, labels: torch.Tensor) -> FrameState:
    """``frame_state`` on the HIP device (csrc/dbscan.hip: sampt_int_frame_state).  ``logits`` f32 (H, W) lives on the device; the
    FN / FP masks stay there as byte planes; 8 integers and one byte per point reach the host."""
    from . import _lib
    lib = _lib.load()
    device = logits.device
    _lib.require_hip(device, "frame_state_device")
    H, W = int(logits.shape[0]), int(logits.shape[1])
    n = int(labels.shape[0])
    with _lib.device_guard(device):
        lg = logits.to(torch.float32).contiguous()
        g = (gt.to(device) != 0).to(torch.uint8).contiguous()
        pxy = xy.reshape(n, 2).to(torch.float32).contiguous().to(device)
        pvis = vis.reshape(n).to(torch.float32).contiguous().to(device)
        plab = labels.reshape(n).to(torch.int32).contiguous().to(device)
        info = torch.empty(8, dtype=torch.int32, device=device)
        cat = torch.zeros(max(n, 1), dtype=torch.uint8, device=device)
        fn_mask, fp_mask = torch.empty_like(g), torch.empty_like(g)
        _lib.check(lib.sampt_int_frame_state(_lib.ptr(lg), _lib.ptr(g), H, W, _lib.ptr(pxy) if n else None, _lib.ptr(pvis) if n else None,
                                             _lib.ptr(plab) if n else None, n, _lib.ptr(info), _lib.ptr(cat), _lib.ptr(fn_mask),
                                             _lib.ptr(fp_mask), _lib.stream_ptr()), "sampt_int_frame_state")
        i = info.cpu().tolist()
        if i[5]:
            raise IndexError(f"a visible point's rounded coordinate is off the {H} x {W} frame")
        return FrameState(i[0], i[1], i[2], i[3], i[4], cat[:n].cpu().numpy(), fn_mask, fp_mask)
