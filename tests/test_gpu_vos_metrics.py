"""DAVIS J&F on the device (csrc/vos_metrics.hip) against the host restatement computed live: every comparison is ``==`` on the six
integer counts, and on J and F too, since both paths apply the same float64 formulas to the same integers."""
import functools
import math

import numpy as np
import pytest
import torch

from sam_pt_amd import vos_metrics as VM
from tests.test_amg_tail_cpu import offset_view, seeded_masks
from tests.test_vos_metrics_cpu import seeded_pair

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 2), (1, 2, 2), (2, 1, 2), (63, 5, 3), (64, 4, 3), (65, 7, 3), (130, 33, 3), (7, 300, 2), (300, 7, 2), (129, 515, 2),
          (480, 854, 4))
RADII = (None, 0, 1, 2, 3, 8, 64)                                         # None: the radius of bound_th = 0.008


@functools.lru_cache(maxsize=None)
def shape_pair(h, w, n):
    return seeded_pair(n, h, w, seed=300 + h + w)                         # (shared by the tests below, never written to)


def assert_counts(got: torch.Tensor, exp: np.ndarray, what=""):
    assert got.dtype == torch.int64 and tuple(got.shape) == exp.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, exp), f"{what}: first differing item {np.argwhere((got != exp).any(1))[:1].tolist()}: " \
                                     f"{got[(got != exp).any(1)][:1].tolist()} != {exp[(got != exp).any(1)][:1].tolist()}"


# -------------------------------------------------------------------------------------------------------- seeded shapes
@pytest.mark.parametrize("radius", RADII, ids=lambda r: "r_bound_th" if r is None else f"r{r}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_seeded_shapes(dev, shape, radius):
    h, w, n = shape
    seg, ann = shape_pair(h, w, n)
    exp = VM.jf_counts(seg, ann, radius=radius)
    got = VM.jf_counts_device(seg.to(dev), ann.to(dev), radius=radius)
    assert_counts(got, exp, f"{shape} r={radius}")
    if radius is None:
        assert VM.boundary_radius(h, w) == math.ceil(0.008 * math.sqrt(h * h + w * w))
        j, f = VM.jf_device(ann.to(dev), seg.to(dev))
        assert np.array_equal(j, VM.db_eval_iou(ann, seg)) and np.array_equal(f, VM.db_eval_boundary(ann, seg))


# ----------------------------------------------------------------------------------------------------------- disk shape
def rim_offsets(r):
    """(inside, outside): per row dy of the first quadrant the last offset of the disk (dy, isqrt(r^2 - dy^2)) and the first one
    beyond it; this holds every (dy, dx) with dy^2 + dx^2 == r^2 (horizontal, vertical and, for r = 5, (3, 4) and (4, 3)) and, per
    row, the next larger attainable distance.  Mirrored in x as well."""
    inside, outside = [], [(r + 1, 0)]
    for dy in range(r + 1):
        k = math.isqrt(r * r - dy * dy)
        inside.append((dy, k))
        outside.append((dy, k + 1))
    inside += [(dy, -dx) for dy, dx in inside if dx and dy]
    outside += [(dy, -dx) for dy, dx in outside if dx and dy]
    return inside, outside


@pytest.mark.parametrize("r", (3, 5, 8))
def test_disk_shape_across_a_band_and_a_tile_edge(dev, r):
    """Two single-pixel masks at an offset d.  The boundary map of a single pixel is the 2 x 2 block that ends at it, so the two
    boundary maps are that block and its copy moved by d.  For |d|^2 <= r^2 every boundary pixel has its counterpart at distance
    |d|: all 4 match on both sides and F = 1.  For d just outside the disk the block's corner that points away from d has its
    nearest counterpart at exactly |d| > r: fewer than 4 match.  The pair straddles row 64 and column 256."""
    h, w = 80, 272
    inside, outside = rim_offsets(r)
    assert any(dy * dy + dx * dx == r * r and dy and dx for dy, dx in inside) == (r == 5)
    offs = inside + outside
    seg = torch.zeros(len(offs), h, w, dtype=torch.bool)
    ann = torch.zeros(len(offs), h, w, dtype=torch.bool)
    for i, (dy, dx) in enumerate(offs):
        y, x = 64 - (dy + 1) // 2, 256 - (abs(dx) + 1) // 2 + (-dx if dx < 0 else 0)
        seg[i, y, x] = True
        ann[i, y + dy, x + dx] = True
    exp = VM.jf_counts(seg, ann, radius=r)
    got = VM.jf_counts_device(seg.to(dev), ann.to(dev), radius=r)
    assert_counts(got, exp, f"r={r}")
    got = got.cpu().numpy()
    assert (got[:, 2] == 4).all() and (got[:, 3] == 4).all()
    k = len(inside)
    assert (got[:k, 4] == 4).all() and (got[:k, 5] == 4).all(), "an offset inside the disk does not match fully"
    assert (got[k:, 4] < 4).all() and (got[k:, 5] < 4).all(), "an offset outside the disk matches fully"
    assert (VM.f_measure(got[:k])[0] == 1.0).all() and (VM.f_measure(got[k:])[0] < 1.0).all()


# ----------------------------------------------------------------------------------------------------- structured masks
@pytest.mark.parametrize("shape", ((70, 260), (65, 7), (129, 515)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_structured_masks(dev, shape):
    h, w = shape
    empty, full = torch.zeros(h, w, dtype=torch.bool), torch.ones(h, w, dtype=torch.bool)
    blob = seeded_masks(1, h, w, seed=77)[0]
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    checker = (yy + xx) % 2 == 0
    last_row, last_col, corners = empty.clone(), empty.clone(), empty.clone()
    last_row[h - 1, :] = True
    last_col[:, w - 1] = True
    corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = True
    pairs = [(empty, empty), (empty, blob), (blob, empty), (full, full), (blob, blob), (checker, checker), (checker, ~checker),
             (checker, blob), (last_row, last_row), (last_row, blob), (last_col, last_col), (blob, last_col), (corners, corners),
             (corners, last_row), (last_col, last_row), (full, blob), (empty, full)]
    seg, ann = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    for r in (VM.boundary_radius(h, w), 3):
        exp = VM.jf_counts(seg, ann, radius=r)
        assert_counts(VM.jf_counts_device(seg.to(dev), ann.to(dev), radius=r), exp, f"{shape} r={r}")
    j, f = VM.jf_device(ann.to(dev), seg.to(dev))
    assert np.array_equal(j, VM.db_eval_iou(ann, seg)) and np.array_equal(f, VM.db_eval_boundary(ann, seg))
    assert j[0] == 1.0 and f[0] == 1.0                                    # empty against empty
    assert j[1] == 0.0 and f[1] == 0.0 and j[2] == 0.0 and f[2] == 0.0    # empty against set, either way
    assert j[3] == 1.0 and f[3] == 1.0                                    # full against full: no boundary at all
    assert j[4] == 1.0 and f[4] == 1.0 and j[5] == 1.0 and f[5] == 1.0    # identical masks


# ------------------------------------------------------------------------------------------------------ all input kinds
def index_maps(T, M, h, w, seed):
    """uint8 (T, h, w) with values 0 .. M: M seeded masks per frame painted over each other."""
    m = seeded_masks(T * M, h, w, seed).reshape(T, M, h, w)
    idx = torch.zeros(T, h, w, dtype=torch.uint8)
    for k in range(M):
        idx[m[:, k]] = k + 1
    return idx


@pytest.mark.parametrize("shape", ((66, 260), (65, 70)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_input_kinds_agree(dev, shape):
    h, w = shape
    T, M, thr = 2, 3, 0.25
    pred, gt = index_maps(T, M, h, w, seed=11), index_maps(T, M, h, w, seed=12)
    gt = torch.where(torch.roll(pred, (1, 1), (1, 2)) == 2, torch.tensor(2, dtype=torch.uint8), gt)   # some agreement
    void = seeded_masks(T, h, w, seed=13) & seeded_masks(T, h, w, seed=14)
    ids = torch.arange(1, M + 1, dtype=torch.uint8)[None, :, None, None]
    seg, ann = pred[:, None] == ids, gt[:, None] == ids                   # (T, M, h, w)
    void4 = void[:, None].expand(T, M, h, w)
    r = VM.boundary_radius(h, w)
    exp = VM.jf_counts(seg, ann, void4)
    assert exp[:, :4].min() > 0 and (exp[:, 4] < exp[:, 2]).any()
    exp_novoid = VM.jf_counts(seg, ann)
    assert not np.array_equal(exp, exp_novoid)
    d = lambda t: t.contiguous().to(dev)
    # bool, leading-dimension form (T, M, h, w)
    assert_counts(VM.jf_counts_device(d(seg), d(ann), d(void4)), exp, "bool")
    assert_counts(VM.jf_counts_device(d(seg), d(ann)), exp_novoid, "bool, no void")
    # uint8 x 255, flat
    u8 = lambda t: d(t.reshape(-1, h, w).to(torch.uint8) * 255)
    assert_counts(VM.jf_counts_device(u8(seg), u8(ann), u8(void4), radius=r), exp, "uint8")
    # f32 logits with a threshold: NaN and values equal to it are clear
    g = torch.Generator().manual_seed(15)
    logits = torch.where(seg, thr + 0.5 + torch.rand(seg.shape, generator=g), thr - 0.5 - torch.rand(seg.shape, generator=g))
    clear = ~seg & (torch.rand(seg.shape, generator=g) < 0.2)
    logits = torch.where(clear & (torch.rand(seg.shape, generator=g) < 0.5), torch.tensor(float("nan")), logits)
    logits = torch.where(clear & ~logits.isnan(), torch.tensor(thr), logits)
    assert logits.isnan().any() and (logits == thr).any() and torch.equal(logits > thr, seg)
    assert_counts(VM.jf_counts_device(d(logits), d(ann), d(void4), seg_threshold=thr), exp, "f32 seg")
    ann_logits = torch.where(ann, 1.0, -1.0)
    assert_counts(VM.jf_counts_device(d(logits), d(ann_logits), d(void4), seg_threshold=thr, ann_threshold=0.0), exp, "f32 both")
    # index maps: M objects share a frame's plane; void shares it too
    values = np.tile(np.arange(1, M + 1), T)
    planes = np.repeat(np.arange(T), M)
    kw = dict(seg_values=values, seg_planes=planes, ann_values=values, ann_planes=planes, void_planes=planes)
    assert_counts(VM.jf_counts_device(d(pred), d(gt), d(void), **kw), exp, "index maps")
    # mixed: an index map against boolean planes
    assert_counts(VM.jf_counts_device(d(pred), d(ann), d(void4), seg_values=values, seg_planes=planes), exp, "index seg, bool ann")
    # a forced split by a small workspace: one and two items at a time
    from sam_pt_amd import _lib
    per = int(_lib.load().sampt_jf_workspace_bytes(1, h, w, r))
    for k in (1, 2, 4):
        assert_counts(VM.jf_counts_device(d(pred), d(gt), d(void), workspace_bytes=k * per + 8, **kw), exp, f"index maps, {k} per call")
        assert_counts(VM.jf_counts_device(d(logits), d(ann), d(void4), seg_threshold=thr, workspace_bytes=k * per), exp, f"f32, {k} per call")
    with pytest.raises(_lib.SamptError):
        VM.jf_counts_device(d(seg), d(ann), workspace_bytes=per - 8)
    # J and F in the leading-dimension form
    j, f = VM.jf_device(d(ann), d(logits), d(void4), threshold=thr)
    assert j.shape == (T, M) and f.shape == (T, M) and j.dtype == np.float64
    assert np.array_equal(j, VM.db_eval_iou(ann, seg, void4)) and np.array_equal(f, VM.db_eval_boundary(ann, seg, void4))
    # bad plane numbers and values are refused on the host
    with pytest.raises(_lib.SamptError):
        VM.jf_counts_device(d(pred), d(gt), seg_values=values, seg_planes=planes + 1, ann_values=values, ann_planes=planes)
    with pytest.raises(_lib.SamptError):
        VM.jf_counts_device(d(pred), d(gt), seg_values=values + 300, seg_planes=planes, ann_values=values, ann_planes=planes)


# ------------------------------------------------------------------------------------------------------ unaligned bases
@pytest.mark.parametrize("shape", ((65, 7), (70, 261)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_unaligned_bases(dev, shape):
    h, w = shape
    n, r, thr = 3, 3, 0.25
    pred, gt = index_maps(n, 2, h, w, seed=41), index_maps(n, 2, h, w, seed=42)
    values = np.array([1, 2, 1])
    ids = torch.as_tensor(values, dtype=torch.uint8)[:, None, None]
    seg, ann = pred == ids, gt == ids                                     # item i: value values[i] of plane i
    void = seeded_masks(n, h, w, seed=43) & seeded_masks(n, h, w, seed=44)
    exp = VM.jf_counts(seg, ann, void, radius=r)
    assert exp[:, 1:4].min() > 0 and exp[:, 0].max() > 0 and not np.array_equal(exp, VM.jf_counts(seg, ann, radius=r))
    v = offset_view(void, dev)
    assert_counts(VM.jf_counts_device(offset_view(seg, dev), offset_view(ann, dev), v, radius=r), exp, "bytes")
    assert_counts(VM.jf_counts_device(offset_view(pred, dev), offset_view(gt, dev), v, radius=r, seg_values=values, ann_values=values),
                  exp, "index maps")
    g = torch.Generator().manual_seed(45)
    logit = lambda m: torch.where(m, thr + 0.01 + torch.rand(m.shape, generator=g), thr - torch.rand(m.shape, generator=g))
    fs, fa = logit(seg), logit(ann)
    assert torch.equal(fs > thr, seg) and torch.equal(fa > thr, ann)
    assert_counts(VM.jf_counts_device(offset_view(fs, dev), offset_view(fa, dev), v, radius=r, seg_threshold=thr, ann_threshold=thr),
                  exp, "f32")
    assert_counts(VM.jf_counts_device(offset_view(fs, dev), offset_view(gt, dev), v, radius=r, seg_threshold=thr, ann_values=values),
                  exp, "f32 seg, index ann")


# ---------------------------------------------------------------------------------------------------- sequence protocol
def test_evaluate_semisupervised_on_index_masks_output(dev):
    from sam_pt_amd import dist
    T, M, h, w = 6, 3, 65, 70
    g = torch.Generator().manual_seed(21)
    z = torch.randn(M, T, h // 8 + 2, w // 8 + 2, generator=g)
    logits = torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False) * 4 - 1
    pred = dist.index_masks(logits.to(dev))
    assert pred.is_cuda and pred.dtype == torch.uint8 and tuple(pred.shape) == (T, h, w)
    gt = torch.roll(pred.cpu(), (2, 1), (1, 2)).clone()
    gt[:, 30:34, 20:40] = 255                                             # a void band
    gt[0, 0, 0] = 255
    assert int(torch.where(gt[0] == 255, 0, gt[0]).max()) == M
    ptr = pred.data_ptr()
    got = VM.evaluate_semisupervised(pred, gt.to(dev))
    assert pred.data_ptr() == ptr
    exp = VM.evaluate_semisupervised(pred.cpu(), gt)
    assert set(got) == set(exp) and exp["J"].shape == (M, T - 2)
    for k in exp:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k]), equal_nan=True), k
    assert 0.0 < exp["J-Mean"] < 1.0 and 0.0 < exp["F-Mean"] < 1.0
    # one object more than either map has: J = F = 1 for it on both paths
    got4, exp4 = VM.evaluate_semisupervised(pred, gt.to(dev), n_objects=4), VM.evaluate_semisupervised(pred.cpu(), gt, n_objects=4)
    assert np.array_equal(got4["J"], exp4["J"]) and np.array_equal(got4["F"], exp4["F"]) and (got4["J"][3] == 1.0).all()
    # a ground truth that stays on the host is uploaded
    mixed = VM.evaluate_semisupervised(pred, gt)
    assert np.array_equal(mixed["J"], exp["J"]) and np.array_equal(mixed["F"], exp["F"])


# -------------------------------------------------------------------------------------------------------- repeatability
def test_two_calls_are_bitwise_equal(dev):
    seg, ann = shape_pair(129, 515, 2)
    s, a = seg.to(dev), ann.to(dev)
    first = VM.jf_counts_device(s, a, radius=8)
    for _ in range(3):
        assert torch.equal(VM.jf_counts_device(s, a, radius=8), first)
