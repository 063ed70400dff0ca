"""CPU side of the DAVIS J&F evaluation (no GPU needed): the host restatement of sam_pt_amd/vos_metrics.py against scipy's binary
dilation and a literal per-pixel boundary map, the precision / recall branches, ``db_statistics`` on hand-computed vectors, the
semi-supervised sequence protocol on a hand-made sequence, and the C ABI surface with its refusals.  The restatement is parity
unpinned against the ``davis2017`` package (absent here)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from sam_pt_amd import vos_metrics as VM
from tests.test_amg_tail_cpu import seeded_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_jf_workspace_bytes", "sampt_jf_counts")


# --------------------------------------------------------------------------------------------------------------------
# seeded pairs shared with tests/test_gpu_vos_metrics.py
# --------------------------------------------------------------------------------------------------------------------
def seeded_pair(n: int, h: int, w: int, seed: int):
    """(seg, ann) bool (n, h, w): seeded blobs with salt noise; seg is ann moved by (1, 2) pixels with its own noise and squares
    on top, so that boundaries partly match."""
    ann = seeded_masks(n, h, w, seed)
    other = seeded_masks(n, h, w, seed + 1000)
    seg = torch.roll(ann, shifts=(1 % h, 2 % w), dims=(1, 2))
    g = torch.Generator().manual_seed(seed + 7)
    pick = torch.rand(n, h, w, generator=g) < 0.1
    seg = torch.where(pick, other, seg)
    return seg, ann


def literal_seg2bmap(m: np.ndarray) -> np.ndarray:
    """The definition, pixel by pixel."""
    h, w = m.shape

    def px(y, x):
        return bool(m[y, x]) if y < h and x < w else False

    b = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            b[y, x] = (px(y, x) ^ px(y, x + 1)) | (px(y, x) ^ px(y + 1, x)) | (px(y, x) ^ px(y + 1, x + 1))
    for x in range(w):
        b[h - 1, x] = px(h - 1, x) ^ px(h - 1, x + 1)
    for y in range(h):
        b[y, w - 1] = px(y, w - 1) ^ px(y + 1, w - 1)
    b[h - 1, w - 1] = False
    return b


# ----------------------------------------------------------------------------------------------------------- dilation
@pytest.mark.parametrize("shape", ((1, 1), (1, 9), (9, 1), (13, 17), (65, 70), (130, 33)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_disk_dilation_equals_scipy(shape):
    from scipy import ndimage
    h, w = shape
    g = np.random.default_rng(31 + h * w)
    maps = [g.random((h, w)) < p for p in (0.01, 0.05, 0.5)] + [np.zeros((h, w), bool), np.ones((h, w), bool)]
    corner = np.zeros((h, w), bool)
    corner[0, 0] = corner[-1, -1] = True
    maps.append(corner)
    for r in (0, 1, 2, 3, 5, 8, 20):
        d = VM.disk(r)
        assert d.shape == (2 * r + 1, 2 * r + 1) and d[r, r] and d[0, r] and d[r, 0]
        assert [int(d[r + dy].sum()) for dy in range(-r, r + 1)] == [2 * math.isqrt(r * r - dy * dy) + 1 for dy in range(-r, r + 1)]
        for b in maps:
            exp = ndimage.binary_dilation(b, structure=d)
            assert np.array_equal(VM.dilate_disk(b, r), exp), (shape, r)
    stack = np.stack(maps[:3])
    assert np.array_equal(VM.dilate_disk(stack, 3), np.stack([ndimage.binary_dilation(b, structure=VM.disk(3)) for b in stack]))


# ----------------------------------------------------------------------------------------------------------- boundary
@pytest.mark.parametrize("shape", ((1, 1), (1, 2), (2, 1), (2, 2), (9, 14), (65, 7)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_seg2bmap_equals_the_definition(shape):
    h, w = shape
    seg, ann = seeded_pair(2, h, w, seed=50 + h + w)
    masks = [m.numpy() for m in seg] + [m.numpy() for m in ann]
    masks += [np.ones((h, w), bool), np.zeros((h, w), bool), (np.indices((h, w)).sum(0) % 2 == 0)]
    for m in masks:
        assert np.array_equal(VM.seg2bmap(m), literal_seg2bmap(m))
    st = np.stack(masks)
    assert np.array_equal(VM.seg2bmap(st), np.stack([literal_seg2bmap(m) for m in masks]))
    assert np.array_equal(VM.seg2bmap(torch.as_tensor(st).to(torch.uint8) * 255), VM.seg2bmap(st))


def test_seg2bmap_hand_cases():
    assert not VM.seg2bmap(np.ones((6, 9), bool)).any()                   # a full mask has no boundary
    assert not VM.seg2bmap(np.zeros((6, 9), bool)).any()
    m = np.zeros((6, 9), bool)
    m[2, 4] = True                                                        # one interior pixel: itself, west, north, north-west
    b = VM.seg2bmap(m)
    assert b.sum() == 4 and b[2, 4] and b[2, 3] and b[1, 4] and b[1, 3]
    m = np.zeros((6, 9), bool)
    m[5, 8] = True                                                        # the corner pixel: only its north-west sees it
    b = VM.seg2bmap(m)
    assert b.sum() == 3 and b[4, 7] and b[4, 8] and b[5, 7] and not b[5, 8]


# ----------------------------------------------------------------------------------------------------------- branches
def test_precision_recall_branches_and_empty_union():
    c = np.array([[0, 5, 0, 7, 0, 0],                                     # no predicted boundary, some truth: P = 1, R = 0
                  [0, 5, 7, 0, 0, 0],                                     # the reverse: P = 0, R = 1
                  [0, 0, 0, 0, 0, 0],                                     # both empty: P = R = 1; empty union: J = 1
                  [3, 4, 10, 8, 5, 2],                                    # P = 0.5, R = 0.25
                  [0, 9, 4, 4, 0, 0]])                                    # nothing matches: P + R = 0 -> F = 0
    f, p, r = VM.f_measure(c)
    assert p.tolist() == [1.0, 0.0, 1.0, 0.5, 0.0] and r.tolist() == [0.0, 1.0, 1.0, 0.25, 0.0]
    assert f.tolist() == [0.0, 0.0, 1.0, 2 * 0.5 * 0.25 / 0.75, 0.0]
    assert VM.jaccard_from_counts(c).tolist() == [0.0, 0.0, 1.0, 0.75, 0.0]
    empty, full = np.zeros((8, 8), bool), np.ones((8, 8), bool)
    blob = np.zeros((8, 8), bool)
    blob[2:5, 2:6] = True
    assert VM.db_eval_iou(empty, empty) == 1.0 and VM.db_eval_boundary(empty, empty) == 1.0
    assert VM.db_eval_iou(blob, empty) == 0.0 and VM.db_eval_boundary(blob, empty) == 0.0
    assert VM.db_eval_boundary(empty, blob) == 0.0
    assert VM.db_eval_iou(blob, blob) == 1.0 and VM.db_eval_boundary(blob, blob) == 1.0
    assert VM.db_eval_boundary(full, full) == 1.0                         # no boundary on either side
    # void: the pixels where they differ are void -> a perfect score
    other = blob.copy()
    other[4, 2:6] = False
    assert VM.db_eval_iou(blob, other) == 8 / 12
    assert VM.db_eval_iou(blob, other, void_pixels=blob ^ other) == 1.0
    j = VM.db_eval_iou(np.stack([blob, empty]), np.stack([other, empty]))
    assert j.shape == (2,) and j.tolist() == [8 / 12, 1.0]
    assert VM.boundary_radius(480, 854) == 8 and VM.boundary_radius(10, 10) == 1 and VM.boundary_radius(480, 854, 3) == 3


def test_jf_counts_equals_scipy_composition():
    from scipy import ndimage
    seg, ann = seeded_pair(3, 65, 70, seed=9)
    void = seeded_masks(3, 65, 70, seed=10) & seeded_masks(3, 65, 70, seed=11)
    for r in (0, 1, 3):
        got = VM.jf_counts(seg, ann, void, radius=r)
        for i in range(3):
            s, a = (seg[i] & ~void[i]).numpy(), (ann[i] & ~void[i]).numpy()
            bs, ba = literal_seg2bmap(s), literal_seg2bmap(a)
            exp = [(s & a).sum(), (s | a).sum(), bs.sum(), ba.sum(),
                   (bs & ndimage.binary_dilation(ba, structure=VM.disk(r))).sum(),
                   (ba & ndimage.binary_dilation(bs, structure=VM.disk(r))).sum()]
            assert got[i].tolist() == [int(v) for v in exp]
    logits = torch.where(seg, 1.0, -1.0)
    logits[0, :3] = 0.25
    logits[1, 0, 0] = float("nan")
    assert np.array_equal(VM.jf_counts(logits, ann, seg_threshold=0.25), VM.jf_counts(logits > 0.25, ann))
    with pytest.raises(ValueError):
        VM.jf_counts(logits, ann)


# --------------------------------------------------------------------------------------------------------- statistics
def test_db_statistics_hand_computed():
    nan = float("nan")
    # length 1: ids = round(linspace(1, 1, 5)) - 1 = [0, 0, 0, 0, 0]: every bin is the one value
    assert VM.db_statistics([0.75]) == (0.75, 1.0, 0.0)
    # length 4: ids = round([1, 1.75, 2.5, 3.25, 4] + 1e-10) - 1 = [0, 1, 2, 2, 3]: first bin v[0:2], last bin v[2:4]
    m, r, d = VM.db_statistics([1.0, 0.5, 0.25, 0.75])
    assert (m, r, d) == (0.625, 0.5, 0.75 - 0.5)
    # length 7: ids = round([1, 2.5, 4, 5.5, 7] + 1e-10) - 1 = [0, 2, 3, 5, 6] (2.5 + 1e-10 and 5.5 + 1e-10 round up):
    # first bin v[0:3], last bin v[5:7]
    v = [1.0, 0.5, 0.75, 0.25, 0.5, 0.25, 0.75]
    m, r, d = VM.db_statistics(v)
    assert m == sum(v) / 7 and r == 3 / 7 and d == (1.0 + 0.5 + 0.75) / 3 - 0.5
    # a NaN is left out of the mean and of the bins, and counts as "not above 0.5" in the recall
    m, r, d = VM.db_statistics([1.0, nan, 0.75, 0.25])
    assert m == 2.0 / 3 and r == 0.5 and d == 1.0 - 0.5


# --------------------------------------------------------------------------------------------------- sequence protocol
def tiny_sequence():
    """T = 5 frames of 6 x 8, two objects.  Object 1 is a 3 x 3 square that the prediction tracks exactly except on frame 2, where
    it misses one row, and on frame 3, where it misses the same row but the truth marks that row void (label 255); object 2 is a
    2 x 2 square that the prediction never has (one object too few).  Frames 0 and 4 are wrong on purpose: the protocol drops
    them."""
    T, H, W = 5, 6, 8
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        gt[t, 1:4, 1:4] = 1
        gt[t, 4:6, 5:7] = 2
        pred[t, 1:4, 1:4] = 1
    pred[2, 3, 1:4] = 0                                                   # frame 2: the prediction misses object 1's last row
    gt[3, 3, 1:4] = 255                                                   # frame 3: that row is void in the truth
    pred[3, 3, 1:4] = 0                                                   #   ... and the prediction's error there does not count
    pred[0] = 0                                                           # dropped frames: garbage
    pred[4] = 2
    return pred, gt


def test_evaluate_semisupervised_on_a_hand_made_sequence():
    pred, gt = tiny_sequence()
    out = VM.evaluate_semisupervised(pred, gt)
    assert out["J"].shape == (2, 3) and out["F"].shape == (2, 3)
    assert out["J"][0].tolist() == [1.0, 6 / 9, 1.0]                      # frames 1, 2, 3 of object 1 (frame 3: void hides the row)
    assert out["J"][1].tolist() == [0.0, 0.0, 0.0]                        # object 2: empty prediction against a 2 x 2 square
    assert out["F"][1].tolist() == [0.0, 0.0, 0.0]                        # P = 1, R = 0
    assert out["F"][0, 0] == 1.0 and out["F"][0, 2] == 1.0 and 0.0 < out["F"][0, 1] <= 1.0
    # statistics: the mean over the objects of each object's db_statistics
    j0, j1 = VM.db_statistics(out["J"][0]), VM.db_statistics(out["J"][1])
    assert out["J-Mean"] == (j0[0] + j1[0]) / 2 and out["J-Recall"] == (1.0 + 0.0) / 2 and out["J-Decay"] == (j0[2] + j1[2]) / 2
    assert out["J-Mean"] == ((1.0 + 6 / 9 + 1.0) / 3 + 0.0) / 2
    assert out["J&F-Mean"] == (out["J-Mean"] + out["F-Mean"]) / 2
    assert set(out) == {"J", "F", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay", "J&F-Mean"}
    # the same from torch tensors, and with the object count given: a third object nobody has scores J = F = 1
    again = VM.evaluate_semisupervised(torch.as_tensor(pred), torch.as_tensor(gt))
    assert all(np.array_equal(out[k], again[k]) for k in out)
    three = VM.evaluate_semisupervised(pred, gt, n_objects=3)
    assert three["J"].shape == (3, 3) and np.array_equal(three["J"][:2], out["J"]) and three["J"][2].tolist() == [1.0, 1.0, 1.0]
    assert three["F"][2].tolist() == [1.0, 1.0, 1.0]
    # the number of objects comes from the first frame, void excluded
    gt2 = gt.copy()
    gt2[0, 0, 0] = 255
    assert VM.evaluate_semisupervised(pred, gt2)["J"].shape == (2, 3)
    with pytest.raises(ValueError):
        VM.evaluate_semisupervised(pred[:2], gt[:2])
    with pytest.raises(ValueError):
        VM.evaluate_semisupervised(pred, gt[:, :5])


def test_device_functions_refuse_cpu_tensors():
    from sam_pt_amd._lib import SamptError
    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    with pytest.raises(SamptError):
        VM.jf_counts_device(m, m, radius=1)
    with pytest.raises(SamptError):
        VM.jf_device(m, m)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_c_abi_declares_binds_and_exports_the_jf_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
    res, args = _lib._SIGS["sampt_jf_counts"]                             # house style: int return code, workspace and stream last
    assert res is _lib.c_int and args[-1] is _lib._P and args[-2] is _lib.c_size_t and args[-3] is _lib._P
    assert _lib._SIGS["sampt_jf_workspace_bytes"][0] is _lib.c_size_t


def test_abi_refuses_bad_arguments_without_touching_memory():
    from sam_pt_amd import _lib
    lib = _lib.load()
    wsb = lib.sampt_jf_workspace_bytes
    assert wsb(1, 46341, 46341, 8) == 0                                   # h * w >= 2^31
    assert wsb(1, 0, 5, 8) == 0 and wsb(1, 5, 0, 8) == 0 and wsb(0, 8, 8, 8) == 0 and wsb(-1, 8, 8, 8) == 0
    assert wsb(1, 8, 8, -1) == 0 and wsb(1, 8, 8, 65) == 0
    per = wsb(1, 480, 854, 8)
    assert per == 2 * 8 * 854 * 8                                         # two bit-planes of 8 bands x 854 columns x 8 bytes
    assert wsb(5, 480, 854, 64) == 5 * per and wsb(1, 1, 1, 0) == 16
    # addresses that must never be read or written: every refusal below happens before any use of them
    fake = ctypes.c_void_p(1 << 20)

    def call(seg=fake, sk=0, ann=fake, ak=0, vals=None, n=1, h=8, w=8, r=1, counts=fake, ws=fake, ws_bytes=1 << 20):
        return lib.sampt_jf_counts(seg, sk, 0.0, vals, None, ann, ak, 0.0, vals, None, None, None, n, h, w, r, counts, ws, ws_bytes, None)

    for kw in (dict(seg=None), dict(ann=None), dict(counts=None), dict(ws=None)):
        assert call(**kw) == -1, kw
        assert b"null" in lib.sampt_last_error()
    assert call(sk=2) == -1 and b"null" in lib.sampt_last_error()         # an index map without its values
    assert call(ak=2) == -1
    for kw in (dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3)):
        assert call(**kw) == -1, kw
        assert b"shape" in lib.sampt_last_error()
    assert call(h=46341, w=46341) == -1 and b"2^31" in lib.sampt_last_error()
    for r in (-1, 65):
        assert call(r=r) == -1 and b"radius" in lib.sampt_last_error()
    for kw in (dict(sk=3), dict(sk=-1), dict(ak=3), dict(ak=7)):
        assert call(**kw) == -1, kw
        assert b"kind" in lib.sampt_last_error()
    assert call(ws=ctypes.c_void_p((1 << 20) + 8)) == -1                  # misaligned workspace
    assert call(seg=ctypes.c_void_p((1 << 20) + 2), sk=1) == -1           # misaligned f32
    need = wsb(3, 70, 9, 2)
    assert call(n=3, h=70, w=9, r=2, ws_bytes=need - 1) == -4             # SAMPT_ERR_WORKSPACE
    assert b"workspace" in lib.sampt_last_error()
    assert call(n=3, h=70, w=9, r=2, ws_bytes=0) == -4
