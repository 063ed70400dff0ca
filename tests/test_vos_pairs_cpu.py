"""All-pairs J&F counts and the DAVIS unsupervised protocol on the host (sam_pt_amd.vos_metrics.jf_pairs_counts,
evaluate_unsupervised): the pair counts equal ``jf_counts`` pair by pair, the protocol a brute-force loop over ``db_eval_iou`` /
``db_eval_boundary`` and ``linear_sum_assignment``.  The protocol is restated from the published DAVIS toolkit: parity unpinned."""
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from sam_pt_amd import _lib
from sam_pt_amd import vos_metrics as VM
from tests.test_amg_tail_cpu import seeded_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_planes(n, T, h, w, seed):
    """bool (n, T, h, w) numpy."""
    return seeded_masks(n * T, h, w, seed).reshape(n, T, h, w).numpy()


def seeded_index(n, T, h, w, seed, void=False):
    """uint8 (T, h, w): n objects, later ones painted over earlier ones; ``void`` adds a 255 block and speckle."""
    planes = seeded_planes(n, T, h, w, seed)
    idx = np.zeros((T, h, w), dtype=np.uint8)
    for i in range(n):
        idx[planes[i]] = i + 1
    if void:
        idx[:, h // 3:h // 3 + 4, w // 4:w // 4 + 9] = 255
        idx[np.random.default_rng(seed).random((T, h, w)) < 0.01] = 255
    return idx


@functools.lru_cache(maxsize=None)
def sequence(P, K, T=5, h=37, w=45):
    """(pred index, gt index with void): the ground truth's objects and, as proposals, unrelated blobs followed by moved copies of the
    objects in another order (shared by the tests below, never written to)."""
    gt = seeded_index(K, T, h, w, 40 + K, void=True)
    clean = np.where(gt == 255, 0, gt)
    pred = np.zeros_like(gt)
    extra = seeded_planes(max(P, 1), T, h, w, 90 + P)
    off = max(P - K, 0)                                                   # the copies are the last proposals
    for p in range(P):
        k = ((p - off) * 2 + 1) % max(K, 1) if off <= p < off + K else None
        m = np.roll(clean == k + 1, (1, 2), axis=(1, 2)) if k is not None else extra[p] & (pred == 0)
        pred[m] = p + 1
    if P:
        pred[:, 0, p % w] = P                                             # (so that max(pred) is P whatever was painted over)
    return pred, gt


def test_pairs_equal_jf_counts_pair_by_pair():
    S, A = seeded_planes(3, 2, 33, 41, 1), seeded_planes(2, 2, 33, 41, 2)
    void = seeded_masks(2, 33, 41, 3).numpy()
    for v in (None, void):
        for radius in (None, 0, 3):
            out, ss, sa = VM.jf_pairs_counts(S, A, v, radius=radius, return_stats=True)
            assert out.shape == (3, 2, 2, 6) and out.dtype == np.int64
            keep = np.ones_like(void) if v is None else ~v
            assert np.array_equal(ss[..., 0], (S & keep).sum(axis=(2, 3))) and np.array_equal(sa[..., 0], (A & keep).sum(axis=(2, 3)))
            for p in range(3):
                for k in range(2):
                    assert np.array_equal(out[p, k], VM.jf_counts(S[p], A[k], v, radius=radius)), (p, k, radius)
                    assert np.array_equal(out[p, k, :, 2], ss[p, :, 1]) and np.array_equal(out[p, k, :, 3], sa[k, :, 1])


def test_pairs_of_index_maps_and_floats():
    pred, gt = sequence(3, 2)
    void = gt == 255
    out = VM.jf_pairs_counts(pred, gt, void, seg_values=[1, 2, 3], ann_values=[1, 2])
    for p in range(3):
        for k in range(2):
            assert np.array_equal(out[p, k], VM.jf_counts(pred == p + 1, gt == k + 1, void))
    f = np.random.default_rng(0).standard_normal((2, 2, 9, 11)).astype(np.float32)
    f[0, 0, 0, 0], f[1, 1, 2, 3] = np.nan, 0.25
    A = seeded_planes(1, 2, 9, 11, 5)
    out = VM.jf_pairs_counts(f, A, seg_threshold=0.25, radius=1)
    assert np.array_equal(out[1, 0], VM.jf_counts(f[1], A[0], seg_threshold=0.25, radius=1))
    with pytest.raises(ValueError):
        VM.jf_pairs_counts(f, A)                                          # a float side needs its threshold
    with pytest.raises(ValueError):
        VM.jf_pairs_counts(A, A[:, :1])


def brute_force(pred_planes, gt, K, bound_th=0.008):
    """The protocol, literally: pad, drop the end frames, J and F of every pair, assign."""
    void = gt == 255
    P = len(pred_planes)
    if P < K:
        pred_planes = np.concatenate([pred_planes, np.zeros((K - P,) + pred_planes.shape[1:], dtype=bool)])
    J = np.zeros((len(pred_planes), K, len(gt) - 2))
    F = np.zeros_like(J)
    for p in range(len(pred_planes)):
        for k in range(K):
            J[p, k] = VM.db_eval_iou(gt[1:-1] == k + 1, pred_planes[p, 1:-1], void[1:-1])
            F[p, k] = VM.db_eval_boundary(gt[1:-1] == k + 1, pred_planes[p, 1:-1], void[1:-1], bound_th=bound_th)
    rows, cols = linear_sum_assignment(-((J.mean(axis=2) + F.mean(axis=2)) / 2))
    return J, F, rows, cols


@pytest.mark.parametrize("P,K", [(2, 4), (3, 3), (6, 3), (1, 1)], ids=lambda v: str(v))
def test_unsupervised_equals_brute_force(P, K):
    pred, gt = sequence(P, K)
    planes = pred[None] == np.arange(1, P + 1, dtype=np.uint8)[:, None, None, None]
    J, F, rows, cols = brute_force(planes, gt, K)
    for given in (pred, planes, torch.from_numpy(pred)):
        r = VM.evaluate_unsupervised(given, gt)
        assert np.array_equal(r["J_all"], J) and np.array_equal(r["F_all"], F)
        assert np.array_equal(r["assignment"][0], rows) and np.array_equal(r["assignment"][1], cols)
        assert r["J"].shape == (K, len(gt) - 2) and np.array_equal(r["J"], J[rows, cols]) and np.array_equal(r["F"], F[rows, cols])
        jm = np.mean([VM.db_statistics(v)[0] for v in J[rows, cols]])
        fd = np.mean([VM.db_statistics(v)[2] for v in F[rows, cols]])
        assert r["J-Mean"] == jm and r["F-Decay"] == fd and r["J&F-Mean"] == (r["J-Mean"] + r["F-Mean"]) / 2
    score = (J.mean(axis=2) + F.mean(axis=2)) / 2
    assert sorted(cols.tolist()) == list(range(K)) and score[rows, cols].sum() >= score[np.arange(K), np.arange(K)].sum()
    if P >= K and K > 1:                                                  # the moved copies find their objects, in their other order
        assert cols.tolist() != list(range(K)) and score[rows, cols].sum() > score[np.arange(K), np.arange(K)].sum()
    if P > K:
        assert rows.tolist() != list(range(K))                            # not the first K proposals
    if P < K:
        assert J[P:].max() < 1 and (r["J_all"][P:, :, :] == J[P:]).all()  # the padding rows are empty masks


def test_unsupervised_refusals_and_edges():
    pred, gt = sequence(21, 3)
    with pytest.raises(ValueError, match="max_n_proposals"):
        VM.evaluate_unsupervised(pred, gt)
    assert VM.evaluate_unsupervised(pred, gt, max_n_proposals=21)["J"].shape == (3, 3)
    with pytest.raises(ValueError, match="max_n_proposals"):
        VM.evaluate_unsupervised(np.zeros((21,) + gt.shape, dtype=bool), gt)
    with pytest.raises(ValueError, match="at least 3 frames"):
        VM.evaluate_unsupervised(pred[:2], gt[:2])
    with pytest.raises(ValueError):
        VM.evaluate_unsupervised(pred[:, 1:], gt)
    pred, gt = sequence(3, 3)
    r = VM.evaluate_unsupervised(np.zeros_like(pred), gt)                 # no proposal at all: three empty ones
    assert r["J"].shape == (3, 3) and r["J-Mean"] < 0.2
    r = VM.evaluate_unsupervised(pred, gt, n_objects=2)
    assert r["J"].shape == (2, 3) and r["J_all"].shape == (3, 2, 3)
    r = VM.evaluate_unsupervised(pred, np.zeros_like(gt))
    assert r["J"].shape == (0, 3) and np.isnan(r["J&F-Mean"])


def test_abi_is_declared():
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_\w+)\s*\(", hdr))
    for name in ("sampt_jf_pairs_workspace_bytes", "sampt_jf_pairs_counts"):
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
    res, args = _lib._SIGS["sampt_jf_pairs_counts"]                       # house style: int return code, workspace and stream last
    assert res is _lib.c_int and len(args) == 24 and args[-2] is _lib.c_size_t
    assert _lib._SIGS["sampt_jf_pairs_workspace_bytes"][0] is _lib.c_size_t
    proto = re.search(r"int sampt_jf_pairs_counts\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == 24
    assert "vos_pairs.hip" in open(os.path.join(ROOT, "sam_pt_amd", "csrc", "Makefile")).read()
