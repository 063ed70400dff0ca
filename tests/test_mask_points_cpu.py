"""Rank -> pixel on bit-planes and the two-step query-point selection, on the host: the NumPy restatement of
``sampt_bits_row_prefix`` / ``sampt_bits_select`` against ``nonzero()``, the rank step + a source of pixels against the selectors of
sam_pt_amd/query_points.py (same points with ``==``, same generator state), and the factored re-initialisation rule against the
code it was lifted from."""
import os

import numpy as np
import pytest
import torch

from sam_pt_amd import mask_points as MP
from sam_pt_amd import query_points as QP
from sam_pt_amd.vis_metrics import pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["reinit-on-horizon-and-sync-masks", "reinit-at-median-of-area-diff", "reinit-on-similar-mask-area",
            "reinit-on-similar-mask-area-and-sync-masks"]


def _planes(h, w, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((6, h, w), dtype=bool)
    m[1] = True
    m[2, h - 1, w - 1] = True
    m[3, 0, 0] = True
    m[4] = rng.random((h, w)) < 0.02
    m[5] = rng.random((h, w)) < 0.5
    return m


@pytest.mark.parametrize("h,w", [(1, 1), (63, 5), (64, 64), (65, 3), (130, 67)])
def test_restatement_equals_nonzero(h, w):
    m = _planes(h, w, h * 1000 + w)
    bits = pack_bits(m)
    prefix = MP.row_prefix(bits, h)
    assert prefix.dtype == np.int32 and prefix.shape == (6, h + 1)
    assert np.array_equal(prefix[:, 1:], np.cumsum(m.sum(axis=2), axis=1)) and not prefix[:, 0].any()
    for i in range(6):
        for invert in (0, 1):
            nz = np.argwhere(~m[i] if invert else m[i])
            q = np.array([(i, invert, r) for r in range(len(nz))], dtype=np.int64).reshape(-1, 3)
            got = MP.select_ranks(bits, prefix, h, q)
            assert got.dtype == np.float32 and np.array_equal(got, nz.astype(np.float32)), (i, invert)
            bad = MP.select_ranks(bits, prefix, h, [(i, invert, -1), (i, invert, len(nz)), (6, invert, 0), (-1, invert, 0)])
            assert np.array_equal(bad, np.full((4, 2), -1.0, dtype=np.float32))


def test_restatement_takes_mixed_queries_in_any_order():
    h, w = 70, 37
    m = _planes(h, w, 3)
    bits, prefix = pack_bits(m), None
    prefix = MP.row_prefix(bits, h)
    rng = np.random.default_rng(1)
    q, want = [], []
    for i in (4, 5, 1, 2):
        for invert in (0, 1):
            nz = np.argwhere(~m[i] if invert else m[i])
            for r in rng.choice(len(nz), size=min(20, len(nz)), replace=False):
                q.append((i, invert, int(r)))
                want.append(nz[r])
    order = rng.permutation(len(q))
    got = MP.select_ranks(bits, prefix, h, np.array(q)[order])
    assert np.array_equal(got, np.array(want, dtype=np.float32)[order])


# ---------------------------------------------------------------------------------------------- the rank split
def _masks_and_images():
    """Four masks of 48 x 40: a blob (draw branch), three pixels (repeat branch), empty, a second blob."""
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(48), torch.arange(40), indexing="ij")
    masks = torch.zeros(4, 48, 40)
    masks[0] = (((yy - 20) ** 2 + (xx - 18) ** 2) <= 12 ** 2).float()
    masks[1, 5, 5] = masks[1, 6, 7] = masks[1, 40, 2] = 1
    masks[3] = ((yy > 8) & (yy < 30) & (xx > 22) & (xx < 37)).float()
    images = torch.randint(0, 256, (3, 3, 48, 40), generator=g, dtype=torch.uint8)
    return masks, images, torch.tensor([0.0, 2.0, 1.0, 1.0])


def _both_routes(host, split, seed=5):
    torch.manual_seed(seed)
    a = host()
    state_a = torch.get_rng_state()
    torch.manual_seed(seed)
    b = split()
    state_b = torch.get_rng_state()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    assert torch.equal(state_a, state_b)                       # the same draws were made


@pytest.mark.parametrize("n", [1, 5, 8])
def test_rank_split_equals_random_selector(n):
    masks, images, ts = _masks_and_images()
    stats = {}
    _both_routes(lambda: [QP.extract_random_mask_points(m, n) for m in masks],
                 lambda: QP.select_query_points(MP.HostMasks(masks), images, ts, "random", n, stats=stats))
    assert stats["draw"] >= 1 and stats["empty"] == 1 and (n <= 3 or stats["repeat"] == 1)


@pytest.mark.parametrize("n", [2, 5])
def test_rank_split_equals_kmedoid_selector(n):
    masks, images, ts = _masks_and_images()
    stats = {}
    _both_routes(lambda: [QP.extract_kmedoid_points(m, n) for m in masks],
                 lambda: QP.select_query_points(MP.HostMasks(masks), images, ts, "kmedoids", n, stats=stats))
    assert stats["draw"] >= 2 and stats["empty"] == 1


@pytest.mark.parametrize("n", [1, 4, 12])
def test_rank_split_equals_mixed_selector(n):
    """n = 12: three k-medoid, four Shi-Tomasi (with their k-medoid top-up where fewer corners are found) and five random points."""
    masks, images, ts = _masks_and_images()
    _both_routes(lambda: QP.extract_mixed_points(masks, ts, images, n),
                 lambda: QP.select_query_points(MP.HostMasks(masks), images, ts, "mixed", n))


@pytest.mark.parametrize("pos,n_pos,neg,n_neg", [("kmedoids", 4, "mixed", 1), ("random", 3, "mixed", 12), ("shi-tomasi", 5, "random", 2),
                                                 ("mixed", 12, "kmedoids", 3)])
def test_rank_split_equals_extract_query_points(pos, n_pos, neg, n_neg):
    """Positives of all masks, then negatives from the complements: SamPt.extract_query_points' order of draws."""
    masks, images, ts = _masks_and_images()

    def host():
        xy = QP.extract_query_points_xy(images, masks, ts, pos, n_pos)
        ng = QP.extract_query_points_xy(images, [1 - m for m in masks], ts, neg, n_neg)
        return [torch.cat(x, dim=0) for x in zip(xy, ng)]

    _both_routes(host, lambda: QP.select_query_points(MP.HostMasks(masks), images, ts, pos, n_pos, neg, n_neg))


def test_rank_step_branches():
    assert QP.rank_step(0, 4) is None
    state = torch.get_rng_state()
    assert QP.rank_step(3, 8).tolist() == [0, 1, 2, 0, 1, 2, 0, 1]
    assert torch.equal(state, torch.get_rng_state())           # neither branch above draws
    torch.manual_seed(2)
    want = torch.randperm(100)
    torch.manual_seed(2)
    assert torch.equal(QP.rank_step(100, 8), want[:8])
    torch.manual_seed(2)
    assert torch.equal(QP.rank_step(100, 8, cut=30), want[:30])


# ---------------------------------------------------------------------------------------------- the re-initialisation rule
def _inlined_rule(pred_area, target, cur_t, start, H, variant):
    """The rule as it stood inside SamPt._forward_w_reinit_inner (sam_pt.py:467-505 of the reference)."""
    area = pred_area.clone().float()
    area[area <= 25] = torch.nan
    if H // 4 < area.shape[1]:
        area[:, :H // 4] = torch.nan
    n_i = area.shape[0]
    if variant == "reinit-on-horizon-and-sync-masks":
        nxt = H - 1 - 1
        others = cur_t[cur_t > start]
        if len(others) > 0:
            nxt = min(nxt, others.min() - start - 1)
        q_t = torch.full((n_i,), nxt, dtype=torch.int64)
    elif variant == "reinit-at-median-of-area-diff":
        q_t = area.nanmedian(dim=1).indices
    elif variant == "reinit-on-similar-mask-area":
        diff = torch.abs(area - target[:, None])
        diff[diff.isnan()] = torch.inf
        q_t = diff.argmin(dim=1)
    else:
        diff = torch.abs(area - target[:, None]) / target[:, None]
        diff[diff.isnan()] = 720
        per_frame = diff.sum(dim=0)
        others = cur_t[cur_t > start]
        if len(others) > 0:
            per_frame[others.min().item() - start - 1] -= 36
        q_t = torch.full((n_i,), per_frame.argmin(dim=0), dtype=torch.int64)
    return q_t, area[torch.arange(n_i), q_t] <= 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_factored_reinit_rule_equals_inlined_code(variant):
    from sam_pt_amd.sam_pt import reinit_query_frames
    g = torch.Generator().manual_seed(7)
    for case in range(40):
        H = [5, 8, 24][case % 3]
        n_i = 1 + case % 4
        frames = H                                             # (a last, shorter segment never reaches the rule)
        area = torch.randint(0, 4000, (n_i, frames - 1), generator=g)
        area[torch.rand(area.shape, generator=g) < 0.3] = 0    # empty and tiny masks: NaN in the rule
        area[torch.rand(area.shape, generator=g) < 0.2] = 20
        if case % 4 == 0:
            area[0] = 0                                        # an all-NaN row
        if case % 7 == 0:
            area[:] = 3                                        # all rows NaN
        target = torch.randint(0, 4000, (n_i,), generator=g)
        if case % 6 == 0:
            target[0] = 0
        start = case % 3
        cur_t = torch.cat([torch.full((n_i,), start), torch.randint(0, start + H, (case % 3,), generator=g)]).int()
        want_q, want_inv = _inlined_rule(area, target, cur_t, start, H, variant)
        before = area.clone()
        got_q, got_inv = reinit_query_frames(area.float(), target, cur_t, start, H, variant)
        assert torch.equal(got_q, want_q) and torch.equal(got_inv, want_inv)
        assert got_q.dtype == torch.int64 and torch.equal(area, before)
    with pytest.raises(ValueError):
        reinit_query_frames(torch.ones(1, 4), torch.ones(1).long(), torch.zeros(1).int(), 0, 5, "no-such-variant")


# ---------------------------------------------------------------------------------------------- wiring
def test_keyword_default_and_fallbacks():
    from sam_pt_amd.sam_pt import SamPt

    class Predictor:
        model = torch.nn.Identity()

        def encode_frames(self, *a, **k):
            raise AssertionError

        def track_decode(self, *a, **k):
            raise AssertionError

    class Stepwise:
        model = torch.nn.Identity()

    class Tracker(torch.nn.Module):
        results_on_device = False

    class WithMasks(Tracker):
        def set_masks(self, masks):
            pass

    class OnDevice:
        is_cuda = True

    def model(tracker=None, predictor=None, **kw):
        return SamPt(tracker or Tracker(), predictor or Predictor(), sam_iou_threshold=0.0, **kw).eval()

    on, cpu = OnDevice(), torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    assert model().device_reinit is False and not model()._device_reinit_active(on)
    assert model(device_reinit=True)._device_reinit_active(on)
    assert not model(device_reinit=True)._device_reinit_active(cpu)
    assert not model(WithMasks(), device_reinit=True)._device_reinit_active(on)
    assert not model(predictor=Stepwise(), device_reinit=True)._device_reinit_active(on)
    # device_tracks with re-initialisation: the host path unless device_reinit is active too
    assert not model(device_tracks=True, use_point_reinit=True)._device_tracks_active(on)
    assert model(device_tracks=True, use_point_reinit=True, device_reinit=True)._device_tracks_active(on)
    assert not model(device_tracks=True, use_point_reinit=True, device_reinit=True)._device_tracks_active(cpu)


def test_entry_points_are_declared_bound_and_built():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    for name in ("sampt_bits_row_prefix", "sampt_bits_select"):
        assert f"int {name}(" in hdr, f"{name} is not declared in include/sampt_hip.h"
        assert name in open(os.path.join(ROOT, "sam_pt_amd", "_lib.py")).read()
    assert " mask_points.hip " in open(os.path.join(ROOT, "sam_pt_amd", "csrc", "Makefile")).read()
    assert _lib is not None
