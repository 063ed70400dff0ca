"""All-pairs J&F counts on the device (csrc/vos_pairs.hip) and the unsupervised protocol on HIP tensors, against the host
restatement computed live and against the pairwise kernel (``jf_counts_device``) fed the flattened pairs: every comparison is ``==``
on integers, and on J, F and the figures too, since both paths apply the same float64 formulas to the same integers.

The shapes cross every seam of the kernels: w < 4 (element loads), w % 4 != 0 (unaligned 4-pixel loads), more than one block of 256
columns, two, three and four bands of 64 rows; radius 64 runs on the 200-row image, where the k = 64 branch sees a band above and
below; (P, K) = (20, 7) is more than one 4 x 4 pair tile with both edges ragged, (2, 5) a ragged tile in both directions."""
import functools

import numpy as np
import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import vos_metrics as VM
from tests.test_amg_tail_cpu import offset_view, seeded_masks
from tests.test_vos_pairs_cpu import sequence

pytestmark = pytest.mark.gpu

SHAPES = ((5, 3), (64, 4), (70, 261), (130, 90), (200, 517))
PKT = ((1, 1, 1), (3, 2, 2), (20, 7, 3), (2, 5, 2))
SHAPE_RADII = [(s, r) for s in SHAPES for r in (0, 1, 3)] + [((200, 517), 64)]
THR = 0.25


@functools.lru_cache(maxsize=None)
def inputs(h, w, P, K, T):
    """Everything the tests below read, never written to: bool planes S (P, T, h, w) and A (K, T, h, w), void (T, h, w), the float
    form of S (above THR where set; NaN and THR itself where clear), and index maps made of S and A."""
    S = seeded_masks(P * T, h, w, 500 + h + w + P).reshape(P, T, h, w)
    A = torch.roll(seeded_masks(K * T, h, w, 700 + h + w + K), shifts=(1 % h, 2 % w), dims=(1, 2)).reshape(K, T, h, w)
    if K > 1 and P > 1:
        A[1] = S[0]                                                       # an exact match among the pairs
    void = seeded_masks(T, h, w, 900 + h + w) & seeded_masks(T, h, w, 901 + h + w)
    g = torch.Generator().manual_seed(h * w + P)
    f = torch.where(S, THR + 0.01 + torch.rand(S.shape, generator=g), THR - 0.01 - torch.rand(S.shape, generator=g))
    odd = torch.rand(S.shape, generator=g)
    f = torch.where(~S & (odd < 0.1), torch.full_like(f, float("nan")), f)
    f = torch.where(~S & (odd > 0.9), torch.full_like(f, THR), f)
    smap, amap = torch.zeros((T, h, w), dtype=torch.uint8), torch.zeros((T, h, w), dtype=torch.uint8)
    for p in range(P):
        smap[S[p]] = p + 1
    for k in range(K):
        amap[A[k]] = 2 * k + 3                                            # values that are not 1 .. K
    return S, A, void, f.float(), smap, amap


@functools.lru_cache(maxsize=None)
def host_planes(h, w, P, K, T, radius, with_void):
    S, A, void = inputs(h, w, P, K, T)[:3]
    return VM.jf_pairs_counts(S.numpy(), A.numpy(), void.numpy() if with_void else None, radius=radius, return_stats=True)


def assert_same(got, exp, what):
    assert len(got) == len(exp) == 3
    for g, e, name in zip(got, exp, ("counts", "seg stats", "ann stats")):
        assert g.dtype == torch.int64 and tuple(g.shape) == e.shape, f"{what}: {name} {g.dtype} {tuple(g.shape)} != {e.shape}"
        g = g.cpu().numpy()
        assert np.array_equal(g, e), f"{what}: {name} differ first at {np.argwhere(g != e)[:1].tolist()}: " \
                                     f"{g[g != e][:3].tolist()} != {e[g != e][:3].tolist()}"


def flattened_pairs(S, A, void, radius):
    """The (P, K, T) pairs as items of the pairwise kernel, sharing planes: (P, K, T, 6)."""
    (P, T), K = S.shape[:2], A.shape[0]
    p, k, t = np.meshgrid(np.arange(P), np.arange(K), np.arange(T), indexing="ij")
    kw = dict(seg_planes=(p * T + t).reshape(-1), ann_planes=(k * T + t).reshape(-1))
    if void is not None:
        kw["void_planes"] = t.reshape(-1)
    return VM.jf_counts_device(S, A, void, radius=radius, **kw).reshape(P, K, T, 6)


@pytest.mark.parametrize("shape,radius", SHAPE_RADII, ids=lambda v: str(v).replace(", ", "x"))
def test_shapes_and_radii(dev, shape, radius):
    (h, w), (P, K, T) = shape, PKT[1]
    S, A, void = (x.to(dev) for x in inputs(h, w, P, K, T)[:3])
    got = VM.jf_pairs_counts_device(S, A, void, radius=radius, return_stats=True)
    assert_same(got, host_planes(h, w, P, K, T, radius, True), f"{shape} r={radius}")
    assert torch.equal(got[0], flattened_pairs(S, A, void, radius))


@pytest.mark.parametrize("pkt", PKT, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_tiles(dev, shape, pkt):
    (h, w), (P, K, T) = shape, pkt
    S, A, void = (x.to(dev) for x in inputs(h, w, P, K, T)[:3])
    for with_void in (False, True):
        got = VM.jf_pairs_counts_device(S, A, void if with_void else None, radius=3, return_stats=True)
        assert_same(got, host_planes(h, w, P, K, T, 3, with_void), f"{shape} {pkt} void={with_void}")
    assert torch.equal(got[0], flattened_pairs(S, A, void, 3))
    assert torch.equal(VM.jf_pairs_counts_device(S, A, void, radius=3), got[0])        # repeatable, and without the stats


@pytest.mark.parametrize("with_void", (False, True), ids=("plain", "void"))
@pytest.mark.parametrize("source", ("bytes", "f32", "index"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sources(dev, shape, source, with_void):
    (h, w), (P, K, T) = shape, PKT[1]
    S, A, void, f, smap, amap = inputs(h, w, P, K, T)
    v = void.to(dev) if with_void else None
    if source == "bytes":                                                 # uint8 with values above 1 on one side, bool on the other
        got = VM.jf_pairs_counts_device((S.to(torch.uint8) * 7).to(dev), A.to(dev), v, radius=1, return_stats=True)
        exp = host_planes(h, w, P, K, T, 1, with_void)
    elif source == "f32":                                                 # NaN and the threshold itself are clear
        assert torch.isnan(f).any() and (f == THR).any() and torch.equal(f > THR, S)
        got = VM.jf_pairs_counts_device(f.to(dev), A.to(dev), v, radius=1, seg_threshold=THR, return_stats=True)
        exp = host_planes(h, w, P, K, T, 1, with_void)
        assert_same(VM.jf_pairs_counts_device(A.to(dev), f.to(dev), v, radius=1, ann_threshold=THR, return_stats=True),
                    VM.jf_pairs_counts(A.numpy(), f.numpy(), void.numpy() if with_void else None, radius=1, ann_threshold=THR,
                                       return_stats=True), f"{shape} f32 ann")
    else:                                                                 # the masks of a frame share its plane
        kw = dict(radius=1, seg_values=np.arange(1, P + 1), ann_values=2 * np.arange(K) + 3, return_stats=True)
        got = VM.jf_pairs_counts_device(smap.to(dev), amap.to(dev), v, **kw)
        exp = VM.jf_pairs_counts(smap.numpy(), amap.numpy(), void.numpy() if with_void else None, **kw)
        mixed = VM.jf_pairs_counts_device(smap.to(dev), A.to(dev), v, radius=1, seg_values=np.arange(1, P + 1), return_stats=True)
        assert torch.equal(mixed[1], got[1]) and torch.equal(mixed[2], torch.as_tensor(host_planes(h, w, P, K, T, 1, with_void)[2]).to(dev))
    assert_same(got, exp, f"{shape} {source} void={with_void}")


@pytest.mark.parametrize("shape", ((65, 7), (70, 261)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_unaligned_bases(dev, shape):
    """Every source one element into its storage: no row and no 4-pixel load is aligned."""
    (h, w), (P, K, T) = shape, PKT[3]
    S, A, void, f, smap, amap = inputs(h, w, P, K, T)
    v = offset_view(void, dev)
    exp = host_planes(h, w, P, K, T, 3, True)
    assert_same(VM.jf_pairs_counts_device(offset_view(S, dev), offset_view(A, dev), v, radius=3, return_stats=True), exp, f"{shape} bytes")
    assert_same(VM.jf_pairs_counts_device(offset_view(f, dev), offset_view(A, dev), v, radius=3, seg_threshold=THR, return_stats=True), exp,
                f"{shape} f32")
    kw = dict(radius=3, seg_values=np.arange(1, P + 1), ann_values=2 * np.arange(K) + 3, return_stats=True)
    assert_same(VM.jf_pairs_counts_device(offset_view(smap, dev), offset_view(amap, dev), v, **kw),
                VM.jf_pairs_counts(smap.numpy(), amap.numpy(), void.numpy(), **kw), f"{shape} index maps")


@pytest.mark.parametrize("shape", ((5, 3), (130, 90)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_empty_and_full_masks(dev, shape):
    h, w = shape
    S = torch.zeros((3, 2, h, w), dtype=torch.bool)
    S[1], S[2, 0] = True, True                                            # empty, full, full then empty
    A = torch.stack([S[1], S[0], inputs(h, w, 3, 2, 2)[0][0]])
    for radius in (0, 3):
        got = VM.jf_pairs_counts_device(S.to(dev), A.to(dev), radius=radius, return_stats=True)
        assert_same(got, VM.jf_pairs_counts(S.numpy(), A.numpy(), radius=radius, return_stats=True), f"{shape} r={radius}")
        c = got[0].cpu().numpy()
        assert c[0, 1].tolist() == [[0] * 6] * 2 and c[1, 0, 0].tolist() == [h * w, h * w, 0, 0, 0, 0]   # a full frame has no boundary
        assert got[1].cpu().numpy()[:, :, 0].tolist() == [[0, 0], [h * w, h * w], [h * w, 0]]
    void = torch.ones((2, h, w), dtype=torch.bool)                        # everything void: nothing is left
    assert not VM.jf_pairs_counts_device(S.to(dev), A.to(dev), void.to(dev), radius=1).any()


def test_workspace_split_by_frames(dev):
    (h, w), (P, K, T) = (70, 261), PKT[2]
    S, A, void = (x.to(dev) for x in inputs(h, w, P, K, T)[:3])
    exp = host_planes(h, w, P, K, T, 3, True)
    lib = _lib.load()
    per = int(lib.sampt_jf_pairs_workspace_bytes(P, K, 1, h, w, 3))
    assert per == 3 * (P + K) * 2 * w * 8 and int(lib.sampt_jf_pairs_workspace_bytes(P, K, T, h, w, 3)) == T * per
    assert int(lib.sampt_jf_pairs_workspace_bytes(P, K, T, h, w, 65)) == 0
    for frames, extra in ((1, 0), (2, 8), (3, 0)):                        # one frame per call; two, then the odd one; all at once
        got = VM.jf_pairs_counts_device(S, A, void, radius=3, return_stats=True, workspace_bytes=frames * per + extra)
        assert_same(got, exp, f"{frames} frames per call")
    smap, amap = (x.to(dev) for x in inputs(h, w, P, K, T)[4:])
    kw = dict(radius=3, seg_values=np.arange(1, P + 1), ann_values=2 * np.arange(K) + 3)
    assert torch.equal(VM.jf_pairs_counts_device(smap, amap, void, workspace_bytes=per, **kw), VM.jf_pairs_counts_device(smap, amap, void, **kw))
    with pytest.raises(_lib.SamptError, match="workspace"):
        VM.jf_pairs_counts_device(S, A, void, radius=3, workspace_bytes=per - 8)
    with pytest.raises(_lib.SamptError, match="radius"):
        VM.jf_pairs_counts_device(S, A, void, radius=65)
    with pytest.raises(_lib.SamptError):
        VM.jf_pairs_counts_device(S, A[:, :2], void)


@pytest.mark.parametrize("P,K", [(2, 4), (3, 3), (6, 3)], ids=lambda v: str(v))
def test_unsupervised_on_the_device_equals_the_host(dev, P, K):
    pred, gt = sequence(P, K)
    planes = pred[None] == np.arange(1, P + 1, dtype=np.uint8)[:, None, None, None]
    exp = VM.evaluate_unsupervised(pred, gt)
    for given in (torch.from_numpy(pred).to(dev), torch.from_numpy(planes).to(dev)):
        got = VM.evaluate_unsupervised(given, torch.from_numpy(gt).to(dev))
        for k in ("J", "F", "J_all", "F_all"):
            assert np.array_equal(got[k], exp[k]), k
        assert np.array_equal(got["assignment"][0], exp["assignment"][0]) and np.array_equal(got["assignment"][1], exp["assignment"][1])
        for k in ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay"):
            assert got[k] == exp[k], k
    with pytest.raises(ValueError, match="max_n_proposals"):
        VM.evaluate_unsupervised(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), max_n_proposals=P - 1)
