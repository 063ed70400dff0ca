"""``sampt_bits_row_prefix`` / ``sampt_bits_select`` (csrc/mask_points.hip) on planes packed by ``sampt_bits_pack`` from f32 logits:
the prefix against the host's cumulative row counts and EVERY rank of every plane, set and inverted, against ``nonzero()``, with
``==``.  Shapes: a single pixel, widths below / at / across a 64-column group and a 256-column tile, heights below / at / across a
64-row band and over two bands."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(h, w) for h in (1, 63, 64, 65, 130) for w in (1, 3, 5, 64, 255, 257)]


def _planes(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    m = np.zeros((6, h, w), dtype=bool)
    m[1] = True
    m[2, h - 1, w - 1] = True
    m[3, 0, 0] = True
    m[4] = rng.random((h, w)) < 0.02
    m[5] = rng.random((h, w)) < 0.5
    return m


def _pack(m, dev):
    from sam_pt_amd.vis_metrics import bits_pack_device
    logits = torch.from_numpy(np.where(m, 1.5, -0.5).astype(np.float32)).to(dev)
    return bits_pack_device(logits, threshold=0.0)


@pytest.mark.parametrize("h,w", SHAPES)
def test_prefix_and_every_rank_equal_nonzero(dev, h, w):
    from sam_pt_amd.mask_points import row_prefix_device, select_device
    m = _planes(h, w)
    n = len(m)
    bits, area = _pack(m, dev)
    assert np.array_equal(area.cpu().numpy(), m.sum(axis=(1, 2)))
    prefix = row_prefix_device(bits, h)
    want_prefix = np.zeros((n, h + 1), dtype=np.int32)
    want_prefix[:, 1:] = np.cumsum(m.sum(axis=2), axis=1)
    assert prefix.dtype == torch.int32 and np.array_equal(prefix.cpu().numpy(), want_prefix)
    # every rank of every plane, both polarities, the out-of-range ranks and a plane index n: ONE launch, shuffled
    queries, want = [], []
    for i in range(n):
        for invert in (0, 1):
            nz = np.argwhere(~m[i] if invert else m[i]).astype(np.float32)
            queries.append(np.stack([np.full(len(nz), i), np.full(len(nz), invert), np.arange(len(nz))], axis=1).astype(np.int32))
            want.append(nz)
            queries.append(np.array([(i, invert, -1), (i, invert, len(nz)), (n, invert, 0), (-1, invert, 0)], dtype=np.int32))
            want.append(np.full((4, 2), -1.0, dtype=np.float32))
    queries, want = np.concatenate(queries), np.concatenate(want)
    assert len(queries) == n * (h * w + 8)                     # a plane's set and clear pixels are all its pixels
    order = np.random.default_rng(w).permutation(len(queries))
    got = select_device(bits, prefix, h, queries[order])
    assert got.dtype == torch.float32 and got.shape == (len(queries), 2)
    got = got.cpu().numpy()
    bad = np.nonzero((got != want[order]).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(queries)} queries differ; first: {queries[order][bad[0]]} -> {got[bad[0]]}, want {want[order][bad[0]]}"


def test_equals_host_restatement_and_queries_on_the_device(dev):
    """The kernels against sam_pt_amd/mask_points.py's restatement on the same words; queries handed over as a device tensor."""
    from sam_pt_amd import mask_points as MP
    h, w = 130, 257
    m = _planes(h, w)
    bits, _ = _pack(m, dev)
    words = bits.cpu().numpy().view(np.uint64)
    prefix = MP.row_prefix_device(bits, h)
    assert np.array_equal(prefix.cpu().numpy(), MP.row_prefix(words, h))
    rng = np.random.default_rng(9)
    q = np.stack([rng.integers(-1, 7, 500), rng.integers(0, 2, 500), rng.integers(-2, h * w + 2, 500)], axis=1).astype(np.int32)
    got = MP.select_device(bits, prefix, h, torch.from_numpy(q).to(dev))
    assert np.array_equal(got.cpu().numpy(), MP.select_ranks(words, prefix.cpu().numpy(), h, q))


def test_no_queries_no_planes_and_bad_shapes(dev):
    from sam_pt_amd import _lib
    from sam_pt_amd.mask_points import row_prefix_device, select_device
    bits, _ = _pack(_planes(65, 5), dev)
    prefix = row_prefix_device(bits, 65)
    assert select_device(bits, prefix, 65, np.zeros((0, 3), dtype=np.int32)).shape == (0, 2)        # nq = 0: success
    lib = _lib.load()
    q = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    out = torch.full((2, 2), 7.0, device=dev)
    with _lib.device_guard(dev):
        s = _lib.stream_ptr()
        assert lib.sampt_bits_select(_lib.ptr(bits), _lib.ptr(prefix), 6, 65, 5, _lib.ptr(q), 0, _lib.ptr(out), s) == 0
        assert lib.sampt_bits_select(_lib.ptr(bits), _lib.ptr(prefix), 0, 65, 5, _lib.ptr(q), 2, _lib.ptr(out), s) == 0    # n = 0: a no-op
        assert lib.sampt_bits_row_prefix(_lib.ptr(bits), 0, 65, 5, _lib.ptr(prefix), s) == 0
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        by = torch.empty(16, dtype=torch.uint8, device=dev)
        for hh, ww in ((0, 5), (65, 0), (-1, 5), (1 << 16, 1 << 15)):                                # the code bp_shape_ok gives elsewhere
            bad = lib.sampt_bits_unpack(_lib.ptr(bits), 1, hh, ww, _lib.ptr(by), s)
            assert bad != 0
            assert lib.sampt_bits_row_prefix(_lib.ptr(bits), 1, hh, ww, _lib.ptr(prefix), s) == bad
            assert lib.sampt_bits_select(_lib.ptr(bits), _lib.ptr(prefix), 1, hh, ww, _lib.ptr(q), 2, _lib.ptr(out), s) == bad
        assert lib.sampt_bits_select(_lib.ptr(bits), _lib.ptr(prefix), 6, 65, 5, _lib.ptr(q), -1, _lib.ptr(out), s) != 0
        assert lib.sampt_bits_select(_lib.ptr(bits), None, 6, 65, 5, _lib.ptr(q), 2, _lib.ptr(out), s) != 0
