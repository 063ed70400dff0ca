"""The four kernels that read pixels through the bit-plane tile reader (csrc/bitplane.h) against each other: ``bits_pack_device``
(csrc/vis_eval.hip), ``rle_encode_device`` (csrc/rle.hip), ``jf_counts_device`` (csrc/vos_metrics.hip) and ``jf_pairs_counts_device``
(csrc/vos_pairs.hip) see the same stack of masks, given as bytes, as float32 logits and as a uint8 index map.  Every comparison
is ``==`` on integers.

The shapes: narrower than 4 (element loads), exactly 4 wide and exactly one band, a width that is no multiple of 4 with a second
band of one row, more than one block of 256 columns, three bands with three column blocks."""
import numpy as np
import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd import vis_metrics as VI
from sam_pt_amd import vos_metrics as VM
from tests.test_amg_tail_cpu import seeded_masks

pytestmark = pytest.mark.gpu

THR, VALUE = 0.25, 7


def three_kinds(h, w):
    """bool masks (3, h, w) and the same masks as uint8 bytes, as float32 logits (set iff > THR; THR itself and NaN among the clear
    pixels) and as a uint8 index map (set iff == VALUE; other non-zero values among the clear pixels)."""
    masks = seeded_masks(3, h, w, seed=600 + h + w)
    g = torch.Generator().manual_seed(h * w)
    odd = torch.rand(masks.shape, generator=g)
    f = torch.where(masks, THR + 0.01 + torch.rand(masks.shape, generator=g), THR - 0.01 - torch.rand(masks.shape, generator=g))
    f = torch.where(~masks & (odd < 0.1), torch.full_like(f, float("nan")), f)
    f = torch.where(~masks & (odd > 0.9), torch.full_like(f, THR), f).float()
    index = torch.where(masks, VALUE, torch.where(odd < 0.3, 2, torch.where(odd > 0.8, 255, 0))).to(torch.uint8)
    assert torch.equal(f > THR, masks) and torch.equal(index == VALUE, masks)
    return masks, {"bytes": (masks.to(torch.uint8) * 255, {}, {}, {}),
                   "f32": (f, dict(threshold=THR), dict(seg_threshold=THR, ann_threshold=THR), dict(seg_threshold=THR, ann_threshold=THR)),
                   "index": (index, dict(values=[VALUE] * 3), dict(seg_values=[VALUE] * 3, ann_values=[VALUE] * 3),
                             dict(seg_values=[VALUE], ann_values=[VALUE]))}


@pytest.mark.parametrize("shape", ((5, 3), (64, 4), (65, 7), (70, 261), (129, 515)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_four_readers_agree(dev, shape):
    h, w = shape
    masks, kinds = three_kinds(h, w)
    areas = masks.flatten(1).sum(1)
    assert areas.max() > 0
    lib = _lib.load()
    packed = {}
    for kind, (x, pack_kw, jf_kw, pairs_kw) in kinds.items():
        x = x.to(dev)
        bits, area = VI.bits_pack_device(x, **pack_kw)
        packed[kind] = bits
        back = torch.empty((3, h, w), dtype=torch.uint8, device=dev)
        with _lib.device_guard(dev):
            _lib.check(lib.sampt_bits_unpack(_lib.ptr(bits), 3, h, w, _lib.ptr(back), _lib.stream_ptr()), "sampt_bits_unpack")
        assert torch.equal(back.cpu(), masks.to(torch.uint8)), f"{kind}: pack -> unpack is not the input"
        assert area.cpu().tolist() == areas.tolist(), kind
        if kind != "index":                                               # (the encoder has no index-map input)
            assert A.rle_encode_device(x, threshold=pack_kw.get("threshold"))[1].cpu().tolist() == area.cpu().tolist(), kind
        counts = VM.jf_counts_device(x, x, radius=3, **jf_kw)
        assert counts[:, 0].cpu().tolist() == counts[:, 1].cpu().tolist() == area.cpu().tolist(), kind
        sides = (x, x) if kind == "index" else (x[None], x[None])         # one mask per frame: (T, h, w) map or (1, T, h, w) planes
        _, seg_stat, ann_stat = VM.jf_pairs_counts_device(*sides, radius=3, return_stats=True, **pairs_kw)
        assert seg_stat[0, :, 0].cpu().tolist() == ann_stat[0, :, 0].cpu().tolist() == area.cpu().tolist(), kind
    assert torch.equal(packed["bytes"], packed["f32"]) and torch.equal(packed["bytes"], packed["index"])
    assert np.array_equal(packed["bytes"].cpu().numpy().view(np.uint64), VI.pack_bits(masks.numpy()))
