"""GPU tests of the automatic mask generator's device tail: the small-region clean-up (``sampt_amg_regions``), greedy box NMS
(``sampt_amg_nms``) and the generator with ``device_tail=True`` against ``False``.  Every expectation is computed live on the
CPU by the host functions of sam_pt_amd/automatic_mask_generator.py (``remove_small_regions`` holes-then-islands,
``batched_mask_to_box``, ``nms``); every comparison is ``torch.equal`` / ``==``: integer and threshold logic has no tolerance."""
import numpy as np
import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd.sam_predictor import SamHip, SamPredictor
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
from tests.test_amg_tail_cpu import THRESHOLDS, host_clean, same_records, seeded_masks, tie_mask
from tests.util import synthetic_clip

pytestmark = pytest.mark.gpu

CFG = SAM_CONFIGS["vit_test"]


def _expect(masks: torch.Tensor, min_area):
    """masks bool (n, h, w) on the CPU -> (masks, changed, areas, boxes) of the host tail."""
    outs, changed = [], []
    for m in masks.numpy():
        o, c = host_clean(m, min_area)
        outs.append(torch.as_tensor(o))
        changed.append(c)
    out = torch.stack(outs) if outs else masks.clone()
    return out, torch.tensor(changed, dtype=torch.bool), out.flatten(-2).sum(-1), A.batched_mask_to_box(out)


def _check(dev, masks: torch.Tensor, min_area, what="", **kw):
    e_m, e_c, e_a, e_b = _expect(masks, min_area)
    g_m, g_c, g_a, g_b = A.remove_small_regions_device(masks.to(dev), min_area, **kw)
    assert g_m.dtype == torch.bool and g_c.dtype == torch.bool and g_a.dtype == torch.int64 and g_b.dtype == torch.int64
    assert g_m.device.type == "cuda" and g_b.shape == (masks.shape[0], 4)
    g_m, g_c, g_a, g_b = g_m.cpu(), g_c.cpu(), g_a.cpu(), g_b.cpu()
    bad = [i for i in range(masks.shape[0]) if not torch.equal(g_m[i], e_m[i])]
    assert not bad, f"{what} min_area {min_area}: masks {bad} differ ({[int((g_m[i] ^ e_m[i]).sum()) for i in bad]} pixels)"
    assert torch.equal(g_c, e_c), (what, min_area, g_c.tolist(), e_c.tolist())
    assert torch.equal(g_a, e_a), (what, min_area, g_a.tolist(), e_a.tolist())
    assert torch.equal(g_b, e_b), (what, min_area, g_b.tolist(), e_b.tolist())
    return e_c


# ------------------------------------------------------------------------------------------------------------ clean-up
@pytest.mark.parametrize("shape", [(96, 128, 12), (90, 121, 6), (7, 300, 3), (300, 7, 3), (1, 1, 2), (576, 1024, 4)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_regions_seeded_masks_vs_host(dev, shape):
    h, w, n = shape
    masks = seeded_masks(n, h, w, seed=100 + h + w)
    if (h, w) == (1, 1):
        masks[0], masks[1] = True, False
    for min_area in THRESHOLDS:
        changed = _check(dev, masks, min_area, f"{h}x{w}")
        if min(h, w) >= 90:                                      # the recipe: nothing changes at 1, every mask does above
            assert int(changed.sum()) == (0 if min_area == 1 else n)


def test_regions_trivial_and_tie_masks(dev):
    for min_area in THRESHOLDS:
        flat = torch.stack([torch.zeros(33, 70, dtype=torch.bool), torch.ones(33, 70, dtype=torch.bool)])
        _check(dev, flat, min_area, "all-False / all-True")
        _check(dev, torch.as_tensor(tie_mask())[None], min_area, "tie")
    m, changed, area, box = A.remove_small_regions_device(torch.as_tensor(tie_mask())[None].to(dev), 6)
    assert bool(changed[0]) and int(area[0]) == 2 and box[0].tolist() == [3, 1, 4, 1]     # the first in raster order survives
    empty = A.remove_small_regions_device(torch.zeros(0, 5, 5, dtype=torch.bool, device=dev), 6)
    assert empty[0].shape == (0, 5, 5) and empty[1].shape == (0,) and empty[3].shape == (0, 4)


def _structured(h, w):
    """Masks that stress the seam merge (tiles are 64 x 16) and the length of the label chains."""
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    snake = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == w - 1)) | ((yy % 4 == 3) & (xx == 0))      # one 1-px path over the frame
    comb = (yy == 0) | (xx % 2 == 0)
    checker = (yy + xx) % 2 == 0                                                          # linked only diagonally
    rings = (torch.maximum((yy - h // 2).abs(), (xx - w // 2).abs()) // 2) % 2 == 0       # holes in islands in holes
    corners = ((yy % 16 == 15) & (xx % 64 == 63)) | ((yy % 16 == 0) & (xx % 64 == 0))      # diagonal pairs across tile corners
    anti = ((yy % 16 == 15) & (xx % 64 == 0)) | ((yy % 16 == 0) & (xx % 64 == 63))
    blocks = ((yy % 16 == 15) | (yy % 16 == 0)) & ((xx % 64 == 63) | (xx % 64 == 0))       # 2 x 2 blocks on four tiles each
    vsnake = (xx % 2 == 0) | ((xx % 4 == 1) & (yy == h - 1)) | ((xx % 4 == 3) & (yy == 0))    # the same, column-wise
    stack = torch.stack([snake, comb, checker, rings, corners, anti, blocks, vsnake])
    return torch.cat([stack, ~stack])


@pytest.mark.parametrize("hw", [(96, 128), (90, 121), (131, 197)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_regions_structured_masks_vs_host(dev, hw):
    masks = _structured(*hw)
    for min_area in THRESHOLDS + (3, 200):
        _check(dev, masks, min_area, f"structured {hw}")


def test_regions_chunked_workspace_and_repeatability(dev):
    lib = _lib.load()
    masks = seeded_masks(12, 96, 128, seed=7)
    small_ws = lib.sampt_amg_regions_workspace_bytes(5, 96, 128)                 # 12 masks through a 5-mask workspace: 5 + 5 + 2
    assert small_ws < lib.sampt_amg_regions_workspace_bytes(12, 96, 128)
    for min_area in (6, 100):
        _check(dev, masks, min_area, "chunked", workspace_bytes=small_ws)
        _check(dev, masks, min_area, "one at a time", workspace_bytes=lib.sampt_amg_regions_workspace_bytes(1, 96, 128))
    big = seeded_masks(3, 576, 1024, seed=8).to(dev)
    a = A.remove_small_regions_device(big, 100)
    b = A.remove_small_regions_device(big, 100)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(_lib.SamptError, match="workspace"):
        A.remove_small_regions_device(masks.to(dev), 6, workspace_bytes=lib.sampt_amg_regions_workspace_bytes(1, 96, 128) - 16)


# ----------------------------------------------------------------------------------------------------------------- NMS
def _nms_check(dev, boxes: torch.Tensor, scores: torch.Tensor, what=""):
    for thr in (0.3, 0.7):
        exp = A.nms(boxes, scores, thr)
        got = A.nms_device(boxes.to(dev), scores.to(dev), thr)
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        assert got.cpu().tolist() == exp.tolist(), f"{what} thr {thr}: {len(got)} kept on the device, {len(exp)} on the host"


def test_nms_integer_boxes_vs_host(dev):
    rng = np.random.default_rng(4)                                   # the boxes of tests/test_amg.py::test_nms_vs_bruteforce
    for n in (0, 1, 40, 300):
        xy = rng.integers(0, 80, size=(n, 2))
        wh = rng.integers(0, 40, size=(n, 2))                        # includes degenerate (zero-area) boxes
        boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
        scores = rng.random(n).astype(np.float32)
        if n >= 40:
            boxes[5], scores[5] = boxes[3], scores[3]                # exact duplicate with a tied score
        _nms_check(dev, torch.from_numpy(boxes), torch.from_numpy(scores), f"integer n={n}")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300, 3072])
def test_nms_float_boxes_vs_host(dev, n):
    g = torch.Generator().manual_seed(1000 + n)
    span = 40.0 + 0.15 * n                                           # keeps the share of overlapping pairs interesting at every n
    xy = torch.rand(n, 2, generator=g) * span
    wh = torch.rand(n, 2, generator=g) * 30.0
    boxes = torch.cat([xy, xy + wh], dim=1)
    if n >= 63:
        boxes[7] = boxes[2]                                          # duplicates, shifted copies (IoU right around the thresholds)
        boxes[9] = boxes[4] + torch.tensor([0.0, 0.0, wh[4, 0] * 3 / 7, 0.0])
        boxes[11, 2:] = boxes[11, :2]                                # zero-area box: 0 / 0 with itself only
    scores = torch.rand(n, generator=g)
    _nms_check(dev, boxes, scores, f"float n={n}")
    _nms_check(dev, boxes, torch.full((n,), 0.5), f"all scores equal n={n}")
    _nms_check(dev, boxes, (torch.rand(n, generator=g) < 0.8).float(), f"scores in {{0, 1}} n={n}")
    if n:
        kept = A.nms_device(boxes.to(dev), scores.to(dev), 0.7)
        assert 0 < len(kept) <= n and len(set(kept.tolist())) == len(kept)


# ----------------------------------------------------------------------------------------------------------- generator
def _image(h, w, seed):
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


@pytest.mark.parametrize("case", ["fused crops + clean-up", "fused plain", "unfused crops + clean-up"])
def test_generator_device_tail_equals_host_tail(dev, case):
    sd = init_sam_state_dict(CFG, 72)
    pred = SamPredictor(SamHip(config=CFG, state_dict=sd, precision="f32").to(dev))
    img = _image(96, 128, 3)
    kw = dict(points_per_side=8, points_per_batch=16, pred_iou_thresh=0.0, stability_score_thresh=0.0, stability_score_offset=0.02)
    if "crops" in case:
        kw.update(points_per_side=4, crop_n_layers=1, crop_n_points_downscale_factor=2, min_mask_region_area=6)
    fused = case.startswith("fused")
    auto = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=fused, **kw)
    assert auto.device_tail is True                                  # None resolves to the device tail on a HIP predictor
    dev_gen = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=fused, device_tail=True, **kw)
    host_gen = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=fused, device_tail=False, **kw)
    assert dev_gen.device_tail is True and host_gen.device_tail is False
    d, h = dev_gen.generate(img), host_gen.generate(img)
    print(f"{case}: {len(d)} records on the device tail, {len(h)} on the host tail")
    assert len(h) > 0
    same_records(d, h)
    for r in d:
        assert r["area"] == int(r["segmentation"].sum())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    with pytest.raises(_lib.SamptError):
        A.remove_small_regions_device(torch.zeros(2, 8, 8, dtype=torch.bool), 6)                  # a CPU tensor
    with pytest.raises(_lib.SamptError):
        A.nms_device(torch.zeros(3, 4), torch.zeros(3), 0.7)
    with pytest.raises(_lib.SamptError):
        A.remove_small_regions_device(torch.zeros(2, 8, 8, dtype=torch.uint8, device=dev), 6)     # not bool
    with pytest.raises(_lib.SamptError):
        A.remove_small_regions_device(torch.zeros(8, 8, dtype=torch.bool, device=dev), 6)         # not a stack
    with pytest.raises(_lib.SamptError):
        A.nms_device(torch.zeros(3, 5, device=dev), torch.zeros(3, device=dev), 0.7)              # not (n, 4)
    with pytest.raises(_lib.SamptError):
        A.nms_device(torch.zeros(3, 4, device=dev), torch.zeros(2, device=dev), 0.7)
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.uint8, device=dev)                                            # never read: refused on the shape
    rc = lib.sampt_amg_regions(_lib.ptr(t), 1, 46341, 46341, 6, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t),
                               64, _lib.stream_ptr())
    assert rc != 0 and b"2^31" in lib.sampt_last_error()
    assert lib.sampt_amg_regions_workspace_bytes(1, 46341, 46341) == 0
