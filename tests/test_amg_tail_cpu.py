"""CPU side of the automatic mask generator's device tail (no GPU needed): the C ABI surface, the generator's resolution of
``device_tail`` on a CPU predictor, and the "min-root" restatement of the small-region clean-up — connected components
labelled by the smallest linear pixel index — that csrc/amg_tail.hip implements, pinned on ``A.remove_small_regions``.
The seeded masks of the GPU tests (tests/test_gpu_amg_tail.py) are built here."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sam_ref as R
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_amg_regions_workspace_bytes", "sampt_amg_regions", "sampt_amg_nms_workspace_bytes", "sampt_amg_nms")
THRESHOLDS = (1, 6, 100, 10 ** 9)


# --------------------------------------------------------------------------------------------------------------------
# seeded masks: blobs (upsampled noise), speckle, a few stamped squares
# --------------------------------------------------------------------------------------------------------------------
def seeded_masks(n: int, h: int, w: int, seed: int) -> torch.Tensor:
    """bool (n, h, w): randn(n, 1, h//8+2, w//8+2) upsampled bilinearly and thresholded at 0.3, XOR a 0.4 % speckle, then six
    random 2-11 px squares of random value per mask."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 1, h // 8 + 2, w // 8 + 2, generator=g)
    m = F.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)[:, 0] > 0.3
    m = m ^ (torch.rand(n, h, w, generator=g) < 0.004)
    for i in range(n):
        for _ in range(6):
            s = int(torch.randint(2, 12, (1,), generator=g))
            y = int(torch.randint(0, max(1, h - s + 1), (1,), generator=g))
            x = int(torch.randint(0, max(1, w - s + 1), (1,), generator=g))
            m[i, y:y + s, x:x + s] = bool(torch.randint(0, 2, (1,), generator=g))
    return m


def offset_view(x: torch.Tensor, dev) -> torch.Tensor:
    """x on the HIP device ``dev``, as a view that starts one element into its storage: 1 byte (bool, uint8) or 4 bytes (float32)
    past an allocation's alignment, so that no row and no 4-pixel load is aligned (the device allocator aligns to 16 bytes and
    more; the assert below holds the helper to that)."""
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=dev)
    flat[1:] = x.flatten().to(dev)
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == x.element_size() and view.is_contiguous()
    return view


def tie_mask() -> np.ndarray:
    """6 x 6, two 2-px components: with every component small the first in raster order survives."""
    m = np.zeros((6, 6), dtype=bool)
    m[1, 3:5] = True
    m[4, 0:2] = True
    return m


def host_clean(mask: np.ndarray, min_area):
    """The yardstick: holes, then islands, as ``_postprocess_small_regions`` calls them."""
    m, changed_h = A.remove_small_regions(mask, min_area, mode="holes")
    m, changed_i = A.remove_small_regions(m, min_area, mode="islands")
    return m, bool(changed_h or changed_i)


# --------------------------------------------------------------------------------------------------------------------
# the min-root restatement
# --------------------------------------------------------------------------------------------------------------------
def min_root_labels(work: np.ndarray) -> np.ndarray:
    """int64 (h, w): for a work pixel the smallest linear index of its 8-connected component, h * w elsewhere."""
    h, w = work.shape
    big = h * w
    lab = np.where(work, np.arange(big, dtype=np.int64).reshape(h, w), big)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        nb = np.min(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)
        new = np.where(work, nb, big)
        if np.array_equal(new, lab):
            return lab
        lab = new


def min_root_clean(mask: np.ndarray, min_area):
    """Holes then islands on min-root labels: sizes are counted at the root's index, so ``argmax`` over them returns, among
    the largest components, the one with the smallest root = the one whose first pixel comes first in raster order."""
    h, w = mask.shape
    work = ~mask
    lab = min_root_labels(work)
    sizes = np.bincount(lab[work], minlength=h * w + 1)
    fill = work & (sizes[lab] < min_area)
    changed_h = bool(fill.any())
    m = mask | fill
    lab = min_root_labels(m)
    sizes = np.bincount(lab[m], minlength=h * w + 1)
    small = m & (sizes[lab] < min_area)
    changed_i = bool(small.any())
    keep = m & ~small
    if changed_i and not keep.any():
        keep = lab == int(np.argmax(sizes[:h * w]))
    return keep, changed_h or changed_i


# --------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_binds_and_exports_the_tail_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
    for name in ("sampt_amg_regions", "sampt_amg_nms"):            # house style: int return code, stream last
        res, args = _lib._SIGS[name]
        assert res is _lib.c_int and args[-1] is _lib._P


def test_abi_refuses_bad_shapes_without_touching_memory():
    from sam_pt_amd import _lib
    lib = _lib.load()
    assert lib.sampt_amg_regions_workspace_bytes(1, 46341, 46341) == 0           # h * w >= 2^31
    assert lib.sampt_amg_regions_workspace_bytes(3, 96, 128) >= 3 * 96 * 128 * 8
    assert lib.sampt_amg_regions(None, 1, 46341, 46341, 6, None, None, None, None, None, 0, None) != 0
    assert b"2^31" in lib.sampt_last_error()
    assert lib.sampt_amg_regions(None, 1, 0, 5, 6, None, None, None, None, None, 0, None) != 0
    assert lib.sampt_amg_regions(None, 1, 8, 8, 6, None, None, None, None, None, 0, None) != 0     # null pointers
    assert lib.sampt_amg_nms(None, None, -1, 0.7, None, None, None, 0, None) != 0
    assert lib.sampt_amg_nms(None, None, 5, 0.7, None, None, None, 0, None) != 0
    assert lib.sampt_amg_nms_workspace_bytes(3072) >= 3072 * 48 * 8


def _image(h, w, seed):
    from sam_pt_amd.synth import synthetic_clip
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


def same_records(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        assert ra["segmentation"].dtype == rb["segmentation"].dtype and np.array_equal(ra["segmentation"], rb["segmentation"])
        for k in ("area", "bbox", "predicted_iou", "point_coords", "crop_box"):
            assert ra[k] == rb[k] and type(ra[k]) is type(rb[k]), k
        sa, sb = ra["stability_score"], rb["stability_score"]
        assert sa == sb or (np.isnan(sa) and np.isnan(sb))


def test_generator_device_tail_resolves_to_host_on_a_cpu_predictor():
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    img = _image(96, 128, 3)
    kw = dict(points_per_side=2, points_per_batch=8, pred_iou_thresh=0.0, stability_score_thresh=0.0,
              stability_score_offset=0.02, crop_n_layers=1, crop_n_points_downscale_factor=2, min_mask_region_area=6)
    auto = A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), device_tail=None, **kw)
    host = A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), device_tail=False, **kw)
    assert auto.device_tail is False and host.device_tail is False
    a, b = auto.generate(img), host.generate(img)
    assert len(a) > 0
    same_records(a, b)
    with pytest.raises(ValueError, match="device_tail"):
        A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, cfg), device_tail=True, **kw)


def test_device_functions_refuse_cpu_tensors():
    from sam_pt_amd._lib import SamptError
    with pytest.raises(SamptError):
        A.nms_device(torch.zeros(3, 4), torch.zeros(3), 0.7)
    with pytest.raises(SamptError):
        A.remove_small_regions_device(torch.zeros(2, 8, 8, dtype=torch.bool), 6)


@pytest.mark.parametrize("min_area", THRESHOLDS)
def test_min_root_restatement_equals_remove_small_regions(min_area):
    stacks = [seeded_masks(4, 96, 128, 11).numpy(), seeded_masks(2, 90, 121, 12).numpy()]
    n_changed = 0
    for stack in stacks:
        for m in stack:
            exp, exp_changed = host_clean(m, min_area)
            got, got_changed = min_root_clean(m, min_area)
            assert np.array_equal(got, exp) and got_changed == exp_changed
            n_changed += int(exp_changed)
    assert n_changed == (0 if min_area == 1 else 6)              # the recipe: nothing changes at 1, every mask does above
    for m in (tie_mask(), np.zeros((9, 13), dtype=bool), np.ones((9, 13), dtype=bool)):
        exp, exp_changed = host_clean(m, min_area)
        got, got_changed = min_root_clean(m, min_area)
        assert np.array_equal(got, exp) and got_changed == exp_changed


def test_tie_rule_keeps_the_first_component_in_raster_order():
    out, changed = host_clean(tie_mask(), 6)
    assert changed and out[1, 3:5].all() and int(out.sum()) == 2
    got, _ = min_root_clean(tie_mask(), 6)
    assert np.array_equal(got, out)
