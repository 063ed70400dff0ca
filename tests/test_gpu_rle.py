"""GPU tests of the device run-length encoder (csrc/rle.hip: ``rle_encode_device`` / ``encode_rle``), the generator's RLE output
modes on the device tail and the VIS adapter's ``rle_results``.  Every expectation is computed live on the CPU by the host
functions of sam_pt_amd/automatic_mask_generator.py (``mask_to_rle``, ``coco_rle_string``, ``rle_to_mask``); every comparison
is ``==``: run lengths are integers."""
import numpy as np
import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd.sam_predictor import SamHip, SamPredictor
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
from tests.test_amg_tail_cpu import seeded_masks
from tests.test_rle_cpu import checkerboard, column_ends_set, last_pixel_only, stub_vos
from tests.util import synthetic_clip

pytestmark = pytest.mark.gpu

CFG = SAM_CONFIGS["vit_test"]


def _check(dev, masks: torch.Tensor, what="", **kw):
    """masks bool (n, h, w) on the CPU: counts, strings and areas of the device encoder against the host functions."""
    exp = A.mask_to_rle(masks)
    got, areas = A.rle_encode_device(masks.to(dev), **kw)
    assert areas.dtype == torch.int64 and areas.device.type == "cuda" and areas.shape == (masks.shape[0],)
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g["size"] == e["size"], (what, i)
        assert g["counts"] == e["counts"], f"{what}: mask {i}: {len(g['counts'])} runs on the device, {len(e['counts'])} on the host"
    assert areas.cpu().tolist() == masks.flatten(-2).sum(-1).tolist(), what
    comp, areas_c = A.rle_encode_device(masks.to(dev), compressed=True, **kw)
    assert [c["size"] for c in comp] == [e["size"] for e in exp]
    for i, (c, e) in enumerate(zip(comp, exp)):
        assert isinstance(c["counts"], str) and c["counts"] == A.coco_rle_string(e["counts"]), (what, i)
    assert torch.equal(areas_c, areas)
    return exp


# ---------------------------------------------------------------------------------------------------------- byte input
@pytest.mark.parametrize("shape", [(1, 1, 2), (63, 5, 3), (64, 4, 3), (65, 7, 3), (130, 33, 3), (65, 261, 3), (7, 300, 2), (300, 7, 2),
                                   (96, 128, 12), (576, 1024, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_seeded_stacks_vs_host(dev, shape):
    h, w, n = shape
    masks = seeded_masks(n, h, w, seed=300 + h + w)
    if (h, w) == (1, 1):
        masks[0], masks[1] = True, False
    exp = _check(dev, masks, f"{h}x{w}")
    if (h, w) == (576, 1024):
        print(f"576 x 1024: runs per mask {[len(e['counts']) for e in exp]}")
        assert all(len(e["counts"]) > 10000 for e in exp)


def test_uint8_and_leading_dimensions(dev):
    masks = seeded_masks(6, 65, 8, seed=9)
    exp = A.mask_to_rle(masks)
    got, areas = A.rle_encode_device((masks.to(torch.uint8) * 255).reshape(2, 3, 65, 8).to(dev))
    assert got == exp and areas.shape == (6,)
    one, _ = A.rle_encode_device(masks[2].to(dev))                   # a bare (H, W)
    assert one == exp[2:3]


def test_degenerate_and_structured_masks(dev):
    h, w = 70, 9
    flat = torch.stack([torch.zeros(h, w, dtype=torch.bool), torch.ones(h, w, dtype=torch.bool)])
    got, areas = A.rle_encode_device(flat.to(dev))
    assert got[0]["counts"] == [h * w] and got[1]["counts"] == [0, h * w] and areas.tolist() == [0, h * w]
    comp, _ = A.rle_encode_device(flat.to(dev), compressed=True)
    assert [c["counts"] for c in comp] == ["fc0", "0fc0"]
    for hh, ww in ((70, 9), (64, 8), (128, 256), (65, 260)):         # a set mask after a set mask: the carry stays inside a mask
        both = torch.ones(3, hh, ww, dtype=torch.bool)
        both[1, 0, 0] = False
        got = _check(dev, both, f"set after set {hh}x{ww}")
        assert got[0]["counts"] == [0, hh * ww] and got[2]["counts"] == [0, hh * ww] and got[1]["counts"] == [1, hh * ww - 1]
    cb = _check(dev, checkerboard()[None], "checkerboard")
    assert len(cb[0]["counts"]) == 938 and sum(cb[0]["counts"]) == 960
    _check(dev, checkerboard(64, 256)[None], "checkerboard 64x256")   # every bit of every word of a full tile
    _check(dev, checkerboard(64, 261)[None], "checkerboard 64x261")   # ... and of the lane that loads a row's last 4 pixels
    _check(dev, torch.stack([column_ends_set(), ~column_ends_set()]), "column ends")
    for hh in (128, 129):
        _check(dev, torch.stack([column_ends_set(hh, 8), ~column_ends_set(hh, 8)]), f"column ends, aligned, h = {hh}")
    for hh, ww in ((65, 7), (64, 4), (128, 260), (1, 5), (5, 1)):
        lp = _check(dev, last_pixel_only(hh, ww)[None], f"last pixel {hh}x{ww}")
        assert lp[0]["counts"] == [hh * ww - 1, 1]


def test_unaligned_base(dev):
    stack = seeded_masks(4, 65, 7, seed=21).to(dev)
    view = stack[1:]
    assert view.data_ptr() % 4 != 0
    got, areas = A.rle_encode_device(view)
    assert got == A.mask_to_rle(stack[1:].cpu()) and areas.cpu().tolist() == stack[1:].flatten(-2).sum(-1).cpu().tolist()
    wide = seeded_masks(3, 33, 12, seed=22).to(dev)                  # w % 4 == 0 and an odd byte offset: unaligned 4-pixel loads
    flat = torch.zeros(3 * 33 * 12 + 1, dtype=torch.bool, device=dev)
    flat[1:] = wide.flatten()
    off = flat[1:].view(3, 33, 12)
    assert off.data_ptr() % 4 == 1
    got, _ = A.rle_encode_device(off)
    assert got == A.mask_to_rle(wide.cpu())


# --------------------------------------------------------------------------------------------------------- float input
@pytest.mark.parametrize("shape", [(65, 7), (96, 128), (130, 33), (65, 261)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float_input_with_threshold(dev, shape):
    h, w = shape
    g = torch.Generator().manual_seed(31 + h)
    for thr in (0.0, 0.25, -1.5):
        x = torch.randn(3, h, w, generator=g)
        x[0, ::3, ::2] = thr                                         # exactly the threshold: clear
        x[0, 1::3, 1::2] = float(np.nextafter(np.float32(thr), np.float32(np.inf)))   # the next float above it: set
        x[1, 5, :] = -0.0
        x[1, 6, :] = 0.0
        x[1, 0, 0] = float("nan")
        x[1, 7, ::2] = float("nan")
        x[2, 9, :] = float("inf")
        x[2, 10, :] = float("-inf")
        exp = A.mask_to_rle(x > thr)
        got, areas = A.rle_encode_device(x.to(dev), threshold=thr)
        assert got == exp, (h, w, thr)
        assert areas.cpu().tolist() == (x > thr).flatten(-2).sum(-1).tolist()
        comp, _ = A.rle_encode_device(x.to(dev), threshold=thr, compressed=True)
        assert [c["counts"] for c in comp] == [A.coco_rle_string(e["counts"]) for e in exp]
        assert A.encode_rle(x.to(dev), threshold=thr, compressed=True) == comp
    view = torch.randn(3 * h * w + 1, generator=g).to(dev)[1:].view(3, h, w)      # 4-byte but not 16-byte aligned
    assert view.data_ptr() % 16 == 4
    assert A.rle_encode_device(view, threshold=0.0)[0] == A.mask_to_rle(view.cpu() > 0.0)


# ------------------------------------------------------------------------------------- chunking, repeatability, n = 0
def test_chunked_workspace_repeatability_and_empty(dev):
    lib = _lib.load()
    masks = seeded_masks(5, 96, 128, seed=7)
    two = lib.sampt_rle_workspace_bytes(2, 96, 128)                  # 5 masks through a 2-mask workspace: 2 + 2 + 1
    assert two < lib.sampt_rle_workspace_bytes(5, 96, 128)
    _check(dev, masks, "chunked", workspace_bytes=two)
    _check(dev, masks, "one at a time", workspace_bytes=lib.sampt_rle_workspace_bytes(1, 96, 128))
    with pytest.raises(_lib.SamptError, match="workspace"):
        A.rle_encode_device(masks.to(dev), workspace_bytes=lib.sampt_rle_workspace_bytes(1, 96, 128) - 16)
    big = seeded_masks(3, 576, 1024, seed=8).to(dev)
    a, b = A.rle_encode_device(big, compressed=True), A.rle_encode_device(big, compressed=True)
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    recs, areas = A.rle_encode_device(torch.zeros(0, 5, 5, dtype=torch.bool, device=dev))
    assert recs == [] and areas.shape == (0,) and areas.dtype == torch.int64
    assert A.encode_rle(torch.zeros(0, 5, 5, device=dev), threshold=0.0, compressed=True) == []


def test_refusals(dev):
    with pytest.raises(_lib.SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8, device=dev))                       # float without a threshold
    with pytest.raises(_lib.SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8, dtype=torch.bool, device=dev), threshold=0.0)
    with pytest.raises(_lib.SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8, dtype=torch.int32, device=dev))
    with pytest.raises(_lib.SamptError):
        A.rle_encode_device(torch.zeros(8, dtype=torch.bool, device=dev))
    with pytest.raises(_lib.SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8, dtype=torch.float64, device=dev), threshold=0.0)


# ----------------------------------------------------------------------------------------------------------- generator
def _image(h, w, seed):
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


@pytest.mark.parametrize("min_area", [0, 6])
def test_generator_rle_modes_on_the_device_tail(dev, min_area):
    sd = init_sam_state_dict(CFG, 72)
    pred = SamPredictor(SamHip(config=CFG, state_dict=sd, precision="f32").to(dev))
    img = _image(96, 128, 3)
    kw = dict(points_per_side=4, points_per_batch=16, pred_iou_thresh=0.0, stability_score_thresh=0.0, stability_score_offset=0.02,
              min_mask_region_area=min_area)
    gens = {(mode, tail): A.SamAutomaticMaskGenerator(None, predictor=pred, output_mode=mode, device_tail=tail, **kw)
            for mode, tail in (("uncompressed_rle", True), ("uncompressed_rle", False), ("coco_rle", True), ("binary_mask", True))}
    d, h = gens["uncompressed_rle", True].generate(img), gens["uncompressed_rle", False].generate(img)
    assert len(h) > 0 and len(d) == len(h)
    for rd, rh in zip(d, h):                                         # field for field
        assert set(rd) == set(rh)
        for k in rh:
            if k == "stability_score":
                assert rd[k] == rh[k] or (np.isnan(rd[k]) and np.isnan(rh[k]))
            else:
                assert rd[k] == rh[k] and type(rd[k]) is type(rh[k]), k
        assert isinstance(rd["segmentation"]["counts"], list) and rd["area"] == A.area_from_rle(rd["segmentation"])
    c, b = gens["coco_rle", True].generate(img), gens["binary_mask", True].generate(img)
    assert len(c) == len(b) == len(d)
    for rc, rb, rd in zip(c, b, d):
        assert set(rc["segmentation"]) == {"size", "counts"} and isinstance(rc["segmentation"]["counts"], str)
        assert rc["segmentation"]["size"] == [96, 128]
        assert np.array_equal(A.rle_to_mask(rc["segmentation"]), rb["segmentation"])
        assert rc["segmentation"]["counts"] == A.coco_rle_string(rd["segmentation"]["counts"])
        assert {k: v for k, v in rc.items() if k not in ("segmentation", "stability_score")} == \
               {k: v for k, v in rb.items() if k not in ("segmentation", "stability_score")}
    with pytest.raises(NotImplementedError):
        A.SamAutomaticMaskGenerator(None, predictor=pred, output_mode="coco_rle", device_tail=False, **kw)


# ------------------------------------------------------------------------------------------------------------- adapter
def test_vis_adapter_rle_results_from_hip_logits(dev):
    from sam_pt_amd.vis_to_vos_adapter import SamBasedVisToVosAdapter, instances_to_ytvis_json
    T, h, w = 3, 96, 128
    sd = init_sam_state_dict(CFG, 72)
    pred = SamPredictor(SamHip(config=CFG, state_dict=sd, precision="f32").to(dev))
    gen = A.SamAutomaticMaskGenerator(None, predictor=pred, points_per_side=4, points_per_batch=16, pred_iou_thresh=0.0,
                                      stability_score_thresh=0.0, stability_score_offset=0.02, box_nms_thresh=1.0)
    frames, _ = synthetic_clip(T=T, H=h, W=w, seed=3)
    inputs = [{"video_id": 4, "image": [f.to(dev) for f in frames], "height": h, "width": w, "length": T}]
    model, produced = stub_vos(T, h, w, device=dev)
    out = SamBasedVisToVosAdapter(model, gen, max_num_masks=3, masks_batch_size=2, rle_results=True)(inputs)
    assert len(produced) == 3 and "pred_masks" not in out and "pred_logits" not in out
    exp = [A.encode_rle(x, threshold=0.0, compressed=True) for x in produced]       # the CPU encoding of the same logits
    assert out["pred_rles"] == exp
    model2, produced2 = stub_vos(T, h, w, device=dev)
    plain = SamBasedVisToVosAdapter(model2, gen, max_num_masks=3, masks_batch_size=2)(inputs)
    assert all(torch.equal(a, b) for a, b in zip(produced, produced2))
    assert plain["pred_masks"][0].device.type == "cuda"
    assert instances_to_ytvis_json(inputs, plain) == instances_to_ytvis_json(inputs, out)
