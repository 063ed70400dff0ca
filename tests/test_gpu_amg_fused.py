"""GPU tests of the fused automatic-mask-generator path: batched multimask decoding of point prompts against one image
(``sampt_sam_decode_points``), HQ-SAM's multimask rule, the scoring tail on low-res masks (``sampt_amg_score`` /
``sampt_amg_binarize``) and the generator end to end.  Every expectation is computed live on the CPU (oracle, and the
helpers of tests/test_amg_fused_cpu.py) from seeded inputs.

Bars: the project's own for this decoder at this geometry (test_predict_torch_multimask_vs_oracle): low-res logits 3e-4
max-abs, predicted IoU 1e-4; record matching as test_automatic_mask_generator_hip_vs_oracle."""
import numpy as np
import pytest
import torch

from oracle import sam_ref as R
from sam_pt_amd import _lib
from sam_pt_amd import automatic_mask_generator as A
from sam_pt_amd.sam_predictor import SamHip, SamPredictor
from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
from tests.test_amg_fused_cpu import hq_mask_decoder_ref, score_record_ref
from tests.util import max_abs, synthetic_clip

pytestmark = pytest.mark.gpu

LOW_BAR, IOU_BAR = 3e-4, 1e-4
FRAMES = {"96x128": (96, 128, 3), "90x121": (90, 121, 5)}      # the second: non-identity second resize, odd width
CFG = SAM_CONFIGS["vit_test"]


def _image(key):
    h, w, seed = FRAMES[key]
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


def _grid_points(key, n=8):
    h, w, _ = FRAMES[key]
    return A.build_point_grid(n) * np.array([[w, h]])


@pytest.fixture(scope="module")
def sd():
    return init_sam_state_dict(CFG, 72)


@pytest.fixture(scope="module")
def sd_hq():
    return init_sam_state_dict(CFG, 72, hq=True)


@pytest.fixture(scope="module")
def pred16(dev, sd):
    """SAM predictor whose decoder handle takes 16 prompts per chain: 37 prompts run as chunks 16 + 16 + 5."""
    return SamPredictor(SamHip(config=CFG, state_dict=sd, precision="f32", max_decode_batch=16).to(dev))


@pytest.fixture(scope="module")
def pred_hq(dev, sd_hq):
    return SamPredictor(SamHip(config=CFG, state_dict=sd_hq, precision="f32", hq=True).to(dev))


def _prompts(key, k, n=37):
    """n prompts of k points in input-frame pixels: the first n grid points (k = 1), or seeded random triples labelled 1, 1, 0."""
    h, w, seed = FRAMES[key]
    tr = R._Transform(CFG.img_size)
    if k == 1:
        pts = _grid_points(key)[:n, None, :]
        lab = torch.ones(n, 1, dtype=torch.int)
    else:
        rng = np.random.default_rng(100 + seed)
        pts = rng.uniform(0.05, 0.95, (n, k, 2)) * np.array([w, h])
        lab = torch.tensor([[1, 1, 0]], dtype=torch.int).repeat(n, 1)
    return torch.as_tensor(tr.apply_coords(pts, (h, w)), dtype=torch.float), lab


_LOW_CACHE = {}


def _device_low(pred16, key, dev):
    """Device low-res masks of the 37 single-point prompts (multimask): (111, 4g, 4g) — what tests 5 and 7 share."""
    if key not in _LOW_CACHE:
        pred16.set_image(_image(key))
        pts, lab = _prompts(key, 1)
        low, _ = pred16.predict_points_batch(pts.to(dev), lab.to(dev), multimask_output=True)
        _LOW_CACHE[key] = low.flatten(0, 1).clone()
    else:
        pred16.set_image(_image(key))
    return _LOW_CACHE[key]


# ------------------------------------------------------------------------------------------------------------ test 5
@pytest.mark.parametrize("key", list(FRAMES))
@pytest.mark.parametrize("k", [1, 3])
def test_predict_points_batch_vs_oracle_and_single_calls(dev, sd, pred16, key, k):
    img = _image(key)
    ref = R.SamPredictorRef(sd, CFG)
    ref.set_image(img), pred16.set_image(img)
    pts, lab = _prompts(key, k)
    L = 4 * CFG.grid
    for multi, m in ((True, 3), (False, 1)):
        _, iou_o, low_o = ref.predict_torch(pts, lab, None, None, multi, True)
        low, iou = pred16.predict_points_batch(pts.to(dev), lab.to(dev), multimask_output=multi)
        assert low.shape == (37, m, L, L) and iou.shape == (37, m) and low.dtype == iou.dtype == torch.float32
        e_low = max(max_abs(low[i], low_o[i]) for i in range(37))
        e_iou = max(max_abs(iou[i], iou_o[i]) for i in range(37))
        print(f"{key} k={k} multi={multi}: batch vs oracle low-res {e_low:.3g} IoU {e_iou:.3g}")
        assert e_low < LOW_BAR and e_iou < IOU_BAR
        _, iou_s, low_s = pred16.predict_torch(pts.to(dev), lab.to(dev), None, None, multi, True)
        e_low2, e_iou2 = max_abs(low, low_s), max_abs(iou, iou_s)
        print(f"{key} k={k} multi={multi}: batch vs per-prompt predict_torch low-res {e_low2:.3g} IoU {e_iou2:.3g}")
        assert e_low2 < 2 * LOW_BAR and e_iou2 < 2 * IOU_BAR
        low_b, iou_b = pred16.predict_points_batch(pts.to(dev), lab.to(dev), multimask_output=multi)
        assert torch.equal(low, low_b) and torch.equal(iou, iou_b)          # the same call twice: bitwise equal
    # a caller may chunk below the handle's capacity; a single prompt is a batch of one
    low_c, iou_c = pred16.predict_points_batch(pts.to(dev), lab.to(dev), multimask_output=True, max_chunk=7)
    _, iou_o, low_o = ref.predict_torch(pts, lab, None, None, True, True)
    assert max_abs(low_c, low_o) < LOW_BAR and max_abs(iou_c, iou_o) < IOU_BAR
    low_1, iou_1 = pred16.predict_points_batch(pts[:1].to(dev), lab[:1].to(dev))
    assert max_abs(low_1, low_o[:1]) < LOW_BAR and max_abs(iou_1, iou_o[:1]) < IOU_BAR


# ------------------------------------------------------------------------------------------------------------ test 6
def _hq_expect(sd_hq, key):
    """Helper 3 on the 64 grid prompts of a frame: (low (64,1,L,L), iou (64,1), usable (64,) bool, oracle predictor)."""
    h, w, _ = FRAMES[key]
    ref = R.SamPredictorRef(sd_hq, CFG, hq=True)
    ref.set_image(_image(key))
    pts = torch.as_tensor(ref.transform.apply_coords(_grid_points(key)[:, None, :], (h, w)), dtype=torch.float)
    lab = torch.ones(64, 1, dtype=torch.int)
    with torch.no_grad():
        sp, de = R.prompt_encoder(sd_hq, CFG, (pts, lab), None, None)
        low, iou, iou3 = hq_mask_decoder_ref(sd_hq, CFG, ref.features, ref._pe, sp, de, ref.hq_feat, multimask_output=True)
    top2 = iou3.sort(dim=1, descending=True).values
    margin = top2[:, 0] - top2[:, 1]
    usable = margin >= 1e-3               # closer than 10 x the IoU bar: the other token is a legitimate choice
    chosen = iou3.argmax(dim=1)
    print(f"{key}: chosen tokens {[int((chosen == j).sum()) for j in range(3)]}, smallest margin {float(margin.min()):.3g}, "
          f"left out {int((~usable).sum())}")
    assert int((~usable).sum()) <= 2
    return pts, lab, low, iou, usable, ref


@pytest.mark.parametrize("key", list(FRAMES))
def test_hq_multimask_batch_and_predict_torch_vs_helper(dev, sd_hq, pred_hq, key):
    h, w, _ = FRAMES[key]
    pts, lab, low_e, iou_e, usable, ref = _hq_expect(sd_hq, key)
    pred_hq.set_image(_image(key))
    L = 4 * CFG.grid
    low, iou = pred_hq.predict_points_batch(pts.to(dev), lab.to(dev), multimask_output=True)
    assert low.shape == (64, 1, L, L) and iou.shape == (64, 1)
    e_low, e_iou = max_abs(low[usable], low_e[usable]), max_abs(iou[usable], iou_e[usable])
    print(f"{key}: HQ batch vs helper low-res {e_low:.3g} IoU {e_iou:.3g}")
    assert e_low < LOW_BAR and e_iou < IOU_BAR
    masks, iou_t, low_t = pred_hq.predict_torch(pts.to(dev), lab.to(dev), multimask_output=True, return_logits=True)
    assert masks.shape == (64, 1, h, w) and iou_t.shape == (64, 1) and low_t.shape == (64, 1, L, L)
    e_low, e_iou = max_abs(low_t[usable], low_e[usable]), max_abs(iou_t[usable], iou_e[usable])
    print(f"{key}: HQ predict_torch vs helper low-res {e_low:.3g} IoU {e_iou:.3g}")
    assert e_low < LOW_BAR and e_iou < IOU_BAR
    full_e = R.postprocess_masks(CFG, low_e, ref.input_size, ref.original_size)
    assert max_abs(masks[usable], full_e[usable]) < LOW_BAR
    # multimask_output=False is the path it always was: mask token 0 + the HQ mask
    _, iou_0, low_0 = pred_hq.predict_torch(pts[:5].to(dev), lab[:5].to(dev), multimask_output=False, return_logits=True)
    _, iou_r, low_r = ref.predict_torch(pts[:5], lab[:5], None, None, False, True)
    assert max_abs(low_0, low_r) < LOW_BAR and max_abs(iou_0, iou_r) < IOU_BAR
    low_b0, iou_b0 = pred_hq.predict_points_batch(pts[:5].to(dev), lab[:5].to(dev), multimask_output=False)
    assert max_abs(low_b0, low_r) < LOW_BAR and max_abs(iou_b0, iou_r) < IOU_BAR


# ------------------------------------------------------------------------------------------------------------ test 7
def _postprocess_each(pred, low):
    """sampt_postprocess_masks of every mask of ``low`` (N,L,L) -> logits (N,H,W) on the device."""
    lib = _lib.load()
    (oh, ow), (ih, iw) = pred.original_size, pred.input_size
    L = low.shape[-1]
    out = torch.empty((low.shape[0], oh, ow), dtype=torch.float32, device=low.device)
    for i in range(low.shape[0]):
        one, dst = low[i].contiguous(), torch.empty((oh, ow), dtype=torch.float32, device=low.device)
        _lib.check(lib.sampt_postprocess_masks(_lib.ptr(one), L, CFG.img_size, ih, iw, _lib.ptr(dst), oh, ow, _lib.stream_ptr()),
                   "sampt_postprocess_masks")
        out[i] = dst
    return out


@pytest.mark.parametrize("key", list(FRAMES))
def test_score_and_binarize_are_exact(dev, pred16, key):
    h, w, _ = FRAMES[key]
    low = _device_low(pred16, key, dev)
    L = low.shape[-1]
    low = torch.cat([low, torch.full((1, L, L), -1.0, device=dev), torch.full((1, L, L), 1.0, device=dev)])
    logits = _postprocess_each(pred16, low)
    for off in (0.02, 1.0):
        rec = pred16.score_masks(low, off)
        exp = score_record_ref(logits.cpu(), 0.0, off)
        assert rec.dtype == torch.int32 and rec.shape == (low.shape[0], 8)
        bad = (rec.cpu() != exp).any(dim=1).nonzero().flatten().tolist()
        assert torch.equal(rec.cpu(), exp), (off, bad[:5], rec.cpu()[bad[:5]].tolist(), exp[bad[:5]].tolist())
        assert rec[-2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]                                   # constant -1: empty
        assert rec[-1].tolist() == [0 if off >= 1.0 else h * w, h * w, h * w, 0, 0, w - 1, h - 1, 0]   # constant +1: the frame
        if off == 1.0:
            assert int(rec[:, 0].sum()) == 0                        # seeded weights: no logit clears 1.0 (the degenerate branch)
        else:
            assert int((rec[:-2, 0] > 0).sum()) > 0 and int((rec[:-2, 0] < rec[:-2, 1]).sum()) > 0
        assert torch.equal(pred16.score_masks(low, off), rec)       # integer reductions: reproducible
    rows = torch.randperm(low.shape[0], generator=torch.Generator().manual_seed(7))[:29]
    got = pred16.binarize_masks(low, rows.to(dev))
    assert got.dtype == torch.bool and got.shape == (29, h, w)
    assert torch.equal(got, logits[rows.to(dev)] > 0)
    one = pred16.binarize_masks(low, [5])                           # a single row: a short, unaligned tail on the odd-width frame
    assert torch.equal(one, logits[5:6] > 0)
    none = pred16.binarize_masks(low, torch.zeros(0, dtype=torch.int64))
    assert none.shape == (0, h, w) and none.dtype == torch.bool
    assert pred16.score_masks(low[:0], 0.02).shape == (0, 8)


# ------------------------------------------------------------------------------------------------------------ test 8
def _box_of(seg):
    ys, xs = np.nonzero(seg)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())] if seg.any() else [0, 0, 0, 0]


def _oracle_thresholds(sd, key):
    """pred_iou_thresh in the widest gap of the middle 40 sorted oracle IoU predictions, stability threshold 0.65 — asserted to
    be far enough from every oracle candidate that none can change sides within the bars."""
    h, w, _ = FRAMES[key]
    ref = R.SamPredictorRef(sd, CFG)
    ref.set_image(_image(key))
    pts = torch.as_tensor(ref.transform.apply_coords(_grid_points(key)[:, None, :], (h, w)), dtype=torch.float)
    logits, iou, _ = ref.predict_torch(pts, torch.ones(64, 1, dtype=torch.int), None, None, True, True)
    ious = np.sort(iou.flatten().numpy().astype(np.float64))
    mid = ious[76:116]
    gaps = np.diff(mid)
    j = int(np.argmax(gaps))
    thr, half = float((mid[j] + mid[j + 1]) / 2), float(gaps[j] / 2)
    stab = A.calculate_stability_score(logits.flatten(0, 1), 0.0, 0.02).numpy()
    near = float(np.nanmin(np.abs(stab - 0.65)))
    print(f"{key}: pred_iou_thresh {thr:.6f} +- {half:.3g}; nearest stability to 0.65: {near:.3g}; "
          f"{int((stab >= 0.65).sum())} of 192 pass stability")
    assert half >= 5e-4 and near >= 0.03
    return thr


def _match_records(ours, ref):
    matched = 0
    for r in ours:
        cands = [q for q in ref if q["point_coords"] == r["point_coords"] and abs(q["predicted_iou"] - r["predicted_iou"]) < 1e-3]
        if cands:
            matched += 1
            diff = min(int((r["segmentation"] ^ q["segmentation"]).sum()) for q in cands)
            assert diff <= max(3, 0.01 * r["area"]), (diff, r["area"])
    return matched


@pytest.mark.parametrize("key", list(FRAMES))
def test_generator_fused_vs_unfused_vs_oracle(dev, sd, key):
    h, w, _ = FRAMES[key]
    img = _image(key)
    thr = _oracle_thresholds(sd, key)
    kw = dict(points_per_side=8, points_per_batch=16, stability_score_offset=0.02, box_nms_thresh=1.0, crop_nms_thresh=1.0,
              pred_iou_thresh=thr, stability_score_thresh=0.65)
    pred = SamPredictor(SamHip(config=CFG, state_dict=sd, precision="f32").to(dev))
    gen_f = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=True, **kw)
    assert A.SamAutomaticMaskGenerator(None, predictor=pred, **kw).fused is True           # the default with the HIP predictor
    fused = gen_f.generate(img)
    plain = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=False, **kw).generate(img)
    oracle = A.SamAutomaticMaskGenerator(None, predictor=R.SamPredictorRef(sd, CFG), **kw).generate(img)
    print(f"{key}: records fused {len(fused)}, unfused {len(plain)}, oracle {len(oracle)}")
    assert len(fused) == len(plain) > 0
    assert sorted(map(str, (r["point_coords"] for r in fused))) == sorted(map(str, (r["point_coords"] for r in plain)))
    free = list(range(len(plain)))
    for r in fused:
        seg = r["segmentation"]
        assert seg.shape == (h, w) and seg.dtype == bool and r["area"] == int(seg.sum()) and r["bbox"] == _box_of(seg)
        cands = [i for i in free if plain[i]["point_coords"] == r["point_coords"]
                 and abs(plain[i]["predicted_iou"] - r["predicted_iou"]) < 1e-3]
        assert cands, r["point_coords"]
        best = min(cands, key=lambda i: int((plain[i]["segmentation"] ^ seg).sum()))
        diff = int((plain[best]["segmentation"] ^ seg).sum())
        assert diff <= max(3, 0.01 * r["area"]), (diff, r["area"])
        assert abs(plain[best]["stability_score"] - r["stability_score"]) <= 0.02
        free.remove(best)
    # ... and against the oracle generator
    assert abs(len(fused) - len(oracle)) <= max(1, len(oracle) // 10)
    assert _match_records(fused, oracle) >= 0.9 * len(fused)
    ious = [r["predicted_iou"] for r in fused]
    assert ious == sorted(ious, reverse=True)
    # default NMS, then one crop layer + small-region clean-up, end to end on the fused path
    nms = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=True, **{**kw, "box_nms_thresh": 0.7}).generate(img)
    assert 0 < len(nms) <= len(fused) and all(r["segmentation"].shape == (h, w) for r in nms)
    ious = [r["predicted_iou"] for r in nms]
    assert ious == sorted(ious, reverse=True)
    more = A.SamAutomaticMaskGenerator(None, predictor=pred, fused=True, points_per_side=2, points_per_batch=8, pred_iou_thresh=0.0,
                                       stability_score_thresh=0.0, crop_n_layers=1, crop_n_points_downscale_factor=2,
                                       min_mask_region_area=6).generate(img)
    assert more and all(r["segmentation"].shape == (h, w) and r["segmentation"].dtype == bool for r in more)
    by_crop = {}
    for r in more:
        by_crop.setdefault(tuple(r["crop_box"]), []).append(r["predicted_iou"])
    assert all(v == sorted(v, reverse=True) for v in by_crop.values())
    assert set(by_crop) <= {tuple(A.box_xyxy_to_xywh(b)) for b in A.generate_crop_boxes((h, w), 1, 512 / 1500)[0]}


# ------------------------------------------------------------------------------------------------------------ test 9
@pytest.mark.parametrize("key", list(FRAMES))
def test_hq_generator_one_record_per_point(dev, sd_hq, pred_hq, key):
    h, w, _ = FRAMES[key]
    _, _, low_e, iou_e, usable, ref = _hq_expect(sd_hq, key)
    exp = (R.postprocess_masks(CFG, low_e, ref.input_size, ref.original_size)[:, 0] > 0).numpy()
    gen = A.SamAutomaticMaskGenerator(None, predictor=pred_hq, points_per_side=8, points_per_batch=16, pred_iou_thresh=0.0,
                                      stability_score_thresh=0.0, stability_score_offset=0.02, box_nms_thresh=1.0,
                                      crop_nms_thresh=1.0)
    assert gen.fused is True
    recs = gen.generate(_image(key))
    assert len(recs) == 64
    grid = _grid_points(key)
    seen = set()
    for r in recs:
        (px, py), = r["point_coords"]
        i = int(np.abs(grid - np.array([[px, py]])).sum(axis=1).argmin())
        assert np.abs(grid[i] - np.array([px, py])).sum() < 1e-9 and i not in seen
        seen.add(i)
        assert r["segmentation"].shape == (h, w) and r["area"] == int(r["segmentation"].sum())
        if bool(usable[i]):
            diff = int((r["segmentation"] ^ exp[i]).sum())
            assert diff <= max(3, 0.01 * r["area"]), (i, diff, r["area"])
            assert abs(r["predicted_iou"] - float(iou_e[i, 0])) < 1e-3
    assert len(seen) == 64


# ----------------------------------------------------------------------------------------------------------- test 10
def test_vis_adapter_over_fused_generator_and_hip_sampt(dev, sd):
    from oracle.make_golden import sampt_kwargs
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.vis_to_vos_adapter import SamBasedVisToVosAdapter
    from sam_pt_amd.weights import init_pips_state_dict
    T, h, w = 4, 96, 128
    frames, _ = synthetic_clip(T=T, H=h, W=w, seed=3)
    sam = SamHip(config=CFG, state_dict=sd, precision="f32").to(dev)
    gen = A.SamAutomaticMaskGenerator(sam, points_per_side=8, points_per_batch=16, pred_iou_thresh=0.0, stability_score_thresh=0.0,
                                      stability_score_offset=0.02)
    assert gen.fused is True
    kw = dict(sampt_kwargs(4, 0), positive_point_selection_method="random", negative_point_selection_method="random",
              sam_iou_threshold=-1e9)
    model = SamPt(PipsPointTracker(state_dict=init_pips_state_dict(72)), SamPredictor(sam), **kw).eval()
    n_keep = 5
    adapter = SamBasedVisToVosAdapter(model, gen, max_num_masks=n_keep, masks_batch_size=2)
    torch.manual_seed(5)
    out = adapter([{"video_id": 0, "image": [f.to(dev) for f in frames], "height": h, "width": w}])
    n = len(out["pred_masks"])
    assert 0 < n <= n_keep
    assert out["image_size"] == (h, w) and out["pred_labels"] == [0] * n and len(out["pred_scores"]) == n
    assert out["pred_masks"][0].shape == (T, h, w) and out["pred_masks"][0].dtype == torch.bool
    assert len(out["pred_logits"]) == n and out["pred_logits"][0].shape == (T, h, w)
    assert out["trajectories"].shape[:2] == (T, n) and out["trajectories"].shape[-1] == 2
    assert out["visibilities"].shape[:2] == (T, n)
