"""CPU side of the device run-length encoder (no GPU needed): the C ABI surface and its refusals, the COCO string codec
(``coco_rle_string`` / ``coco_rle_counts``, restated from maskApi.c — pycocotools is absent, so the vectors are hand-worked from
the published algorithm), the "column word" restatement of csrc/rle.hip pinned on ``mask_to_rle``, ``encode_rle`` on CPU
tensors, and the VIS adapter's ``rle_results`` / ``instances_to_ytvis_json`` on the CPU oracle predictor."""
import os
import re

import numpy as np
import pytest
import torch

from sam_pt_amd import automatic_mask_generator as A
from tests.test_amg_tail_cpu import seeded_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_rle_workspace_bytes", "sampt_rle_count", "sampt_rle_emit", "sampt_rle_string_workspace_bytes",
               "sampt_rle_string_sizes", "sampt_rle_string_emit")
WORD_SHAPES = ((1, 1), (63, 5), (64, 4), (65, 7), (130, 33), (7, 300))


# --------------------------------------------------------------------------------------------------------------------
# structured masks shared with tests/test_gpu_rle.py
# --------------------------------------------------------------------------------------------------------------------
def checkerboard(h=40, w=24) -> torch.Tensor:
    """Alternating pixels, (0, 0) set.  With an even h the last pixel of a column equals the first of the next, so every column
    but the first opens without a transition: h * w - (w - 1) transitions + the closing run (40 x 24: 938 counts)."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return (x + y) % 2 == 0


def column_ends_set(h=70, w=9) -> torch.Tensor:
    """Every column ends set and the next one starts set: the run crosses the column boundary (the carry of a column's first
    word is the last pixel of the column before it)."""
    m = torch.zeros(h, w, dtype=torch.bool)
    m[-3:, :] = True
    m[:2, :] = True
    return m


def last_pixel_only(h=65, w=7) -> torch.Tensor:
    m = torch.zeros(h, w, dtype=torch.bool)
    m[h - 1, w - 1] = True
    return m


def trivial_masks(h=70, w=9):
    return torch.zeros(h, w, dtype=torch.bool), torch.ones(h, w, dtype=torch.bool)


# --------------------------------------------------------------------------------------------------------------------
# the column-word restatement of csrc/rle.hip
# --------------------------------------------------------------------------------------------------------------------
def column_word_rle(mask: np.ndarray):
    """One mask (h, w) -> (counts, area) the way the kernels work: per column x and block of 64 rows a 64-bit word (bit j = row
    y0 + j), transitions = word ^ ((word << 1) | carry) masked to the valid rows, carry = pixel (y0 - 1, x), or (h - 1, x - 1)
    for a column's first word, or 0 for the mask's first pixel; positions p = x * h + y0 + bit in (x, row block) order;
    counts[k] = pos[k] - pos[k - 1] with pos[-1] = 0, closed by h * w - pos[last]."""
    h, w = mask.shape
    full = (1 << 64) - 1
    pos, area = [], 0
    for x in range(w):
        for y0 in range(0, h, 64):
            rows = min(64, h - y0)
            valid = (1 << rows) - 1
            word = 0
            for j in range(rows):
                word |= int(mask[y0 + j, x]) << j
            if y0 > 0:
                carry = int(mask[y0 - 1, x])
            elif x > 0:
                carry = int(mask[h - 1, x - 1])
            else:
                carry = 0
            tr = (word ^ (((word << 1) & full) | carry)) & valid
            area += bin(word).count("1")
            pos += [x * h + y0 + j for j in range(rows) if (tr >> j) & 1]
    counts, prev = [], 0
    for p in pos:
        counts.append(p - prev)
        prev = p
    counts.append(h * w - prev)
    return counts, area


# --------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_binds_and_exports_the_rle_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
    for name in ("sampt_rle_count", "sampt_rle_emit", "sampt_rle_string_sizes", "sampt_rle_string_emit"):
        res, args = _lib._SIGS[name]                                 # house style: int return code, stream last
        assert res is _lib.c_int and args[-1] is _lib._P


def test_abi_refuses_bad_arguments_without_touching_memory():
    from sam_pt_amd import _lib
    lib = _lib.load()
    assert lib.sampt_rle_workspace_bytes(1, 46341, 46341) == 0                   # h * w >= 2^31
    assert lib.sampt_rle_workspace_bytes(1, 0, 5) == 0 and lib.sampt_rle_workspace_bytes(-1, 8, 8) == 0
    per = lib.sampt_rle_workspace_bytes(1, 576, 1024)
    assert 12 * 9 * 1024 <= per <= 16 * 9 * 1024 + 64                             # about 12 - 16 B per 64 pixels of a column
    assert lib.sampt_rle_workspace_bytes(5, 576, 1024) == 5 * per
    for is_f32 in (0, 1):
        assert lib.sampt_rle_count(None, is_f32, 0.0, 1, 46341, 46341, None, None, None, 0, None) == -1
        assert b"2^31" in lib.sampt_last_error()
        assert lib.sampt_rle_count(None, is_f32, 0.0, 1, 0, 5, None, None, None, 0, None) == -1           # h = 0
        assert b"shape" in lib.sampt_last_error()
        assert lib.sampt_rle_count(None, is_f32, 0.0, -1, 8, 8, None, None, None, 0, None) == -1          # negative n
        assert lib.sampt_rle_count(None, is_f32, 0.0, 1, 8, 8, None, None, None, 0, None) == -1           # null pointers
        assert b"null" in lib.sampt_last_error()
    assert lib.sampt_rle_emit(1, 46341, 46341, None, None, None, 0, None) == -1
    assert lib.sampt_rle_emit(1, 0, 5, None, None, None, 0, None) == -1
    assert lib.sampt_rle_emit(-1, 8, 8, None, None, None, 0, None) == -1
    assert lib.sampt_rle_emit(1, 8, 8, None, None, None, 0, None) == -1
    assert lib.sampt_rle_string_workspace_bytes(0) == 0 and lib.sampt_rle_string_workspace_bytes(5000) >= 8
    assert lib.sampt_rle_string_sizes(None, None, 1, 5, None, None, 0, None) == -1
    assert lib.sampt_rle_string_sizes(None, None, -1, 5, None, None, 0, None) == -1
    assert lib.sampt_rle_string_emit(None, None, 1, 5, None, None, None, 0, None) == -1
    assert b"sampt_rle_string_emit" in lib.sampt_last_error()


# ------------------------------------------------------------------------------------------------------- string codec
def test_coco_string_hand_worked_vectors():
    # 3 -> '3'; 2 -> '2'; 20 = 0x14: bit 4 set and the rest is 0, not -1 -> continuation 'd' (0x14 | 0x20 = 52, + 48), then '0';
    # 1 - 2 = -1: chunk 31, the rest is -1 and bit 4 is set -> stop: chr(31 + 48) = 'O'
    assert A.coco_rle_string([3, 2, 20, 1]) == "32d0O"
    assert A.coco_rle_counts("32d0O") == [3, 2, 20, 1]
    # an empty and a full 70 x 9 mask (computed from the algorithm, not from pycocotools)
    assert A.coco_rle_string([630]) == "fc0"
    assert A.coco_rle_string([0, 630]) == "0fc0"
    assert A.coco_rle_counts("fc0") == [630] and A.coco_rle_counts(b"0fc0") == [0, 630]
    # small values around the sign bit of a chunk: 15 fits one chunk, 16 needs a second, -16 fits one, -17 needs two
    assert A.coco_rle_string([15]) == "?" and A.coco_rle_string([16]) == "`0"
    assert A.coco_rle_string([0, 0, 0, 0, 0, 16, 17]) == "00000`0a0"
    # 0 - 16 = -16: chunk 16, the rest is -1 with bit 4 set -> one chunk '@'; 0 - 17 = -17: chunk 15 (bit 4 clear, rest -1) continues
    assert A.coco_rle_string([1, 16, 1, 0]) == "1`01@" and A.coco_rle_string([1, 17, 1, 0]) == "1a01_O"


def test_coco_string_round_trip():
    stacks = [seeded_masks(3, 130, 33, seed) for seed in (1, 2)]
    masks = [m for s in stacks for m in s] + list(trivial_masks()) + [checkerboard(), column_ends_set(), last_pixel_only()]
    for m in masks:
        rle, = A.mask_to_rle(m[None])
        s = A.coco_rle_string(rle["counts"])
        assert isinstance(s, str) and all(48 <= ord(c) < 48 + 64 for c in s)
        assert A.coco_rle_counts(s) == rle["counts"]
        rec = {"size": rle["size"], "counts": s}
        assert np.array_equal(A.rle_to_mask(rec), m.numpy())
        assert A.area_from_rle(rec) == int(m.sum()) == A.area_from_rle(rle)
    big = [0, 2 ** 31 - 1, 1, 0, 2 ** 31 - 1, 5, 0]                    # the largest deltas either way
    assert A.coco_rle_counts(A.coco_rle_string(big)) == big


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", WORD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_column_word_restatement_equals_mask_to_rle(shape):
    h, w = shape
    masks = list(seeded_masks(3, h, w, seed=200 + h + w))
    masks += [torch.zeros(h, w, dtype=torch.bool), torch.ones(h, w, dtype=torch.bool), checkerboard(h, w), last_pixel_only(h, w)]
    if h > 5:
        masks.append(column_ends_set(h, w))
    for m in masks:
        exp, = A.mask_to_rle(m[None])
        counts, area = column_word_rle(m.numpy())
        assert counts == exp["counts"] and area == int(m.sum())


def test_structured_masks_are_what_they_claim():
    cb, = A.mask_to_rle(checkerboard()[None])
    assert len(cb["counts"]) == 938 and sum(cb["counts"]) == 960
    ce, = A.mask_to_rle(column_ends_set()[None])
    assert ce["counts"][0] == 0 and ce["counts"][1] == 2 and ce["counts"][3] == 5       # 3 px + the next column's 2 in one run
    lp, = A.mask_to_rle(last_pixel_only()[None])
    assert lp["counts"] == [65 * 7 - 1, 1]


# ------------------------------------------------------------------------------------------------------- Python surface
def test_rle_encode_device_refuses_cpu_tensors():
    from sam_pt_amd._lib import SamptError
    with pytest.raises(SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8, dtype=torch.bool))
    with pytest.raises(SamptError):
        A.rle_encode_device(torch.zeros(2, 8, 8), threshold=0.0, compressed=True)


def test_encode_rle_on_cpu_tensors_equals_mask_to_rle():
    masks = seeded_masks(3, 65, 7, seed=5)
    exp = A.mask_to_rle(masks)
    assert A.encode_rle(masks) == exp
    assert A.encode_rle(masks.to(torch.uint8) * 3) == exp
    assert A.encode_rle(masks.reshape(3, 1, 65, 7)) == exp
    comp = A.encode_rle(masks, compressed=True)
    assert [r["counts"] for r in comp] == [A.coco_rle_string(r["counts"]) for r in exp]
    assert all(r["size"] == [65, 7] for r in comp)
    logits = torch.randn(3, 65, 7, generator=torch.Generator().manual_seed(6))
    logits[0, :3] = 0.25                                             # equal to the threshold: clear
    logits[1, 0, 0] = float("nan")
    assert A.encode_rle(logits, threshold=0.25) == A.mask_to_rle(logits > 0.25)
    with pytest.raises(ValueError):
        A.encode_rle(logits)
    assert A.encode_rle(torch.zeros(0, 5, 5, dtype=torch.bool)) == []


# ------------------------------------------------------------------------------------------------- adapter / generator
@pytest.fixture(scope="module")
def oracle_predictor():
    from oracle import sam_ref as R
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    return R.SamPredictorRef(init_sam_state_dict(cfg, 72), cfg)


def _image(h, w, seed):
    from sam_pt_amd.synth import synthetic_clip
    frames, _ = synthetic_clip(T=1, H=h, W=w, seed=seed)
    return frames[0].permute(1, 2, 0).contiguous().numpy()


def stub_vos(T, h, w, device="cpu"):
    """A VOS model whose logits are seeded noise with entries exactly 0 (clear at threshold 0), on ``device``."""
    produced = []

    class StubVos(torch.nn.Module):
        def forward(self, video):
            M = video["query_masks"].shape[0]
            g = torch.Generator().manual_seed(40 + len(produced))
            logits = []
            for _ in range(M):
                x = torch.randn(T, h, w, generator=g)
                x[:, ::7, ::5] = 0.0
                produced.append(x)
                logits.append(x.to(device))
            return {"logits": logits, "trajectories": torch.zeros(T, M, 4, 2), "visibilities": torch.ones(T, M, 4),
                    "scores": [0.5 + 0.01 * m for m in range(M)]}

    return StubVos(), produced


def test_vis_adapter_rle_results_on_the_oracle_predictor(oracle_predictor):
    from sam_pt_amd.vis_to_vos_adapter import SamBasedVisToVosAdapter, instances_to_ytvis_json
    T, h, w = 3, 96, 128
    frames = [torch.as_tensor(_image(h, w, seed=7 + t)).permute(2, 0, 1).contiguous() for t in range(T)]
    gen = A.SamAutomaticMaskGenerator(None, points_per_side=3, points_per_batch=9, pred_iou_thresh=0.0,
                                      stability_score_thresh=0.0, box_nms_thresh=1.0, predictor=oracle_predictor)
    inputs = [{"video_id": 17, "image": frames, "height": h, "width": w, "length": T}]
    outs = {}
    for rle_results in (False, True):
        model, produced = stub_vos(T, h, w)
        adapter = SamBasedVisToVosAdapter(model, gen, max_num_masks=5, masks_batch_size=2, rle_results=rle_results)
        outs[rle_results] = adapter(inputs)
    plain, rle = outs[False], outs[True]
    n = len(plain["pred_masks"])
    assert n >= 3 and len(produced) == n
    assert "pred_masks" not in rle and "pred_logits" not in rle
    assert set(rle) == (set(plain) - {"pred_masks", "pred_logits"}) | {"pred_rles"}
    for k in ("image_size", "pred_scores", "pred_labels"):
        assert rle[k] == plain[k]
    assert torch.equal(rle["trajectories"], plain["trajectories"]) and torch.equal(rle["visibilities"], plain["visibilities"])
    assert len(rle["pred_rles"]) == n
    for i in range(n):
        assert len(rle["pred_rles"][i]) == T
        for t in range(T):
            rec = rle["pred_rles"][i][t]
            assert rec["size"] == [h, w] and isinstance(rec["counts"], str)
            assert np.array_equal(A.rle_to_mask(rec), (produced[i][t] > 0).numpy())
            assert np.array_equal(A.rle_to_mask(rec), plain["pred_masks"][i][t].numpy())
    a, b = instances_to_ytvis_json(inputs, plain), instances_to_ytvis_json(inputs, rle)
    assert a == b and len(a) == n
    assert set(a[0]) == {"video_id", "score", "category_id", "segmentations"}
    assert a[0]["video_id"] == 17 and a[0]["category_id"] == 0 and a[1]["score"] == plain["pred_scores"][1]
    assert len(a[0]["segmentations"]) == T and isinstance(a[0]["segmentations"][0]["counts"], str)


def test_generator_coco_rle_needs_the_device_tail(oracle_predictor):
    with pytest.raises(NotImplementedError):
        A.SamAutomaticMaskGenerator(None, output_mode="coco_rle", predictor=oracle_predictor)
    with pytest.raises(NotImplementedError):
        A.SamAutomaticMaskGenerator(None, output_mode="coco_rle", predictor=oracle_predictor, device_tail=False)
    gen = A.SamAutomaticMaskGenerator(None, output_mode="uncompressed_rle", predictor=oracle_predictor, points_per_side=2,
                                      pred_iou_thresh=0.0, stability_score_thresh=0.0)
    assert gen.device_tail is False
    recs = gen.generate(_image(96, 128, 3))
    assert recs and all(isinstance(r["segmentation"]["counts"], list) for r in recs)
