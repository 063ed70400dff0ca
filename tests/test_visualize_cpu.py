"""The definitions of sam_pt_amd/visualize.py on the host: palette, blend tables, contour band, markers, the drop-in's signature
and the C ABI of csrc/viz.hip.  No GPU."""
import ast
import inspect
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_pt_amd import visualize as V
from tests.test_amg_tail_cpu import seeded_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_viz_band", "sampt_viz_compose")
BAND_SHAPES = [(5, 3), (64, 4), (65, 7), (70, 261)]


def band_masks(h: int, w: int) -> np.ndarray:
    """bool (7, h, w): empty, full, one pixel in a corner, checkerboard, and three seeded masks."""
    m = np.zeros((7, h, w), dtype=bool)
    m[1] = True
    m[2, h - 1, 0] = True
    m[3] = (np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0
    m[4:] = seeded_masks(3, h, w, seed=h * 1000 + w).numpy()
    return m


# ------------------------------------------------------------------------------------------------------------ palette
def test_palette_is_matplotlibs_tab10_clipped_at_index_9():
    # asked of a fresh interpreter: other loaders of this suite register empty stand-ins for matplotlib in sys.modules
    ask = "import json, matplotlib.pyplot as plt; print(json.dumps(plt.get_cmap('tab10')(list(range(12))).tolist()))"
    run = subprocess.run([sys.executable, "-c", ask], capture_output=True, text=True)
    if run.returncode != 0:
        pytest.skip("matplotlib does not import")
    colours = np.array(json.loads(run.stdout))                         # as the reference: integer indices into a ListedColormap
    for m in range(12):
        assert (V.mask_colour(m) == colours[m][:3]).all()
        assert V.marker_colour(m) == tuple(int(c * 255) for c in colours[m][:3])
    assert (V.mask_colour(11) == V.mask_colour(9)).all() and not (V.mask_colour(8) == V.mask_colour(9)).all()


# ------------------------------------------------------------------------------------------------------------- tables
def literal_blend(v: int, colour, alpha: float) -> int:
    """One channel of add_mask_to_frame in Python floats (float64); colour None: a clear pixel."""
    f = v / 255
    o = f if colour is None else 1.0 * colour
    return int(math.trunc((f * alpha + o * (1 - alpha)) * 255))


def test_blend_tables_equal_the_literal_formula_for_every_byte_colour_bit_and_alpha():
    for alpha in (V.MASK_ALPHA, V.BAND_ALPHA):
        colours = [None, 1.0] + [float(c) for c in V.TAB10.reshape(-1)]
        for colour in colours:
            t = V.blend_table(colour, alpha)
            assert t.dtype == np.uint8 and t.tolist() == [literal_blend(v, colour, alpha) for v in range(256)]
    L = V.lookup_tables()
    assert L.shape == (62, 256) and L.dtype == np.uint8
    for ci in range(10):
        for ch in range(3):
            for bit in range(2):
                for band in range(2):
                    row = (ci * 3 + ch) * 2 + band if bit else 60 + band
                    want = [literal_blend(literal_blend(v, float(V.TAB10[ci, ch]) if bit else None, 0.5), 1.0 if band else None, 0.1)
                            for v in range(256)]
                    assert L[row].tolist() == want


def add_mask_to_frame_literal(frame, mask, color, alpha):
    """sam_pt/utils/util.py:295-328 with cv2.addWeighted(a, alpha, b, beta, 0) written out (float64: a * alpha + b * beta + 0)."""
    frame = frame / 255
    overlay = np.ones((mask.shape[0], mask.shape[1], 3))
    overlay *= color
    overlay = np.where(mask[..., None] > 0, overlay, frame)
    masked_frame = frame * alpha + overlay * (1 - alpha) + 0
    masked_frame = masked_frame * 255
    return masked_frame.astype(np.uint8)


def test_table_application_equals_add_mask_to_frame_step_by_step():
    rng = np.random.default_rng(5)
    T, H, W, n = 2, 37, 53, 12
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    frames[0, :8, :32] = np.arange(256, dtype=np.uint8).reshape(8, 32)[..., None]          # every byte value is there
    masks = seeded_masks(n * T, H, W, seed=3).numpy().reshape(n, T, H, W)
    bands = V.contour_band(masks, 3)
    want = frames.copy()
    for t in range(T):
        img = frames[t].copy()
        for m in range(n):
            img = add_mask_to_frame_literal(img, masks[m, t].astype(np.uint8), V.TAB10[min(m, 9)], alpha=0.5)
            img = add_mask_to_frame_literal(img, bands[m, t].astype(np.uint8), [1, 1, 1], alpha=0.1)
        want[t] = img
    got = V.apply_tables(frames, masks, bands)
    assert (got == want).all()
    assert (got != frames).any() and (V.apply_tables(frames, masks[:0], bands[:0]) == frames).all()
    # clear pixels go through the same formula (the tables of rows 60 / 61), whatever it gives
    none = np.zeros((1, T, H, W), dtype=bool)
    assert (V.apply_tables(frames, none, none) == V.lookup_tables()[60][frames]).all()


# --------------------------------------------------------------------------------------------------------------- band
@pytest.mark.parametrize("h,w", BAND_SHAPES)
def test_band_words_equal_scipys_dilations_and_distance_transform(h, w):
    ndi = pytest.importorskip("scipy.ndimage")
    masks = band_masks(h, w)
    for r in (0, 1, 2, 3, 5, 7, 64):
        got = V.contour_band(masks, r)
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        disk = yy * yy + xx * xx <= r * r
        for i, m in enumerate(masks):
            if r <= 7 or i in (2, 4):                                  # (scipy's dilation with a 129 x 129 structure is slow)
                dil = ndi.binary_dilation(m, structure=disk, border_value=0) & ndi.binary_dilation(~m, structure=disk, border_value=0)
                assert (got[i] == dil).all(), (i, r)
            if m.any() and not m.all():                                # the reference's form, with the Euclidean transform
                dist = ndi.distance_transform_edt(m) - ndi.distance_transform_edt(~m)
                assert (got[i] == ((dist <= r) & (dist >= -r) & (r > 0))).all(), (i, r)
        assert not got[0].any() and not got[1].any()                   # an empty and a full mask have no band
    assert not V.contour_band(masks, 0).any()
    with pytest.raises(ValueError):
        V.contour_band(masks, 65)


def test_chamfer_ball_equals_the_euclidean_disk_up_to_radius_3():
    for r in (1, 2, 3):
        assert V.chamfer_offsets(r) == V.disk_offsets(r)
    assert (0, 3) in V.disk_offsets(3) and (2, 2) in V.disk_offsets(3) and (1, 3) not in V.disk_offsets(3)


# ------------------------------------------------------------------------------------------------------------ markers
def test_ring_pixels_lie_between_the_two_radii():
    for R, w in ((8, 4), (8, 3), (5, 1), (1, 4), (0, 2), (6, 0)):
        u, v = np.meshgrid(np.arange(-20, 21), np.arange(-20, 21))
        hit = V.marker_covers(V.RING, R, w, 0, 0, u, v)
        d = np.sqrt(u * u + v * v)
        lo, hi = max(R - w / 2, 0), R + w / 2
        assert (hit == ((d >= lo - 1e-9) & (d <= hi + 1e-9))).all(), (R, w)
    assert V.marker_covers(V.RING, 8, 4, 3, 5, 3 + 8, 5) and not V.marker_covers(V.RING, 8, 4, 3, 5, 3, 5)


def test_cross_arms_have_the_stated_length():
    for size in (8, 5, 0):
        L = size // 2 + 1
        u, v = np.meshgrid(np.arange(-12, 13), np.arange(-12, 13))
        thin = V.marker_covers(V.CROSS, L, 1, 0, 0, u, v)             # width 1: the two diagonals themselves
        assert (thin == ((np.abs(u) == np.abs(v)) & (np.abs(u) <= L))).all()
        wide = V.marker_covers(V.CROSS, L, 4, 0, 0, u, v)             # width 4: within 2 of a diagonal segment
        a, b = u.astype(float), v.astype(float)
        dist = []
        for sgn in (1.0, -1.0):
            s = np.clip((a + sgn * b) / 2, -L, L)                      # the nearest point of the segment is (s, sgn * s)
            dist.append(np.hypot(a - s, b - sgn * s))
        assert (wide == (np.minimum(*dist) <= 2 + 1e-9)).all()
    t = V.marker_table(np.zeros((1, 1, 3, 2)), np.ones((1, 1, 3)), positive_points_per_mask=1, annot_size=8, annot_line_width=4)
    assert t[0, :, 2].tolist() == [V.RING, V.CROSS, V.CROSS] and t[0, :, 3].tolist() == [8, 5, 5] and t[0, :, 5].tolist() == [10, 7, 7]


def test_markers_clip_at_the_borders_nan_draws_around_minus_one_and_the_later_marker_wins():
    H, W, pad = 40, 50, 16
    tr = np.array([[[[0.0, 0.0], [49.9, 39.2], [-3.7, 20.0], [25.0, 44.0], [np.nan, np.nan], [200.0, -100.0]]]])
    vi = np.ones((1, 1, 6))
    table = V.marker_table(tr, vi, positive_points_per_mask=3)
    assert table[0, :, :2].tolist() == [[0, 0], [49, 39], [-3, 20], [25, 44], [-1, -1], [200, -100]]   # truncation toward zero
    small = V.paint_markers(np.zeros((1, H, W, 3), dtype=np.uint8), table)
    moved = table.copy()
    moved[..., :2] += pad
    big = V.paint_markers(np.zeros((1, H + 2 * pad, W + 2 * pad, 3), dtype=np.uint8), moved)
    assert (small == big[:, pad:pad + H, pad:pad + W]).all() and small.any()
    nan_only = V.paint_markers(np.zeros((1, H, W, 3), dtype=np.uint8), table[:, 4:5])
    at_minus_one = V.paint_markers(np.zeros((1, H, W, 3), dtype=np.uint8), V.marker_table(np.full((1, 1, 1, 2), -1.0), np.ones((1, 1, 1)),
                                                                                          positive_points_per_mask=0))
    assert (nan_only == at_minus_one).all() and nan_only.any()
    # two masks' rings on one centre: mask 1 is painted after mask 0
    both = V.marker_table(np.full((1, 2, 1, 2), 20.0), np.ones((1, 2, 1)))
    img = V.paint_markers(np.zeros((1, H, W, 3), dtype=np.uint8), both)
    assert {tuple(c) for c in img[img.any(axis=-1)].tolist()} == {V.marker_colour(1)}


def test_marker_colours_follow_the_visibility_codes():
    vi = np.array([[[1, 0, -1, -2, -3, -4, 7, np.nan]]], dtype=np.float64)
    t = V.marker_table(np.zeros((1, 1, 8, 2)), vi)
    pack = lambda c: c[0] | c[1] << 8 | c[2] << 16
    own, inv = pack(V.marker_colour(0)), pack(V.INVISIBLE_COLOR)
    assert t[0, :, 6].tolist() == [own] + [inv] * 7
    assert t[0, :, 7].tolist() == [own, inv, pack((255, 255, 255)), pack((236, 240, 241)), pack((0, 0, 0)), pack((255, 255, 0)), inv, inv]
    tb = V.marker_table(np.zeros((1, 1, 2, 2)), np.array([[[True, False]]]))
    assert tb[0, :, 6].tolist() == [own, inv]
    # the table built with torch operations (the device path's) is the same table
    g = torch.Generator().manual_seed(4)
    tr = (torch.rand(3, 12, 5, 2, generator=g) - 0.25) * 400
    tr[0, 0, 0], tr[1, 2, 3, 1], tr[2, 1, 1, 0] = float("nan"), float("inf"), -1e12
    vis = torch.randint(-5, 3, (3, 12, 5), generator=g).float()
    for n_pos in (None, 0, 2, 1e9):
        assert (V.marker_table_device(tr, vis, n_pos, 7, 3).numpy() == V.marker_table(tr, vis, n_pos, 7, 3)).all()


# ------------------------------------------------------------------------------------------------------- whole frames
def test_panels_sources_and_query_timesteps_on_the_host():
    rng = np.random.default_rng(11)
    T, H, W, n = 3, 33, 41, 2
    frames = rng.integers(0, 256, (T, 3, H, W), dtype=np.uint8)
    masks = seeded_masks(n * T, H, W, seed=8).reshape(n, T, H, W)
    logits = torch.where(masks, torch.rand(n, T, H, W) + 0.01, -torch.rand(n, T, H, W))
    tr, vi = rng.random((T, n, 4, 2)) * [W, H], rng.integers(-4, 2, (T, n, 4))
    kw = dict(positive_points_per_mask=2)
    pred = V.render_predictions(frames, masks, tr, vi, **kw)
    assert pred.shape == (T, H, W, 3) and pred.dtype == np.uint8
    assert (V.render_predictions(frames.transpose(0, 2, 3, 1), logits, tr, vi, **kw) == pred).all()       # interleaved input, logits
    index = (masks[0].to(torch.uint8) * 5)
    one = V.render_predictions(frames, index, tr[:, :1], vi[:, :1], values=[5], **kw)
    assert (one == V.render_predictions(frames, masks[:1], tr[:, :1], vi[:, :1], **kw)).all()
    stacked = V.render_predictions(frames, masks, tr, vi, panel="stacked", **kw)
    assert stacked.shape == (T, 2 * H, W, 3) and (stacked[:, H:] == pred).all()
    assert (stacked[:, :H] == V.render_predictions(frames, masks, tr, vi, panel="input", **kw)).all()
    cleared = V.render_predictions(frames, masks, tr, vi, query_timesteps=[0, 2], **kw)
    assert (cleared[2] == pred[2]).all() and (cleared[0] != pred[0]).any()
    dropped = masks.clone()
    dropped[1, :2] = False
    assert (cleared == V.render_predictions(frames, dropped, tr, vi, **kw)).all()
    with pytest.raises(ValueError):
        V.render_predictions(frames, masks, panel="sideways")
    with pytest.raises(ValueError):
        V.render_predictions(frames, masks[:, :2])


def test_visualize_predictions_returns_frames_and_logs_the_references_videos():
    rng = np.random.default_rng(12)
    T, H, W, n = 2, 20, 24, 2
    images = torch.from_numpy(rng.integers(0, 256, (T, 3, H, W), dtype=np.uint8))
    logits = torch.randn(n, T, H, W)
    tr, vi = torch.rand(T, n, 3, 2) * 20, torch.ones(T, n, 3)
    qp = torch.zeros(n, 3, 3)
    frames = V.visualize_predictions(images, 0, qp, tr, vi, None, torch.ones(n), logits, positive_points_per_mask=2)
    assert isinstance(frames, list) and len(frames) == T and frames[0].shape == (H, W, 3) and frames[0].dtype == np.uint8
    assert (np.stack(frames) == V.render_predictions(images, logits, tr, vi, positive_points_per_mask=2)).all()
    logged = {}
    again = V.visualize_predictions(images, 0, qp, tr, vi, None, torch.ones(n), logits, sam_per_frame_scores=torch.full((T, n), 0.5),
                                    additional_log_images=images, positive_points_per_mask=2, log_fn=logged.__setitem__)
    assert (np.stack(again) == np.stack(frames)).all()
    assert set(logged) == {"captions", "verbose/input-only", "verbose/predictions-only", "verbose/predictions-with-trajectories",
                           "verbose/input-with-trajectories", "predictions/sam_video_masks"}
    assert logged["captions"][1] == "Frame 1\n[0] Sam IoU prediction: 50.00\n[1] Sam IoU prediction: 50.00"
    assert logged["predictions/sam_video_masks"][0].shape == (3 * H, W, 3)
    assert (np.stack(logged["verbose/input-only"]) == images.permute(0, 2, 3, 1).numpy()).all()
    quiet = {}
    V.visualize_predictions(images, 0, qp, tr, vi, None, torch.ones(n), logits, verbose=False, log_fn=quiet.__setitem__)
    assert set(quiet) == {"captions", "predictions/sam_video_masks"}


def test_visualize_predictions_has_the_references_parameter_list():
    from oracle.reference_loader import REF
    path = os.path.join(REF, "sam_pt", "utils", "util.py")
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    fn = next(node for node in ast.parse(open(path).read()).body
              if isinstance(node, ast.FunctionDef) and node.name == "visualize_predictions")
    names = [a.arg for a in fn.args.args]
    ours = inspect.signature(V.visualize_predictions).parameters
    positional = [k for k, p in ours.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional == names
    assert [k for k, p in ours.items() if p.kind is p.KEYWORD_ONLY] == ["log_fn"]
    defaults = dict(zip(names[len(names) - len(fn.args.defaults):], fn.args.defaults))
    for k, node in defaults.items():
        if isinstance(node, ast.Constant):
            assert ours[k].default == node.value, k
        elif isinstance(node, ast.Tuple):
            assert ours[k].default == tuple(e.value for e in node.elts), k
    assert ours["visibility_to_color"].default is V.VISIBILITY_TO_COLOR


def test_the_module_needs_no_cv2_wandb_matplotlib_or_oracle():
    src = open(os.path.join(ROOT, "sam_pt_amd", "visualize.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(cv2|wandb|matplotlib|oracle)\b", src, flags=re.M)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_c_abi_declares_binds_and_exports_the_viz_entry_points():
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
        res, args = _lib._SIGS[name]                                   # house style: int return code, stream last
        assert res is _lib.c_int and args[-1] is _lib._P


def test_abi_refuses_bad_arguments_without_touching_memory():
    from sam_pt_amd import _lib
    lib = _lib.load()
    assert lib.sampt_viz_band(None, 1, 8, 8, 3, None, None) == -1                  # null planes
    assert lib.sampt_viz_band(None, 1, 8, 8, 65, None, None) == -1                 # radius
    assert lib.sampt_viz_band(None, 1, 0, 8, 3, None, None) == -1                  # shape
    assert lib.sampt_viz_band(None, 0, 8, 8, 3, None, None) == 0                   # nothing to do
    assert lib.sampt_viz_compose(None, 0, 1, 8, 8, None, None, 0, None, None, 0, 2, None, None) == -1    # null frames
    assert lib.sampt_viz_compose(None, 0, 1, 8, 8, None, None, 0, None, None, 0, 4, None, None) == -1    # panel
    assert lib.sampt_viz_compose(None, 0, 0, 8, 8, None, None, 0, None, None, 0, 2, None, None) == 0     # no frames
    with pytest.raises(_lib.SamptError):
        V.render_predictions_device(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
