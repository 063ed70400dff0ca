"""Prediction overlays: the frames of a clip with every mask's tint, its contour band and the point markers, as the reference's
``visualize_predictions`` (``sam_pt/utils/util.py:331-612``, with ``add_mask_to_frame`` at ``:295-328``) draws them for the demo and
for the evaluator's visual log - without cv2, matplotlib, wandb or a download of the logits.

The definitions are written down once, in the host restatement below (NumPy), which is also what the device path
(``csrc/viz.hip``) is held to with ``==``:

* **Masks**: ``(n_masks, T, H, W)`` float32 logits (set iff ``x > threshold``), bool / uint8 masks (set iff non-zero), or a
  ``(T, H, W)`` uint8 index map with ``values`` (mask ``m`` is set where the map equals ``values[m]``).  ``query_timesteps`` clears
  mask ``m`` on the frames before ``query_timesteps[m]``.
* **Colours**: mask ``m`` takes ``TAB10[min(m, 9)]`` (the reference indexes a 10-entry ``ListedColormap`` with integers, which
  clips); the tint uses the float colour, the markers ``int(c * 255)`` per channel.
* **Blend**: ``add_mask_to_frame`` operation by operation in float64 - ``f = v / 255``, ``o = colour if set else f``,
  ``r = f * alpha + o * (1 - alpha)``, ``uint8(trunc(r * 255))`` - per frame and for each mask in order with the mask's colour at
  ``alpha = 0.5``, then with white on the contour band at ``alpha = 0.1``; uint8 after every step.  Every step maps a byte to a byte
  and depends on the bit, the colour and the channel only, so it is a 256-entry table (``blend_table``); ``lookup_tables`` holds the
  mask step followed by the band step for every colour, channel, bit and band bit, and both paths only look bytes up.  Clear pixels
  go through the same formula and are not special-cased (rows 60 and 61): the reference's behaviour, kept.
* **Contour band**: the reference tests ``|dt(m) - dt(1 - m)| <= contour_radius``, i.e. a pixel is in the band iff a pixel of the
  other class lies within the radius: ``dil_r(m) & dil_r(~m)`` with the disk ``dx^2 + dy^2 <= r^2``, ``~m`` taken inside the image,
  everything outside the image 0 (``band_words``, on 64-bit column words as the device computes it).  The reference measures with
  cv2's 3 x 3 chamfer ``DIST_L2`` (weights 0.955 and 1.3693): for ``r <= 3`` its ball and the Euclidean disk are the same offsets
  (``chamfer_offsets`` / ``disk_offsets``, compared by a test); beyond, this band is Euclidean by definition.
* **Markers**: centres are ``nan_to_num(nan=-1)`` then truncated toward zero (and clamped to +-2^20, far off any frame); point ``i``
  of a mask is a ring if ``i < positive_points_per_mask``, else a cross.  cv2's rasteriser is not restated; the integer predicates
  are this project's own (``marker_covers``).  Markers are painted mask-major, then in point order; the last one wins.  A visible
  point (visibility 1) has its mask's marker colour; any other is ``INVISIBLE_COLOR`` on the predictions panel (the reference's "for
  paper and demos" rule) and ``VISIBILITY_TO_COLOR[int(vis)]`` on the input panel (a code the table lacks: ``INVISIBLE_COLOR``).
* **Not drawn**: the Hershey-font point indices and the debug text box; ``frame_captions`` returns the text of the box per frame.
* **Panels**: ``"predictions"`` (frame, every mask's tint and band, markers: the reference's return value), ``"input"`` (frame and
  markers), ``"stacked"`` (input above predictions: the reference's ``predictions/sam_video_masks`` video).

Output: uint8 ``(T, H, W, 3)``, or ``(T, 2H, W, 3)`` for the stacked panel."""
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

TAB10_255 = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
             (127, 127, 127), (188, 189, 34), (23, 190, 207))
TAB10 = np.array(TAB10_255, dtype=np.float64) / 255.0          # matplotlib's tab10 (its literals are the shortest repr of n / 255)
WHITE = (1.0, 1.0, 1.0)
MASK_ALPHA, BAND_ALPHA = 0.5, 0.1
INVISIBLE_COLOR = (255, 0, 0)
# PointVisibilityType: VISIBLE 1, INVISIBLE 0, REINIT_FAILED -1, OUTSIDE_FRAME -2, PATCH_NON_SIMILAR -3, REJECTED_AFTER_... -4
VISIBILITY_TO_COLOR = {1: None, 0: (255, 0, 0), -4: (255, 255, 0), -2: (236, 240, 241), -3: (0, 0, 0), -1: (255, 255, 255)}
MAX_RADIUS = 64                                                # JF_MAX_R of csrc/jf_bits.h
CENTRE_LIMIT = 1 << 20
PANELS = {"input": 1, "predictions": 2, "stacked": 3}
N_TABLES, CLEAR_TABLE = 62, 60                                 # rows of lookup_tables
RING, CROSS = 0, 1
MARKER_FIELDS = 8                                              # x, y, kind, size, width, reach, colour, input-panel colour


# --------------------------------------------------------------------------------------------------------------------
# definitions: colours and tables
# --------------------------------------------------------------------------------------------------------------------
def mask_colour(m: int) -> np.ndarray:
    """The float RGB of mask ``m``: ``cmap(list(range(n_masks)))`` clips integer indices to the last of the 10 entries."""
    return TAB10[min(int(m), 9)]


def marker_colour(m: int) -> Tuple[int, int, int]:
    c = mask_colour(m)
    return int(c[0] * 255), int(c[1] * 255), int(c[2] * 255)


def blend_table(colour: Optional[float], alpha: float) -> np.ndarray:
    """uint8 [256]: one channel of ``add_mask_to_frame`` for every byte value, in float64.  ``colour``: the overlay's value in this
    channel where the mask is set; None: the mask is clear there and the overlay is the frame itself."""
    f = np.arange(256, dtype=np.uint8) / 255
    o = f if colour is None else np.ones(256, dtype=np.float64) * colour
    r = f * alpha + o * (1 - alpha)
    return (r * 255).astype(np.uint8)


def lookup_tables() -> np.ndarray:
    """uint8 [62][256]: what one mask does to a byte - the tint at alpha 0.5, then the band step at alpha 0.1.  Row
    ``(colour * 3 + channel) * 2 + band`` for a set pixel, row ``60 + band`` for a clear one."""
    band = [blend_table(None, BAND_ALPHA), blend_table(WHITE[0], BAND_ALPHA)]
    t = np.empty((N_TABLES, 256), dtype=np.uint8)
    for ci in range(10):
        for ch in range(3):
            tint = blend_table(TAB10[ci, ch], MASK_ALPHA)
            for b in range(2):
                t[(ci * 3 + ch) * 2 + b] = band[b][tint]
    clear = blend_table(None, MASK_ALPHA)
    for b in range(2):
        t[CLEAR_TABLE + b] = band[b][clear]
    return t


def apply_tables(frames: np.ndarray, masks: np.ndarray, bands: np.ndarray, tables: Optional[np.ndarray] = None) -> np.ndarray:
    """frames uint8 (T, H, W, 3) with masks and bands bool (n, T, H, W) -> the tinted frames, mask after mask."""
    tables = lookup_tables() if tables is None else tables
    out = np.array(frames, dtype=np.uint8, copy=True)
    for m in range(masks.shape[0]):
        bd = bands[m].astype(np.intp)
        for ch in range(3):
            rows = np.where(masks[m], (min(m, 9) * 3 + ch) * 2 + bd, CLEAR_TABLE + bd)
            out[..., ch] = tables[rows, out[..., ch]]
    return out


# --------------------------------------------------------------------------------------------------------------------
# definitions: the contour band
# --------------------------------------------------------------------------------------------------------------------
def disk_offsets(r: int) -> set:
    return {(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r}


def chamfer_offsets(r: int, a: float = 0.955, b: float = 1.3693) -> set:
    """The offsets within distance ``r`` under the 3 x 3 chamfer metric (axial step ``a``, diagonal step ``b``, cv2's DIST_L2
    mask): the cheapest 8-connected path to (dy, dx) takes min(|dy|, |dx|) diagonal steps and the rest axial ones."""
    out = set()
    for dy in range(-2 * r - 2, 2 * r + 3):
        for dx in range(-2 * r - 2, 2 * r + 3):
            lo, hi = sorted((abs(dy), abs(dx)))
            if np.float32(lo * b + (hi - lo) * a) <= r:
                out.add((dy, dx))
    return out


def _isqrt(v: int) -> int:
    s = 0
    while (s + 1) * (s + 1) <= v:
        s += 1
    return s


def _row_masks(h: int, nb: int) -> np.ndarray:
    rows = np.minimum(64, h - 64 * np.arange(nb))
    return np.array([(1 << int(k)) - 1 for k in rows], dtype=np.uint64)


def dilate_words(words: np.ndarray, r: int) -> np.ndarray:
    """The disk dilation of bit-planes uint64 (n, nb, w), everything outside 0 (bits of rows >= h are not cleared): the vertical
    dilations V_k grow by shifts across the bands, the disk is the union over dx of V_isqrt(r^2 - dx^2) moved by dx columns."""
    n, nb, w = words.shape
    mid = np.zeros((n, nb, w + 2 * r), dtype=np.uint64)
    mid[:, :, r:r + w] = words
    up, dn = np.zeros_like(mid), np.zeros_like(mid)
    up[:, 1:], dn[:, :-1] = mid[:, :-1], mid[:, 1:]
    V, D = mid.copy(), np.zeros((n, nb, w), dtype=np.uint64)
    for k in range(r + 1):
        if k > 0:
            if k < 64:
                s, c = np.uint64(k), np.uint64(64 - k)
                V |= (mid << s) | (up >> c) | (mid >> s) | (dn << c)
            else:
                V |= up | dn
        lo = 0 if k == r else _isqrt(r * r - (k + 1) * (k + 1)) + 1
        for dx in range(lo, _isqrt(r * r - k * k) + 1):
            D |= V[:, :, r - dx:r - dx + w] | V[:, :, r + dx:r + dx + w]
    return D


def band_words(words: np.ndarray, h: int, r: int) -> np.ndarray:
    """Bit-planes uint64 (n, nb, w) of masks of height ``h`` -> the bit-planes of their contour bands ``dil_r(m) & dil_r(~m)``."""
    if not 0 <= int(r) <= MAX_RADIUS:
        raise ValueError(f"contour_radius must be in 0 .. {MAX_RADIUS}; got {r}")
    words = np.asarray(words, dtype=np.uint64)
    rm = _row_masks(h, words.shape[1])[None, :, None]
    return dilate_words(words, int(r)) & dilate_words(~words & rm, int(r)) & rm


def contour_band(masks, r: int) -> np.ndarray:
    """bool (..., H, W) -> bool (..., H, W): the pixels with a pixel of the other class within ``r``."""
    from .vis_metrics import pack_bits, unpack_bits
    m = np.asarray(masks).astype(bool)
    flat = m.reshape((-1,) + m.shape[-2:])
    return unpack_bits(band_words(pack_bits(flat), m.shape[-2], r), m.shape[-2]).reshape(m.shape)


# --------------------------------------------------------------------------------------------------------------------
# definitions: markers
# --------------------------------------------------------------------------------------------------------------------
def marker_covers(kind: int, size: int, width: int, x: int, y: int, u, v):
    """Does the marker centred at (x, y) cover pixel (u, v)?  (``u``, ``v``: integers or integer arrays.)
    Ring of radius R = ``size``: ``max(2R - w, 0)^2 <= 4 ((u - x)^2 + (v - y)^2) <= (2R + w)^2``.
    Cross of arm L = ``size``, with a = u - x, b = v - y: the diagonal ``s = clamp(a + b, -2L, 2L)``,
    ``(2a - s)^2 + (2b - s)^2 <= w^2``, or the anti-diagonal ``s = clamp(a - b, -2L, 2L)``, ``(2a - s)^2 + (2b + s)^2 <= w^2``."""
    a, b = np.asarray(u, dtype=np.int64) - int(x), np.asarray(v, dtype=np.int64) - int(y)
    size, width = int(size), int(width)
    if kind == RING:
        d4 = 4 * (a * a + b * b)
        return (max(2 * size - width, 0) ** 2 <= d4) & (d4 <= (2 * size + width) ** 2)
    s = np.clip(a + b, -2 * size, 2 * size)
    hit = (2 * a - s) ** 2 + (2 * b - s) ** 2 <= width * width
    s = np.clip(a - b, -2 * size, 2 * size)
    return hit | ((2 * a - s) ** 2 + (2 * b + s) ** 2 <= width * width)


def _pack_rgb(c) -> int:
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def _marker_shape(n_points: int, positive_points_per_mask, annot_size: int, annot_line_width: int):
    """Per point of a mask: kind, size, and the reach every covered pixel stays within (both axes)."""
    annot_size, annot_line_width = int(annot_size), int(annot_line_width)
    if annot_size < 0 or annot_line_width < 0 or annot_size > 4096 or annot_line_width > 4096:
        raise ValueError(f"annot_size and annot_line_width must be in 0 .. 4096; got {annot_size}, {annot_line_width}")
    n_pos = n_points if positive_points_per_mask is None else positive_points_per_mask
    kind = np.array([RING if i < n_pos else CROSS for i in range(n_points)], dtype=np.int32)
    size = np.where(kind == RING, annot_size, annot_size // 2 + 1).astype(np.int32)
    return kind, size, (size + (annot_line_width + 1) // 2).astype(np.int32)


def _input_colours(visibility_to_color) -> List[int]:
    """The packed input-panel colours of the codes 0, -1, -2, -3, -4 (a code the table lacks: INVISIBLE_COLOR)."""
    table = VISIBILITY_TO_COLOR if visibility_to_color is None else visibility_to_color
    return [_pack_rgb(table.get(-c) or INVISIBLE_COLOR) for c in range(5)]


def marker_table(trajectories, visibilities, positive_points_per_mask=None, annot_size: int = 8, annot_line_width: int = 4,
                 visibility_to_color=None) -> np.ndarray:
    """int32 (T, n_masks * n_points, 8), mask-major: centre x, centre y, kind, size, width, reach, colour on the predictions panel,
    colour on the input panel (r | g << 8 | b << 16), from trajectories (T, n_masks, n_points, 2) and visibilities (T, n_masks,
    n_points).  ``positive_points_per_mask`` None: every point is positive."""
    tr = np.asarray(trajectories.detach().cpu() if isinstance(trajectories, torch.Tensor) else trajectories)
    vi = np.asarray(visibilities.detach().cpu() if isinstance(visibilities, torch.Tensor) else visibilities)
    T, M, P = vi.shape
    if tr.shape != (T, M, P, 2):
        raise ValueError(f"trajectories {tr.shape} do not match visibilities {vi.shape}")
    kind, size, reach = _marker_shape(P, positive_points_per_mask, annot_size, annot_line_width)
    xy = np.nan_to_num(tr.astype(np.float64), nan=-1.0, posinf=CENTRE_LIMIT, neginf=-CENTRE_LIMIT)
    xy = np.trunc(np.clip(xy, -CENTRE_LIMIT, CENTRE_LIMIT)).astype(np.int32)
    code = np.trunc(np.clip(np.nan_to_num(vi.astype(np.float64), nan=0.0, posinf=8, neginf=-8), -8, 8)).astype(np.int64)
    own = np.array([_pack_rgb(marker_colour(m)) for m in range(M)], dtype=np.int32)[None, :, None]
    by_code = np.array(_input_colours(visibility_to_color), dtype=np.int32)
    known = (code <= 0) & (code >= -4)
    t = np.empty((T, M, P, MARKER_FIELDS), dtype=np.int32)
    t[..., 0], t[..., 1] = xy[..., 0], xy[..., 1]
    t[..., 2], t[..., 3], t[..., 4], t[..., 5] = kind, size, int(annot_line_width), reach
    t[..., 6] = np.where(code == 1, own, _pack_rgb(INVISIBLE_COLOR))
    t[..., 7] = np.where(code == 1, own, by_code[np.where(known, -code, 0)])
    return t.reshape(T, M * P, MARKER_FIELDS)


def marker_table_device(trajectories: torch.Tensor, visibilities: torch.Tensor, positive_points_per_mask=None, annot_size: int = 8,
                        annot_line_width: int = 4, visibility_to_color=None) -> torch.Tensor:
    """``marker_table`` with torch operations on the tensors' device: nothing comes back to the host."""
    dev = trajectories.device
    T, M, P = visibilities.shape
    if tuple(trajectories.shape) != (T, M, P, 2):
        raise ValueError(f"trajectories {tuple(trajectories.shape)} do not match visibilities {tuple(visibilities.shape)}")
    kind, size, reach = _marker_shape(P, positive_points_per_mask, annot_size, annot_line_width)
    shape = torch.from_numpy(np.stack([kind, size, np.full(P, int(annot_line_width), dtype=np.int32), reach], axis=-1)).to(dev)
    own = torch.tensor([_pack_rgb(marker_colour(m)) for m in range(M)], dtype=torch.int32, device=dev)[None, :, None]
    by_code = torch.tensor(_input_colours(visibility_to_color), dtype=torch.int32, device=dev)
    xy = torch.nan_to_num(trajectories.to(torch.float64), nan=-1.0, posinf=CENTRE_LIMIT, neginf=-CENTRE_LIMIT)
    xy = xy.clamp(-CENTRE_LIMIT, CENTRE_LIMIT).trunc().to(torch.int32)
    code = torch.nan_to_num(visibilities.to(torch.float64), nan=0.0, posinf=8, neginf=-8).clamp(-8, 8).trunc().to(torch.int64)
    known = (code <= 0) & (code >= -4)
    invisible = torch.full_like(own, _pack_rgb(INVISIBLE_COLOR)).expand(T, M, P)
    t = torch.empty((T, M, P, MARKER_FIELDS), dtype=torch.int32, device=dev)
    t[..., 0:2] = xy
    t[..., 2:6] = shape
    t[..., 6] = torch.where(code == 1, own.expand(T, M, P), invisible)
    t[..., 7] = torch.where(code == 1, own.expand(T, M, P), by_code[torch.where(known, -code, torch.zeros_like(code))])
    return t.reshape(T, M * P, MARKER_FIELDS)


def paint_markers(frames: np.ndarray, table: np.ndarray, colour_field: int = 6) -> np.ndarray:
    """Paints the markers of ``table`` (T, K, 8) onto uint8 (T, H, W, 3) in place, in table order (the last one wins)."""
    T, H, W, _ = frames.shape
    for t in range(T):
        for x, y, kind, size, width, reach, *cols in table[t].tolist():
            x0, x1, y0, y1 = max(x - reach, 0), min(x + reach, W - 1), max(y - reach, 0), min(y + reach, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            hit = marker_covers(kind, size, width, x, y, np.arange(x0, x1 + 1)[None, :], np.arange(y0, y1 + 1)[:, None])
            c = cols[colour_field - 6]
            frames[t, y0:y1 + 1, x0:x1 + 1][hit] = (c & 255, (c >> 8) & 255, (c >> 16) & 255)
    return frames


def frame_captions(n_frames: int, n_masks: int = 0, sam_per_frame_scores=None, additional_frame_annotations=None) -> List[str]:
    """The text the reference puts into each frame's debug box (not drawn here)."""
    out = []
    for t in range(n_frames):
        lines = [f"Frame {t}"]
        if sam_per_frame_scores is not None:
            lines += [f"[{m}] Sam IoU prediction: {float(sam_per_frame_scores[t][m]) * 100:.2f}" for m in range(n_masks)]
        if additional_frame_annotations is not None:
            lines += list(additional_frame_annotations[t])
        out.append("\n".join(lines))
    return out


# --------------------------------------------------------------------------------------------------------------------
# rendering
# --------------------------------------------------------------------------------------------------------------------
def _is_hip(x) -> bool:
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def _frame_layout(shape) -> Tuple[bool, int, int, int]:
    """(interleaved, T, H, W) of uint8 frames (T, 3, H, W) or (T, H, W, 3); (T, 3, H, 3) reads as planar."""
    if len(shape) != 4 or (shape[1] != 3 and shape[3] != 3):
        raise ValueError(f"frames must be (T, 3, H, W) or (T, H, W, 3); got {tuple(shape)}")
    if shape[1] == 3:
        return False, int(shape[0]), int(shape[2]), int(shape[3])
    return True, int(shape[0]), int(shape[1]), int(shape[2])


def _mask_items(masks, values, T: int, H: int, W: int):
    """(n_masks, values per item, planes per item) with item m * T + t, after checking the stack against the frames."""
    if masks is None:
        return 0, None, None
    shape = tuple(masks.shape)
    if values is not None:
        values = [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]
        if shape != (T, H, W):
            raise ValueError(f"an index map must be (T, H, W) = {(T, H, W)}; got {shape}")
        n = len(values)
        return n, [values[m] for m in range(n) for _ in range(T)], [t for _ in range(n) for t in range(T)]
    if len(shape) != 4 or shape[1:] != (T, H, W):
        raise ValueError(f"masks must be (n_masks, T, H, W) with (T, H, W) = {(T, H, W)}; got {shape}")
    return shape[0], None, None


def _check(panel: str, contour_radius: int):
    if panel not in PANELS:
        raise ValueError(f"panel must be one of {sorted(PANELS)}; got {panel!r}")
    if not 0 <= int(contour_radius) <= MAX_RADIUS:
        raise ValueError(f"contour_radius must be in 0 .. {MAX_RADIUS}; got {contour_radius}")


def _timesteps(query_timesteps, n: int) -> Optional[List[int]]:
    if query_timesteps is None:
        return None
    q = [int(v) for v in (query_timesteps.tolist() if hasattr(query_timesteps, "tolist") else query_timesteps)]
    if len(q) != n:
        raise ValueError(f"{len(q)} query_timesteps for {n} masks")
    return q


def render_predictions_host(images, masks=None, trajectories=None, visibilities=None, *, threshold: float = 0.0, values=None,
                            query_timesteps=None, positive_points_per_mask=None, annot_size: int = 8, annot_line_width: int = 4,
                            contour_radius: int = 3, panel: str = "predictions", visibility_to_color=None) -> np.ndarray:
    """The restatement of the module's definitions in NumPy; tensors are downloaded first."""
    from .vis_metrics import bits_pack, unpack_bits
    _check(panel, contour_radius)
    frames = np.asarray(images.detach().cpu() if isinstance(images, torch.Tensor) else images)
    if frames.dtype != np.uint8:
        raise ValueError(f"frames must be uint8; got {frames.dtype}")
    interleaved, T, H, W = _frame_layout(frames.shape)
    frames = np.ascontiguousarray(frames if interleaved else frames.transpose(0, 2, 3, 1))
    n, item_values, item_planes = _mask_items(masks, values, T, H, W)
    table = None
    if trajectories is not None and visibilities is not None and visibilities.shape[1] * visibilities.shape[2] > 0:
        table = marker_table(trajectories, visibilities, positive_points_per_mask, annot_size, annot_line_width, visibility_to_color)
        if table.shape[0] != T:
            raise ValueError(f"{table.shape[0]} frames of trajectories for {T} frames")
    panels = []
    if PANELS[panel] & 1:
        panels.append(frames.copy() if table is None else paint_markers(frames.copy(), table, 7))
    if PANELS[panel] & 2:
        pred = frames.copy()
        if n:
            x = masks.detach().cpu() if isinstance(masks, torch.Tensor) else np.asarray(masks)
            is_float = (x.dtype.is_floating_point if isinstance(x, torch.Tensor) else x.dtype.kind == "f") and values is None
            words = bits_pack(x, threshold=float(threshold) if is_float else None, values=item_values, planes=item_planes)[0]
            words = words.reshape(n, T, -1, W)
            for m, q in enumerate(_timesteps(query_timesteps, n) or []):
                words[m, :max(q, 0)] = 0
            bands = band_words(words.reshape(n * T, -1, W), H, int(contour_radius))
            pred = apply_tables(pred, unpack_bits(words.reshape(n * T, -1, W), H).reshape(n, T, H, W),
                                unpack_bits(bands, H).reshape(n, T, H, W))
        panels.append(pred if table is None else paint_markers(pred, table, 6))
    return panels[0] if len(panels) == 1 else np.concatenate(panels, axis=1)


_TABLES_ON: Dict[Any, torch.Tensor] = {}


def _tables_on(dev) -> torch.Tensor:
    if dev not in _TABLES_ON:
        _TABLES_ON[dev] = torch.from_numpy(lookup_tables()).to(dev)
    return _TABLES_ON[dev]


def contour_band_device(bits: torch.Tensor, h: int, contour_radius: int) -> torch.Tensor:
    """``band_words`` on the HIP device: bit-planes int64 (n, nb, w) (``vis_metrics.bits_pack_device``) -> their bands, same layout."""
    from . import _lib
    who = "contour_band_device"
    _lib.require_hip(getattr(bits, "device", None), who)
    if bits.dim() != 3 or bits.dtype != torch.int64 or bits.shape[1] != (h + 63) // 64 or not bits.is_contiguous():
        raise _lib.SamptError(f"{who}: contiguous int64 bit-planes (n, ceil(h / 64), w) are required; got {tuple(bits.shape)} {bits.dtype}")
    if not 0 <= int(contour_radius) <= MAX_RADIUS:
        raise _lib.SamptError(f"{who}: contour_radius must be in 0 .. {MAX_RADIUS}; got {contour_radius}")
    n, _, w = bits.shape
    with _lib.device_guard(bits.device):
        band = torch.empty_like(bits)
        if n:
            _lib.check(_lib.load().sampt_viz_band(_lib.ptr(bits), n, int(h), w, int(contour_radius), _lib.ptr(band), _lib.stream_ptr()),
                       "sampt_viz_band")
    return band


def render_predictions_device(images: torch.Tensor, masks=None, trajectories=None, visibilities=None, *, threshold: float = 0.0,
                              values=None, query_timesteps=None, positive_points_per_mask=None, annot_size: int = 8,
                              annot_line_width: int = 4, contour_radius: int = 3, panel: str = "predictions",
                              visibility_to_color=None) -> torch.Tensor:
    """The overlays on the HIP device (``csrc/viz.hip``): masks -> bit-planes (``sampt_bits_pack``) -> bands (``sampt_viz_band``) ->
    frames (``sampt_viz_compose``), on torch's current stream, without a host synchronisation.  uint8 on the device."""
    from . import _lib
    from .vis_metrics import bits_pack_device
    who = "render_predictions_device"
    dev = getattr(images, "device", None)
    _lib.require_hip(dev, who)
    _check(panel, contour_radius)
    if images.dtype != torch.uint8:
        raise _lib.SamptError(f"{who}: frames must be uint8; got {images.dtype}")
    interleaved, T, H, W = _frame_layout(images.shape)
    if H == 0 or W == 0 or H * W >= 1 << 31:
        raise _lib.SamptError(f"{who}: 0 < h * w < 2^31 is required; got {H} x {W}")
    n, item_values, item_planes = _mask_items(masks, values, T, H, W)
    code = PANELS[panel]
    lib = _lib.load()
    with _lib.device_guard(dev):
        frames = images.contiguous()
        bits = band = lut = None
        if n and T and code & 2:
            if not isinstance(masks, torch.Tensor) or masks.device != dev:
                raise _lib.SamptError(f"{who}: the masks must be a tensor on {dev}")
            is_float = masks.dtype.is_floating_point and values is None
            bits = bits_pack_device(masks, threshold=float(threshold) if is_float else None, values=item_values, planes=item_planes)[0]
            q = _timesteps(query_timesteps, n) if not isinstance(query_timesteps, torch.Tensor) else query_timesteps
            if q is not None:
                if isinstance(q, torch.Tensor) and q.numel() != n:
                    raise _lib.SamptError(f"{who}: {q.numel()} query_timesteps for {n} masks")
                q = torch.as_tensor(q, device=dev).reshape(n, 1).to(torch.int64)
                keep = torch.arange(T, device=dev)[None, :] >= q
                bits = (bits.view(n, T, -1, W) * keep[:, :, None, None].to(torch.int64)).view(n * T, -1, W)
            band = contour_band_device(bits, H, int(contour_radius))
            lut = _tables_on(dev)
        table, K = None, 0
        if trajectories is not None and visibilities is not None and visibilities.shape[1] * visibilities.shape[2] > 0:
            # (SamPt.forward leaves these two on the host: they are uploaded, a few KB; nothing is downloaded)
            table = marker_table_device(torch.as_tensor(trajectories).to(dev), torch.as_tensor(visibilities).to(dev),
                                        positive_points_per_mask, annot_size, annot_line_width, visibility_to_color)
            if table.shape[0] != T:
                raise _lib.SamptError(f"{who}: {table.shape[0]} frames of trajectories for {T} frames")
            K = int(table.shape[1])
        out = torch.empty((T, H * (2 if code == 3 else 1), W, 3), dtype=torch.uint8, device=dev)
        if T:
            _lib.check(lib.sampt_viz_compose(_lib.ptr(frames), int(interleaved), T, H, W, _lib.ptr(bits), _lib.ptr(band),
                                             n if bits is not None else 0, _lib.ptr(lut), _lib.ptr(table), K, code, _lib.ptr(out),
                                             _lib.stream_ptr()), "sampt_viz_compose")
    return out


def render_predictions(images, masks=None, trajectories=None, visibilities=None, *, threshold: float = 0.0, values=None,
                       query_timesteps=None, positive_points_per_mask=None, annot_size: int = 8, annot_line_width: int = 4,
                       contour_radius: int = 3, panel: str = "predictions", visibility_to_color=None):
    """The overlays of a clip: the device path for HIP tensors (a uint8 tensor there), the host restatement otherwise (an ndarray).
    See the module's docstring for the definitions."""
    fn = render_predictions_device if _is_hip(images) else render_predictions_host
    return fn(images, masks, trajectories, visibilities, threshold=threshold, values=values, query_timesteps=query_timesteps,
              positive_points_per_mask=positive_points_per_mask, annot_size=annot_size, annot_line_width=annot_line_width,
              contour_radius=contour_radius, panel=panel, visibility_to_color=visibility_to_color)


def _to_numpy(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def visualize_predictions(images, step, query_points, trajectories, visibilities, query_masks, query_scores, sam_masks_logits,
                          sam_per_frame_scores=None, additional_log_images=None, additional_frame_annotations=None,
                          query_point_color=(0, 0, 255), visibility_to_color=VISIBILITY_TO_COLOR, positive_points_per_mask=1e9, fps=5,
                          annot_size=8, annot_line_width=4, visualize_query_masks=True, contour_radius=3, verbose=True, log_fmt="mp4",
                          *, log_fn: Optional[Callable[[str, Any], None]] = None) -> List[np.ndarray]:
    """Drop-in for ``sam_pt.utils.util.visualize_predictions`` (same parameters, same order): returns the predictions frames as a
    list of HWC uint8 ndarrays.  Nothing is logged to wandb; ``log_fn(key, frames)`` receives the videos the reference would have
    logged under the reference's keys (the ``verbose/`` ones only with ``verbose``), each as a list of HWC uint8 ndarrays, and
    ``log_fn("captions", [str per frame])`` the text of the debug boxes, which are not drawn.  ``step``, ``fps``, ``log_fmt``,
    ``query_masks``, ``query_scores``, ``query_point_color`` and ``visualize_query_masks`` are accepted and unused: the per-mask
    query-proposal images are wandb mask overlays and are not produced.  ``positive_points_per_mask`` None draws crosses only, as
    the reference's code does."""
    n_pos = 0 if positive_points_per_mask is None else positive_points_per_mask
    kw = dict(positive_points_per_mask=n_pos, annot_size=annot_size, annot_line_width=annot_line_width, contour_radius=contour_radius,
              visibility_to_color=visibility_to_color)

    def frames_of(x) -> List[np.ndarray]:
        return [f for f in _to_numpy(x)]

    if log_fn is None:
        return frames_of(render_predictions(images, sam_masks_logits, trajectories, visibilities, panel="predictions", **kw))
    n_frames, n_masks = len(images), len(query_points)
    log_fn("captions", frame_captions(n_frames, n_masks, sam_per_frame_scores, additional_frame_annotations))
    if verbose:
        log_fn("verbose/input-only", frames_of(render_predictions(images, panel="input")))
        log_fn("verbose/predictions-only", frames_of(render_predictions(images, sam_masks_logits, panel="predictions", **kw)))
    stacked = _to_numpy(render_predictions(images, sam_masks_logits, trajectories, visibilities, panel="stacked", **kw))
    H = stacked.shape[1] // 2
    predictions = [f for f in stacked[:, H:]]
    if verbose:
        log_fn("verbose/predictions-with-trajectories", predictions)
        log_fn("verbose/input-with-trajectories", [f for f in stacked[:, :H]])
    video = [f for f in stacked]
    if additional_log_images is not None:
        extra = _to_numpy(additional_log_images).transpose(0, 2, 3, 1)
        video = [np.concatenate((a, f), axis=0) for a, f in zip(extra, video)]
    log_fn("predictions/sam_video_masks", video)
    return predictions


def render_outputs(video: Dict[str, Any], outputs: Dict[str, Any], **kwargs):
    """The overlays of what ``SamPt.forward(video)`` returned: the frames of ``video["image"]`` (resized to the logits' size the way
    the demo does when they differ), the logits, trajectories and visibilities of ``outputs``, every mask cleared before its query
    frame (``video["query_points"][:, 0, 0]``, when the clip has query points).  Keyword arguments go to ``render_predictions``."""
    logits = outputs["logits"]
    logits = torch.stack(list(logits)) if not isinstance(logits, torch.Tensor) else logits
    images = video["image"]
    images = torch.stack([torch.as_tensor(f) for f in images]) if not isinstance(images, torch.Tensor) else images
    images = images.to(logits.device)
    if tuple(images.shape[-2:]) != tuple(logits.shape[-2:]):
        images = torch.nn.functional.interpolate(images.float(), tuple(logits.shape[-2:]), mode="bilinear").type(torch.uint8)
    if images.dtype != torch.uint8:
        images = images.type(torch.uint8)
    qp = video.get("query_points")
    if qp is not None and "query_timesteps" not in kwargs:
        kwargs["query_timesteps"] = torch.as_tensor(qp)[:, 0, 0].to(torch.int64).tolist()
    return render_predictions(images, logits, outputs.get("trajectories"), outputs.get("visibilities"), **kwargs)
