"""TEST INFRASTRUCTURE ONLY: what it takes to run the reference's own BDD100K evaluator (``BDD100KEvaluator.evaluate`` and
``BDD100KEvaluation._evaluate_semisupervised`` of vos_eval/bdd100keval.py) in place on the CPU, and the seeded data set the golden
file tests/golden/bdd100k_ref.npz is made of.

The evaluator imports ``davis2017.metrics`` / ``davis2017.utils``, a package that is absent: the project's own ``db_eval_iou``,
``db_eval_boundary`` and ``db_statistics`` are registered under those names before the reference file is imported by path, so what
is pinned is the protocol (frame selection, visibility split, length bins, the tables), not J and F themselves.  Nothing of the
reference is copied.  ``available()`` is false where the reference tree is absent (the GPU tests never need it: they read the golden
file).
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

from oracle.reference_loader import REF
from sam_pt_amd import vos_metrics as VM

REF_FILE = os.path.join(REF, "sam_pt", "vos_eval", "bdd100keval.py")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bdd100k_ref.npz")
KINDS = ("J", "F", "J_vis", "F_vis", "J_nonvis", "F_nonvis")
SEQ_COLUMNS = ("J-Mean", "F-Mean", "J-Mean-Vis", "F-Mean-Vis", "J-Mean-NonVis", "F-Mean-NonVis")
COUNT_COLUMNS = ("n_frames", "visible_frames", "nonvisible_frames")
H, W = 70, 90


def available() -> bool:
    if not os.path.isfile(REF_FILE):
        return False
    try:
        import pandas  # noqa: F401  (the reference's tables)
        import PIL  # noqa: F401
        import tqdm  # noqa: F401
    except ImportError:
        return False
    return True


def load():
    """The reference module, imported in place with the stand-in ``davis2017``."""
    assert available(), "reference tree not present"
    key = "_sampt_ref_bdd100keval"
    if key in sys.modules:
        return sys.modules[key]
    sys.dont_write_bytecode = True                                      # never write __pycache__ into the reference tree
    if "davis2017.metrics" not in sys.modules:
        pkg, metrics, utils = types.ModuleType("davis2017"), types.ModuleType("davis2017.metrics"), types.ModuleType("davis2017.utils")
        metrics.db_eval_iou, metrics.db_eval_boundary, utils.db_statistics = VM.db_eval_iou, VM.db_eval_boundary, VM.db_statistics
        pkg.metrics, pkg.utils = metrics, utils
        sys.modules["davis2017"], sys.modules["davis2017.metrics"], sys.modules["davis2017.utils"] = pkg, metrics, utils
    spec = importlib.util.spec_from_file_location(key, REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[key] = mod                                              # before executing: the process pool pickles a static method
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------ seeded data set
def _ellipse(cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def _paint(frame, mask, idx):
    frame[mask] = idx


def seeded_dataset(seed: int = 7):
    """{name: (gt (T, H, W) uint8, pred (T, H, W) uint8, planes (T, K + 1, H, W) bool)} of 70 x 90 frames.  Later objects are painted
    over earlier ones.  Added by hand, and asserted by the tests:

    ``a`` (40 frames): object 1, an ellipse that drifts along the left border and is visible on every frame (long); object 2, a
    ring that appears on frame 3, is gone on frames 10 .. 14 and returns until frame 22 (medium), with a prediction on frame 11,
    where the truth is invisible, and none on frame 12, where both are empty; object 3, a thin line that first appears on the last
    frame (the degenerate record, short).
    ``b`` (9 frames): object 1, a cross of one-pixel lines on frames 0 .. 3 (short); object 2, an ellipse that covers the whole frame
    on frame 5 and is predicted as the whole frame there.
    ``c`` (12 frames): object 1, an ellipse with a hole on frames 2 .. 11 whose prediction is missing on two frames; object 2, a
    thin diagonal band on every frame."""
    rng = np.random.default_rng(seed)
    data = {}

    def jitter():
        return rng.integers(-2, 3, size=2)

    # ---- a
    T = 40
    gt, pr = np.zeros((T, H, W), dtype=np.uint8), np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        dy, dx = jitter()
        _paint(gt[t], _ellipse(12 + t, 6, 11, 9), 1)
        _paint(pr[t], _ellipse(12 + t + dy, 6 + dx, 10, 9), 1)
        if 3 <= t <= 9 or 15 <= t <= 22:
            ring = _ellipse(30, 40 + t, 14, 12) & ~_ellipse(30, 40 + t, 7, 6)
            _paint(gt[t], ring, 2)
        if (3 <= t <= 9 or 15 <= t <= 22 or t in (11, 25)) and t != 12:
            dy, dx = jitter()
            _paint(pr[t], _ellipse(30 + dy, 40 + t + dx, 14, 12) & ~_ellipse(30 + dy, 40 + t + dx, 6, 6), 2)
    gt[T - 1, 60, 50:85] = 3
    pr[T - 1, 61, 50:80] = 3
    data["a"] = (gt, pr)
    # ---- b
    T = 9
    gt, pr = np.zeros((T, H, W), dtype=np.uint8), np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        _paint(gt[t], _ellipse(40, 50 + 2 * t, 15, 20), 2)
        _paint(pr[t], _ellipse(41, 51 + 2 * t, 16, 19), 2)
        if t <= 3:
            gt[t, 20 + t, 10:60], gt[t, 5:40, 30 + t] = 1, 1
            pr[t, 20 + t, 12:60], pr[t, 5:38, 31 + t] = 1, 1
        if t == 4:
            pr[t, 22, 10:40] = 1                                        # predicted where the truth is invisible
    gt[5], pr[5] = 2, 2
    data["b"] = (gt, pr)
    # ---- c
    T = 12
    gt, pr = np.zeros((T, H, W), dtype=np.uint8), np.zeros((T, H, W), dtype=np.uint8)
    y, x = np.mgrid[:H, :W]
    for t in range(T):
        if t >= 2:
            dy, dx = jitter()
            _paint(gt[t], _ellipse(35, 30 + 3 * t, 20, 16) & ~_ellipse(33, 30 + 3 * t, 8, 5), 1)
            if t not in (6, 9):
                _paint(pr[t], _ellipse(35 + dy, 30 + 3 * t + dx, 19, 17) & ~_ellipse(33, 30 + 3 * t, 7, 6), 1)
        _paint(gt[t], np.abs(y - x + 10 - t) <= 1, 2)
        _paint(pr[t], np.abs(y - x + 11 - t) <= 1, 2)
    data["c"] = (gt, pr)
    out = {}
    for name, (gt, pr) in data.items():
        K = int(gt.max())
        planes = pr[:, None] == np.arange(K + 1, dtype=np.uint8)[None, :, None, None]
        grow = planes.copy()                                            # overlapping objects: every object grows by one pixel
        grow[:, 1:, 1:, :] |= planes[:, 1:, :-1, :]
        grow[:, 1:, :, 1:] |= planes[:, 1:, :, :-1]
        grow[:, 1:, :-1, :] |= planes[:, 1:, 1:, :]
        out[name] = (gt, pr, grow)
    return out


# -------------------------------------------------------------------------------------------------- running the reference
def _write_png(path, arr):
    from PIL import Image
    im = Image.frombytes("P", (arr.shape[1], arr.shape[0]), np.ascontiguousarray(arr).tobytes())
    im.putpalette([(37 * i) % 256 for i in range(768)])
    im.save(path)


def run_reference(dataset, short_object_threshold=5, long_object_threshold=30):
    """(table_g, table_seq) of ``BDD100KEvaluator.evaluate()`` on the data set written as indexed PNGs to a temporary directory."""
    mod = load()
    with tempfile.TemporaryDirectory() as root:
        res = os.path.join(root, "results")
        for name, (gt, pr, _) in dataset.items():
            for sub in (os.path.join(root, "data", "Annotations", name), os.path.join(root, "data", "JPEGImages", name), os.path.join(res, name)):
                os.makedirs(sub)
            for t in range(len(gt)):
                _write_png(os.path.join(root, "data", "Annotations", name, f"{t:05d}.png"), gt[t])
                _write_png(os.path.join(res, name, f"{t:05d}.png"), pr[t])
                open(os.path.join(root, "data", "JPEGImages", name, f"{t:05d}.jpg"), "wb").close()
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            ev = mod.BDD100KEvaluator(res, os.path.join(root, "data"), short_object_threshold=short_object_threshold,
                                      long_object_threshold=long_object_threshold)
            table_g, table_seq = ev.evaluate()
    return table_g, table_seq


def run_reference_frames(gt, pred, overlapping: bool):
    """The seven dictionaries of ``_evaluate_semisupervised(mp_pool=False)``; the reference reads its masks as float arrays."""
    mod = load()
    res = pred if overlapping else pred.astype(np.float64)
    return mod.BDD100KEvaluation._evaluate_semisupervised(gt.astype(np.float64), res, ("J", "F"), overlapping, mp_pool=False)


def reference_arrays(dataset) -> dict:
    """What the golden file records of the reference's outputs, as flat arrays."""
    table_g, table_seq = run_reference(dataset)
    out = {"g_names": np.array(list(table_g.index)), "g_values": np.array([table_g[k][0] for k in table_g.index], dtype=np.float64),
           "seq_Sequence": np.array(list(table_seq["Sequence"])), "seq_label": np.array(list(table_seq["short-medium-long"]))}
    for c in SEQ_COLUMNS:
        out["seq_" + c] = np.asarray(table_seq[c], dtype=np.float64)
    for c in COUNT_COLUMNS:
        out["seq_" + c] = np.asarray(table_seq[c], dtype=np.int64)
    for name, (gt, pr, planes) in dataset.items():
        for mode, pred in (("index", pr), ("overlap", planes)):
            dicts = run_reference_frames(gt, pred, mode == "overlap")
            for kind, d in zip(KINDS, dicts[:6]):
                for k in sorted(d):
                    out[f"frames_{mode}_{name}_{kind}_{k}"] = np.asarray(d[k], dtype=np.float64)
            out[f"frames_{mode}_{name}_count"] = np.array([dicts[6][k] for k in sorted(dicts[6])], dtype=np.int64)
    return out


def input_arrays(dataset) -> dict:
    out = {"in_names": np.array(list(dataset))}
    for name, (gt, pr, planes) in dataset.items():
        out[f"in_{name}_gt"], out[f"in_{name}_pred"] = gt, pr
        out[f"in_{name}_planes_shape"], out[f"in_{name}_planes_bits"] = np.array(planes.shape), np.packbits(planes)
    return out


def dataset_of(arr) -> dict:
    """The data set of the ``in_*`` arrays of the golden file."""
    out = {}
    for name in arr["in_names"]:
        name = str(name)
        shape = tuple(int(v) for v in arr[f"in_{name}_planes_shape"])
        planes = np.unpackbits(arr[f"in_{name}_planes_bits"])[:int(np.prod(shape))].reshape(shape).astype(bool)
        out[name] = (arr[f"in_{name}_gt"], arr[f"in_{name}_pred"], planes)
    return out


# ---------------------------------------------------------------------------------------------------------- our side
def our_arrays(dataset, to=lambda x: x) -> dict:
    """The same arrays from ``sam_pt_amd.vos_metrics``; ``to`` moves an input array where the evaluation is to run."""
    ev = VM.BDD100KEval()
    out = {}
    for name, (gt, pr, planes) in dataset.items():
        res = ev.add(name, to(pr), to(gt))
        over = VM.evaluate_bdd100k_sequence(to(planes), to(gt), object_overlapping_allowed=True)
        for mode, r in (("index", res), ("overlap", over)):
            for kind in KINDS:
                for k, v in enumerate(r[kind]):
                    out[f"frames_{mode}_{name}_{kind}_{k}"] = v
            out[f"frames_{mode}_{name}_count"] = np.stack([r["n_frames"], r["visible_frames"], r["nonvisible_frames"]], axis=1)
    g, table = ev.summarize()
    out["g_names"], out["g_values"] = np.array(list(g)), np.array(list(g.values()), dtype=np.float64)
    out["seq_Sequence"], out["seq_label"] = np.array(table["Sequence"]), np.array(table["short-medium-long"])
    for c in SEQ_COLUMNS:
        out["seq_" + c] = np.asarray(table[c], dtype=np.float64)
    for c in COUNT_COLUMNS:
        out["seq_" + c] = np.asarray(table[c], dtype=np.int64)
    return out


def assert_same(got: dict, exp: dict):
    """``==`` on every recorded array: names and labels, counts, and floats with NaN equal to NaN."""
    keys = [k for k in exp if not k.startswith("in_")]
    assert keys, "nothing to compare"
    for k in keys:
        assert k in got, f"{k} is missing"
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, f"{k}: shape {g.shape} != {e.shape}"
        if e.dtype.kind in "US":
            assert g.tolist() == e.tolist(), f"{k}: {g.tolist()} != {e.tolist()}"
        elif e.dtype.kind in "iu":
            assert g.dtype.kind in "iu" and np.array_equal(g, e), f"{k}: {g.tolist()} != {e.tolist()}"
        else:
            assert np.array_equal(g, e, equal_nan=True), f"{k} differs: {g.tolist()} != {e.tolist()}"
    extra = [k for k in got if k not in exp]
    assert not extra, f"unexpected arrays {extra[:4]}"


def check_conditions(dataset, ref):
    """What the issue asks of the data set and of the reference's figures on it."""
    assert np.isfinite(ref["g_values"]).all(), f"a global figure of the reference is not finite: {ref['g_values']}"
    assert len(ref["g_values"]) == 22 and tuple(ref["g_names"].tolist()) == VM.BDD100K_GLOBAL_NAMES
    assert set(ref["seq_label"].tolist()) == {"short", "medium", "long"}
    assert 2 <= len(dataset) <= 3 and all(9 <= len(gt) <= 40 for gt, _, _ in dataset.values())
    full = border = returns = ghost = both_empty = last = False
    for gt, pr, _ in dataset.values():
        T = len(gt)
        for k in range(1, int(gt.max()) + 1):
            g, p = gt == k, pr == k
            area, parea = g.sum(axis=(1, 2)), p.sum(axis=(1, 2))
            full |= bool((area == g[0].size).any())
            border |= bool(g[:, 0].any() or g[:, -1].any() or g[:, :, 0].any() or g[:, :, -1].any())
            vis = area > 0
            first = int(np.argmax(vis))
            gone = np.flatnonzero(~vis[first:]) + first
            returns |= bool(len(gone) and vis[gone[0]:].any())
            ghost |= bool(((~vis) & (parea > 0))[first + 1:].any())
            both_empty |= bool(((~vis) & (parea == 0))[first + 1:].any())
            last |= first == T - 1
    assert full and border and returns and ghost and both_empty and last, (full, border, returns, ghost, both_empty, last)
