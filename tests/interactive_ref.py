"""TEST INFRASTRUCTURE ONLY: the seeded cases of the interactive point-correction tests, and what it takes to run the reference's own
``extract_largest_cluster_points`` and ``SamPtInteractive.forward`` (sam_pt/modeling/sam_pt_interactive.py) in place on the CPU.

The reference file imports packages that are absent.  ``sklearn_extra.cluster.KMedoids`` is backed by the project's
``kmedoids_alternate`` and ``davis2017.metrics`` by ``vos_metrics.db_eval_iou`` / ``db_eval_boundary`` (as tests/bdd100k_ref.py
does), so what is pinned is the DBSCAN, the cluster choice, the RNG consumption and the loop's control flow, not k-medoids, J or F
themselves.  ``cv2``, ``imageio``, ``wandb`` and ``matplotlib.pyplot`` become objects whose calls do nothing.  Nothing of the
reference is copied.  ``available()`` is false where the reference tree is absent; the tests then read
tests/golden/interactive_ref.npz (written by tools/make_interactive_golden.py).
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch import nn

from oracle import reference_loader as RL
from sam_pt_amd import vos_metrics as VM
from sam_pt_amd.query_points import kmedoids_alternate

REF_FILE = os.path.join(RL.REF, "sam_pt", "modeling", "sam_pt_interactive.py")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interactive_ref.npz")
H, W, T = 64, 96, 5
ACTIONS = (("remove", "negative"), ("remove", "positive"), ("add", "positive"), ("add", "negative"))
HISTORY_FIELDS = ("action", "type", "frame_idx", "point_idx", "iou_before", "iou_after", "interaction_idx", "current_iou_threshold",
                  "overall_iou_before", "overall_iou_after", "boundary_score_before", "boundary_score_after",
                  "overall_boundary_score_before", "overall_boundary_score_after", "jf_score_before", "jf_score_after")


def available() -> bool:
    if not os.path.isfile(REF_FILE):
        return False
    try:
        import PIL  # noqa: F401
        import sklearn  # noqa: F401
        import tqdm  # noqa: F401
    except ImportError:
        return False
    return True


def sklearn_available() -> bool:
    try:
        import sklearn.cluster  # noqa: F401
    except ImportError:
        return False
    return True


# ------------------------------------------------------------------------------------------------------------- DBSCAN cases
def _rects(shape, rects):
    m = np.zeros(shape, dtype=bool)
    for r0, r1, c0, c1 in rects:
        m[r0:r1, c0:c1] = True
    return m


def _sample(mask, n, rng):
    X = np.argwhere(mask).astype(np.float32)
    return X[rng.permutation(len(X))[:n]]


def dbscan_cases(big: bool = True) -> dict:
    """{name: (X float32 (n, 2) of (row, col) pixels, eps, min_samples)}, regenerated from seeds."""
    rng = np.random.default_rng(20240611)
    row = lambda cols: np.array([[0, c] for c in cols], dtype=np.float32)  # noqa: E731
    cases = {}
    cases["n1"] = (np.array([[5, 5]], dtype=np.float32), 1.5, 3)
    cases["all_noise"] = (np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.float32), 1.5, 5)
    # eps 2.3 (r2 = 5) on one pixel row: neighbours are the columns at most 2 away.  With min_samples 4 a run of 5 columns has 3 core
    # columns in the middle and a border column at each end; column 6 between the runs 0 .. 4 and 8 .. 12 is a border of both.
    # The right run comes first, so it is cluster 0 and the bridge must take 0.
    cases["bridge"] = (row([8, 9, 10, 11, 12, 6, 0, 1, 2, 3, 4]), 2.3, 4)
    cases["bridge_shuffled"] = (row([3, 6, 12, 0, 9, 1, 11, 4, 8, 2, 10]), 2.3, 4)
    # point 0 is the border column of the left run, whose core columns all come after the right run's: the right run is cluster 0, the
    # left one cluster 1, yet the left one appears first.  Both have 5 members: the tie of largest_cluster goes to cluster 1.
    cases["first_member_is_border"] = (row([0, 20, 21, 22, 23, 24, 1, 2, 3, 4]), 2.3, 4)
    cases["tie_in_id_order"] = (row([0, 1, 2, 3, 4, 20, 21, 22, 23, 24]), 2.3, 4)
    # knight's moves: every consecutive pair is at d^2 = 5 exactly.  eps 2.24 -> r2 = 5 (neighbours), eps 2.23 -> r2 = 4 (none)
    knights = np.array([[i, 2 * i] for i in range(6)], dtype=np.float32)
    cases["exact_r2_in"] = (knights, 2.24, 2)
    cases["exact_r2_out"] = (knights, 2.23, 2)
    blob = rng.random((30, 44)) < 0.45
    for n in (63, 64, 65, 257):
        cases[f"n{n}"] = (_sample(blob, n, rng), 2.3, 4)
    # the reference's eps rule with 1000 points of a 40 x 60 frame: 2.4 * 2400 / 1000 = 5.76.  Twelve blocks with gaps of 6 empty rows
    # or columns between them (nearest pixels 7 apart): many small clusters
    blocks = _rects((40, 60), [(r0, r1, c0, c1) for r0, r1 in ((0, 6), (12, 18), (24, 30), (36, 40)) for c0, c1 in ((0, 17), (23, 40), (46, 60))])
    cases["n1000"] = (_sample(blocks, 1000, rng), 2.4 * 40 * 60 / 1000, 10)
    cases["duplicates"] = (np.concatenate([_sample(blob, 200, rng)] * 2), 1.5, 6)
    if big:   # the reference's real setting: 18 000 points of two rectangles on 480 x 854
        cases["ref_18000"] = (_sample(_rects((480, 854), [(40, 254, 60, 340), (300, 420, 500, 786)]), 18000, rng), 2.4 * 480 * 854 / 18000, 10)
    return cases


def sklearn_labels(X, eps, min_samples) -> np.ndarray:
    from sklearn.cluster import DBSCAN
    return DBSCAN(eps=eps, min_samples=min_samples).fit(X).labels_.astype(np.int64)


# ------------------------------------------------------------------------------------------------- click-selection cases
def extract_cases() -> dict:
    """{name: (mask bool (H, W), n_points_to_select, seed)}: the three branches of extract_largest_cluster_points (and the fourth,
    no cluster at all)."""
    rng = np.random.default_rng(7)
    ragged = _rects((200, 310), [(20, 120, 30, 200), (150, 185, 220, 290)]) & (rng.random((200, 310)) < 0.9)
    return {
        "large_cluster": (ragged, 3, 11),                                                    # eps 8.27: one cluster of ~15 000 points
        "below_min_points": (_rects((120, 160), [(10, 20, 10, 20), (60, 70, 100, 110), (100, 112, 30, 42)]), 3, 12),   # eps 2.56
        "no_cluster": (_rects((64, 96), [(10, 40, 20, 70)]), 3, 13),                         # eps 0.82: r2 = 0, nothing is core
        "two_pixels": (_rects((64, 96), [(30, 31, 40, 42)]), 2, 14),                         # mask.sum() < 3
    }


# ------------------------------------------------------------------------------------------------------ the reference module
class _Nothing:
    """An object whose attributes are itself and whose calls do nothing."""

    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


class _KMedoids:
    def __init__(self, n_clusters):
        self.n_clusters = n_clusters

    def fit(self, X):
        X = np.asarray(X)
        self.cluster_centers_ = X[kmedoids_alternate(X, self.n_clusters)]
        return self


def load():
    """The reference module, imported in place over the stand-ins."""
    assert available(), "reference tree not present"
    key = "sam_pt.modeling.sam_pt_interactive"
    if key in sys.modules:
        return sys.modules[key]
    RL.load_sam_pt()                                                    # sam_pt.modeling.sam_pt over its own stand-ins
    for name in ("cv2", "imageio", "wandb"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    if "davis2017.metrics" not in sys.modules:
        pkg, metrics, utils = types.ModuleType("davis2017"), types.ModuleType("davis2017.metrics"), types.ModuleType("davis2017.utils")
        metrics.db_eval_iou, metrics.db_eval_boundary, utils.db_statistics = VM.db_eval_iou, VM.db_eval_boundary, VM.db_statistics
        pkg.metrics, pkg.utils = metrics, utils
        sys.modules["davis2017"], sys.modules["davis2017.metrics"], sys.modules["davis2017.utils"] = pkg, metrics, utils
    try:
        importlib.import_module("matplotlib.pyplot")
    except Exception:
        mpl = sys.modules.setdefault("matplotlib", types.ModuleType("matplotlib"))
        mpl.pyplot = sys.modules["matplotlib.pyplot"] = types.ModuleType("matplotlib.pyplot")
    mod = importlib.import_module(key)
    mod.KMedoids = _KMedoids
    mod.cv2 = mod.imageio = mod.wandb = mod.plt = _Nothing()
    mod.tqdm = lambda it, *a, **k: it
    return mod


def reference_extract(mask, n_points, seed) -> np.ndarray:
    mod = load()
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return mod.extract_largest_cluster_points(torch.from_numpy(mask), n_points).numpy()


def our_extract(mask, n_points, seed, device=None) -> np.ndarray:
    from sam_pt_amd.interactive import extract_largest_cluster_points
    torch.manual_seed(seed)
    m = torch.from_numpy(mask)
    return extract_largest_cluster_points(m.to(device) if device is not None else m, n_points, device=device).numpy()


# ---------------------------------------------------------------------------------------------------------------- the loop
class ScriptedTracker(nn.Module):
    """A point tracker with a known smooth motion: every query point moves by (vx, vy) pixels per frame from its query frame and stays
    visible (the [0.01, 0.99] border rule of ``_track_points`` still applies)."""

    def __init__(self, vx=3.0, vy=1.0):
        super().__init__()
        self.v = torch.tensor([vx, vy], dtype=torch.float32)
        self.calls = 0

    def evaluate_batch(self, rgbs, query_points):
        self.calls += 1
        n_frames = rgbs.shape[1]
        q = query_points[0].float().cpu()                                # (N, 3) = t, x, y
        t = torch.arange(n_frames, dtype=torch.float32)[:, None] - q[None, :, 0]
        traj = q[None, :, 1:] + t[:, :, None] * self.v[None, None, :]
        dev = query_points.device
        return {"trajectories_pred": traj[None].to(dev), "visibilities_pred": torch.ones((1, n_frames, q.shape[0]), device=dev)}


def clip(seed=3):
    """(images uint8 (T, 3, H, W), gt bool (T, H, W)): an ellipse that moves by (3, 1) pixels per frame over a textured background."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    base = rng.integers(0, 90, size=(3, H, W))
    images, gts = [], []
    for t in range(T):
        g = ((y - (26 + t)) / 13.0) ** 2 + ((x - (34 + 3 * t)) / 19.0) ** 2 <= 1.0
        img = base.copy()
        img[:, g] = img[:, g] // 2 + 150
        images.append(img.astype(np.uint8))
        gts.append(g)
    return torch.from_numpy(np.stack(images)), torch.from_numpy(np.stack(gts))


def video_of(images, gts, to=lambda x: x):
    # two positive query points off the ellipse (incorrect positives) and one negative point on it (an incorrect negative): the
    # removals happen whatever the predictor says, after them no positive point is left, so the mask is empty and a positive point
    # is added; the seeded SAM then over-segments, which brings the negative additions
    qp = torch.tensor([[[0., 80., 52.], [0., 10., 58.], [0., 30., 22.]]])
    return {"image": [to(f) for f in images], "gt_masks": [g[None] for g in gts], "query_points": qp, "target_hw": (H, W),
            "video_id": "clip"}


SAM_PT_KW = dict(sam_iou_threshold=0.7, positive_point_selection_method="kmedoids", negative_point_selection_method="mixed",
                 positive_points_per_mask=2, negative_points_per_mask=1, add_other_objects_positive_points_as_negative_points=True,
                 max_other_objects_positive_points=None, point_tracker_mask_batch_size=5, iterative_refinement_iterations=0,
                 use_patch_matching_filtering=False, patch_size=3, patch_similarity_threshold=0.01, use_point_reinit=False,
                 reinit_point_tracker_horizon=24, reinit_horizon=24, reinit_variant="reinit-at-median-of-area-diff")
LOOP_CONFIGS = {
    "offline": dict(interactions_max=15, interactions_max_per_frame=3),
    "online": dict(interactions_max=15, interactions_max_per_frame=3, online=True, online_interactive_iou_threshold=0.9),
    "no_tracking": dict(interactions_max=15, interactions_max_per_frame=3, disable_point_tracking=True),
    # the refinement branch of predict_mask: a box from the mask and a third pass
    "refine": dict(interactions_max=9, interactions_max_per_frame=2, online=True, online_interactive_iou_threshold=0.9,
                   iterative_refinement_iterations=1),
}
ALL_FOUR = ("offline", "online")          # the configurations whose recorded run takes every action
SAM_SEED = 72


def cpu_predictor():
    """The oracle's CPU SAM at its smallest test configuration over seeded weights, with the one method of upstream's transform that
    the simulator calls and the oracle's stand-in lacks (float32 arithmetic, as upstream's)."""
    from oracle import sam_ref as R
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    pred = R.SamPredictorRef(init_sam_state_dict(cfg, SAM_SEED), cfg)

    def apply_coords_torch(coords, original_size):
        oh, ow = original_size
        nh, nw = R.get_preprocess_shape(oh, ow, cfg.img_size)
        c = coords.clone().to(torch.float)
        c[..., 0] = c[..., 0] * (nw / ow)
        c[..., 1] = c[..., 1] * (nh / oh)
        return c

    pred.transform.apply_coords_torch = apply_coords_torch
    return pred


def history_rows(history) -> list:
    return [tuple(getattr(h, f) for f in HISTORY_FIELDS) for h in history]


def run_reference_loop(name, predictor=None, tracker=None):
    """(history rows, logits (T, H, W)) of the reference's own forward, run in a temporary working directory."""
    mod = load()
    predictor, tracker = predictor or cpu_predictor(), tracker or ScriptedTracker()
    images, gts = clip()
    model = mod.SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, **{**SAM_PT_KW, **LOOP_CONFIGS[name]}).eval()
    cwd = os.getcwd()
    torch.manual_seed(5)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                out = model(video_of(images, gts))
            import json
            with open(os.path.join(tmp, "interactions", "clip", "history.json")) as fh:
                rows = [tuple(r) for r in json.load(fh)]
        finally:
            os.chdir(cwd)
    return rows, out["logits"][0].numpy()


def run_our_loop(name, predictor=None, tracker=None, to=lambda x: x, **kw):
    """(history rows, logits (T, H, W), last_run) of ``sam_pt_amd.sam_pt_interactive.SamPtInteractive`` on the same clip."""
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    predictor, tracker = predictor or cpu_predictor(), tracker or ScriptedTracker()
    images, gts = clip()
    model = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, **{**SAM_PT_KW, **LOOP_CONFIGS[name], **kw}).eval()
    torch.manual_seed(5)
    out = model(video_of(images, gts, to))
    return history_rows(model.last_run["interaction_history"]), out["logits"][0].cpu().numpy(), model.last_run


def actions_of(rows) -> set:
    return {(r[0], r[1]) for r in rows}


# -------------------------------------------------------------------------------------------------------------- the golden
def history_arrays(prefix, rows, logits) -> dict:
    out = {f"{prefix}_logits": np.asarray(logits, dtype=np.float32), f"{prefix}_n": np.array(len(rows))}
    for k, f in enumerate(HISTORY_FIELDS):
        col = [r[k] for r in rows]
        out[f"{prefix}_{f}"] = np.array(col) if f in ("action", "type") else np.array(col, dtype=np.int64 if isinstance(col[0], int) else np.float64)
    return out


def rows_of(arr, prefix) -> list:
    cols = [arr[f"{prefix}_{f}"].tolist() for f in HISTORY_FIELDS]
    return [tuple(c[i] for c in cols) for i in range(int(arr[f"{prefix}_n"]))]


# ------------------------------------------------------------------------------------------------------------ the GPU clip
def gpu_loop_setup(dev):
    """(video, tracker, predictor, constructor keywords) of the GPU loop tests: SamHip at the smallest test configuration, the PIPS
    tracker, 5 frames of 128 x 256 with a moving disc; an incorrect positive off the disc, a correct positive on it, an incorrect
    negative on it."""
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.synth import synthetic_clip
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    Hh, Ww, Tt = 128, 256, 5
    frames, centres = synthetic_clip(T=Tt, H=Hh, W=Ww, seed=72)
    yy, xx = torch.meshgrid(torch.arange(Hh), torch.arange(Ww), indexing="ij")
    gts = [(((xx - c[0]) ** 2 + (yy - c[1]) ** 2) <= 20.0 ** 2)[None] for c in centres]
    c0 = centres[0]
    qp = torch.tensor([[[0., 200., 30.], [0., float(c0[0]), float(c0[1])], [0., float(c0[0]) + 6, float(c0[1]) - 5]]])
    video = {"image": [f.to(dev) for f in frames], "gt_masks": gts, "query_points": qp, "target_hw": (Hh, Ww), "video_id": "disc"}
    tracker = PipsPointTracker(state_dict=init_pips_state_dict(72))
    predictor = SamPredictor(SamHip(config=cfg, state_dict=init_sam_state_dict(cfg, 72), precision="f32").to(dev))
    return video, tracker, predictor, {**SAM_PT_KW, "interactions_max": 12, "interactions_max_per_frame": 3}


def decode_batch_differences(setup, last_run, batch=4) -> list:
    """[(state name, largest |logit difference|, largest |logit|, frames with a visible negative)] of ``decode_batch=batch`` against
    ``decode_batch=1`` on fixed point states: the final state of a run, and the same with the negative points hidden on the first three
    frames, so that one pass holds single-pass and two-pass chains side by side."""
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    video, tracker, predictor, kw = setup
    one = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, decode_batch=1, **kw).eval()
    many = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, decode_batch=batch, **kw).eval()
    traj, vis, lab = last_run["trajectories"], last_run["visibilities"], last_run["point_labels"]
    mixed = vis.clone()
    mixed[:3, 0, lab == 0] = 0
    out = []
    for name, v in (("final state of the run", vis), ("negatives hidden on frames 0 .. 2", mixed)):
        l1, lb = one.decode_state(video, traj, v, lab), many.decode_state(video, traj, v, lab)
        assert l1.shape == lb.shape == (vis.shape[0],) + tuple(video["target_hw"])
        has_neg = [bool(((v[t, 0] == 1) & (lab == 0)).any()) for t in range(vis.shape[0])]
        out.append((name, float((l1 - lb).abs().max()), float(l1.abs().max()), has_neg))
    return out
