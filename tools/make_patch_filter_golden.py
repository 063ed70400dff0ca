"""Records tests/golden/patch_filter.npz: the reference's own ``SamPt._track_points`` with the patch-similarity filter on, run in
place on the CPU over a stub tracker that returns prescribed trajectories and visibilities.

The reference (sam_pt/modeling/sam_pt.py:545-692) is loaded through oracle/reference_loader.py.  skimage is absent, so the reference's
``color.rgb2lab`` is substituted by this project's restatement exactly as oracle/make_golden.py::make_patch_golden does: the
fixture pins everything of the filter except that one function (parity unpinned).

The clip: ``synthetic_clip(T=7, H=37, W=53, seed=72, disc_r=4)`` — a background that moves by (-2, -1) px per frame under a small
disc that stays in the middle band.  Two objects of six points, ``patch_size`` 3, threshold THRESHOLD.  A point is prescribed frame by
frame: "on" = it follows the background from its query (similarity 1 up to the arithmetic, or a little less with the sub-pixel
jitter some points carry), "off" = it sits somewhere else (non-similar), or it stands still / walks at random and the clip decides.

  point  query frame   what it is for
  0      0             integer coordinates, on all the way: every code 1
  1      0             fractional; off from frame 4: first hit forward, -4 behind it
  2      0             first -3 at frame T - 1
  3      3             off at 1 and 5 (and beyond): -4 both before and after a middle query frame
  4      3             off AT the query frame: a -3 that starts nothing
  5      T - 1         first -3 at frame 0
  6      T - 1         off at frame 2 with raw visibility 0: stays 0, starts nothing
  7      0             walks out of the frame on the left (x < 0): -2
  8      0             jumps right of and below the frame at frame 4
  9      3             stands still within one pixel of the top and right borders
  10     3             stands still within one pixel of the bottom and left borders
  11     0             random walk of 0.8 px per frame, some raw visibilities 0

Stored: frames (7,3,37,53) uint8, query_points (2,6,3), trajectories (7,12,2), visibilities_raw (7,12), codes (7,2,6) — the
reference's —, similarities (7,12) — the host path's, float32, of every item —, similarities_f64, threshold, patch_size, floor_sim and
bar_sim = 8 x floor_sim, where floor_sim is the largest difference between the host path in float32 and the same formulas carried
through in float64 (tests/patch_filter_ref.py) on these items: the project's usual rule of 8 x the restatement's own noise.

The script REFUSES to write the file unless: the five codes 1, 0, -2, -3 and -4 all occur; -4 occurs both after and before a middle
query frame; at least a fifth of the raw-visible items lie on each side of the threshold; every raw-visible item's similarity is
at least 4 x bar_sim from the threshold; and this repository's host path gives the reference's codes.

    python tools/make_patch_filter_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_loader as RL                      # noqa: E402
from sam_pt_amd.sam_pt import rgb2lab                          # noqa: E402
from sam_pt_amd.synth import synthetic_clip                    # noqa: E402
from tests import patch_filter_ref as R                        # noqa: E402

T, H, W, PS, THRESHOLD = 7, 37, 53, 3, 0.01
MOTION = torch.tensor([-2.0, -1.0])                            # the background's displacement per frame
ELSEWHERE = torch.tensor([[26.0, 5.0], [7.5, 20.25], [46.0, 22.0], [30.25, 33.5]])   # where "off" items sit (cycled)


def on_track(t0, xy, jitter=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    tr = torch.tensor(xy)[None] + (torch.arange(T)[:, None] - t0) * MOTION[None]
    return tr + jitter * (torch.rand(T, 2, generator=g) - 0.5) * (torch.arange(T)[:, None] != t0)


def prescribed():
    """query_points (12,3), trajectories (7,12,2), raw visibilities (7,12)."""
    q, tr = [], []

    def add(t0, xy, track, off=(), first=0):
        q.append((float(t0), *xy))
        track = track.clone()
        for i, t in enumerate(off):
            track[t] = ELSEWHERE[(len(q) + first + i) % len(ELSEWHERE)]
        tr.append(track)

    add(0, (45.0, 8.0), on_track(0, (45.0, 8.0)))
    add(0, (40.25, 32.5), on_track(0, (40.25, 32.5), 0.3, 1), off=(4, 5, 6))
    add(0, (50.0, 10.5), on_track(0, (50.0, 10.5)), off=(6,))
    add(3, (24.5, 31.25), on_track(3, (24.5, 31.25), 0.3, 3), off=(0, 1, 5, 6))
    add(3, (8.0, 6.0), on_track(3, (8.0, 6.0)), off=(3,))
    add(T - 1, (38.5, 9.25), on_track(T - 1, (38.5, 9.25), 0.3, 5), off=(0,), first=1)
    add(T - 1, (10.5, 27.0), on_track(T - 1, (10.5, 27.0)), off=(2,))
    add(0, (5.0, 33.0), on_track(0, (5.0, 33.0)) + torch.tensor([[0.0, 0.0]] * 2 + [[-0.25, 0.0]] * 5))
    far = on_track(0, (49.0, 33.5))
    far[4] = torch.tensor([54.5, 38.25])
    add(0, (49.0, 33.5), far, off=(5, 6))
    add(3, (52.25, 0.75), torch.tensor([[52.25, 0.75]] * T))
    add(3, (0.6, 36.4), torch.tensor([[0.6, 36.4]] * T))
    g = torch.Generator().manual_seed(72)
    walk = torch.tensor([12.0, 8.0])[None] + torch.cat([torch.zeros(1, 2), 0.8 * torch.randn(T - 1, 2, generator=g)]).cumsum(0)
    add(0, (12.0, 8.0), walk)
    vis = torch.ones(T, len(q))
    vis[2, 6] = 0            # off and raw-invisible
    vis[1, 11] = vis[5, 11] = vis[4, 9] = 0
    return torch.tensor(q, dtype=torch.float32), torch.stack(tr, dim=1).float(), vis


def reference_codes(frames, q, traj, vis):
    RefSamPt = RL.load_sam_pt()
    sys.modules["skimage"].color.rgb2lab = lambda a: rgb2lab(torch.from_numpy(np.ascontiguousarray(a))).numpy()
    mod = sys.modules[RefSamPt.__module__]
    if hasattr(mod, "color"):
        mod.color.rgb2lab = sys.modules["skimage"].color.rgb2lab
    pred = types.SimpleNamespace(model=torch.nn.Module())
    pred.model.device = torch.device("cpu")
    kw = dict(sam_iou_threshold=0.0, positive_point_selection_method="random", negative_point_selection_method="random",
              positive_points_per_mask=6, negative_points_per_mask=0, add_other_objects_positive_points_as_negative_points=True,
              max_other_objects_positive_points=None, point_tracker_mask_batch_size=5, iterative_refinement_iterations=0,
              use_patch_matching_filtering=True, patch_size=PS, patch_similarity_threshold=THRESHOLD, use_point_reinit=False,
              reinit_point_tracker_horizon=24, reinit_horizon=24, reinit_variant="reinit-at-median-of-area-diff")
    ref = RefSamPt(R.StubTracker(traj, vis), pred, **kw)
    tr, codes = ref._track_points(frames, q.reshape(2, 6, 3))
    assert torch.equal(tr.reshape(T, 12, 2), traj)
    return codes


def main():
    frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72, disc_r=4.0)
    q, traj, vis = prescribed()
    codes = reference_codes(frames, q, traj, vis)
    s32 = R.similarities(frames, q, traj, PS)
    s64 = R.similarities(frames, q, traj, PS, torch.float64)
    floor_sim = float((s32.double() - s64).abs().max())
    bar_sim = 8 * floor_sim
    torch.set_printoptions(precision=4, linewidth=200, sci_mode=False)
    print("similarities (frames down, points across):")
    print(s32)
    print("codes:")
    print(codes.reshape(T, 12).int())
    print(f"float32 against float64: {floor_sim:.3e} -> bar_sim {bar_sim:.3e}")

    # ---- the conditions
    flat = codes.reshape(T, 12)
    present = sorted(set(flat.flatten().tolist()))
    assert present == [-4.0, -3.0, -2.0, 0.0, 1.0], f"codes present: {present}"
    for i in (3,):
        t0 = int(q[i, 0])
        assert 0 < t0 < T - 1 and (flat[t0 + 1:, i] == -4).any() and (flat[:t0, i] == -4).any(), "-4 on both sides of a middle query frame"
    assert flat[3, 4] == -3 and (flat[:, 4] != -4).all(), "a -3 at a query frame that starts nothing"
    assert flat[T - 1, 2] == -3 and (flat[:T - 1, 2] == 1).all(), "first -3 at frame T - 1"
    assert flat[0, 5] == -3 and (flat[1:, 5] == 1).all(), "first -3 at frame 0"
    assert vis[2, 6] == 0 and s32[2, 6] < THRESHOLD and flat[2, 6] == 0 and (flat[:, 6] != -4).all(), "raw 0 on a non-similar frame"
    assert sorted(set(q[:, 0].tolist())) == [0.0, 3.0, float(T - 1)]
    assert (traj[..., 0] < 0).any() and ((traj[..., 0] > W) & (traj[..., 1] > H)).any()
    for near in (traj[..., 0] < 1, traj[..., 0] > W - 1, traj[..., 1] < 1, traj[..., 1] > H - 1):
        assert (near & (traj[..., 0] >= 0) & (traj[..., 0] <= W) & (traj[..., 1] >= 0) & (traj[..., 1] <= H)).any()
    assert (traj == traj.round()).all(-1).any() and (traj != traj.round()).all(-1).any()
    raw = vis == 1
    similar = s32 > THRESHOLD
    share = float(similar[raw].float().mean())
    margin = float((s32[raw] - THRESHOLD).abs().min())
    print(f"{int(raw.sum())} raw-visible items, {share:.0%} similar; closest to the threshold: {margin:.3e} (need {4 * bar_sim:.3e})")
    assert 0.2 <= share <= 0.8, "at least a fifth of the raw-visible items on each side of the threshold"
    assert margin >= 4 * bar_sim, "a raw-visible item's similarity is too close to the threshold"
    ours = R.host_codes(frames, q, traj, vis, PS, THRESHOLD)
    assert torch.equal(ours, flat), "this repository's host path and the reference disagree"

    np.savez_compressed(R.GOLDEN, frames=frames.numpy(), query_points=q.reshape(2, 6, 3).numpy(), trajectories=traj.numpy(),
                        visibilities_raw=vis.numpy(), codes=codes.numpy().astype(np.float32), similarities=s32.numpy(),
                        similarities_f64=s64.numpy(), threshold=np.float64(THRESHOLD), patch_size=np.int64(PS),
                        floor_sim=np.float64(floor_sim), bar_sim=np.float64(bar_sim))
    print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
