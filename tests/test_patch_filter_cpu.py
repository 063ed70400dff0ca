"""Patch-similarity filter, without a GPU: the fixture tests/golden/patch_filter.npz (the reference's own ``_track_points`` over a stub
tracker, tools/make_patch_filter_golden.py) against this repository's host path, the conditions the fixture was written under, the
dispatch of ``SamPt._track_points`` for CPU tensors, and the argument checks of the device wrapper."""
import types

import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import patch_filter as PF
from sam_pt_amd.sam_pt import SamPt, rgb2lab
from tests import patch_filter_ref as R


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def flat_inputs(g):
    return g["frames"], g["query_points"].reshape(-1, 3), g["trajectories"], g["visibilities_raw"]


def test_fixture_equals_host_path(gold):
    """The reference's codes == SamPt._patch_similarity_filter + the border lines on the fixture's inputs: pins the fixture to the
    host path and the host path to the reference (rgb2lab substituted in both: parity unpinned)."""
    frames, q, traj, vis = flat_inputs(gold)
    ours = R.host_codes(frames, q, traj, vis, gold["patch_size"], gold["threshold"])
    assert torch.equal(ours, gold["codes"].reshape(ours.shape))
    # ... and the stored similarities are the host path's, to within the noise the fixture measured for it on the machine that
    # wrote it (a CPU with another vector width sums the norm in another order)
    s32 = R.similarities(frames, q, traj, gold["patch_size"])
    assert float((s32 - gold["similarities"]).abs().max()) <= gold["bar_sim"]


def test_fixture_meets_its_conditions(gold):
    frames, q, traj, vis = flat_inputs(gold)
    T, N = vis.shape
    assert (T, tuple(frames.shape[1:]), tuple(gold["query_points"].shape), gold["patch_size"]) == (7, (3, 37, 53), (2, 6, 3), 3)
    H, W = frames.shape[-2:]
    codes, sim, thr, bar = gold["codes"].reshape(T, N), gold["similarities"], gold["threshold"], gold["bar_sim"]
    assert sorted(set(codes.flatten().tolist())) == [-4.0, -3.0, -2.0, 0.0, 1.0]
    assert sorted(set(q[:, 0].tolist())) == [0.0, 3.0, float(T - 1)]
    t0 = q[:, 0].long()
    frames_idx = torch.arange(T)[:, None]
    middle = (t0 > 0) & (t0 < T - 1)
    after = ((codes == -4) & (frames_idx > t0[None])).any(0)
    before = ((codes == -4) & (frames_idx < t0[None])).any(0)
    assert (middle & after & before).any(), "-4 both after and before a middle query frame"
    assert (codes[t0, torch.arange(N)] == -3).any(), "a -3 at a query frame"
    first_fwd = [next((t for t in range(int(t0[i]) + 1, T) if codes[t, i] == -3), None) for i in range(N)]
    first_bwd = [next((t for t in range(int(t0[i]) - 1, -1, -1) if codes[t, i] == -3), None) for i in range(N)]
    assert T - 1 in first_fwd and 0 in first_bwd, "a first -3 at frame T - 1 and one at frame 0"
    assert ((vis == 0) & ~(sim > thr) & (codes == 0)).any(), "a raw visibility of 0 on a non-similar frame"
    x, y = traj[..., 0], traj[..., 1]
    inside = (x >= 0) & (x <= W) & (y >= 0) & (y <= H)
    for near in (x < 1, x > W - 1, y < 1, y > H - 1):
        assert (near & inside).any(), "a point within one pixel of each border"
    assert (x < 0).any() and ((x > W) & (y > H)).any(), "a point left of the frame, one right of and below it"
    assert (traj == traj.round()).all(-1).any() and (traj != traj.round()).all(-1).any(), "integer and fractional coordinates"
    raw = vis == 1
    share = float((sim > thr)[raw].float().mean())
    assert 0.2 <= share <= 0.8
    assert float((sim[raw] - thr).abs().min()) >= 4 * bar
    assert bar == 8 * gold["floor_sim"]
    assert float((sim.double() - gold["similarities_f64"]).abs().max()) == gold["floor_sim"]
    assert 0 < bar < 1e-3


def test_companding_table_is_rgb2lab_s():
    """The table the kernel reads holds, for every byte, what rgb2lab's first two lines give; a grey pixel through the table and the
    rest of the formulas in float64 is rgb2lab's Lab (to a last-place float64 difference of the host's matrix product and pow)."""
    tab = PF.companding_table()
    assert tab.dtype == torch.float64 and tab.shape == (256,) and tab[0] == 0 and tab[255] == 1 and (tab[1:] > tab[:-1]).all()
    g = torch.Generator().manual_seed(3)
    px = torch.randint(0, 256, (4096, 3), generator=g, dtype=torch.uint8)
    lin = tab[px.long()]
    m = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=torch.float64)
    xyz = torch.stack([(lin * m[i]).sum(-1) for i in range(3)], -1) / torch.tensor([0.95047, 1.0, 1.08883], dtype=torch.float64)
    f = torch.where(xyz > 0.008856, torch.from_numpy(xyz.numpy() ** (1.0 / 3.0)), 7.787 * xyz + 16.0 / 116.0)
    lab = torch.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], -1)
    assert float((lab - rgb2lab(px)).abs().max()) < 1e-12


def test_tap_arithmetic_is_torchs_grid_sample():
    """The kernel's tap, modelled in NumPy float32 with every fused multiply-add as one rounding of the float64 result: source index
    fma(g + 1, size / 2, -0.5), weights from i - floor(i), value fma(se, w_se, fma(sw, w_sw, fma(ne, w_ne, nw * w_nw))), corners off
    the frame 0.  Where this project is built the model equals F.grid_sample bit for bit (the count is printed); asserted is 4 ulps of
    the largest value, which a torch build that contracts differently still meets."""
    import numpy as np
    from torch.nn import functional as F
    f32, H, W = np.float32, 37, 53
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, H, W, generator=g) * 200 - 100).float()
    xy = torch.rand(1, 600, 1, 2, generator=g) * torch.tensor([W + 6.0, H + 6.0]) - 3.0
    xy[:, :100] = xy[:, :100].round()
    grid = ((xy + 0.5) / torch.tensor([W, H])) * 2 - 1
    want = F.grid_sample(img, grid.float(), align_corners=False, mode="bilinear")[0, :, :, 0].numpy()        # (3, 600)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    gx, gy = grid.float().numpy()[0, :, 0, 0], grid.float().numpy()[0, :, 0, 1]
    ix = fma(gx + f32(1), np.full_like(gx, W / 2), np.full_like(gx, -0.5))
    iy = fma(gy + f32(1), np.full_like(gy, H / 2), np.full_like(gy, -0.5))
    x0, y0 = np.floor(ix), np.floor(iy)
    we, ws = ix - x0, iy - y0
    ww, wn = f32(1) - we, f32(1) - ws
    out = None
    for cx, cy, wgt in ((x0, y0, wn * ww), (x0 + 1, y0, wn * we), (x0, y0 + 1, ws * ww), (x0 + 1, y0 + 1, ws * we)):
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        v = np.where(ok[None], img[0].numpy()[:, np.clip(cy, 0, H - 1).astype(int), np.clip(cx, 0, W - 1).astype(int)], f32(0))
        out = v * wgt[None] if out is None else fma(v, np.broadcast_to(wgt[None], v.shape), out)
    print(f"{int((out != want).sum())} of {want.size} samples differ in a bit; max |difference| {float(np.abs(out - want).max()):.3e}")
    assert float(np.abs(out - want).max()) <= 4 * 2.0 ** -23 * 100


class _MustNotRun:
    def __getattr__(self, name):
        raise AssertionError(f"the HIP library was reached ({name})")


def test_cpu_tensors_take_the_host_path(gold, monkeypatch):
    frames, q, traj, vis = flat_inputs(gold)
    monkeypatch.setattr(_lib, "load", lambda: _MustNotRun())
    monkeypatch.setattr(PF, "patch_similarity_filter", lambda *a, **k: pytest.fail("device path taken for CPU tensors"))
    assert SamPt.patch_filter_on_device is True
    pred = types.SimpleNamespace(model=types.SimpleNamespace(device=torch.device("cpu")))
    for batch in (1, 5):
        m = SamPt(R.StubTracker(traj, vis), pred, sam_iou_threshold=0.0, point_tracker_mask_batch_size=batch,
                  use_patch_matching_filtering=True, patch_size=gold["patch_size"], patch_similarity_threshold=gold["threshold"])
        tr, codes = m._track_points(frames, gold["query_points"])
        assert torch.equal(codes, gold["codes"]) and torch.equal(tr.reshape(traj.shape), traj)


def test_wrapper_refuses_before_any_library_call(gold, monkeypatch):
    frames, q, traj, vis = flat_inputs(gold)
    monkeypatch.setattr(_lib, "load", lambda: _MustNotRun())
    f = PF.patch_similarity_filter
    with pytest.raises(_lib.SamptError, match="HIP device only"):
        f(frames, q, traj, vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"patch_size must be an integer in 1 \.\. 15; got 16"):
        f(frames, q, traj, vis, PF.MAX_PATCH_SIZE + 1, 0.01)
    with pytest.raises(_lib.SamptError, match="patch_size"):
        f(frames, q, traj, vis, 0, 0.01)
    with pytest.raises(_lib.SamptError, match=r"rgbs must be \(T, 3, H, W\)"):
        f(frames[:, :2], q, traj, vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"query_points must be \(N, 3\)"):
        f(frames, gold["query_points"], traj, vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"trajectories must be \(T, N, 2\)"):
        f(frames, q, traj[:-1], vis, 3, 0.01)
    with pytest.raises(_lib.SamptError, match=r"visibilities must be \(T, N\)"):
        f(frames, q, traj, vis[:, :-1], 3, 0.01)
    with pytest.raises(_lib.SamptError, match="must be a tensor"):
        f(frames.numpy(), q, traj, vis, 3, 0.01)


def test_symbol_is_declared_everywhere():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sampt_hip.h")).read()
    assert "int sampt_patch_filter(" in header and f"#define SAMPT_PATCH_FILTER_MAX_PATCH_SIZE {PF.MAX_PATCH_SIZE}\n" in header
    assert "sampt_patch_filter" in _lib.exported_symbols()
    assert " patch_filter.hip " in open(os.path.join(root, "sam_pt_amd", "csrc", "Makefile")).read()
