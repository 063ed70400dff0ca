"""Records tests/golden/raft_ref.npz from the reference's RAFT point tracker run in place on the CPU (tests/raft_ref.py).

Seeded weights (weights.init_raft_state_dict), a synthetic clip of 4 frames at 131 x 140 — padded by 5 -> (2, 3) and 4 ->
(2, 2), coarse grid 17 x 18, pyramid 17 x 18, 8 x 9, 4 x 4, 2 x 2: odd floor pooling at every level and the smallest size the
tracker accepts — and query points on frames 0, 1 and 3.  Stored:

  frames, query_points, trajectories, visibilities       the tracker's input and output
  flow_low (2,3,2,17,18)                                 1/8-resolution flows of the six pair-directions (forward stack first)
  flow_up (2,131,140)                                    the full-resolution forward flow of pair 1
  rows                                                   the coarse pixels (every 9th) whose per-pixel data is stored
  pyr0..pyr3 (rows, h_l, w_l), coords (rows,2), lookup (rows,324), net (rows,128)
                                                         forward direction of pair 1, iteration ITER: correlation planes, the
                                                         lookup's input coordinates and output, the hidden state after the step
  mask_rows, mask (3,18,576), mask_flow_low (2,17,18)    the last iteration's up-sampling mask on three coarse rows (top, middle,
                                                         bottom) and the flow it is applied to
  floor_f64, floor_perturbed, floor_px, bar_px           the reference's own arithmetic noise at this shape (below) and 8 x it

Noise floor (the recipe of oracle/noise_floor.py): the larger of (a) the f32 run against a float64 run of the same weights and
(b) the f32 run against an f32 run with every weight multiplied by 1 + 1e-7 N(0, 1), over all six full-resolution flows.

The script asserts that every reference trajectory coordinate lies at least 0.01 px from a rounding boundary and from the
frame edge, drawing the next query seed until that holds, so that the tests' index-space comparison excludes nothing.

    python tools/make_raft_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.noise_floor import perturbed                       # noqa: E402
from sam_pt_amd.synth import synthetic_clip                    # noqa: E402
from sam_pt_amd.weights import init_raft_state_dict            # noqa: E402
from tests import raft_ref as R                                # noqa: E402

T, H, W, ITERS, ITER, PAIR = 4, 131, 140, 32, 5, 1
MASK_ROWS = (0, 8, 16)


def all_flows(trk, frames, iters=ITERS):
    low, up = [[], []], [[], []]
    for t in range(frames.shape[0] - 1):
        for d, (a, b) in enumerate(((t, t + 1), (t + 1, t))):
            lo, u = R.reference_flow(trk, frames[a], frames[b], iters)
            low[d].append(lo.float())
            up[d].append(u.float())
    return torch.stack([torch.stack(x) for x in low]), torch.stack([torch.stack(x) for x in up])


def float64_flows(sd, frames):
    """The reference in float64: its two explicit .float() casts and its default-dtype constants follow the module's dtype."""
    orig_float, orig_default = torch.Tensor.float, torch.get_default_dtype()
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.set_default_dtype(torch.float64)
    try:
        trk = R.reference_tracker(sd, torch.float64)
        return all_flows(trk, frames)
    finally:
        torch.Tensor.float = orig_float
        torch.set_default_dtype(orig_default)


def record_iteration(trk, core, frames):
    """Pair PAIR forward: the correlation pyramid, and the update block's inputs / hidden state at iteration ITER and its mask
    at the last one."""
    seen = {"pyr": None, "steps": []}

    class Spy(core.CorrBlock):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["pyr"] = [c[:, 0].clone() for c in self.corr_pyramid]

    def hook(mod, args, out):
        seen["steps"].append((args[2][0].clone(), args[3][0].clone(), out[0][0].clone(), out[1][0].clone()))

    orig = core.CorrBlock
    core.CorrBlock = Spy
    h = trk.model.model.update_block.register_forward_hook(hook)
    try:
        low, up = R.reference_flow(trk, frames[PAIR], frames[PAIR + 1], ITERS)
    finally:
        core.CorrBlock = orig
        h.remove()
    corr, flow, net, _ = seen["steps"][ITER]
    return seen["pyr"], corr, flow, net, seen["steps"][-1][3], low, up


def main():
    sd = init_raft_state_dict(72)
    frames, _ = synthetic_clip(T=T, H=H, W=W, seed=72)
    _, _, core = R.load_reference()
    trk = R.reference_tracker(sd)
    low, up = all_flows(trk, frames)
    assert torch.isfinite(up).all()
    low64, up64 = float64_flows(sd, frames)
    lowp, upp = all_flows(R.reference_tracker(perturbed(sd, 1e-7)), frames)
    floor64, floorp = float((up - up64).abs().max()), float((up - upp).abs().max())
    floor = max(floor64, floorp)
    low12, up12 = all_flows(trk, frames, 12)
    print(f"|flow| max {float(up.abs().max()):.3f} px, mean {float(up.abs().mean()):.3f} px; 32 vs 12 iterations differ by "
          f"{float((up - up12).abs().max()):.3f} px")
    print(f"noise floor: f32 vs f64 {floor64:.3e} px, f32 vs 1e-7 perturbed weights {floorp:.3e} px -> bar = 8 x {floor:.3e}")

    pyr, corr, flow, net, mask, low1, up1 = record_iteration(trk, core, frames)
    assert torch.equal(low1, low[0, PAIR]) and torch.equal(up1, up[0, PAIR])
    h8, w8 = low.shape[-2:]
    rows = torch.arange(0, h8 * w8, 9)
    coords = (flow + R.grid(h8, w8)).reshape(2, -1).t()[rows]

    # query points on frames 0, 1 and 3, every trajectory coordinate clear of rounding boundaries and frame edges
    for seed in range(100):
        g = torch.Generator().manual_seed(1000 + seed)
        n = 12
        qt = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 3], dtype=torch.float32)
        qx = 20 + torch.rand(n, generator=g) * (W - 40)
        qy = 20 + torch.rand(n, generator=g) * (H - 40)
        q = torch.stack([qt, qx, qy], 1)
        with torch.no_grad():
            traj, vis = trk.forward(frames[None], q[None])
        fr = traj - traj.floor()
        clear = bool(((fr - 0.5).abs() > 0.01).all())
        inside = bool(((traj[..., 0] > 0.01) & (traj[..., 0] < W - 0.01) & (traj[..., 1] > 0.01) & (traj[..., 1] < H - 0.01)).all())
        if clear and inside and bool(vis.all()):
            break
    else:
        raise AssertionError("no query seed keeps every coordinate 0.01 px from a rounding boundary and the frame edge")
    assert ((fr - 0.5).abs() > 0.01).all() and inside
    print(f"query seed {1000 + seed}; trajectories span x {float(traj[..., 0].min()):.1f}..{float(traj[..., 0].max()):.1f}, "
          f"y {float(traj[..., 1].min()):.1f}..{float(traj[..., 1].max()):.1f}")

    out = dict(frames=frames.numpy(), query_points=q.numpy(), trajectories=traj[0].numpy(), visibilities=vis[0].numpy(),
               flow_low=low.numpy(), flow_up=up[0, PAIR].numpy(), pair=np.int32(PAIR), iteration=np.int32(ITER), iters=np.int32(ITERS),
               rows=rows.numpy().astype(np.int32), coords=coords.numpy(), lookup=corr.reshape(324, -1).t()[rows].numpy(),
               net=net.reshape(128, -1).t()[rows].numpy(), mask_rows=np.asarray(MASK_ROWS, dtype=np.int32),
               mask=mask.permute(1, 2, 0)[list(MASK_ROWS)].numpy(), mask_flow_low=low[0, PAIR].numpy(),
               floor_f64=np.float64(floor64), floor_perturbed=np.float64(floorp), floor_px=np.float64(floor),
               bar_px=np.float64(8 * floor), flow_abs_max=np.float64(up.abs().max()), flow_abs_mean=np.float64(up.abs().mean()),
               iters12_vs_32=np.float64((up - up12).abs().max()))
    for l in range(4):
        out[f"pyr{l}"] = pyr[l][rows].numpy()
    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
