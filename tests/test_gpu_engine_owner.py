"""Engine replacement on the device: a tracker whose engine is destroyed and rebuilt (what a move to another device does, here
on the same one) computes the same bits with the new engine, and the old handle went back to the library exactly once."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _clip(T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (1, T, 3, H, W), generator=g, dtype=torch.uint8)
    t = torch.randint(0, T, (3, 1), generator=g).float()
    xy = torch.rand(3, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    return frames, torch.cat([t, xy], dim=1)[None]


def _trackers():
    from sam_pt_amd.point_tracker import PipsPointTracker, RaftPointTracker
    from sam_pt_amd.weights import init_pips_state_dict, init_raft_state_dict
    # the smallest frames the engines take: PIPS needs 16 x stride per side, RAFT 128 per padded side
    return [(PipsPointTracker(state_dict=init_pips_state_dict(72)), _clip(8, 64, 96, 1)),
            (RaftPointTracker(state_dict=init_raft_state_dict(72), iters=2), _clip(3, 128, 136, 2))]


@pytest.mark.parametrize("which", [0, 1], ids=["pips", "raft"])
def test_replaced_engine_computes_the_same_bits(dev, which):
    trk, (frames, q) = _trackers()[which]
    frames, q = frames.to(dev), q.to(dev)
    traj0, vis0 = (t.cpu() for t in trk(frames, q))
    h0 = trk._h.value
    assert trk.engines_destroyed == 0 and trk._device == dev
    trk.forget_engine_device()
    traj1, vis1 = (t.cpu() for t in trk(frames, q))
    assert trk.engines_destroyed == 1 and trk._h.value is not None and trk._device == dev
    assert traj0.shape == (1, frames.shape[1], 3, 2) and torch.isfinite(traj0).all()
    assert torch.equal(traj0, traj1) and torch.equal(vis0, vis1)
    print(f"engine {h0:#x} -> {trk._h.value:#x}")
