"""RAFT point tracker, host side: the restatement of tests/raft_ref.py pinned to the live reference (where its tree exists)
and to tests/golden/raft_ref.npz (always), the BatchNorm folding of pack.pack_raft, checkpoint loading, the refusal of frames
too small for the four-level pyramid, and the reference's raft.yaml building our class.

The flow tolerance is read from the golden file: 8 x the reference's own arithmetic noise at the test shape, measured by
tools/make_raft_golden.py (f32 against float64 and against a 1e-7 relative weight perturbation, whichever is larger)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import init_raft_state_dict
from tests import hydra_lite as Hy
from tests import raft_ref as R
from tests.util import max_abs

CONFIGS = os.path.join(R.REF, "configs")
needs_ref = pytest.mark.skipif(not R.available(), reason="reference tree not present (GPU box)")
FP32_GRADE = 2e-5          # x max |reference|: the bar of the PIPS correlation tests (tests/test_gpu_kernels.py)


@pytest.fixture(scope="module")
def gold():
    return {k: v for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def sd():
    return init_raft_state_dict(72)


@pytest.fixture(scope="module")
def restated(gold, sd):
    """The restatement on the golden clip: (flows_forward, flows_backward, flow_low)."""
    return R.flows(sd, torch.from_numpy(gold["frames"]), int(gold["iters"]))


def test_golden_file_is_what_the_issue_asks_for(gold):
    assert gold["frames"].shape == (4, 3, 131, 140) and gold["flow_low"].shape == (2, 3, 2, 17, 18)
    assert [gold[f"pyr{l}"].shape[1:] for l in range(4)] == [(17, 18), (8, 9), (4, 4), (2, 2)]
    assert sorted(set(gold["query_points"][:, 0].tolist())) == [0.0, 1.0, 3.0]
    fr = gold["trajectories"] - np.floor(gold["trajectories"])
    assert (np.abs(fr - 0.5) > 0.01).all()                     # no coordinate near a rounding boundary
    assert float(gold["bar_px"]) == 8 * max(float(gold["floor_f64"]), float(gold["floor_perturbed"]))
    assert 1e-6 < float(gold["bar_px"]) < 1e-2 and float(gold["iters12_vs_32"]) > 1.0
    assert os.path.getsize(R.GOLDEN) < 1 << 20


def test_seeded_weights_have_the_checkpoint_layout(sd):
    assert not any(k.startswith("module.") for k in sd)
    assert sd["update_block.gru.convz1.weight"].shape == (128, 384, 1, 5) and sd["update_block.gru.convq2.weight"].shape == (128, 384, 5, 1)
    assert sd["cnet.layer2.0.downsample.1.running_var"] is sd["cnet.layer2.0.norm3.running_var"]
    assert "fnet.norm1.weight" not in sd and "cnet.norm1.running_mean" in sd
    rv, g = sd["cnet.layer1.0.norm1.running_var"], sd["cnet.layer1.0.norm1.weight"]
    assert float(rv.min()) >= 0.5 and float(rv.max()) <= 1.5 and float((rv - 1).abs().max()) > 0.2 and float((g - 1).abs().max()) > 0.05
    if R.available():                                          # the reference's own module tree accepts it, strictly
        R.reference_tracker(sd)


def test_restatement_matches_the_golden(gold, sd, restated):
    fwd, bwd, low = restated
    bar = float(gold["bar_px"])
    assert max_abs(low, torch.from_numpy(gold["flow_low"])) < bar / 8             # flow_low counts coarse cells of 8 px
    assert max_abs(fwd[int(gold["pair"])], torch.from_numpy(gold["flow_up"])) < bar
    q = torch.from_numpy(gold["query_points"])
    traj, vis = R.chain(fwd, bwd, q)
    want = torch.from_numpy(gold["trajectories"])
    assert max_abs(traj, want) < bar * gold["frames"].shape[0]
    assert (traj.round() == want.round()).all() and (vis.numpy() == gold["visibilities"]).all()


def test_restated_pieces_match_the_golden(gold, sd):
    """Pyramid rows, the lookup at the recorded coordinates and the hidden state of the recorded iteration."""
    frames = torch.from_numpy(gold["frames"])
    p, it, rows = int(gold["pair"]), int(gold["iteration"]), torch.from_numpy(gold["rows"]).long()
    with torch.no_grad():
        fmap, net, inp = R.features(sd, frames[p:p + 2])
        rec = {"iter": it}
        R.pair_flow(sd, fmap[0], fmap[1], net[0], inp[0], it + 1, rec)
    for l in range(4):
        want = torch.from_numpy(gold[f"pyr{l}"])
        assert max_abs(rec["levels"][l][rows], want) < FP32_GRADE * float(want.abs().max())
    levels = [torch.from_numpy(gold[f"pyr{l}"]) for l in range(4)]
    want = torch.from_numpy(gold["lookup"])
    assert max_abs(R.lookup(levels, torch.from_numpy(gold["coords"])), want) < FP32_GRADE * float(want.abs().max())
    # a transposed window is a different answer, so the channel order is pinned
    swapped = R.lookup(levels, torch.from_numpy(gold["coords"])).reshape(-1, 4, 9, 9).transpose(2, 3).reshape(-1, 324)
    assert max_abs(swapped, want) > 100 * FP32_GRADE * float(want.abs().max())
    want = torch.from_numpy(gold["net"])
    assert max_abs(rec["net"].reshape(128, -1).t()[rows], want) < FP32_GRADE * float(want.abs().max())


def test_restated_upsampling_matches_the_golden(gold):
    low = torch.from_numpy(gold["mask_flow_low"])
    mask = torch.zeros(17, 18, 576)
    mask[gold["mask_rows"].tolist()] = torch.from_numpy(gold["mask"])
    up = R.unpad(R.upsample(low, mask.permute(2, 0, 1)), 131, 140)
    want = torch.from_numpy(gold["flow_up"])
    for r in gold["mask_rows"].tolist():
        y0, y1 = max(8 * r - 2, 0), min(8 * r + 8 - 2, 131)
        assert max_abs(up[:, y0:y1], want[:, y0:y1]) < FP32_GRADE * float(want.abs().max())


@needs_ref
def test_restatement_matches_the_live_reference(gold, sd, restated):
    frames = torch.from_numpy(gold["frames"])
    trk = R.reference_tracker(sd)
    bar = float(gold["bar_px"])
    fwd, bwd, low = restated
    ref = {}
    for t in range(3):
        for d, (a, b) in enumerate(((t, t + 1), (t + 1, t))):
            lo, up = R.reference_flow(trk, frames[a], frames[b], int(gold["iters"]))
            ref[(d, t)] = up
            assert max_abs(low[d, t], lo) < bar / 8 and max_abs((fwd, bwd)[d][t], up) < bar
    # the golden is this reference's, recorded on another machine: the CPU convolutions sum in an order that depends on the machine
    # and its thread count, so the two runs agree within the reference's own noise, not to the bit
    assert max_abs(ref[(0, int(gold["pair"]))], torch.from_numpy(gold["flow_up"])) < bar
    # the chain, given the same flows, is the reference's to the bit
    calls = iter([ref[(d, t)] for t in range(3) for d in (0, 1)])
    trk.model.forward = lambda a, b, iters=32: (next(calls)[None], None)
    q = torch.from_numpy(gold["query_points"])
    with torch.no_grad():
        want_traj, want_vis = trk.forward(frames[None], q[None])
    rf, rb = torch.stack([ref[(0, t)] for t in range(3)]), torch.stack([ref[(1, t)] for t in range(3)])
    traj, vis = R.chain(rf, rb, q)
    assert (traj == want_traj[0]).all() and (vis == want_vis[0]).all()
    want = torch.from_numpy(gold["trajectories"])
    assert max_abs(want_traj[0], want) < bar * frames.shape[0] and (want_traj[0].round() == want.round()).all()
    assert (want_vis[0].numpy() == gold["visibilities"]).all()


def test_folded_batchnorm_reproduces_cnet(sd):
    from sam_pt_amd.pack import pack_raft
    w = pack_raft(sd, "cpu")
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 64, 72, generator=g) * 2 - 1

    def conv(name, t, k, stride, pad, cin):
        wt = w[name + ".weight"].reshape(-1, k, k, cin).permute(0, 3, 1, 2)
        return F.conv2d(t, wt, w[name + ".bias"], stride=stride, padding=pad)

    with torch.no_grad():
        want = R.encoder({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, "cnet", x.double())
        t = F.relu(conv("cnet.conv1", F.pad(x, (0, 0, 0, 0, 0, 1)), 7, 2, 3, 4))
        cin = 64
        for li, (dim, stride) in enumerate(((64, 1), (96, 2), (128, 2)), start=1):
            for bi in (0, 1):
                p, st = f"cnet.layer{li}.{bi}", (stride if bi == 0 else 1)
                y = F.relu(conv(p + ".conv1", t, 3, st, 1, cin))
                y = F.relu(conv(p + ".conv2", y, 3, 1, 1, dim))
                if st != 1:
                    t = conv(p + ".downsample.0", t, 1, st, 0, cin)
                t, cin = F.relu(t + y), dim
        got = conv("cnet.conv2", t, 1, 1, 0, 128)
    assert max_abs(got, want) < FP32_GRADE * float(want.abs().max())
    assert w["update_block.encoder.convc1.weight"].shape == (256, 352) and w["update_block.flow_head.conv2.weight"].shape == (4, 2304)
    assert w["update_block.gru.convzr1.weight"].shape == (256, 5 * 384) and w["update_block.encoder.convf1.weight"].shape == (98, 128)
    assert float(w["update_block.encoder.convc1.weight"][:, 324:].abs().max()) == 0.0


def test_checkpoint_loading_strips_the_dataparallel_prefix(tmp_path, sd):
    from sam_pt_amd.point_tracker import RaftPointTracker
    path = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k: v for k, v in sd.items()}, path)
    trk = RaftPointTracker(path)
    assert set(trk._sd) == set(sd) and torch.equal(trk._sd["fnet.conv1.weight"], sd["fnet.conv1.weight"])
    assert trk.iters == 32 and trk.checkpoint_path == path
    with pytest.raises(FileNotFoundError):
        RaftPointTracker(str(tmp_path / "absent.pth"))


def test_small_frames_are_refused_by_name(sd):
    from sam_pt_amd import _lib
    from sam_pt_amd.pack import pack_raft
    from sam_pt_amd.point_tracker import RaftPointTracker
    trk = RaftPointTracker(state_dict=sd)
    with pytest.raises(ValueError, match="128"):
        trk(torch.zeros(1, 2, 3, 120, 140, dtype=torch.uint8), torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="128"):
        trk.flows(torch.zeros(2, 3, 140, 100, dtype=torch.uint8))
    with pytest.raises(_lib.SamptError):                       # large enough, but no device: there is no CPU fallback
        trk(torch.zeros(1, 2, 3, 128, 136, dtype=torch.uint8), torch.zeros(1, 1, 3))
    # the library says the same (a handle only stores its weight pointers; sizing a workspace reads none of them)
    lib = _lib.load()
    w = pack_raft(sd, "cpu")
    names, ptrs, n = _lib.name_table(w)
    h = C.c_void_p()
    assert lib.sampt_raft_create(names, ptrs, n, C.byref(h)) == 0
    try:
        nbytes = C.c_size_t()
        assert lib.sampt_raft_workspace_bytes(h, 4, 120, 140, 3, C.byref(nbytes)) == -3
        assert b"128" in lib.sampt_last_error()
        assert lib.sampt_raft_workspace_bytes(h, 4, 131, 140, 3, C.byref(nbytes)) == 0 and nbytes.value > 0
        three = nbytes.value
        assert lib.sampt_raft_workspace_bytes(h, 4, 131, 140, 1, C.byref(nbytes)) == 0 and 0 < nbytes.value < three
    finally:
        lib.sampt_raft_destroy(h)
    del w["update_block.mask.2.bias"]
    names, ptrs, n = _lib.name_table(w)
    assert lib.sampt_raft_create(names, ptrs, n, C.byref(h)) == -1 and b"update_block.mask.2.bias" in lib.sampt_last_error()


class FakeRaftLib:
    """The four seam-1d calls RaftPointTracker makes, computed by the restatement on CPU tensors."""

    def __init__(self, sd):
        self.sd, self.calls = sd, []

    def sampt_raft_create(self, names, ptrs, n, out):
        self.calls.append("create")
        self.names = set(names)
        out._obj.value = 1
        return 0

    def sampt_raft_destroy(self, h):
        self.calls.append("destroy")

    def sampt_raft_workspace_bytes(self, h, T, H, W, pairs, out):
        self.calls.append(("workspace", T, H, W, pairs))
        out._obj.value = 64
        return 0

    def sampt_raft_flows_f32(self, h, frames, T, H, W, iters, fwd, bwd, low, ws, ws_bytes, stream):
        self.calls.append(("flows", T, H, W, iters))
        f, b, lo = R.flows(self.sd, frames, iters)
        fwd.copy_(f), bwd.copy_(b)
        if low is not None:
            low.copy_(lo)
        return 0

    def sampt_raft_chain(self, fwd, bwd, T, H, W, q, n, traj, vis, stream):
        self.calls.append(("chain", T, n))
        t, v = R.chain(fwd, bwd, q)
        traj.copy_(t), vis.copy_(v.to(torch.uint8))
        return 0


@needs_ref
def test_reference_yaml_builds_our_tracker(monkeypatch, sd):
    """configs/model/point_tracker/raft.yaml with the `_target_` override of INTEGRATION.md instantiates RaftPointTracker, which
    then runs over a fake of the four C-ABI calls and returns the reference's shapes and dtypes."""
    import contextlib
    from sam_pt_amd import _lib
    from sam_pt_amd.point_tracker import RaftPointTracker
    cfg = {"model": Hy.compose(CONFIGS, "model", "sam_pt", {"point_tracker": "raft", "sam@sam_predictor.sam_model": "sam_vit_base"})}
    assert cfg["model"]["point_tracker"]["_target_"] == "sam_pt.point_tracker.raft.RaftPointTracker"
    Hy.apply_overrides(cfg, ["model.point_tracker._target_=sam_pt_amd.point_tracker.RaftPointTracker"])
    node = Hy.resolve(cfg, cwd="/nonexistent")["model"]["point_tracker"]
    assert node["checkpoint_path"] == "/nonexistent/models/raft_ckpts/raft-things.pth"
    with pytest.raises(FileNotFoundError):                     # as the reference: a configured checkpoint must exist
        Hy.instantiate(node)
    Hy.apply_overrides(cfg, ["model.point_tracker.checkpoint_path=null"])
    trk = Hy.instantiate(Hy.resolve(cfg, cwd="/nonexistent")["model"]["point_tracker"])
    assert type(trk) is RaftPointTracker and trk.iters == 32 and trk.checkpoint_path is None
    assert set(trk._sd) == set(sd) and torch.equal(trk._sd["cnet.conv2.bias"], sd["cnet.conv2.bias"])      # the seeded init

    fake = FakeRaftLib(trk._sd)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(_lib, "name_table", lambda named: (named, None, len(named)))
    monkeypatch.setattr(_lib, "require_hip", lambda device, who: None)
    monkeypatch.setattr(_lib, "device_guard", lambda device: contextlib.nullcontext())
    trk.iters = 3                                              # the fake computes with the restatement: keep it short
    from sam_pt_amd.synth import synthetic_clip
    frames, _ = synthetic_clip(T=3, H=128, W=136, seed=3)
    q = torch.tensor([[0.0, 40.0, 50.0], [2.0, 100.0, 90.0]])
    traj, vis = trk(torch.stack([frames, frames.flip(0)]), torch.stack([q, q]))
    assert traj.shape == (2, 3, 2, 2) and traj.dtype == torch.float32 and vis.shape == (2, 3, 2) and vis.dtype == torch.bool
    want_t, want_v = R.track(trk._sd, frames, q, 3)
    assert torch.equal(traj[0], want_t) and torch.equal(vis[0], want_v)
    assert torch.equal(traj[0, 0, 0], q[0, 1:]) and torch.equal(traj[1, 2, 1], q[1, 1:])
    assert fake.calls.count("create") == 1 and ("flows", 3, 128, 136, 3) in fake.calls and ("chain", 3, 2) in fake.calls
    assert "update_block.gru.convzr1.weight" in fake.names
