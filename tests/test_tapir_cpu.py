"""TAPIR on the CPU: what of the restatement (tests/tapir_ref.py) can be pinned, the golden file, the checkpoint loader and the adapter.

PARITY UNPINNED for the model itself: the reference needs JAX, Haiku and a checkpoint, none of which exists where this project is
built.  Pinned here: ``convert_grid_coordinates`` against the reference's NumPy-only utils/transforms.py; the two bilinear reads
against scipy.ndimage.map_coordinates; TensorFlow's "SAME" padding against its closed formula; and the adapter against the
reference's own ``TapirPointTracker.forward`` (tapir/tracker.py:72-108) run in place over small stand-in modules, with ``==``."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import (init_tapir_state_dict, load_tapir_checkpoint, tapir_haiku_key_map, tapir_state_dict_to_haiku)
from tests import tapir_ref as R
from tests.util import max_abs, synthetic_clip

needs_ref = pytest.mark.skipif(not R.available(), reason="reference tree not present (GPU box)")


@pytest.fixture(scope="module")
def sd():
    return init_tapir_state_dict(72)


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def fresh(gold, sd):
    frames01 = F.interpolate(gold["frames"] / 255, (256, 256), mode="bilinear", align_corners=False, antialias=True)
    video = (frames01 * 2 - 1).permute(0, 2, 3, 1)
    return video, R.forward(sd, video, gold["video_q"], stages=True)


# ---------------------------------------------------------------------------------------------- pins
@needs_ref
def test_convert_grid_coordinates_equals_the_reference():
    """(coords * output size) / input size, in that order: equal in float64 (NumPy promotes the reference's product with the integer
    sizes to float64), and the float32 restatement is that value rounded."""
    ref = R.load_transforms().convert_grid_coordinates
    g = np.random.default_rng(0)
    xy = g.uniform(-20, 300, (7, 5, 2))
    for a, b in (((256, 256), (64, 64)), ((256, 256), (32, 32)), ((32, 32), (256, 256)), ((854, 480), (256, 256))):
        assert np.array_equal(R.convert_grid_coordinates(torch.from_numpy(xy), a, b).numpy(), ref(xy, a, b))
        got32 = R.convert_grid_coordinates(torch.from_numpy(xy.astype(np.float32)), a, b).numpy()
        assert got32.dtype == np.float32 and np.allclose(got32, ref(xy.astype(np.float32), a, b), rtol=2e-7, atol=0)
    tyx = g.uniform(0, 200, (9, 3))
    want = ref(tyx, (5, 256, 256), (5, 32, 32), coordinate_format="tyx")
    assert np.array_equal(R.convert_grid_coordinates(torch.from_numpy(tyx), (5, 256, 256), (5, 32, 32)).numpy(), want)


def test_bilinear_reads_against_scipy():
    """'nearest' is scipy's 'nearest'.  JAX's 'constant' zeroes each CORNER outside the map, which scipy calls 'grid-constant'; scipy's
    own 'constant' returns 0 for every sample outside the map's extent, so the two agree inside the map and from one cell outside on,
    and differ only in the one-cell band around it, where the reference (JAX) interpolates towards zero."""
    from scipy.ndimage import map_coordinates
    g = torch.Generator().manual_seed(1)
    H, W, C = 6, 9, 3
    grid = torch.randn(H, W, C, generator=g, dtype=torch.float64)
    yx = torch.rand(400, 2, generator=g, dtype=torch.float64) * torch.tensor([H + 4.0, W + 4.0]) - 2.5
    yx = torch.cat([yx, torch.tensor([[0.0, 0.0], [H - 1.0, W - 1.0], [-1.0, 3.0], [2.0, W * 1.0], [-0.5, -0.5], [H - 0.5, W - 0.5], [2.5, 3.0]],
                                     dtype=torch.float64)])

    def sp(mode):
        return np.stack([map_coordinates(grid[..., c].numpy(), yx.t().numpy(), order=1, mode=mode) for c in range(C)], -1)

    assert np.allclose(R.bilinear(grid, yx, "nearest").numpy(), sp("nearest"), rtol=0, atol=1e-12)
    ours = R.bilinear(grid, yx, "constant").numpy()
    assert np.allclose(ours, sp("grid-constant"), rtol=0, atol=1e-12)
    y, x = yx[:, 0].numpy(), yx[:, 1].numpy()
    inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    far = (y <= -1) | (y >= H) | (x <= -1) | (x >= W)
    band = ~inside & ~far
    assert inside.sum() > 50 and far.sum() > 50 and band.sum() > 50
    assert np.allclose(ours[inside | far], sp("constant")[inside | far], rtol=0, atol=1e-12)
    assert (sp("constant")[band] == 0).all() and (np.abs(ours[band]).max(-1) > 0).any()


@pytest.mark.parametrize("side,k,stride,want", [(256, 7, 2, (2, 3)), (128, 3, 1, (1, 1)), (128, 3, 2, (0, 1)), (64, 3, 2, (0, 1)), (128, 1, 2, (0, 0)),
                                               (32, 3, 2, (0, 1)), (15, 3, 2, (1, 1)), (15, 7, 2, (3, 3)), (13, 1, 2, (0, 0)), (9, 5, 3, (1, 1)),
                                               (10, 5, 3, (2, 2)), (11, 5, 3, (1, 2))])
def test_same_padding_closed_formula(side, k, stride, want):
    """TensorFlow: out = ceil(n / s); total = max((out - 1) s + k - n, 0); before = total // 2, after = the rest."""
    out = -(-side // stride)
    total = max((out - 1) * stride + k - side, 0)
    assert R.same_padding(side, k, stride) == (total // 2, total - total // 2) == want
    g = torch.Generator().manual_seed(side)
    x, w = torch.randn(1, 2, side, side + 1, generator=g), torch.randn(3, 2, k, k, generator=g)
    y = R.conv_same(x, w, stride)
    assert y.shape[2:] == (out, -(-(side + 1) // stride))
    # the same numbers from an explicitly padded copy, with the window of output (0, 0) starting `before` cells outside
    xp = torch.zeros(1, 2, side + total, side + 1 + sum(R.same_padding(side + 1, k, stride)))
    xp[:, :, want[0]:want[0] + side, R.same_padding(side + 1, k, stride)[0]:R.same_padding(side + 1, k, stride)[0] + side + 1] = x
    assert torch.equal(y, F.conv2d(xp, w, stride=stride))


# ---------------------------------------------------------------------------------------------- the restatement and its golden
def test_f32_against_f64(gold, sd, fresh):
    video, o32 = fresh
    o64 = R.forward(sd, video, gold["video_q"], dtype=torch.float64)
    for i in range(R.ITERS + 1):
        assert max_abs(o32["iter_tracks"][i], o64["iter_tracks"][i].float()) <= float(gold["floor_px"]) * 1.0001
        assert max_abs(o32["iter_occlusion"][i], o64["iter_occlusion"][i].float()) <= float(gold["floor_logit"]) * 1.0001
    assert float(gold["bar_px"]) == 8 * float(gold["floor_px"]) and float(gold["bar_logit"]) == 8 * float(gold["floor_logit"])
    assert float(gold["min_gap"]) > 1e-3


def test_golden_equals_a_fresh_run(gold, fresh):
    _, o = fresh
    bar_px, bar_logit = float(gold["bar_px"]), float(gold["bar_logit"])
    assert max_abs(torch.stack(o["iter_tracks"]), gold["iter_tracks"]) < bar_px
    assert max_abs(torch.stack(o["iter_occlusion"]), gold["iter_occlusion"]) < bar_logit
    assert max_abs(torch.stack(o["iter_expected_dist"]), gold["iter_expected_dist"]) < bar_logit
    rows = gold["map_rows"].long()
    assert max_abs(o["hires"].reshape(5, -1, 128)[:, rows], gold["hires_rows"]) < 1e-5
    assert max_abs(o["lowres"].reshape(5, -1, 256)[:, rows[rows < 1024]], gold["lowres_rows"]) < 1e-5
    assert max_abs(o["qf"], gold["qf"]) < 1e-5 and max_abs(o["logits"], gold["logits"]) < 1e-4
    vis = R.visibility_probability(o["occlusion"], o["expected_dist"]).t() > float(gold["threshold"])
    assert torch.equal(vis, gold["visibilities"]) and 0 < int(vis.sum()) < vis.numel()
    # the six queries are what the issue asks for: frame 0, the last frame, a corner patch, a cell border, two interior
    q = gold["video_q"]
    assert q[:, 0].tolist() == [0, 4, 2, 1, 3, 2] and abs(float(q[3, 1]) - 128) < 1e-4 and abs(float(q[3, 2]) - 96) < 1e-4
    assert float(gold["x0"][2, 2, 388:].abs().min()) == 0.0


def test_stages_compose(sd, gold, fresh):
    """mixer_input + mixer == refine, and a mixer block is its two halves."""
    _, o = fresh
    with torch.no_grad():
        x0, base = R.mixer_input(o["hires"], o["lowres"], o["qf"], o["iter_tracks"][0], o["iter_occlusion"][0], o["iter_expected_dist"][0], None)
        assert max_abs(x0, gold["x0"]) < 1e-4 and x0.shape == (6, 5, 486)       # (its occlusion columns carry the head's gain)
        res = R.mixer(sd, x0)
        assert torch.equal(o["iter_tracks"][0] + res[..., :2], o["iter_tracks"][1])
        h = x0 @ sd["mixer.in.weight"].t() + sd["mixer.in.bias"]
        assert max_abs(R.mixer_block(sd, 0, h), gold["block0"]) < 1e-4
        one = R.temporal_half(sd, "mixer.blocks.0.", h[:, :1])                  # T = 1: both neighbours are padding
        assert one.shape == (6, 1, 512) and not torch.equal(one, R.temporal_half(sd, "mixer.blocks.0.", h)[:, :1])


# ---------------------------------------------------------------------------------------------- checkpoint loader
def test_checkpoint_round_trip(tmp_path, sd):
    params = tapir_state_dict_to_haiku(sd)
    assert params["tapir/~/resnet/~/initial_conv"]["w"].shape == (7, 7, 3, 64)
    assert params["tapir/~/pips_mlp_mixer/block_3/mlp1_up"]["w"].shape == (3, 1, 2048)
    assert params["tapir/~/pips_mlp_mixer/block/mlp2_up"]["w"].shape == (512, 2048)
    assert params["tapir/~/cost_volume_occlusion_1"]["w"].shape == (3, 3, 16, 32)
    params["tapir/~/regression_hid"] = {"w": np.zeros((3, 128), np.float32), "b": np.zeros(128, np.float32)}      # a head that is never called
    params["tapir/~/conv_stats_conv1"] = {"w": np.zeros((5, 5, 1, 256), np.float32), "b": np.zeros(256, np.float32)}
    path = os.path.join(tmp_path, "tapir_checkpoint.npy")
    np.save(path, {"params": params, "state": {}}, allow_pickle=True)
    back = load_tapir_checkpoint(path)
    assert list(back) == list(tapir_haiku_key_map()) and set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    del params["tapir/~/pips_mlp_mixer/block_7/mlp1_up_1"]
    np.save(path, {"params": params, "state": {}}, allow_pickle=True)
    with pytest.raises(KeyError, match="block_7/mlp1_up_1"):
        load_tapir_checkpoint(path)


def test_pack_layouts(sd):
    from sam_pt_amd.pack import pack_tapir
    w = pack_tapir(sd, "cpu")
    assert w["resnet.initial_conv.weight"].shape == (64, 7 * 7 * 4) and "resnet.initial_conv.weight_hl" not in w
    assert w["resnet.g1.b0.conv0.weight"].shape == (128, 9 * 64) and w["resnet.g1.b0.conv0.weight_hl"].shape == (2, 128, 9 * 64)
    assert w["resnet.g2.b0.shortcut.weight_hl"].dtype == torch.float16
    assert torch.equal(w["heads.hid3.weight"][5, 7], sd["heads.hid3.weight"][:, 5, 2, 1])
    assert w["mixer.in.weight"].shape == (512, 496) and (w["mixer.in.weight"][:, 486:] == 0).all()
    assert w["mixer.blocks.0.dw1.weight"].shape == (3, 2048) and not w["mixer.zeros"].any()


# ---------------------------------------------------------------------------------------------- adapter and constructor
def _cpu_tracker(model, **kw):
    """Our tracker with the device model replaced by ``model`` (the reference's ``jitted_forward`` signature)."""
    from sam_pt_amd.point_tracker import TapirPointTracker
    trk = TapirPointTracker(state_dict={}, **kw)

    def run(frames01, q_tyx):
        video = (frames01.cpu().numpy() * 2 - 1).transpose(0, 1, 3, 4, 2)
        return {k: torch.from_numpy(np.asarray(v).copy()) for k, v in model(video, q_tyx.numpy()).items()}

    trk._model = run
    return trk


@needs_ref
def test_adapter_equals_the_reference_adapter(sd):
    """Non-square frames, B = 2: the same model behind the reference's forward and behind ours -> identical trajectories and
    visibilities.  Once with a cheap stand-in model whose outputs straddle the threshold, once with the restated model."""
    frames, _ = synthetic_clip(T=3, H=40, W=56, seed=3)
    rgbs = torch.stack([frames, frames.flip(0)])
    g = torch.Generator().manual_seed(4)
    q = torch.stack([torch.randint(0, 3, (2, 5), generator=g).float(), torch.rand(2, 5, generator=g) * 56, torch.rand(2, 5, generator=g) * 40], -1)
    seen = []

    def stand_in(video, query):
        seen.append((np.asarray(video).copy(), np.asarray(query).copy()))
        B, T, N = video.shape[0], video.shape[1], query.shape[1]
        r = np.random.default_rng(5)
        tracks = query[:, :, None, 2:0:-1] + r.normal(0, 3, (B, N, T, 2)).astype(np.float32) + video.mean((2, 3, 4))[:, None, :, None]
        return {"tracks": tracks.astype(np.float32), "occlusion": r.normal(0, 2, (B, N, T)).astype(np.float32),
                "expected_dist": r.normal(0, 2, (B, N, T)).astype(np.float32)}

    for model in (stand_in, R.model_fn(sd)):
        ref_t, ref_v = R.reference_tracker(model, 0.1).forward(rgbs, q)
        our_t, our_v = _cpu_tracker(model, visibility_threshold=0.1).forward(rgbs, q)
        assert ref_t.shape == (2, 3, 5, 2) and ref_v.shape == (2, 3, 5) and ref_v.dtype == torch.bool
        assert torch.equal(our_t, ref_t) and torch.equal(our_v, ref_v)
        assert 0 < int(ref_v.sum()) < ref_v.numel() or model is not stand_in
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])     # both adapters fed the model the same arrays
    assert seen[0][0].shape == (2, 3, 256, 256, 3) and seen[0][0].min() >= -1 and seen[0][0].max() <= 1


def test_adapter_contract_without_the_reference():
    """tracker.py:72-108 spelled out: scaling by 256 / W and 256 / H, the (t, y, x) flip, the visibility rule, the division back."""
    frames, _ = synthetic_clip(T=2, H=24, W=40, seed=1)
    q = torch.tensor([[[1.0, 10.0, 6.0], [0.0, 39.0, 23.0]]])

    def model(video, query):
        assert video.shape == (1, 2, 256, 256, 3) and np.allclose(query[0, 0], [1.0, 6.0 * 256 / 24, 10.0 * 256 / 40])
        tracks = np.broadcast_to(query[:, :, None, 2:0:-1], (1, 2, 2, 2)).copy()
        return {"tracks": tracks, "occlusion": np.array([[[-3.0, 3.0], [0.0, -3.0]]], np.float32),
                "expected_dist": np.array([[[-3.0, -3.0], [2.0, 2.0]]], np.float32)}

    traj, vis = _cpu_tracker(model).forward(frames[None], q)
    assert torch.allclose(traj[0, 0], q[0, :, 1:], atol=1e-5) and torch.allclose(traj[0, 1], q[0, :, 1:], atol=1e-5)
    assert vis[0].tolist() == [[True, False], [False, True]]            # probabilities (frame, query): 0.907, 0.060; 0.045, 0.114


@needs_ref
def test_reference_yaml_builds_our_tracker():
    """`model/point_tracker=tapir model.point_tracker._target_=sam_pt_amd.point_tracker.TapirPointTracker`."""
    from sam_pt_amd.point_tracker import PointTracker, TapirPointTracker
    from tests import hydra_lite as H
    cfg = {"model": {"point_tracker": H.compose(os.path.join(R.REF, "configs"), "model/point_tracker", "tapir")}}
    H.apply_overrides(cfg, ["model.point_tracker._target_=sam_pt_amd.point_tracker.TapirPointTracker", "model.point_tracker.checkpoint_path=null"])
    trk = H.instantiate(H.resolve(cfg)["model"]["point_tracker"])
    assert type(trk) is TapirPointTracker and isinstance(trk, PointTracker) and trk.visibility_threshold == 0.1 and trk.checkpoint_path is None
    assert set(trk._sd) == set(init_tapir_state_dict(72)) and trk.iters == 4


def test_refusals_before_any_launch_carry_a_message():
    """A workspace that is too small is refused with a text in sampt_last_error; a null handle has launched nothing."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2 * 8 * 4)
    p = x.data_ptr()
    assert lib.sampt_instance_norm_workspace_bytes(2, 8, 4) > 16
    assert lib.sampt_instance_norm_affine_nhwc(p, p, p, p, None, 2, 8, 4, 1e-5, 1, p, 16, None) == -4
    assert b"sampt_instance_norm_affine_nhwc" in lib.sampt_last_error() and b"workspace" in lib.sampt_last_error()
    assert lib.sampt_instance_norm_affine_nhwc(None, p, p, p, None, 2, 8, 4, 1e-5, 1, p, 16, None) == -1
    assert lib.sampt_tapir_launches(None) == 0


def test_constructor_and_missing_library_paths(tmp_path, sd):
    from sam_pt_amd._lib import SamptError
    from sam_pt_amd.point_tracker import TapirPointTracker
    np.save(os.path.join(tmp_path, "ck.npy"), {"params": tapir_state_dict_to_haiku(sd), "state": {}}, allow_pickle=True)
    trk = TapirPointTracker(checkpoint_path=os.path.join(tmp_path, "ck.npy"), visibility_threshold=0.3)
    assert torch.equal(trk._sd["mixer.out.weight"], sd["mixer.out.weight"]) and trk.visibility_threshold == 0.3
    frames, _ = synthetic_clip(T=2, H=24, W=40, seed=1)
    with pytest.raises(SamptError):                                     # no CPU fallback: the model runs on the HIP device only
        trk(frames[None], torch.zeros(1, 1, 3))
