"""TapNet on the CPU: what of the restatement (tests/tapnet_ref.py) can be pinned, the golden file, the checkpoint loader and the adapter.

PARITY UNPINNED for the model itself: the reference needs JAX, Haiku and a checkpoint, none of which exists where this project is
built.  Pinned here: the trilinear 'nearest' read against scipy.ndimage.map_coordinates; the max-pool against ``F.max_pool2d`` on a
-inf-padded input; the temporal shift against an index-by-index loop; the folded BatchNorm against the unfolded formula in float64;
``convert_grid_coordinates`` against the reference's NumPy-only utils/transforms.py; and the adapter against the reference's own
``TapnetPointTracker.forward`` (tapnet/tracker.py:67-103) run in place over small stand-in modules, with ``==``."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import (init_tapnet_state_dict, load_tapnet_checkpoint, tapnet_haiku_key_map, tapnet_state_dict_to_haiku)
from tests import tapnet_ref as R
from tests.util import max_abs, synthetic_clip

needs_ref = pytest.mark.skipif(not R.available(), reason="reference tree not present (GPU box)")


@pytest.fixture(scope="module")
def sd():
    return init_tapnet_state_dict(72)


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in R.golden().items()}


@pytest.fixture(scope="module")
def fresh(gold, sd):
    frames01 = F.interpolate(gold["frames"] / 255, (256, 256), mode="bilinear", align_corners=False, antialias=True)
    video = (frames01 * 2 - 1).permute(0, 2, 3, 1)
    return video, R.forward(sd, video, gold["video_q"], stages=True)


# ---------------------------------------------------------------------------------------------- pins
def test_trilinear_read_against_scipy():
    """map_coordinates(order=1, mode='nearest') over (T, H, W), coordinates inside, outside every face and at a fractional t."""
    from scipy.ndimage import map_coordinates
    g = torch.Generator().manual_seed(1)
    T, H, W, C = 4, 6, 9, 3
    grid = torch.randn(T, H, W, C, generator=g, dtype=torch.float64)
    tyx = torch.rand(500, 3, generator=g, dtype=torch.float64) * torch.tensor([T + 3.0, H + 4.0, W + 4.0]) - torch.tensor([2.0, 2.5, 2.5])
    tyx = torch.cat([tyx, torch.tensor([[0.0, 0.0, 0.0], [T - 1.0, H - 1.0, W - 1.0], [1.5, 2.25, 3.0], [-1.0, -0.5, -0.5], [T * 1.0, H - 0.5, W - 0.5],
                                        [0.5, -3.0, 4.0], [2.75, 2.0, W + 2.0]], dtype=torch.float64)])
    want = np.stack([map_coordinates(grid[..., c].numpy(), tyx.t().numpy(), order=1, mode="nearest") for c in range(C)], -1)
    assert np.allclose(R.trilinear_nearest(grid, tyx).numpy(), want, rtol=0, atol=1e-12)
    t = tyx[:, 0].numpy()
    assert ((t < 0).sum() > 20) and ((t > T - 1).sum() > 20) and ((np.abs(t - np.round(t)) > 0.1).sum() > 100)
    # the model's call: the half pixel comes off y and x only, t is a frame coordinate and is not rounded
    grid2 = torch.randn(5, 32, 32, 2, generator=g, dtype=torch.float64)
    q = torch.tensor([[1.25, 100.0, 36.0], [4.0, 256.0, 0.0]], dtype=torch.float64)
    want2 = np.stack([map_coordinates(grid2[..., c].numpy(), np.stack([q[:, 0], q[:, 1] / 8 - 0.5, q[:, 2] / 8 - 0.5]).astype(np.float64),
                                      order=1, mode="nearest") for c in range(2)], -1)
    assert np.allclose(R.query_features(grid2, q).numpy(), want2, rtol=0, atol=1e-12)


@pytest.mark.parametrize("side", [12, 13, 128])
def test_max_pool_against_a_minus_infinity_padded_pool(side):
    """TensorFlow 'SAME' at 3 x 3 stride 2: nothing before and one after on an even side, one and one on an odd side; all values are
    negative, so a padding that took part as zero would win."""
    g = torch.Generator().manual_seed(side)
    x = -torch.rand(2, 3, side, side + 1, generator=g) - 0.5
    pads = []
    for n in (side + 1, side):                          # F.pad order: (left, right, top, bottom)
        total = max((-(-n // 2) - 1) * 2 + 3 - n, 0)
        pads += [total // 2, total - total // 2]
    assert pads[2:] == ([0, 1] if side % 2 == 0 else [1, 1])
    want = F.max_pool2d(F.pad(x, pads, value=float("-inf")), 3, 2)
    got = R.max_pool_same(x)
    assert got.shape == (2, 3, -(-side // 2), -(-(side + 1) // 2)) and torch.equal(got, want) and float(got.max()) < 0


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("C", [64, 128])
def test_temporal_shift_against_an_index_loop(T, C):
    g = torch.Generator().manual_seed(T * C)
    x = torch.randn(T, 2, 3, C, generator=g)
    n = int(C * 0.125)
    assert n == {64: 8, 128: 16}[C]
    want = torch.zeros_like(x)
    for t in range(T):
        for c in range(C):
            if c < n:
                if t + 1 < T:
                    want[t, ..., c] = x[t + 1, ..., C - n + c]
            elif c >= C - n:
                if t - 1 >= 0:
                    want[t, ..., c] = x[t - 1, ..., c - (C - n)]
            else:
                want[t, ..., c] = x[t, ..., c]
    got = R.temporal_shift(x, 0.125)
    assert torch.equal(got, want)
    assert torch.equal(R.temporal_shift(x, 0.0), x)
    if T == 1:
        assert not got[..., :n].any() and not got[..., C - n:].any()


def test_folded_batchnorm_against_the_unfolded_formula(sd):
    """hk.BatchNorm(is_training=False): (x - mean) * rsqrt(var + eps) * scale + offset with the moving statistics, in float64; the
    packer folds the same way."""
    from sam_pt_amd.pack import fold_batchnorm_affine, pack_tapnet
    s64 = R.cast(sd, torch.float64)
    g = torch.Generator().manual_seed(2)
    for bn, C in (("tsm.u0.b0.bn0", 64), ("tsm.u1.b0.bn1", 128), ("tsm.u2.b1.bn0", 256)):
        x = torch.randn(3, 4, 5, C, generator=g, dtype=torch.float64) * 2
        want = F.relu((x - s64[bn + ".mean"]) * torch.rsqrt(s64[bn + ".var"] + 1e-5) * s64[bn + ".scale"] + s64[bn + ".offset"])
        assert max_abs(R.preact(s64, bn, x), want) < 1e-14
        assert float((s64[bn + ".mean"]).abs().max()) > 0.1 and float((s64[bn + ".var"] - 1).abs().max()) > 0.1       # the fold is exercised
        a, b = R.fold_batchnorm(sd, bn)
        a2, b2 = fold_batchnorm_affine(sd, bn)
        assert torch.equal(a, a2) and torch.equal(b, b2)
    w = pack_tapnet(sd, "cpu")
    assert torch.equal(w["tsm.u1.b0.bn1.a"], R.fold_batchnorm(sd, "tsm.u1.b0.bn1")[0]) and "tsm.u1.b0.bn1.mean" not in w


@needs_ref
def test_convert_grid_coordinates_equals_the_reference():
    ref = R.load_transforms().convert_grid_coordinates
    g = np.random.default_rng(0)
    xy = g.uniform(-20, 300, (7, 5, 2))
    for a, b in (((32, 32), (256, 256)), ((256, 256), (32, 32))):
        assert np.array_equal(R.convert_grid_coordinates(torch.from_numpy(xy), a, b).numpy(), ref(xy, a, b))
    tyx = g.uniform(0, 200, (9, 3))
    for T in (1, 5, 24):
        want = ref(tyx, (T, 256, 256), (T, 32, 32), coordinate_format="tyx")
        assert np.array_equal(R.convert_grid_coordinates(torch.from_numpy(tyx), (T, 256, 256), (T, 32, 32)).numpy(), want)


# ---------------------------------------------------------------------------------------------- the restatement and its golden
def test_f32_against_f64(gold, sd, fresh):
    video, o32 = fresh
    o64 = R.forward(sd, video, gold["video_q"], dtype=torch.float64)
    assert max_abs(o32["tracks"], o64["tracks"].float()) <= float(gold["floor_px"]) * 1.0001
    assert max_abs(o32["occlusion"], o64["occlusion"].float()) <= float(gold["floor_logit"]) * 1.0001
    assert float(gold["bar_px"]) == 8 * float(gold["floor_px"]) and float(gold["bar_logit"]) == 8 * float(gold["floor_logit"])
    assert float(gold["min_gap"]) > 4 * max(float(gold["bar_logit"]), 8 * float(gold["floor_heat"]))
    assert float(gold["min_margin"]) > 4 * float(gold["bar_logit"])


def test_golden_equals_a_fresh_run(gold, fresh):
    _, o = fresh
    bar_px, bar_logit = float(gold["bar_px"]), float(gold["bar_logit"])
    assert max_abs(o["tracks"], gold["tracks"]) < bar_px and max_abs(o["occlusion"], gold["occlusion"]) < bar_logit
    rows = gold["map_rows"].long()
    low = rows[rows < 1024]
    for k, r, c in (("stem", rows, 64), ("unit0", rows, 64), ("unit1", low, 128), ("unit2", low, 256), ("grid", low, 256)):
        assert max_abs(o[k].reshape(5, -1, c)[:, r], gold[k + "_rows"]) < 1e-5, k
    top = o["logits"].reshape(6, 5, -1).topk(2, -1)
    assert max_abs(o["qf"], gold["qf"]) < 1e-5 and max_abs(top.values, gold["logits_top2"]) < 1e-4
    assert torch.equal(top.indices[..., 0].int(), gold["logits_best"])
    vis = R.visibility_probability(o["occlusion"]).t() > float(gold["threshold"])
    assert torch.equal(vis, gold["visibilities"]) and 0 < int(vis.sum()) < vis.numel()
    q = gold["video_q"]
    assert sorted(q[:, 0].tolist()) == [0, 1, 2, 2, 3, 4] and tuple(gold["frames"].shape) == (5, 3, 96, 128)
    for i in range(6):                                             # the query point verbatim on its own frame
        assert torch.equal(o["tracks"][i, int(q[i, 0])], q[i, [2, 1]])
    assert os.path.getsize(R.GOLDEN) < 300 * 1024


def test_the_shift_and_the_projection_matter(sd, fresh):
    """The restated backbone really shifts (a frame's features depend on its neighbours) and T = 1 sees zeros on both sides."""
    video, o = fresh
    with torch.no_grad():
        alone = R.backbone(sd, video[2:3])
        swapped = R.backbone(sd, video[[0, 1, 2, 4, 3]])
    assert max_abs(alone["unit0"][0], o["unit0"][2]) > 1e-3 and max_abs(alone["stem"][0], o["stem"][2]) == 0
    assert max_abs(swapped["grid"][2], o["grid"][2]) > 1e-4 and max_abs(swapped["grid"][0], o["grid"][0]) > 0


# ---------------------------------------------------------------------------------------------- checkpoint loader
def test_checkpoint_round_trip(tmp_path, sd):
    ck = tapnet_state_dict_to_haiku(sd)
    params, state = ck["params"], ck["state"]
    r = "tap_net/~/tsm_resnet_video/"
    assert params[r + "tsm_resnet_stem"]["w"].shape == (7, 7, 3, 64)
    assert params[r + "tsm_resnet_unit_1/block_0/conv_0"]["w"].shape == (3, 3, 64, 128)
    assert params[r + "tsm_resnet_unit_1/block_0/shortcut_conv"]["w"].shape == (1, 1, 64, 128)
    assert params[r + "tsm_resnet_unit_2/block_1/batch_norm_1"]["scale"].shape == (1, 1, 1, 256)
    assert state[r + "tsm_resnet_unit_0/block_0/batch_norm/~/mean_ema"]["average"].shape == (1, 1, 1, 64)
    assert params["tap_net/~/cost_volume_occlusion_1"]["w"].shape == (1, 3, 3, 16, 32) and params["tap_net/~/occlusion_out"]["w"].shape == (16, 1)
    # modules and entries the forward pass never uses
    params["tap_net/~/regression_hid"] = {"w": np.zeros((3, 128), np.float32), "b": np.zeros(128, np.float32)}
    params["tap_net/~/regression_out"] = {"w": np.zeros((128, 2), np.float32), "b": np.zeros(2, np.float32)}
    params[r + "tsm_resnet_unit_3/block_0/conv_0"] = {"w": np.zeros((3, 3, 256, 512), np.float32)}
    state[r + "tsm_resnet_unit_0/block_0/batch_norm/~/mean_ema"]["hidden"] = np.zeros((1, 1, 1, 64), np.float32)
    state[r + "tsm_resnet_unit_0/block_0/batch_norm/~/mean_ema"]["counter"] = np.zeros((), np.int32)
    path = os.path.join(tmp_path, "checkpoint_wo_optstate.npy")
    np.save(path, {"params": params, "state": state}, allow_pickle=True)
    back = load_tapnet_checkpoint(path)
    assert list(back) == list(tapnet_haiku_key_map()) and set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    del state[r + "tsm_resnet_unit_1/block_1/batch_norm_1/~/var_ema"]
    np.save(path, {"params": params, "state": state}, allow_pickle=True)
    with pytest.raises(KeyError, match="unit_1/block_1/batch_norm_1/~/var_ema"):
        load_tapnet_checkpoint(path)


def test_pack_layouts(sd):
    from sam_pt_amd.pack import pack_tapnet
    w = pack_tapnet(sd, "cpu")
    assert w["tsm.stem.weight"].shape == (64, 7 * 7 * 4) and "tsm.stem.weight_hl" not in w
    assert w["tsm.u1.b0.conv0.weight"].shape == (128, 9 * 64) and w["tsm.u1.b0.conv0.weight_hl"].shape == (2, 128, 9 * 64)
    assert w["tsm.u2.b0.shortcut.weight_hl"].dtype == torch.float16 and w["tsm.u2.b0.shortcut.weight"].shape == (256, 128)
    assert torch.equal(w["heads.hid3.weight"][5, 7], sd["heads.hid3.weight"][:, 5, 2, 1])
    assert w["heads.occ_out.weight"].shape == (1, 16) and w["tsm.u0.b1.bn0.a"].shape == (64,)
    assert not any(k.endswith((".mean", ".var", ".scale", ".offset")) for k in w)


# ---------------------------------------------------------------------------------------------- adapter and constructor
def _cpu_tracker(model, **kw):
    """Our tracker with the device model replaced by ``model`` (the reference's ``jitted_forward`` signature)."""
    from sam_pt_amd.point_tracker import TapnetPointTracker
    trk = TapnetPointTracker(state_dict={}, **kw)

    def run(frames01, q_tyx):
        video = (frames01.cpu().numpy() * 2 - 1).transpose(0, 1, 3, 4, 2)
        return {k: torch.from_numpy(np.asarray(v).copy()) for k, v in model(video, q_tyx.numpy()).items()}

    trk._model = run
    return trk


@needs_ref
def test_adapter_equals_the_reference_adapter(sd):
    """Non-square frames, B = 1 and B = 2: the same model behind the reference's forward and behind ours -> identical trajectories and
    visibilities.  Once with a cheap stand-in model whose outputs straddle the threshold, once with the restated model."""
    frames, _ = synthetic_clip(T=3, H=40, W=56, seed=3)
    both = torch.stack([frames, frames.flip(0)])
    g = torch.Generator().manual_seed(4)
    q2 = torch.stack([torch.randint(0, 3, (2, 5), generator=g).float(), torch.rand(2, 5, generator=g) * 56, torch.rand(2, 5, generator=g) * 40], -1)
    seen = []

    def stand_in(video, query):
        seen.append((np.asarray(video).copy(), np.asarray(query).copy()))
        B, T, N = video.shape[0], video.shape[1], query.shape[1]
        r = np.random.default_rng(5)
        tracks = query[:, :, None, 2:0:-1] + r.normal(0, 3, (B, N, T, 2)).astype(np.float32) + video.mean((2, 3, 4))[:, None, :, None]
        return {"tracks": tracks.astype(np.float32), "occlusion": r.normal(0, 2, (B, N, T)).astype(np.float32)}

    for rgbs, q in ((both, q2), (both[:1], q2[:1])):
        for model in (stand_in, R.model_fn(sd)):
            ref_t, ref_v = R.reference_tracker(model, 0.5).forward(rgbs, q)
            our_t, our_v = _cpu_tracker(model, visibility_threshold=0.5).forward(rgbs, q)
            B = rgbs.shape[0]
            assert ref_t.shape == (B, 3, 5, 2) and ref_v.shape == (B, 3, 5) and ref_v.dtype == torch.bool
            assert torch.equal(our_t, ref_t) and torch.equal(our_v, ref_v)
            assert 0 < int(ref_v.sum()) < ref_v.numel() or model is not stand_in
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])     # both adapters fed the model the same arrays
    assert seen[0][0].shape == (2, 3, 256, 256, 3) and seen[0][0].min() >= -1 and seen[0][0].max() <= 1


def test_adapter_contract_without_the_reference():
    """tracker.py:67-103 spelled out: scaling by 256 / W and 256 / H, the (t, y, x) flip, the visibility rule, the division back."""
    frames, _ = synthetic_clip(T=2, H=24, W=40, seed=1)
    q = torch.tensor([[[1.0, 10.0, 6.0], [0.0, 39.0, 23.0]]])

    def model(video, query):
        assert video.shape == (1, 2, 256, 256, 3) and np.allclose(query[0, 0], [1.0, 6.0 * 256 / 24, 10.0 * 256 / 40])
        tracks = np.broadcast_to(query[:, :, None, 2:0:-1], (1, 2, 2, 2)).copy()
        return {"tracks": tracks, "occlusion": np.array([[[-3.0, 3.0], [0.5, -0.5]]], np.float32)}

    traj, vis = _cpu_tracker(model).forward(frames[None], q)
    assert torch.allclose(traj[0, 0], q[0, :, 1:], atol=1e-5) and torch.allclose(traj[0, 1], q[0, :, 1:], atol=1e-5)
    assert vis[0].tolist() == [[True, False], [False, True]]            # 1 - sigmoid: (frame, query) 0.953, 0.378; 0.047, 0.622
    assert _cpu_tracker(model, visibility_threshold=0.3).forward(frames[None], q)[1][0].tolist() == [[True, True], [False, True]]


@needs_ref
def test_reference_yaml_builds_our_tracker():
    """`model/point_tracker=tapnet model.point_tracker._target_=sam_pt_amd.point_tracker.TapnetPointTracker`."""
    from sam_pt_amd.point_tracker import PointTracker, TapnetPointTracker
    from tests import hydra_lite as H
    cfg = {"model": {"point_tracker": H.compose(os.path.join(R.REF, "configs"), "model/point_tracker", "tapnet")}}
    H.apply_overrides(cfg, ["model.point_tracker._target_=sam_pt_amd.point_tracker.TapnetPointTracker", "model.point_tracker.checkpoint_path=null"])
    trk = H.instantiate(H.resolve(cfg)["model"]["point_tracker"])
    assert type(trk) is TapnetPointTracker and isinstance(trk, PointTracker) and trk.visibility_threshold == 0.5 and trk.checkpoint_path is None
    assert set(trk._sd) == set(init_tapnet_state_dict(72))


def test_refusals_before_any_launch():
    """Null pointers and bad counts are refused with a text in sampt_last_error; a null handle has launched nothing."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64)
    p = x.data_ptr()
    assert lib.sampt_tapnet_bn_shift_f32(p, p, p, 1, 1, 8, 6, p, None, None, None, None) == -1
    assert b"sampt_tapnet_bn_shift_f32" in lib.sampt_last_error()
    assert lib.sampt_tapnet_maxpool_nhwc(p, p, 1, 2, 2, 6, None) == -1 and b"sampt_tapnet_maxpool_nhwc" in lib.sampt_last_error()
    assert lib.sampt_tapnet_query_feats_f32(p, 0, p, 1, p, None) == -1
    assert lib.sampt_tapnet_heads_f32(p, 1, p, p, 1, None, p, p, None) == -1
    assert lib.sampt_tapnet_track_f32(None, p, 1, p, 1, p, p, p, 64, None) == -1
    assert lib.sampt_tapnet_set_stem_chunk(None, 2) == -1
    assert lib.sampt_tapnet_launches(None) == 0


def test_constructor_and_missing_library_paths(tmp_path, sd):
    from sam_pt_amd._lib import SamptError
    from sam_pt_amd.point_tracker import TapnetPointTracker
    np.save(os.path.join(tmp_path, "ck.npy"), tapnet_state_dict_to_haiku(sd), allow_pickle=True)
    trk = TapnetPointTracker(checkpoint_path=os.path.join(tmp_path, "ck.npy"), visibility_threshold=0.3)
    assert torch.equal(trk._sd["tsm.u2.b1.conv2.weight"], sd["tsm.u2.b1.conv2.weight"]) and trk.visibility_threshold == 0.3
    frames, _ = synthetic_clip(T=2, H=24, W=40, seed=1)
    with pytest.raises(SamptError):                                     # no CPU fallback: the model runs on the HIP device only
        trk(frames[None], torch.zeros(1, 1, 3))
