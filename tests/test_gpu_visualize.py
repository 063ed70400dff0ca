"""csrc/viz.hip against the host restatement of sam_pt_amd/visualize.py: every comparison is == on integers or bytes."""
import numpy as np
import pytest
import torch

from sam_pt_amd import visualize as V
from sam_pt_amd.vis_metrics import bits_pack_device, pack_bits
from tests.test_amg_tail_cpu import offset_view, seeded_masks
from tests.test_visualize_cpu import band_masks

pytestmark = pytest.mark.gpu

# 129 x 515: three bands and three column blocks; 66 x 520: a width that is a multiple of 4 (12-byte stores) over three column blocks
SHAPES = [(5, 3), (64, 4), (65, 7), (70, 261), (129, 515), (66, 520)]
RADII = (0, 1, 3, 7, 64)
T = 2


def words_i64(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64))


# --------------------------------------------------------------------------------------------------------------- band
@pytest.mark.parametrize("h,w", SHAPES)
def test_band_equals_the_host_for_every_source_and_radius(dev, h, w):
    masks = band_masks(h, w)                                           # empty, full, a corner pixel, checkerboard, three seeded
    n = masks.shape[0]
    m = torch.from_numpy(masks)
    rng = torch.Generator().manual_seed(h * 7 + w)
    logits = torch.where(m, torch.rand(m.shape, generator=rng) + 0.26, 0.25 - torch.rand(m.shape, generator=rng))
    clear = (~m).nonzero()
    logits[tuple(clear[0::3].T)] = float("nan")                        # NaN and at-threshold pixels among the clear ones
    logits[tuple(clear[1::3].T)] = 0.25
    other = torch.randint(0, 7, m.shape, generator=rng).to(torch.uint8)
    index = torch.where(m, torch.tensor(7, dtype=torch.uint8), other)
    sources = {"bytes": bits_pack_device(m.to(dev))[0],
               "logits": bits_pack_device(logits.to(dev), threshold=0.25)[0],
               "index": bits_pack_device(index.to(dev), values=[7] * n, planes=list(range(n)))[0]}
    words = pack_bits(masks)
    for bits in sources.values():
        assert torch.equal(bits.cpu(), words_i64(words))
    for r in RADII:
        want = words_i64(V.band_words(words, h, r))
        for name, bits in sources.items():
            got = V.contour_band_device(bits, h, r)
            assert torch.equal(got.cpu(), want), (name, r)
        if r == 0:
            assert not want.any()
        assert not want[0].any() and not want[1].any()                 # an empty and a full mask have no band
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ compose
def clip(h: int, w: int, n: int, seed: int):
    """Frames, masks (as bytes for 1 mask, logits with NaN for 3, an index map for 12), markers and query timesteps of one case."""
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, (T, 3, h, w), dtype=np.uint8))
    kw = {}
    if n == 12:                                                        # twelve disjoint objects of one index map (the colour clip)
        labels = torch.from_numpy(rng.integers(0, 14, (T, h // 4 + 1, w // 4 + 1), dtype=np.uint8))
        masks = labels.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w].contiguous()
        masks[:, ::3, ::5] = torch.from_numpy(rng.integers(0, 14, masks[:, ::3, ::5].shape, dtype=np.uint8))
        kw["values"] = list(range(1, 13))
    else:
        m = seeded_masks(n * T, h, w, seed=seed).reshape(n, T, h, w)
        if n == 3:
            g = torch.Generator().manual_seed(seed)
            masks = torch.where(m, torch.rand(m.shape, generator=g) + 0.01, -torch.rand(m.shape, generator=g))
            masks[(~m) & (torch.rand(m.shape, generator=g) < 0.1)] = float("nan")
            masks[(~m) & (torch.rand(m.shape, generator=g) < 0.1)] = 0.0
        else:
            masks = m
    P = 12
    tr = torch.from_numpy(rng.random((T, n, P, 2)) * [w + 20, h + 20] - 10).float()      # some off the frame
    fixed = torch.tensor([[255.0, 63.0], [256.9, 64.2], [255.0, 64.0], [256.0, 63.0],    # tile seams, on top of each other
                          [float("nan"), float("nan")], [-30.0, 1e9], [0.0, 0.0], [w - 1.0, h - 1.0]])
    tr[:, 0, :8] = fixed
    vis = torch.from_numpy(rng.integers(-4, 2, (T, n, P))).float()
    vis[0, 0, :6] = torch.tensor([1.0, 0.0, -1.0, -2.0, -3.0, -4.0])                     # every visibility code
    kw.update(positive_points_per_mask=6, query_timesteps=[1] + [0] * (n - 1))           # mask 0 is cleared on frame 0
    return frames, masks, tr, vis, kw


@pytest.mark.parametrize("n", [1, 3, 12])
@pytest.mark.parametrize("h,w", SHAPES)
def test_compose_equals_the_host_on_all_panels_and_layouts(dev, h, w, n):
    frames, masks, tr, vis, kw = clip(h, w, n, seed=h * 31 + w + n)
    want = V.render_predictions_host(frames, masks, tr, vis, panel="stacked", **kw)       # input above predictions, computed once
    assert want.shape == (T, 2 * h, w, 3)
    d = dict(images=frames.to(dev), masks=masks.to(dev), trajectories=tr.to(dev), visibilities=vis.to(dev))
    stacked = V.render_predictions(**d, panel="stacked", **kw)
    assert stacked.dtype == torch.uint8 and stacked.device.type == "cuda"
    assert torch.equal(stacked.cpu(), torch.from_numpy(want))
    assert torch.equal(V.render_predictions(**d, panel="input", **kw).cpu(), torch.from_numpy(want[:, :h]))
    assert torch.equal(V.render_predictions(**d, panel="predictions", **kw).cpu(), torch.from_numpy(want[:, h:]))
    # interleaved frames that start one byte into their storage: no row and no 4-pixel load is aligned
    d["images"] = offset_view(frames.permute(0, 2, 3, 1).contiguous(), dev)
    again = V.render_predictions(**d, panel="stacked", **kw)
    assert torch.equal(again, stacked)                                 # two calls, two layouts: equal bytes
    assert torch.equal(V.render_predictions(**d, panel="stacked", **kw), again)
    if n == 1:                                                         # the mask really is cleared on frame 0, and only there
        bare = dict(images=d["images"], masks=d["masks"], panel="predictions")
        cleared, kept = V.render_predictions(**bare, query_timesteps=[1]), V.render_predictions(**bare)
        assert torch.equal(cleared[1], kept[1]) and torch.equal(cleared[0], kept[0]) == (not bool(masks[0, 0].any()))


def test_no_masks_no_markers_and_wide_markers(dev):
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (T, 3, 70, 261), dtype=np.uint8))
    out = V.render_predictions(frames.to(dev))
    assert torch.equal(out.cpu(), frames.permute(0, 2, 3, 1))
    # 70 markers per frame (more than one wave's worth), large and thick ones across all tiles
    tr = torch.from_numpy(rng.random((T, 2, 35, 2)) * [261, 70]).float()
    vis = torch.ones(T, 2, 35)
    for size, width in ((8, 4), (40, 9), (0, 0), (3, 1)):
        kw = dict(positive_points_per_mask=20, annot_size=size, annot_line_width=width, panel="input")
        want = V.render_predictions_host(frames, None, tr, vis, **kw)
        assert torch.equal(V.render_predictions(frames.to(dev), None, tr.to(dev), vis.to(dev), **kw).cpu(), torch.from_numpy(want))


# --------------------------------------------------------------------------------------------------------- end to end
def test_render_outputs_of_a_sampt_forward_equals_the_host(dev):
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict
    from tests.util import disc_queries, synthetic_clip
    frames, centres = synthetic_clip(T=9, H=128, W=256, seed=72)
    q = disc_queries(centres, n_pos=4, r=9.0)
    video = {"image": [f.to(dev) for f in frames], "target_hw": (128, 256), "query_points": q[None]}
    pred = SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32").to(dev))
    model = SamPt(PipsPointTracker(state_dict=init_pips_state_dict(72)), pred, sam_iou_threshold=-1e9, positive_points_per_mask=4,
                  negative_points_per_mask=0, iterative_refinement_iterations=1).eval()
    out = model(video)
    got = V.render_outputs(video, out, positive_points_per_mask=4, panel="stacked")
    assert got.device.type == "cuda" and got.shape == (9, 256, 256, 3)
    host_video = {**video, "image": [f for f in frames]}
    host_out = {"logits": [m.cpu() for m in out["logits"]], "trajectories": out["trajectories"].cpu(), "visibilities": out["visibilities"].cpu()}
    want = V.render_outputs(host_video, host_out, positive_points_per_mask=4, panel="stacked")
    assert isinstance(want, np.ndarray) and torch.equal(got.cpu(), torch.from_numpy(want))
    assert not torch.equal(got[:, 128:].cpu(), frames.permute(0, 2, 3, 1))           # something was drawn
    listed = V.visualize_predictions(torch.stack(video["image"]), 0, q[None], out["trajectories"], out["visibilities"], None, torch.ones(1),
                                     torch.stack(out["logits"]), positive_points_per_mask=4)
    assert (np.stack(listed) == want[:, 128:]).all()
