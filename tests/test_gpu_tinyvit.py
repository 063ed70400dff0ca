"""TinyViT image encoder (MobileSAM / Light HQ-SAM) on the device (csrc/tinyvit.hip, csrc/engine_tinyvit.hip) against the
restatement of tests/tinyvit_ref.py, run live on the CPU, and against tests/golden/tinyvit_ref.npz recorded from it.  PARITY
UNPINNED: upstream's tiny_vit_sam.py and its checkpoints do not exist where this project is built.

Bars.  The preprocess kernel is exact (``==`` the torch expression).  Single kernels with sums — the depthwise convolution, the
window attention — are held to the project's fp32 grade, 2e-5 x max |reference| (tests/test_gpu_raft.py).  Every stage of the
encoder, the embedding, the HQ tap and the low-resolution logits are held to the bars read from the golden file: 8 x the
restatement's own arithmetic noise at the test shape (f32 against float64, f32 against 1e-7-perturbed weights), measured on the
CPU by tools/make_tinyvit_golden.py — never taken from the device path.  Masks: IoU >= 1 - 1e-5 against the golden, the project's
bar for its fp32-grade modes.  Batch invariance and the fused clip path against the per-frame path are bitwise."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd.weights import init_pips_state_dict, init_sam_state_dict
from tests import tinyvit_ref as R
from tests.util import disc_queries, iou, max_abs, synthetic_clip

pytestmark = pytest.mark.gpu
FP32_GRADE = 2e-5


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def stream():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in R.load_golden().items()}


@pytest.fixture(scope="module")
def inputs():
    """(cfg, sd with the HQ extras, frames uint8 (2,3,144,256), points, labels) of the golden file."""
    from tools.make_tinyvit_golden import golden_inputs
    return golden_inputs()


@pytest.fixture(scope="module")
def restated(inputs):
    """The restatement on the golden frames in f32, computed once, with its stages."""
    cfg, sd, frames, _, _ = inputs
    return R.run(cfg, sd, frames)


def predictor(inputs, dev, hq, **kw):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    cfg, sd = inputs[0], inputs[1]
    if not hq:
        sd = {k: v for k, v in sd.items() if k in init_sam_state_dict(cfg, 72)}
    return SamPredictor(SamHip(config=cfg, state_dict=sd, **kw).to(dev))


@pytest.fixture(scope="module")
def pred_sam(inputs, dev):
    return predictor(inputs, dev, False)


@pytest.fixture(scope="module")
def pred_hq(inputs, dev):
    return predictor(inputs, dev, True)


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 7, 160), (1, 9, 6, 256), (1, 1, 1, 32)])
def test_depthwise_kernel(lib, dev, shape, stride, gelu):
    n, H, W, Cc = shape
    g = torch.Generator().manual_seed(H * 100 + W + stride)
    x, w, b = torch.randn(n, H, W, Cc, generator=g), torch.randn(3, 3, Cc, generator=g) / 3, torch.randn(Cc, generator=g)
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(2, 0, 1)[:, None].double(), b.double(), stride, 1, 1, Cc)
    want = (F.gelu(want) if gelu else want).permute(0, 2, 3, 1)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert tuple(want.shape) == (n, OH, OW, Cc)
    out = torch.full((n, OH, OW, Cc), float("nan"), device=dev)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    rc = lib.sampt_tinyvit_dwconv3x3_nhwc(P(xd), P(wd), P(bd), P(out), n, H, W, Cc, stride, gelu, stream())
    torch.cuda.synchronize()
    assert rc == 0 and not torch.isnan(out).any()
    err, tol = max_abs(out, want), FP32_GRADE * float(want.abs().max())
    print(f"depthwise {shape} stride {stride} gelu {gelu}: max |err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol


def literal_window_attention(qkv, table, pad_qkv, heads, ws):
    """F.pad of the qkv map with the pad row -> partition -> attention over all ws^2 positions -> reverse -> crop, in float64."""
    B, H, W, C3 = qkv.shape
    Cc = C3 // 3
    pb, pr = (ws - H % ws) % ws, (ws - W % ws) % ws
    full = pad_qkv.view(1, 1, 1, C3).expand(B, H + pb, W + pr, C3).clone()
    full[:, :H, :W] = qkv
    nH, nW = (H + pb) // ws, (W + pr) // ws
    t = full.view(B, nH, ws, nW, ws, C3).transpose(2, 3).reshape(B * nH * nW, ws * ws, heads, 96)
    q, k, v = (t[..., i * 32:(i + 1) * 32].permute(0, 2, 1, 3) for i in range(3))
    idx = R.first_appearance_index(ws)
    a = ((q @ k.transpose(-2, -1)) * 32 ** -0.5 + table[:, idx]).softmax(-1) @ v
    o = a.transpose(1, 2).reshape(B, nH, nW, ws, ws, Cc).transpose(2, 3).reshape(B, H + pb, W + pr, Cc)
    return o[:, :H, :W]


@pytest.mark.parametrize("case", [(2, 7, 7, 7, 2), (1, 16, 16, 14, 5), (2, 9, 10, 7, 2), (1, 8, 8, 14, 3)])
def test_window_attention_kernel(lib, dev, case):
    """(the last case has one window that is two-thirds padding: wrong handling of padded keys shows there)"""
    B, H, W, ws, heads = case
    g = torch.Generator().manual_seed(sum(case))
    Cc = 32 * heads
    qkv, pad = torch.randn(B, H, W, 3 * Cc, generator=g) * 1.5, torch.randn(3 * Cc, generator=g) * 1.5
    table = torch.randn(heads, ws * ws, generator=g) * 0.5
    want = literal_window_attention(qkv.double(), table.double(), pad.double(), heads, ws)
    out = torch.full((B, H, W, Cc), float("nan"), device=dev)
    qd, td, pd = qkv.to(dev), table.to(dev), pad.to(dev)
    rc = lib.sampt_tinyvit_window_attention_f32(P(qd), P(td), P(pd), P(out), B, H, W, heads, ws, stream())
    torch.cuda.synchronize()
    assert rc == 0 and not torch.isnan(out).any(), "every real position is written"
    err, tol = max_abs(out, want), FP32_GRADE * float(want.abs().max())
    print(f"window attention {case}: max |err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("chw", [1, 0])
def test_preprocess_kernel_is_exact(lib, dev, inputs, chw):
    cfg, _, frames, _, _ = inputs
    B, _, H, W = frames.shape
    mean, std = torch.tensor(cfg.pixel_mean), torch.tensor(cfg.pixel_std)
    want = F.pad((frames.float() - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1), (0, cfg.img_size - W, 0, cfg.img_size - H))
    want = F.pad(want.permute(0, 2, 3, 1), (0, 1))                                  # NHWC, 4th channel zero
    src = (frames if chw else frames.permute(0, 2, 3, 1)).contiguous().to(dev)
    out = torch.full((B, cfg.img_size, cfg.img_size, 4), float("nan"), device=dev)
    m3, s3 = (C.c_float * 3)(*cfg.pixel_mean), (C.c_float * 3)(*cfg.pixel_std)
    rc = lib.sampt_tinyvit_preprocess(P(src), chw, B, H, W, cfg.img_size, m3, s3, P(out), stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def device_stages(lib, dev, inputs, pred_hq):
    """The engine on the two golden frames in ONE call: its stages, the embedding and the HQ tap, on the CPU."""
    from sam_pt_amd import _lib
    cfg, _, frames, _, _ = inputs
    pred_hq._ensure()
    B, g, r = frames.shape[0], cfg.grid, cfg.resolutions
    dims = cfg.embed_dims
    shapes = [(B, r[0], r[0], dims[0]), (B, r[1] ** 2, dims[1]), (B, r[2] ** 2, dims[2]), (B, r[3] ** 2, dims[3]), (B, r[3] ** 2, dims[3])]
    st = [torch.full(s, float("nan"), device=dev) for s in shapes]
    emb = torch.full((B, g * g, cfg.out_chans), float("nan"), device=dev)
    interm = torch.full((B, g * g, dims[2]), float("nan"), device=dev)
    ws = _lib.workspace("sampt_tinyvit_encode_workspace_bytes", dev, pred_hq._vit, B)
    ms = (C.c_float * 6)()
    fd = frames.to(dev)
    _lib.check(lib.sampt_tinyvit_encode_stages(pred_hq._vit, P(fd), 1, B, frames.shape[2], frames.shape[3], P(emb), P(interm),
                                               _lib.ptr_array(st), ms, P(ws), ws.numel(), stream()), "sampt_tinyvit_encode_stages")
    torch.cuda.synchronize()
    out = {n: t.cpu() for n, t in zip(R.STAGES[:5], st)}
    out["neck"], out["interm"], out["stage_ms"] = emb.cpu(), interm.cpu(), list(ms)
    return out


@pytest.mark.parametrize("stage", R.STAGES)
def test_every_stage_within_its_bar(gold, restated, device_stages, stage):
    want = restated[stage]
    if want.dim() == 4:                                                              # NCHW maps of the restatement -> NHWC
        want = want.permute(0, 2, 3, 1)
    got = device_stages[stage].reshape(want.shape)
    assert not torch.isnan(got).any()
    err, bar = max_abs(got, want), float(gold["bar_" + stage])
    print(f"stage {stage}: max |err| {err:.3e} (bar {bar:.3e}, restatement's noise {float(gold['floor_' + stage].max()):.3e}, max |x| {float(want.abs().max()):.3f})")
    assert err <= bar


def test_embedding_and_hq_tap_within_their_bars(gold, inputs, restated, device_stages):
    cfg = inputs[0]
    g2 = cfg.grid ** 2
    emb_want = restated["neck"].permute(0, 2, 3, 1).reshape(2, g2, -1)
    e_emb, e_int = max_abs(device_stages["neck"], emb_want), max_abs(device_stages["interm"], restated["interm"].reshape(2, g2, -1))
    idx = gold["emb_idx"].long()
    g_emb, g_int = max_abs(device_stages["neck"][:, idx], gold["emb_rows"]), max_abs(device_stages["interm"][:, idx], gold["interm_rows"])
    print(f"embedding: max |err| {e_emb:.3e} vs the restatement, {g_emb:.3e} vs the golden rows (bar {float(gold['bar_emb']):.3e}); "
          f"HQ tap: {e_int:.3e}, {g_int:.3e} (bar {float(gold['bar_interm']):.3e})")
    assert max(e_emb, g_emb) <= float(gold["bar_emb"]) and max(e_int, g_int) <= float(gold["bar_interm"])


def test_batch_invariance_is_bitwise(dev, inputs, pred_hq):
    frames = inputs[2].to(dev)
    both = pred_hq.encode_frames(frames, chw=True)
    one = [pred_hq.encode_frames(frames[i:i + 1], chw=True) for i in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(both.emb[i], one[i].emb[0]) and torch.equal(both.hq[i], one[i].hq[0])


@pytest.mark.parametrize("hq", [False, True])
def test_set_image_and_predict_torch(gold, dev, inputs, pred_sam, pred_hq, hq):
    pred, name = (pred_hq, "hq") if hq else (pred_sam, "sam")
    _, _, frames, pts, labels = inputs
    for i in range(2):
        pred.set_image(frames[i].permute(1, 2, 0).numpy())
        logits, _, low = pred.predict_torch(pts[i:i + 1].to(dev), labels[i:i + 1].to(dev), multimask_output=False, return_logits=True)
        torch.cuda.synchronize()
        err, bar = max_abs(low[0, 0], gold["low_" + name][i]), float(gold["bar_logit"])
        miou = iou(logits[0, 0] > 0, gold["mask_" + name][i])
        print(f"{name} frame {i}: low-res logits max |err| {err:.3e} (bar {bar:.3e}), mask IoU {miou:.7f}")
        assert err <= bar and miou >= 1 - 1e-5
    if hq:
        idx = gold["hq_idx"].long()
        e = max_abs(pred._hq_tokens[idx], gold["hq_rows"][1])
        print(f"HQ features: max |err| {e:.3e} (bar {float(gold['bar_hq']):.3e})")
        assert e <= float(gold["bar_hq"])


@pytest.fixture(scope="module")
def clip_and_per_frame(dev, pred_sam):
    """One SamPt.forward (fused clip path: batched encoder, device-side decode chain) on a 4-frame clip, and the same predictor
    driven frame by frame through set_image / predict_torch with the same points: (fused logits, per-frame logits, per-frame
    embeddings against the clip's), all on the CPU."""
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_pt import SamPt
    frames, centres = synthetic_clip(T=4, H=144, W=256, seed=72)
    q = disc_queries(centres, n_pos=4, r=9.0)[None]
    model = SamPt(PipsPointTracker(state_dict=init_pips_state_dict(72)), pred_sam, sam_iou_threshold=-1e9, positive_points_per_mask=4,
                  negative_points_per_mask=0, iterative_refinement_iterations=0).eval()
    out = model({"image": [f.to(dev) for f in frames], "target_hw": (144, 256), "query_points": q})
    torch.cuda.synchronize()
    traj, vis, fused = out["trajectories"].cpu(), out["visibilities"].cpu(), out["logits"][0].cpu()
    assert tuple(fused.shape) == (4, 144, 256) and bool((vis[:, 0] == 1).any(dim=1).all()), "every frame needs a visible point for this comparison"
    feats = pred_sam.encode_frames(frames.to(dev), chw=True)
    single, emb_equal = [], []
    for t in range(4):
        c, l = model._prepare_points(traj, vis, t, 0, 1)                # the prompt of sam_pt.py:726-758, as the stepwise protocol builds it
        pred_sam.set_image(frames[t].permute(1, 2, 0).numpy())
        emb_equal.append(torch.equal(pred_sam._feat_tokens, feats[t]))
        pc = torch.as_tensor(pred_sam.transform.apply_coords(c, pred_sam.original_size), dtype=torch.float, device=dev)
        logits, _, _ = pred_sam.predict_torch(pc[None], torch.as_tensor(l, dtype=torch.int, device=dev)[None], multimask_output=False,
                                              return_logits=True)
        torch.cuda.synchronize()
        single.append(logits[0, 0].cpu())
    return fused, torch.stack(single), emb_equal


def test_sampt_forward_equals_the_per_frame_path_bitwise(clip_and_per_frame):
    """The fused clip path and the per-frame path may not differ: logits ``==``.

    The embeddings of the two paths are equal bit for bit.  The mask decoder's token-side f32 GEMMs choose their kernel by row count,
    so a chain of 4 items orders a row's sum differently from a predict_torch call (measured on an MI355X: 1.2e-7 .. 1.6e-7 on logits
    of magnitude 0.25 - 0.29, about 35 000 of a frame's 36 864 pixels; the ViT predictors differ the same way).  A TinyViT
    predictor therefore runs its clip path in chains of one item (SamHip.clip_decode_batch = 1), which is what this test holds."""
    fused, single, emb_equal = clip_and_per_frame
    assert all(emb_equal), "the clip path's embeddings are those of set_image, bit for bit"
    for t in range(4):
        d = (fused[t] - single[t]).abs()
        print(f"frame {t}: logits fused-vs-per-frame max |diff| {float(d.max()):.3e}, {int((d > 0).sum())} of {d.numel()} pixels differ")
    for t in range(4):
        assert torch.equal(single[t], fused[t]), f"frame {t}"


def test_sampt_forward_against_the_per_frame_path_at_the_projects_bar(clip_and_per_frame):
    """What the project holds its ViT predictors to for the same comparison (tests/test_gpu_modules.py, fused against stepwise):
    logits within 2e-3, masks at IoU >= 1 - 1e-3 — and here the embeddings of the two paths bit for bit."""
    fused, single, emb_equal = clip_and_per_frame
    assert all(emb_equal)
    assert max_abs(fused, single) < 2e-3
    for t in range(4):
        assert iou(fused[t] > 0, single[t] > 0) >= 1 - 1e-3
