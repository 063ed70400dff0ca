"""Batch-invariant mask decoding on the device (``SamHip(batch_invariant_decode=True)``, sampt_dec_set_batch_invariant): an item of
a decoder chain, of a ``predict_points_batch`` chunk or of the interactive loop's batched chains gets the bits it gets alone.

The decoder is driven directly: seeded random embeddings through ``track_decode`` / ``set_features``, seeded weights, small output
frames, so no encoder runs (except in the two end-to-end tests).  Every comparison is ``torch.equal`` over every item, and every
configuration runs once.  The chain sizes cross the lines at which the default routes change kernel (csrc/gemm.hip
plan_route_f32, csrc/sam_decoder.hip attn_t2i_plan, csrc/engine_dec.hip L::lin):
  * F * Nt <= 16 rows (skinny -> thin) between chains of 1 and 2; F = 16 -> 17 for the heads (M = F);
  * F * P >= 16384 image rows (gemm_x3_wres) at F = 4 on the 64 x 64 grid;
  * thin -> tiled at ceil(M / 64) * ceil(N / 64) >= 128, i.e. M > 192 rows at N = 2048: chains of 17 and 24 with Nt >= 13;
  * M >= 2048 image rows (split-fp16 planes) between F = 1 and F = 2 on the 32 x 32 grid.
Accuracy bars are the ones the default mode is held to, taken from where they are defined."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
from tests.util import disc_queries, iou, max_abs, synthetic_clip

pytestmark = pytest.mark.gpu
OUT_HW = (96, 128)
N_ITEMS = 24


def make_pred(dev, cfg, hq=False, invariant=True, **kw):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    kw.setdefault("max_decode_batch", N_ITEMS)
    pred = SamPredictor(SamHip(config=cfg, seed=72, precision="f32", hq=hq, batch_invariant_decode=invariant, **kw).to(dev))
    pred._ensure()
    return pred


def chain_inputs(dev, cfg, n, hq, seed):
    """n (frame, object) items as SamPt's default configuration hands them to ``track_decode``: seeded embeddings, 2 .. 9 visible
    points each (ragged), positives first and one negative point last (two-pass chains), 8 point slots + the padding SamPt's staging adds."""
    g = torch.Generator().manual_seed(seed)
    P = cfg.grid ** 2
    emb = torch.randn(n, P, cfg.out_chans, generator=g)
    hqf = torch.randn(n, 16 * P, cfg.out_chans // 8, generator=g) if hq else None
    k = torch.tensor([2 + (5 * i + 3) % 8 for i in range(n)], dtype=torch.int32)          # 2 .. 9, every count present
    assert set(k.tolist()) == set(range(2, 10))
    ld = 16
    ih, iw = (cfg.img_size * OUT_HW[0]) // OUT_HW[1], cfg.img_size
    pts = torch.rand(n, ld, 2, generator=g) * torch.tensor([iw - 1.0, ih - 1.0])
    lab = torch.zeros(n, ld, dtype=torch.int32)
    for i in range(n):
        lab[i, :int(k[i]) - 1] = 1                                                          # the last visible point is the negative one
    npos = k - 1
    return {"emb": emb.to(dev), "hq": None if hqf is None else hqf.to(dev), "pts": pts.to(dev), "lab": lab.to(dev), "k": k, "npos": npos}


def run_chain(pred, inp, items, graph=False, R=2):
    """track_decode of the listed items as ONE chain -> (logits (F, H, W), scores (F,)) on the CPU."""
    from sam_pt_amd.sam_predictor import ClipFeatures
    dev = inp["emb"].device
    idx = torch.as_tensor(items, dtype=torch.long, device=dev)
    emb = inp["emb"].index_select(0, idx).contiguous()
    feats = emb if inp["hq"] is None else ClipFeatures(emb, inp["hq"].index_select(0, idx).contiguous())
    pts, lab = inp["pts"].index_select(0, idx).contiguous(), inp["lab"].index_select(0, idx).contiguous()
    ks, ps = inp["k"][list(items)], inp["npos"][list(items)]
    ragged = bool((ks != ks[0]).any())
    out_l = torch.full((len(items),) + OUT_HW, float("nan"), device=dev)
    out_s = torch.full((len(items),), float("nan"), device=dev)
    pred.track_decode(feats, pts, lab, int(ks.max()), int(ps.max()), R, -1e9, OUT_HW, out_l, out_s,
                      k_item=ks.to(dev) if ragged else None, npos_item=ps.to(dev) if ragged else None, graph=graph)
    torch.cuda.synchronize()
    assert not torch.isnan(out_l).any() and not torch.isnan(out_s).any()
    return out_l.cpu(), out_s.cpu()


def chunks(n, F):
    return [list(range(s, min(n, s + F))) for s in range(0, n, F)]


def assert_chains_equal_singles(pred, inp, n, sizes, singles=None):
    if singles is None:
        singles = [run_chain(pred, inp, [i]) for i in range(n)]
    assert float(torch.stack([s[0] for s in singles]).abs().max()) > 0
    for F in sizes:
        bad = []
        for items in chunks(n, F):
            lg, sc = run_chain(pred, inp, items)
            for j, i in enumerate(items):
                if not (torch.equal(lg[j], singles[i][0][0]) and torch.equal(sc[j], singles[i][1][0])):
                    bad.append((i, float((lg[j] - singles[i][0][0]).abs().max())))
        print(f"chains of {F}: {len(bad)} of {n} items differ from their single decode {bad[:4]}")
        assert not bad, f"chains of {F}: items {bad}"
    return singles


# ------------------------------------------------------------------------------------------------------------ the GEMM route
@pytest.mark.parametrize("N,K", [(256, 256), (128, 256), (2048, 256), (256, 2048), (256, 128), (32, 256), (4, 256), (3, 256), (1, 256)])
def test_row_invariant_gemm_kernel(dev, N, K):
    """sampt_gemm_f32_rows(invariant = 1): a row's bits do not depend on M or on where the row sits, with strided A rows, a broadcast
    residual and ReLU; against float64 within the worst-case bound of an fp32 dot product, (K + 2) * 2^-24 * sum |a_k w_k|  (+ the
    same on bias and residual): any order of the sum meets it."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(N * 7 + K)
    M, lda, res_mod = 203, K + 256, 29
    A, W, b, res = torch.randn(M, lda, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(res_mod, N, generator=g)
    Ad, Wd, bd, rd = A.to(dev), W.to(dev), b.to(dev), res.to(dev)

    def gemm(a_rows, m, row0, invariant=1):
        out = torch.full((m, N), float("nan"), device=dev)
        # (the residual row is row % res_mod of the CALL: hand every call the block that starts at its first row)
        r = torch.roll(rd, -(row0 % res_mod), 0).contiguous()
        _lib.check(lib.sampt_gemm_f32_rows(_lib.ptr(a_rows), lda, _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(r), res_mod, _lib.ptr(out), 0, m, N, K, 1,
                                           invariant, None, 0, _lib.stream_ptr()), "sampt_gemm_f32_rows")
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        return out.cpu()

    full = gemm(Ad, M, 0)
    pre = A[:, :K].double() @ W.double().t() + b.double()
    want = torch.relu(pre) + res.double()[torch.arange(M) % res_mod]
    bound = (K + 2) * 2.0 ** -24 * (A[:, :K].abs().double() @ W.abs().double().t() + b.abs().double() + res.abs().double()[torch.arange(M) % res_mod])
    assert bool(((full.double() - want).abs() <= bound).all()), f"max |err| {max_abs(full, want):.3e}"
    for row0, m in ((0, 1), (7, 1), (0, 16), (0, 17), (5, 64), (100, 103), (202, 1)):
        part = gemm(Ad[row0:], m, row0)
        assert torch.equal(part, full[row0:row0 + m]), f"rows {row0} .. {row0 + m} alone differ from their place in M = {M}"


# -------------------------------------------------------------------------------------------------------- chains against singles
@pytest.fixture(scope="module")
def pred64(dev):
    return make_pred(dev, SAM_CONFIGS["vit_t"])


@pytest.fixture(scope="module")
def inputs64(dev):
    return chain_inputs(dev, SAM_CONFIGS["vit_t"], N_ITEMS, False, 1)


def test_chain_equals_single_grid64(pred64, inputs64):
    """The geometry every shipped model has (P = 4096): 24 ragged two-pass items with R = 2 refinement passes (box and mask_input
    prompts), alone against chains of 2, 3, 4, 17 and 24."""
    assert_chains_equal_singles(pred64, inputs64, N_ITEMS, (2, 3, 4, 17, 24))


def test_chain_equals_single_grid32(dev):
    """P = 1024: the 2048-row switch of L::lin lies between one item and two, and Nk / 64 caps the key split at 16."""
    cfg = dataclasses.replace(SAM_CONFIGS["vit_t_test"], name="vit_t_512", img_size=512)
    assert cfg.grid == 32
    pred = make_pred(dev, cfg, max_decode_batch=16)
    inp = chain_inputs(dev, cfg, 16, False, 2)
    assert_chains_equal_singles(pred, inp, 16, (2, 16))


def test_chain_equals_single_hq(dev):
    """MaskDecoderHQ (vit_dim 160, Light HQ-SAM's geometry): alone against chains of 5 and 17."""
    cfg = SAM_CONFIGS["vit_t"]
    assert cfg.hq_dim == 160
    pred = make_pred(dev, cfg, hq=True, max_decode_batch=17)
    inp = chain_inputs(dev, cfg, 17, True, 3)
    assert_chains_equal_singles(pred, inp, 17, (5, 17))


def test_predict_torch_batch_members(dev, pred64, inputs64):
    pred = pred64
    pred.set_features(inputs64["emb"][0], OUT_HW, (768, 1024))
    pts, lab = inputs64["pts"][:5, :4].contiguous(), inputs64["lab"][:5, :4].contiguous()
    lg, io, lw = pred.predict_torch(pts, lab, multimask_output=False, return_logits=True)
    torch.cuda.synchronize()
    for b in range(5):
        l1, i1, w1 = pred.predict_torch(pts[b:b + 1], lab[b:b + 1], multimask_output=False, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(l1[0], lg[b]) and torch.equal(i1[0], io[b]) and torch.equal(w1[0], lw[b]), f"prompt {b}"


def test_predict_points_batch_chunk_invariance(dev, pred64, inputs64):
    pred = pred64
    pred.set_features(inputs64["emb"][1], OUT_HW, (768, 1024))
    pts, lab = inputs64["pts"][:9, :2].contiguous(), inputs64["lab"][:9, :2].contiguous()
    lab[:, 0] = 1
    runs = {}
    for mc in (1, 4, 9):
        low, io = pred.predict_points_batch(pts, lab, multimask_output=True, max_chunk=mc)
        torch.cuda.synchronize()
        assert tuple(low.shape) == (9, 3, 256, 256) and tuple(io.shape) == (9, 3)
        runs[mc] = (low.cpu(), io.cpu())
    for mc in (4, 9):
        d = [i for i in range(9) if not (torch.equal(runs[mc][0][i], runs[1][0][i]) and torch.equal(runs[mc][1][i], runs[1][1][i]))]
        assert not d, f"max_chunk={mc}: prompts {d} differ from max_chunk=1"


def test_graph_replay_and_mode_round_trip(dev, pred64, inputs64):
    """A replayed hipGraph of the mode equals the eager chain; switching the mode off and on again replays the graph captured in the
    mode — not one captured out of it — and gives the first result."""
    from sam_pt_amd.sam_predictor import ClipFeatures  # noqa: F401
    pred, inp = pred64, inputs64
    items = list(range(5))
    eager = run_chain(pred, inp, items)
    idx = torch.as_tensor(items, device=dev)
    emb = inp["emb"].index_select(0, idx).contiguous()
    pts, lab = inp["pts"].index_select(0, idx).contiguous(), inp["lab"].index_select(0, idx).contiguous()
    ks, ps = inp["k"][items].to(dev), inp["npos"][items].to(dev)
    kmax, pmax = int(inp["k"][items].max()), int(inp["npos"][items].max())
    out_l, out_s = torch.empty((5,) + OUT_HW, device=dev), torch.empty((5,), device=dev)

    def call():
        out_l.fill_(float("nan"))
        pred.track_decode(emb, pts, lab, kmax, pmax, 2, -1e9, OUT_HW, out_l, out_s, k_item=ks, npos_item=ps, graph=True)
        torch.cuda.current_stream().synchronize()
        return out_l.cpu().clone(), out_s.cpu().clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c0 = pred.graph_stats()
        first, second, third = call(), call(), call()              # plain launches, capture + launch, replay
        c1 = pred.graph_stats()
        assert c1[1] == c0[1] + 1 and c1[2] >= c0[2] + 2
        for r in (first, second, third):
            assert torch.equal(r[0], eager[0]) and torch.equal(r[1], eager[1])
        pred.set_batch_invariant_decode(False)
        off = [call() for _ in range(3)]                           # its own signature: seen, captured, replayed
        c2 = pred.graph_stats()
        assert c2[1] == c1[1] + 1, "the default mode captures a graph of its own"
        assert torch.equal(off[0][0], off[2][0])
        pred.set_batch_invariant_decode(True)
        again = call()
        c3 = pred.graph_stats()
        assert c3[1] == c2[1], "back in the mode: the graph captured there is replayed"
        assert torch.equal(again[0], eager[0]) and torch.equal(again[1], eager[1])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_default_mode_untouched_by_a_round_trip(dev, inputs64):
    pred = make_pred(dev, SAM_CONFIGS["vit_t"], invariant=False, max_decode_batch=5)
    items = list(range(5))
    before = run_chain(pred, inputs64, items)
    pred.set_batch_invariant_decode(True)
    inside = run_chain(pred, inputs64, items)
    pred.set_batch_invariant_decode(False)
    after = run_chain(pred, inputs64, items)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # the two modes are the same function up to rounding: the bar batched chains are held to against single ones in the default
    # mode (tests/test_gpu_interactive.py BAR = 8 x 1.9e-7), relative to the largest logit
    big = float(before[0].abs().max())
    print(f"mode on against off, chain of 5: max |diff| {max_abs(inside[0], before[0]):.3e} (largest |logit| {big:.3e})")
    assert max_abs(inside[0], before[0]) <= 8 * 1.9e-7 * max(1.0, big)


# ------------------------------------------------------------------------------------------------------------------ end to end
def clip_and_per_frame(dev, pred):
    """tests/test_gpu_tinyvit.py's ``clip_and_per_frame``: one SamPt.forward on a 4-frame clip (fused clip path), and the same
    predictor driven frame by frame through set_image / predict_torch with the same points."""
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_pt import SamPt
    frames, centres = synthetic_clip(T=4, H=144, W=256, seed=72)
    q = disc_queries(centres, n_pos=4, r=9.0)[None]
    model = SamPt(PipsPointTracker(state_dict=init_pips_state_dict(72)), pred, sam_iou_threshold=-1e9, positive_points_per_mask=4,
                  negative_points_per_mask=0, iterative_refinement_iterations=0).eval()
    out = model({"image": [f.to(dev) for f in frames], "target_hw": (144, 256), "query_points": q})
    torch.cuda.synchronize()
    traj, vis, fused = out["trajectories"].cpu(), out["visibilities"].cpu(), out["logits"][0].cpu()
    assert tuple(fused.shape) == (4, 144, 256) and bool((vis[:, 0] == 1).any(dim=1).all())
    feats = pred.encode_frames(frames.to(dev), chw=True)
    single, emb_equal = [], []
    for t in range(4):
        c, l = model._prepare_points(traj, vis, t, 0, 1)
        pred.set_image(frames[t].permute(1, 2, 0).numpy())
        emb_equal.append(torch.equal(pred._feat_tokens, feats[t]))
        pc = torch.as_tensor(pred.transform.apply_coords(c, pred.original_size), dtype=torch.float, device=dev)
        logits, _, _ = pred.predict_torch(pc[None], torch.as_tensor(l, dtype=torch.int, device=dev)[None], multimask_output=False,
                                          return_logits=True)
        torch.cuda.synchronize()
        single.append(logits[0, 0].cpu())
    return fused, torch.stack(single), emb_equal


@pytest.mark.parametrize("name", ["vit_t_test", "vit_test"])
def test_sampt_forward_equals_the_per_frame_path_in_chains_of_4(dev, name):
    """With the mode on and chains of 4 items, SamPt.forward's logits ``==`` the per-frame set_image / predict_torch logits — for the
    TinyViT predictor (which needs chains of one for this without the mode) and for the ViT one (which has it in no other configuration)."""
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    cfg = SAM_CONFIGS[name]
    pred = SamPredictor(SamHip(config=cfg, state_dict=init_sam_state_dict(cfg, 72), precision="f32", clip_decode_batch=4,
                               batch_invariant_decode=True).to(dev))
    fused, single, emb_equal = clip_and_per_frame(dev, pred)
    assert all(emb_equal), "the clip path's embeddings are those of set_image, bit for bit"
    for t in range(4):
        d = (fused[t] - single[t]).abs()
        print(f"{name} frame {t}: fused-vs-per-frame max |diff| {float(d.max()):.3e}, {int((d > 0).sum())} of {d.numel()} pixels differ")
    for t in range(4):
        assert torch.equal(single[t], fused[t]), f"frame {t}"


# -------------------------------------------------------------------------------------------------------------------- accuracy
def test_tinyvit_logits_within_the_golden_bar(dev):
    """tests/test_gpu_tinyvit.py::test_set_image_and_predict_torch with the mode on: the same golden values, the same ``bar_logit``
    (tests/golden/tinyvit_ref.npz) and the same mask bar."""
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from tests import tinyvit_ref as R
    from tools.make_tinyvit_golden import golden_inputs
    gold = {k: torch.from_numpy(v) for k, v in R.load_golden().items()}
    cfg, sd, frames, pts, labels = golden_inputs()
    sd = {k: v for k, v in sd.items() if k in init_sam_state_dict(cfg, 72)}
    pred = SamPredictor(SamHip(config=cfg, state_dict=sd, batch_invariant_decode=True).to(dev))
    for i in range(2):
        pred.set_image(frames[i].permute(1, 2, 0).numpy())
        logits, _, low = pred.predict_torch(pts[i:i + 1].to(dev), labels[i:i + 1].to(dev), multimask_output=False, return_logits=True)
        torch.cuda.synchronize()
        err, bar = max_abs(low[0, 0], gold["low_sam"][i]), float(gold["bar_logit"])
        miou = iou(logits[0, 0] > 0, gold["mask_sam"][i])
        print(f"frame {i}: low-res logits max |err| {err:.3e} (bar {bar:.3e}), mask IoU {miou:.7f}")
        assert err <= bar and miou >= 1 - 1e-5


def test_vit_test_predict_torch_vs_oracle(dev):
    """tests/test_gpu_modules.py::test_predict_torch_vs_oracle's protocol and bars (low-res and full logits 2e-4, IoU prediction
    1e-4, mask IoU 1 - 1e-3; decoding the ORACLE's features isolates the decoder) on ``vit_test`` with the mode on."""
    from oracle import sam_ref as R
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    frames, centres = synthetic_clip(T=1, H=144, W=256, seed=9)
    img = frames[0].permute(1, 2, 0).numpy()
    ref = R.SamPredictorRef(sd, cfg)
    ref.set_image(img)
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    pred = SamPredictor(SamHip(config=cfg, state_dict=sd, precision="f32", batch_invariant_decode=True).to(dev))
    pred._ensure()
    g = cfg.grid
    pred.set_features(ref.features[0].permute(1, 2, 0).reshape(g * g, 256).to(dev), (144, 256))
    q = disc_queries(centres, n_pos=6, r=12.0)[:, 1:]
    pts = torch.as_tensor(pred.transform.apply_coords(q.numpy(), (144, 256)), dtype=torch.float)[None]
    lab = torch.tensor([[1, 1, 1, 1, 0, 0]], dtype=torch.int)
    m0, i0, l0 = ref.predict_torch(pts, lab, None, None, False, True)
    m1, i1, l1 = pred.predict_torch(pts.to(dev), lab.to(dev), None, None, False, True)
    assert max_abs(l1, l0) < 2e-4 and max_abs(i1, i0) < 1e-4 and max_abs(m1, m0) < 2e-4
    assert iou(m1 > 0, m0 > 0) >= 1 - 1e-3
    box = torch.tensor([[[50.0, 25.0, 175.0, 125.0]]])
    m2, i2, l2 = ref.predict_torch(pts, lab, box, l0, False, True)
    m3, i3, l3 = pred.predict_torch(pts.to(dev), lab.to(dev), box.to(dev), l0.to(dev), False, True)
    assert max_abs(l3, l2) < 2e-4 and max_abs(i3, i2) < 1e-4
    assert iou(m3 > 0, m2 > 0) >= 1 - 1e-3


# ------------------------------------------------------------------------------------------------------------ interactive loop
def test_interactive_loop_histories_do_not_depend_on_decode_batch(dev):
    """SamPtInteractive with batched chains: with the mode on, ``decode_batch`` 2 and 4 take the same clicks and give the same logits
    (one flipped pixel would change a ``randperm`` length and every later click).  ``decode_batch=1`` feeds the points in the
    reference's order, the chains feed positives first: another token order, other sums — not compared."""
    from sam_pt_amd.sam_pt_interactive import SamPtInteractive
    from tests import interactive_ref as IR
    video, tracker, predictor, kw = IR.gpu_loop_setup(dev)
    predictor.set_batch_invariant_decode(True)
    runs = {}
    for db in (2, 4):
        model = SamPtInteractive(point_tracker=tracker, sam_predictor=predictor, decode_batch=db, **kw).eval()
        torch.manual_seed(5)
        out = model(video)
        torch.cuda.synchronize()
        runs[db] = (IR.history_rows(model.last_run["interaction_history"]), out["logits"][0].cpu(), model.last_run)
        assert model.last_run["decoder_chains"] < model.last_run["decoder_calls"]
    assert len(runs[2][0]) == 9 and runs[2][0] == runs[4][0]
    assert torch.equal(runs[2][1], runs[4][1])
    assert runs[2][2]["decoder_chains"] > runs[4][2]["decoder_chains"], "the two runs did batch differently"
