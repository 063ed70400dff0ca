"""TinyViT (MobileSAM / Light HQ-SAM image encoder) on the CPU: the packer's arithmetic, the formulation the device kernels use
against the literal restatement (tests/tinyvit_ref.py), the configuration plumbing and the host logic over a recording fake.
PARITY UNPINNED: the restatement follows the written description of upstream's tiny_vit_sam.py, whose source is not available here."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam_pt_amd import pack as P
from sam_pt_amd.weights import SAM_CONFIGS, TinyVitConfig, init_sam_state_dict
from tests import hydra_lite as H
from tests import tinyvit_ref as R
from tests.util import disc_queries, synthetic_clip

CONFIGS = "/root/reference/configs"
needs_ref = pytest.mark.skipif(not os.path.isdir(CONFIGS), reason="reference tree not present (GPU box)")
E = "image_encoder."


@pytest.fixture(scope="module")
def tcfg():
    return SAM_CONFIGS["vit_t_test"]


@pytest.fixture(scope="module")
def tsd(tcfg):
    return init_sam_state_dict(tcfg, 72, hq=True)


@pytest.fixture(scope="module")
def golden_run():
    """The golden tool's inputs and its f32 run (computed once, read-only)."""
    from tools import make_tinyvit_golden as G
    cfg, sd, frames, pts, labels = G.golden_inputs()
    return cfg, sd, frames, pts, labels, G.run_all(cfg, sd, frames, pts, labels, torch.float32)


def test_shipped_hyper_parameters_and_parameter_counts():
    """TinyViT-5M: 5 392 764 parameters with the unused 1000-class head and no neck (the published 5.39 M), 5 743 892 as SAM's
    encoder (no head, with neck) — and the restatement loads init_sam_state_dict's encoder keys strictly."""
    cfg = SAM_CONFIGS["vit_t"]
    assert (cfg.embed_dims, cfg.depths, cfg.num_heads, cfg.window_sizes) == ((64, 128, 160, 320), (2, 2, 6, 2), (2, 4, 5, 10), (7, 7, 14, 7))
    assert (cfg.img_size, cfg.patch_size, cfg.grid, cfg.out_chans, cfg.hq_dim, cfg.resolutions) == (1024, 16, 64, 256, 160, (256, 128, 64, 64))
    sd = init_sam_state_dict(cfg, 72, hq=True)
    m = R.build(cfg, sd)                                                   # strict=True inside
    n = {k: p.numel() for k, p in m.named_parameters()}
    head = sum(v for k, v in n.items() if k.startswith(("head.", "norm_head.")))
    neck = sum(v for k, v in n.items() if k.startswith("neck."))
    assert sum(n.values()) - neck == 5392764 and sum(n.values()) - head == 5743892
    assert "attention_bias_idxs" not in "".join(m.state_dict().keys())      # non-persistent, as upstream
    assert tuple(sd["mask_decoder.compress_vit_feat.0.weight"].shape) == (160, 256, 2, 2)
    assert "mask_decoder.hf_token.weight" not in init_sam_state_dict(cfg, 72)


def test_init_is_off_the_defaults(tsd):
    rv = torch.cat([v.flatten() for k, v in tsd.items() if k.endswith("bn.running_var")])
    rm = torch.cat([v.flatten() for k, v in tsd.items() if k.endswith("bn.running_mean")])
    assert 0.5 <= float(rv.min()) and float(rv.max()) <= 1.5 and float(rv.std()) > 0.2 and float(rm.abs().mean()) > 0.05
    assert float(tsd[E + "layers.0.blocks.0.conv3.bn.weight"].abs().min()) > 0.1
    ab = torch.cat([v.flatten() for k, v in tsd.items() if k.endswith("attention_biases")])
    assert 0.4 < float(ab.std()) < 0.6


@pytest.mark.parametrize("name,groups", [("patch_embed.seq.0", 1), ("layers.0.blocks.1.conv2", 128), ("layers.2.downsample.conv2", 320),
                                         ("layers.1.blocks.0.local_conv", 64), ("layers.0.blocks.0.conv3", 1)])
def test_folded_batchnorm_against_batch_norm_in_float64(tsd, name, groups):
    p = E + name
    w, b = P.fold_conv_bn(tsd, p)
    c = tsd[p + ".c.weight"]
    x = torch.randn(2, c.shape[1] * groups, 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    pad = c.shape[-1] // 2
    ref = F.batch_norm(F.conv2d(x, c.double(), None, 1, pad, 1, groups), tsd[p + ".bn.running_mean"].double(), tsd[p + ".bn.running_var"].double(),
                       tsd[p + ".bn.weight"].double(), tsd[p + ".bn.bias"].double(), False, 0.0, 1e-5)
    got = F.conv2d(x, w.double(), b.double(), 1, pad, 1, groups)
    assert float((got - ref).abs().max()) <= 4e-7 * float(ref.abs().max())           # w', b' are rounded to f32 once


@pytest.mark.parametrize("ws", [7, 14, 3])
def test_bias_index_is_abs_dy_ws_plus_abs_dx(ws):
    assert torch.equal(P.tinyvit_bias_index(ws), R.first_appearance_index(ws))


def window_attention_from_one_row(qkv, table, pad_qkv, heads, ws):
    """What csrc/tinyvit.hip computes, restated: attention per ws x ws window over the UN-padded qkv map (B, H, W, 3C), the
    q / k / v of every position outside the map being the one row ``pad_qkv``; the output exists for real positions only."""
    B, Hh, Ww, C3 = qkv.shape
    C = C3 // 3
    idx = P.tinyvit_bias_index(ws)
    out = torch.full((B, Hh, Ww, C), float("nan"), dtype=qkv.dtype)
    for b in range(B):
        for wy in range(-(-Hh // ws)):
            for wx in range(-(-Ww // ws)):
                rows, real = [], []
                for j in range(ws * ws):
                    y, x = wy * ws + j // ws, wx * ws + j % ws
                    ok = y < Hh and x < Ww
                    rows.append(qkv[b, y, x] if ok else pad_qkv)
                    real.append((y, x) if ok else None)
                t = torch.stack(rows).view(ws * ws, heads, 96)
                q, k, v = t[..., :32].transpose(0, 1), t[..., 32:64].transpose(0, 1), t[..., 64:].transpose(0, 1)
                a = ((q @ k.transpose(1, 2)) * 32 ** -0.5 + table[:, idx]).softmax(-1) @ v       # (heads, N, 32)
                o = a.transpose(0, 1).reshape(ws * ws, C)
                for j, yx in enumerate(real):
                    if yx is not None:
                        out[b, yx[0], yx[1]] = o[j]
    return out


@pytest.mark.parametrize("layer,side", [(1, (9, 10)), (2, (16, 16)), (3, (7, 7)), (2, (8, 8))])
def test_padded_keys_from_one_row_against_the_literal_padded_path(tcfg, tsd, layer, side):
    """pack_tinyvit's pad_qkv row + attention over un-padded maps == F.pad -> partition -> attention -> crop, to 1e-6 relative
    (float64 on both sides: the two differ in the order of a few sums only)."""
    Hh, Ww = side
    C, heads, ws = tcfg.embed_dims[layer], tcfg.num_heads[layer], tcfg.window_sizes[layer]
    blk = R.TinyViTBlock(C, (Hh, Ww), heads, ws, 4, 3).double()
    p = f"{E}layers.{layer}.blocks.0."
    blk.load_state_dict({k[len(p):]: v.double() for k, v in tsd.items() if k.startswith(p)}, strict=True)
    x = torch.randn(2, Hh * Ww, C, dtype=torch.float64, generator=torch.Generator().manual_seed(layer))
    # the literal path, up to "x = res_x + attn": the block with its local_conv and mlp taken out
    with torch.no_grad():
        xp = x.view(2, Hh, Ww, C)
        if (Hh, Ww) != (ws, ws):
            pb, pr = (ws - Hh % ws) % ws, (ws - Ww % ws) % ws
            xp = F.pad(xp, (0, 0, 0, pr, 0, pb))
            nH, nW = (Hh + pb) // ws, (Ww + pr) // ws
            a = blk.attn(xp.view(2, nH, ws, nW, ws, C).transpose(2, 3).reshape(2 * nH * nW, ws * ws, C))
            a = a.view(2, nH, nW, ws, ws, C).transpose(2, 3).reshape(2, Hh + pb, Ww + pr, C)[:, :Hh, :Ww]
        else:
            a = blk.attn(x).view(2, Hh, Ww, C)
        packed = P.pack_tinyvit(tsd, tcfg, "cpu")
        pad_qkv = packed[p + "attn.pad_qkv"]
        assert torch.allclose(pad_qkv.double(), blk.attn.qkv(blk.attn.norm(torch.zeros(1, C, dtype=torch.float64)))[0], rtol=1e-6, atol=1e-7)
        qkv = blk.attn.qkv(blk.attn.norm(x)).view(2, Hh, Ww, 3 * C)
        pad64 = blk.attn.qkv.weight @ blk.attn.norm.bias + blk.attn.qkv.bias
        o = window_attention_from_one_row(qkv, blk.attn.attention_biases.detach(), pad64, heads, ws)
        got = blk.attn.proj(o)
    assert not torch.isnan(o).any()
    assert float((got - a).abs().max()) <= 1e-6 * float(a.abs().max())


def test_stride_is_one_exactly_when_the_merged_width_is_320():
    for out_dim in (64, 96, 128, 160, 192, 256, 320, 384, 448, 576):
        want = 1 if out_dim in (320, 448, 576) else 2
        assert R.PatchMerging((8, 8), 32, out_dim).stride == want
        assert TinyVitConfig("x", (32, 64, 96, out_dim), (1, 1, 1, 1), (1, 2, 3, out_dim // 32), (7, 7, 7, 7)).merge_strides[2] == want
    assert SAM_CONFIGS["vit_t"].merge_strides == (2, 2, 1) and SAM_CONFIGS["vit_t_test"].resolutions == (64, 32, 16, 16)


def test_interm_stage_is_the_input_of_layers_2(golden_run):
    cfg, sd, frames, _, _, _ = golden_run
    m = R.build(cfg, sd)
    seen = []
    m.layers[2].register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    with torch.no_grad():
        out = m(R.preprocess(cfg, frames))
    g = cfg.grid
    assert len(seen) == 1 and torch.equal(out["interm"].reshape(2, g * g, -1), seen[0]) and torch.equal(seen[0], out["layer1"])
    assert tuple(out["interm"].shape) == (2, g, g, cfg.embed_dims[2]) and tuple(out["neck"].shape) == (2, 256, g, g)


def test_pack_tinyvit_shapes(tcfg, tsd):
    o = P.pack_tinyvit(tsd, tcfg, "cpu")
    sh = lambda k: (tuple(o[E + k].shape), o[E + k].dtype)
    assert sh("patch_embed.seq.0.weight") == ((16, 36), torch.float32) and (E + "patch_embed.seq.0.weight_hl") not in o     # Cin 3 -> 4: exact f32
    assert float(o[E + "patch_embed.seq.0.weight"].view(16, 3, 3, 4)[..., 3].abs().max()) == 0
    assert sh("layers.0.blocks.0.conv1.weight") == ((128, 32), torch.float32) and sh("layers.0.blocks.0.conv1.weight_hl") == ((2, 128, 32), torch.float16)
    assert sh("layers.0.blocks.0.conv2.weight") == ((3, 3, 128), torch.float32) and sh("layers.0.blocks.0.conv2.bias") == ((128,), torch.float32)
    assert sh("layers.1.downsample.conv2.weight") == ((3, 3, 96), torch.float32)
    assert sh("layers.2.blocks.1.attn.qkv.weight_hl") == ((2, 288, 96), torch.float16) and sh("layers.2.blocks.1.attn.pad_qkv") == ((288,), torch.float32)
    assert sh("layers.2.blocks.1.attn.attention_biases") == ((3, 196), torch.float32)
    assert torch.equal(o[E + "layers.2.blocks.1.attn.attention_biases"], tsd[E + "layers.2.blocks.1.attn.attention_biases"])
    assert sh("layers.3.blocks.0.local_conv.weight") == ((3, 3, 320), torch.float32)
    assert sh("neck.0.weight_hl") == ((2, 256, 320), torch.float16) and sh("neck.2.weight_khwc_hl") == ((2, 256, 2304), torch.float16)
    assert not any("head" in k or ".bn." in k or k.endswith(".c.weight") or "num_batches" in k for k in o)
    # depthwise layout: [ky][kx][c] of the folded weight
    w, _ = P.fold_conv_bn(tsd, E + "layers.1.blocks.0.local_conv")
    assert torch.equal(o[E + "layers.1.blocks.0.local_conv.weight"][1, 2], w[:, 0, 1, 2])
    full = P.pack_tinyvit(init_sam_state_dict(SAM_CONFIGS["vit_t"], 72), SAM_CONFIGS["vit_t"], "cpu")
    assert tuple(full[E + "patch_embed.seq.2.weight_hl"].shape) == (2, 64, 288)                # 32 -> 64, 3 x 3: split-fp16


@pytest.mark.parametrize("change,field", [
    (dict(num_heads=(1, 2, 2, 10)), "num_heads[2]"),                        # head width 48
    (dict(window_sizes=(7, 7, 16, 7)), "window_sizes[2]"),
    (dict(embed_dims=(32, 64, 96, 336), num_heads=(1, 2, 3, 10)), "embed_dims[3]"),
    (dict(embed_dims=(48, 64, 96, 320)), "embed_dims[0]"),
    (dict(img_size=264), "img_size"),
    (dict(embed_dims=(32, 64, 96, 256), num_heads=(1, 2, 3, 8)), "img_size"),   # a third stride-2 merge: the grid is not img / 16
    (dict(local_conv_size=5), "local_conv_size")])
def test_pack_tinyvit_refuses_by_name(tsd, change, field):
    base = SAM_CONFIGS["vit_t_test"]
    kw = dict(embed_dims=base.embed_dims, depths=base.depths, num_heads=base.num_heads, window_sizes=base.window_sizes, img_size=base.img_size)
    kw.update(change)
    with pytest.raises(ValueError, match=field.replace("[", r"\[").replace("]", r"\]")):
        P.pack_tinyvit(tsd, TinyVitConfig("bad", **kw), "cpu")


def test_golden_file_reproduces_from_the_restatement(golden_run):
    cfg, sd, frames, pts, labels, o = golden_run
    z = R.load_golden()
    clip, _ = synthetic_clip(T=4, H=144, W=256, seed=72)
    assert torch.equal(clip[z["frame_ids"].tolist()], frames) and np.array_equal(z["points"], pts.numpy()) and np.array_equal(z["labels"], labels.numpy())
    g2 = cfg.grid ** 2
    emb = o["neck"].permute(0, 2, 3, 1).reshape(2, g2, -1)[:, z["emb_idx"]].numpy()
    hqf = o["hqfeat"].permute(0, 2, 3, 1).reshape(2, 16 * g2, -1)[:, z["hq_idx"]].numpy()
    interm = o["interm"].reshape(2, g2, -1)[:, z["emb_idx"]].numpy()
    # the same restatement on the same torch build gives the same bits; another build stays far inside the bars
    for name, got, bar in (("emb_rows", emb, "bar_emb"), ("interm_rows", interm, "bar_interm"), ("hq_rows", hqf, "bar_hq"),
                           ("low_sam", o["low_sam"].numpy(), "bar_logit"), ("low_hq", o["low_hq"].numpy(), "bar_logit")):
        assert got.shape == z[name].shape and float(np.abs(got - z[name]).max()) <= float(z[bar]) / 8, name
    for s in R.STAGES + ("emb", "interm", "hq", "logit"):
        assert float(z["bar_" + s]) == 8 * float(z["floor_" + s].max()) > 0
    for m in ("sam", "hq"):
        cover = z["mask_" + m].reshape(2, -1).mean(1)
        assert ((cover >= 0.05) & (cover <= 0.95)).all()


def _compose(sam_option):
    cfg = {"model": H.compose(CONFIGS, "model", "sam_pt", {"point_tracker": "pips", "sam@sam_predictor.sam_model": sam_option})}
    H.apply_overrides(cfg, ["model.point_tracker._target_=sam_pt_amd.point_tracker.PipsPointTracker",
                            "model.sam_predictor._target_=sam_pt_amd.sam_predictor.SamPredictor",
                            "model.sam_predictor.sam_model._target_=sam_pt_amd.sam_predictor.SamHip",
                            "+model.sam_predictor.sam_model._recursive_=false",
                            "model.point_tracker.checkpoint_path=null", "model.sam_predictor.sam_model.checkpoint=null"])
    return H.resolve(cfg, cwd="/nonexistent")["model"]


@needs_ref
@pytest.mark.parametrize("sam_option,hq", [("sam_mobile_vit_tiny", False), ("samhq_light_vit_tiny", True)])
def test_reference_tinyvit_yamls_compose_into_samhip(sam_option, hq):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    pred = H.instantiate(_compose(sam_option)["sam_predictor"])            # (model._target_ stays the reference's own SamPt)
    sam = pred.model
    assert type(pred) is SamPredictor and type(sam) is SamHip and isinstance(sam.cfg, TinyVitConfig)
    assert (sam.cfg.embed_dims, sam.cfg.depths, sam.cfg.window_sizes, sam.cfg.num_heads) == ((64, 128, 160, 320), (2, 2, 6, 2), (7, 7, 14, 7), (2, 4, 5, 10))
    assert sam.hq is hq and sam.cfg.name == "vit_t" and sam.cfg == SAM_CONFIGS["vit_t"]
    assert (sam.image_size, sam.image_embedding_size, sam.prompt_embed_dim, sam.vit_patch_size) == (1024, 64, 256, 16)


def test_variant_by_hand_and_precision_is_accepted_and_inert():
    from sam_pt_amd.sam_predictor import SamHip
    for prec in ("f16", "f16x3", "f32"):
        sam = SamHip(variant="vit_t", precision=prec)
        assert sam.cfg is SAM_CONFIGS["vit_t"] and sam.hq is False
    assert SamHip(variant="vit_t", hq=True).hq is True
    with pytest.raises(ValueError, match="contradicts"):
        SamHip(variant="vit_b", image_encoder={"embed_dims": [64, 128, 160, 320]})


@pytest.mark.parametrize("hq", [False, True])
def test_predictor_and_sampt_over_the_recording_fake(monkeypatch, tcfg, tsd, hq):
    """set_image, encode_frames and one SamPt.forward make tinyvit_* and dec_* calls and no vit_* call (the fake has none to make);
    the ViT-only machinery is refused by name."""
    from sam_pt_amd import _lib
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import ClipFeatures, SamHip, SamPredictor
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.weights import init_pips_state_dict
    from tests import fake_hip_tinyvit
    sd = tsd if hq else {k: v for k, v in tsd.items() if k in init_sam_state_dict(tcfg, 72)}
    psd = init_pips_state_dict(72)
    fake = fake_hip_tinyvit.install(monkeypatch, sd, tcfg, psd, hq=hq)
    pred = SamPredictor(SamHip(config=tcfg, state_dict=sd, precision="f16", max_batch=3))
    assert pred.model.hq is hq and not pred.skip_dead_rows and not pred.bias_correction
    pred_model = pred.model
    frames, centres = synthetic_clip(T=4, H=144, W=256, seed=72)
    pred.set_image(frames[0].permute(1, 2, 0).numpy())
    vit, dec = pred._vit, pred._dec
    assert dict(fake.calls) == {"tinyvit_create": 1, "dec_create": 1, "tinyvit_workspace_bytes": 1, "tinyvit_encode": 1, "tinyvit_encode_frames": 1}
    g = tcfg.grid
    want = R.run(tcfg, sd, frames[:1])["neck"]
    assert torch.equal(pred.features, want) and pred.input_size == (144, 256)
    feats = pred.encode_frames(frames, chw=True, gemm_workgroups=28)        # (the hint SamPt passes beside a tracker: ignored here)
    assert isinstance(feats, ClipFeatures) == hq and tuple(feats.shape) == (4, g * g, 256)
    assert fake.calls["tinyvit_encode"] == 3 and fake.calls["tinyvit_encode_frames"] == 5 and fake.calls["tinyvit_workspace_bytes"] == 3
    assert pred._vit is vit and pred._dec is dec
    pts = torch.tensor([[[centres[0][0], centres[0][1]]]])
    masks, iou, low = pred.predict_torch(pts, torch.ones(1, 1, dtype=torch.int32), multimask_output=False, return_logits=True)
    assert tuple(masks.shape) == (1, 1, 144, 256) and fake.calls["sam_decode"] == 1
    for call, args in (("set_gemm_workgroups", (28,)), ("gemm_profile_begin", ()), ("gemm_profile_end", ())):
        with pytest.raises(_lib.SamptError, match=call):
            getattr(pred, call)(*args)
    pred.skip_dead_rows = True
    with pytest.raises(_lib.SamptError, match="skip_dead_rows"):
        pred.encode_frames(frames[:1])
    pred.skip_dead_rows, pred.bias_correction = False, True
    with pytest.raises(_lib.SamptError, match="bias_correction"):
        pred.encode_frames(frames[:1])
    pred.bias_correction = False
    before = dict(fake.calls)
    video = {"image": [f for f in frames], "target_hw": (144, 256), "query_points": disc_queries(centres, n_pos=4, r=9.0)[None]}
    model = SamPt(PipsPointTracker(state_dict=psd), pred, sam_iou_threshold=-1e9, positive_points_per_mask=4, negative_points_per_mask=0,
                  iterative_refinement_iterations=1).eval()
    out = model(video)
    assert out["logits"][0].shape == (4, 144, 256)
    new = {k: v - before.get(k, 0) for k, v in fake.calls.items() if v != before.get(k, 0) and not k.startswith("pips_")}
    assert pred_model.clip_decode_batch == 1 and SamHip("vit_test", seed=72).clip_decode_batch is None
    assert new == {"sam_track_decode": 4, "sam_track_decode_items": 4, "tinyvit_encode": 2, "tinyvit_encode_frames": 4,
                   "tinyvit_workspace_bytes": 2}       # max_batch 3: frames 0..2, then frame 3; one decoder chain per item
    assert fake.calls["pips_create"] == 1 and fake.calls["pips_fnet_frames"] == 4
    assert not any(k.startswith("vit_") for k in fake.calls)
    del model, pred
    import gc
    gc.collect()
    assert fake.calls["tinyvit_destroy"] == 1 and fake.calls["dec_destroy"] == 1
