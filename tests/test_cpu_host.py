"""CPU tests of the host logic and the C-ABI surface (no GPU compute calls)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def test_c_abi_exports_every_declared_symbol():
    """libsampt_hip.so loads and exports exactly the functions declared in include/sampt_hip.h."""
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr)) - {"sampt_vit_config"}
    lib = _lib.load()                       # AttributeError here if a bound symbol is missing from the .so
    assert lib.sampt_version() >= 1
    bound = set(_lib.exported_symbols())
    assert declared == bound, f"header vs ctypes binding mismatch: {declared ^ bound}"
    for name in declared:
        assert hasattr(lib, name)


def test_product_fails_loudly_without_gpu():
    """No CPU / PyTorch fallback on the product path."""
    from sam_pt_amd import _lib
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict
    trk = PipsPointTracker(state_dict=init_pips_state_dict(1))
    rgbs = torch.zeros(1, 9, 3, 64, 96, dtype=torch.uint8)
    with pytest.raises(_lib.SamptError):
        trk(rgbs, torch.tensor([[[0.0, 10.0, 10.0]]]))
    pred = SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"]))
    with pytest.raises(_lib.SamptError):
        pred.set_image(np.zeros((144, 256, 3), dtype=np.uint8))
    with pytest.raises(RuntimeError):
        pred.predict_torch(torch.zeros(1, 1, 2), torch.ones(1, 1, dtype=torch.int), multimask_output=False)


def test_product_does_not_import_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "sam_pt_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_window_row_map_matches_window_partition():
    """pack.window_row_map == the row permutation of SAM's window_partition (zero padding -> -1)."""
    from oracle import sam_ref as R
    from sam_pt_amd.pack import window_row_map
    for grid, ws, B in [(16, 6, 2), (64, 14, 1), (8, 4, 3)]:
        tok = torch.arange(1, B * grid * grid + 1, dtype=torch.float32).view(B, grid, grid, 1)
        win, _ = R._window_partition(tok, ws)              # (B*nwin, ws, ws, 1); padding = 0
        expect = win.reshape(-1).long() - 1                # token row, -1 on padding
        assert torch.equal(window_row_map(grid, ws, B).long(), expect)


def test_live_window_row_map_is_the_restriction_of_the_full_one():
    """The compact stream of the encoder's dead-row skipping holds the first `rows` token rows of every frame: its window
    map must list, window by window, the same tokens as the full map's first rows/window window rows."""
    from sam_pt_amd.pack import window_row_map
    for grid, ws, B, rows in [(16, 6, 2, 12), (16, 6, 1, 6), (64, 14, 2, 42), (64, 14, 1, 14)]:
        n1 = -(-grid // ws)
        full = window_row_map(grid, ws, B).view(B, n1, n1, ws * ws).long()
        live = window_row_map(grid, ws, B, rows=rows).view(B, rows // ws, n1, ws * ws).long()
        for b in range(B):
            f = full[b, :rows // ws]
            tok = torch.where(f >= 0, f - b * grid * grid, f)              # token index inside the frame
            assert (tok < rows * grid).all()
            assert torch.equal(torch.where(tok >= 0, tok + b * rows * grid, tok), live[b])


def test_pixel_shuffle_maps_match_conv_transpose():
    from sam_pt_amd.pack import _convt_pack, _shuffle_map
    g = torch.Generator().manual_seed(0)
    side, cin, cout, F = 4, 8, 6, 3
    x = torch.randn(F, cin, side, side, generator=g)
    w = torch.randn(cin, cout, 2, 2, generator=g)
    ref = torch.nn.functional.conv_transpose2d(x, w, stride=2).permute(0, 2, 3, 1).reshape(F * 4 * side * side, cout)
    rows = x.permute(0, 2, 3, 1).reshape(F * side * side, cin)
    maps, wp = _shuffle_map(side, F), _convt_pack(w)
    out = torch.zeros_like(ref)
    for z in range(4):
        out[maps[z].long()] = rows @ wp[z].t()
    assert torch.allclose(out, ref, atol=1e-5)


def test_weight_layouts_and_packing():
    from sam_pt_amd.pack import pack_pips
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
    sd = init_pips_state_dict(72)
    assert len(sd) == 200 and sd["delta_block.to_delta.0.weight"].shape == (512, 519)
    assert sd["delta_block.to_delta.3.0.fn.0.weight"].shape == (32, 8, 1)
    p = pack_pips(sd, "cpu")
    assert p["fnet.conv1.weight"].shape == (64, 7 * 7 * 4) and p["delta_block.to_delta.0.weight"].shape == (512, 520)
    w = sd["fnet.layer2.0.conv1.weight"]
    assert torch.equal(p["fnet.layer2.0.conv1.weight"].view(96, 3, 3, 64)[5, 1, 2], w[5, :, 1, 2])
    s = init_sam_state_dict(SAM_CONFIGS["vit_b"], 72)
    assert s["image_encoder.blocks.2.attn.rel_pos_h"].shape == (127, 64)   # global block: 2*64-1
    assert s["image_encoder.blocks.0.attn.rel_pos_h"].shape == (27, 64)    # windowed: 2*14-1
    assert s["mask_decoder.output_upscaling.0.weight"].shape == (256, 64, 2, 2)


def _unsplit(hl):
    """inverse of pack.split_f16x3: half [2][N][K] -> fp32 [N][K] (exact up to the dropped 2^-22 tail)"""
    from sam_pt_amd.pack import F16X3_WSHIFT
    return (hl[0].double() + hl[1].double()).float() / float(1 << F16X3_WSHIFT)


def test_unsplittable_weights_fall_back_per_layer():
    """a weight whose magnitude * 2^8 leaves the fp16 range cannot be split into hi + lo planes.  The decoder and
    the tracker encoder keep their f32 weights beside the planes, so packing leaves out the planes of that ONE layer (the
    engines then run it on the exact f32 MFMA path) instead of refusing the checkpoint; the fp16-ViT ends have no f32 twin
    and still raise, with a message that says what to do."""
    import pytest
    from sam_pt_amd.pack import pack_decoder, pack_pips, pack_vit, split_f16x3
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 3)
    big = "mask_decoder.transformer.layers.0.cross_attn_token_to_image.k_proj.weight"
    ref = pack_decoder(sd, cfg, "cpu", 2)
    sd2 = dict(sd)
    sd2[big] = sd[big].clone()
    sd2[big][0, 0] = 300.0                                       # 300 * 2^8 > 65504
    p = pack_decoder(sd2, cfg, "cpu", 2)
    gone = {k for k in ref if k not in p}
    assert gone == {big + "_hl", "mask_decoder.transformer.layers.0.__kvq_w_hl"}, gone      # the layer itself + its fused form
    assert torch.equal(p[big], sd2[big].float())                 # the f32 weight the fallback multiplies with
    assert split_f16x3(sd2[big], strict=False) is None
    with pytest.raises(ValueError, match="precision='f32'"):
        split_f16x3(sd2[big])
    psd = init_pips_state_dict(72)
    name = "fnet.layer1.0.conv1.weight"
    psd2 = dict(psd)
    psd2[name] = psd[name].clone()
    psd2[name][0, 0, 0, 0] = 1e3
    pp, pr = pack_pips(psd2, "cpu"), pack_pips(psd, "cpu")
    assert {k for k in pr if k not in pp} == {name + "_hl"}
    vsd = dict(sd)
    vsd["image_encoder.neck.2.weight"] = sd["image_encoder.neck.2.weight"].clone()
    vsd["image_encoder.neck.2.weight"][0, 0, 0, 0] = 300.0
    with pytest.raises(ValueError, match="fp16 range"):
        pack_vit(vsd, cfg, "cpu", True, 1)
    pack_vit(vsd, cfg, "cpu", False, 1)                          # the exact mode takes it


def test_decoder_fused_projection_packing():
    """pack_decoder's fused image-side projections: keys @ W^T + b + pe-term must equal the three separate projections of
    the two-way transformer — (keys + pe) Wk, keys Wv, (keys + pe) Wq' (SAM TwoWayAttentionBlock) — and the final
    attention's K | V pair."""
    from sam_pt_amd.pack import pack_decoder
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 3)
    p = pack_decoder(sd, cfg, "cpu", 2)
    g = torch.Generator().manual_seed(0)
    P = cfg.grid * cfg.grid
    keys = torch.randn(2 * P, 256, generator=g)
    pe = p["prompt_encoder.__dense_pe"].repeat(2, 1)
    tr = "mask_decoder.transformer."

    def lin(x, name):
        return x.double() @ sd[name + ".weight"].double().t() + sd[name + ".bias"].double()

    for i in range(cfg.dec_depth):
        lp = f"{tr}layers.{i}."
        want = torch.cat([lin(keys + pe, lp + "cross_attn_token_to_image.k_proj"), lin(keys, lp + "cross_attn_token_to_image.v_proj"),
                          lin(keys + pe, lp + "cross_attn_image_to_token.q_proj")], dim=1)
        got = keys.double() @ p[lp + "__kvq_w"].double().t() + p[lp + "__kvq_b"].double() + p[lp + "__kvq_pe"].double().repeat(2, 1)
        assert got.shape == (2 * P, 384) and (got - want).abs().max() < 2e-5
        assert (_unsplit(p[lp + "__kvq_w_hl"]) - p[lp + "__kvq_w"]).abs().max() < 1e-6       # the planes the GPU multiplies
    want = torch.cat([lin(keys + pe, tr + "final_attn_token_to_image.k_proj"), lin(keys, tr + "final_attn_token_to_image.v_proj")], dim=1)
    got = keys.double() @ p[tr + "__fin_kv_w"].double().t() + p[tr + "__fin_kv_b"].double() + p[tr + "__fin_kv_pe"].double().repeat(2, 1)
    assert got.shape == (2 * P, 256) and (got - want).abs().max() < 2e-5


def test_transposed_convolution_as_one_gemm_with_pixel_shuffle():
    """The decoder's ConvTranspose2d(k=2, s=2) stages run as ONE GEMM over N = 4*Cout columns (dy, dx, channel) whose
    epilogue scatters GEMM row f*g*g + y*g + x, column block z = 2*dy + dx to pixel row f*4*g*g + (2y+dy)*2g + 2x+dx
    (csrc/conv_f16x3.hip, GemmP::shuf_g).  This restates that address arithmetic on the packed planes and checks it
    against torch's conv_transpose2d."""
    from sam_pt_amd.pack import pack_decoder
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 5, hq=True)
    p = pack_decoder(sd, cfg, "cpu", 2, hq=True)
    gen = torch.Generator().manual_seed(1)
    for name, g in [("output_upscaling.0", 5), ("output_upscaling.3", 6), ("embedding_encoder.0", 4), ("compress_vit_feat.3", 3)]:
        w, b = sd[f"mask_decoder.{name}.weight"], sd[f"mask_decoder.{name}.bias"]
        cin, cout = w.shape[0], w.shape[1]
        F_ = 2
        x = torch.randn(F_, cin, g, g, generator=gen)
        ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2).permute(0, 2, 3, 1).reshape(F_ * 4 * g * g, cout)
        hl = p[f"mask_decoder.{name}.weight_packed_hl"]
        assert hl.shape == (2, 4 * cout, cin)
        rows = x.permute(0, 2, 3, 1).reshape(F_ * g * g, cin).double()
        acc = rows @ _unsplit(hl).double().t()                              # [F*g*g][4*cout], columns z*cout + c
        out = torch.zeros_like(ref)
        r = torch.arange(F_ * g * g)
        f, rem = r // (g * g), r % (g * g)
        y, xx = rem // g, rem % g
        for z in range(4):
            orow = f * 4 * g * g + (2 * y + (z >> 1)) * 2 * g + 2 * xx + (z & 1)
            out[orow] = acc[:, z * cout:(z + 1) * cout] + b.double()
        assert (out - ref).abs().max() < 1e-5, name


def test_prompt_assembly_numpy_equals_the_reference_formulation():
    """SamPt._prepare_points on numpy inputs (the fused path converts once per clip) against the reference's per-item torch
    formulation (sam_pt.py:726-758): own visible points, tail points negative, the other objects' visible positives
    appended object by object as negatives."""
    from sam_pt_amd.sam_pt import SamPt
    for nm, npos, nneg in [(1, 8, 0), (5, 16, 0), (3, 8, 2), (2, 4, 4)]:
        m = SamPt.__new__(SamPt)
        m.positive_points_per_mask, m.negative_points_per_mask = npos, nneg
        m.add_other_objects_positive_points_as_negative_points, m.max_other_objects_positive_points = True, None
        g = torch.Generator().manual_seed(nm * 10 + npos)
        traj = torch.rand(6, nm, npos + nneg, 2, generator=g) * 500
        vis = (torch.rand(6, nm, npos + nneg, generator=g) > 0.3).float()
        tn, vn = traj.numpy(), (vis == 1).numpy()
        for t in range(6):
            for o in range(nm):
                pl = np.ones(npos + nneg, dtype=int)
                pl[npos:] = 0
                vm = (vis[t, o] == 1).numpy()
                c_ref, l_ref = traj[t, o].numpy()[vm], pl[vm]
                if nm > 1:
                    oth = torch.cat([traj[t, q, :npos][vis[t, q, :npos] == 1] for q in range(nm) if q != o]).numpy()
                    c_ref, l_ref = np.concatenate([c_ref, oth]), np.concatenate([l_ref, np.zeros(len(oth), dtype=int)])
                for args in ((tn, vn), (traj, vis)):                       # numpy fast path and the tensor entry
                    c, l = m._prepare_points(args[0], args[1], t, o, nm)
                    assert np.array_equal(c, c_ref) and np.array_equal(l, l_ref)


def test_sharding_helpers():
    from sam_pt_amd.dist import frame_batches, index_masks, lpt_assign
    lengths = [104, 34, 50, 80, 69, 40, 90, 75, 60, 45]
    parts = lpt_assign(lengths, 4)
    assert sorted(i for p in parts for i in p) == list(range(10))
    loads = [sum(lengths[i] for i in p) for p in parts]
    assert max(loads) - min(loads) <= max(lengths)
    fb = [frame_batches(50, 4, r, 8) for r in range(4)]
    assert sorted(t for r in fb for b in r for t in b) == list(range(50))
    logits = torch.full((2, 3, 4, 5), -1.0)
    logits[1, :, 1, 2] = 3.0
    m = index_masks(logits)
    assert m.dtype == torch.uint8 and m[:, 1, 2].tolist() == [2, 2, 2] and int(m.sum()) == 6


def test_gather_masks_two_ranks_gloo():
    """The N > 1 path of bench.py (sequence sharding + final uint8 mask gather) with 2 processes on the gloo backend."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from sam_pt_amd.dist import init_from_env, gather_masks, lpt_assign
rank, world, local = init_from_env("gloo")
assert world == 2
mine = lpt_assign([5, 3, 4, 2], world)[rank]
T = 2 + rank
masks = torch.full((T, 4, 6), rank + 1, dtype=torch.uint8)
out = gather_masks(masks, max_frames=3)
if rank == 0:
    assert out.shape == (2, 3, 4, 6)
    assert out[0, :2].eq(1).all() and out[0, 2].eq(0).all() and out[1].eq(2).all()
    print("GATHER_OK", mine)
else:
    assert out is None
dist.barrier(); dist.destroy_process_group()
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import tempfile  # torch.distributed.run needs a script file
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=240)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "GATHER_OK" in r.stdout


def test_pipelined_step_loop_two_ranks_gloo():
    """bench.py's pipelined step loop (ClipsInFlight: submit clip i + 1, then collect clip i with the VOS tail and the mask
    gather) with 2 gloo processes: every rank issues its gathers in the same order, rank 0 receives each step's masks of
    both ranks, nothing is left in flight at the closing barrier."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
import bench
from sam_pt_amd.dist import init_from_env
rank, world, local = init_from_env("gloo")
assert world == 2

class FakeModel:
    device = torch.device("cpu")
    def forward_begin(self, step):
        return step
    def forward_end(self, step):     # one object, 2 frames; rank r, step s marks pixel (r, s) as foreground
        logits = torch.full((1, 2, 3, 5), -4.0)
        logits[0, :, rank, step] = 4.0
        return {"logits": [logits[0]]}

seen = []
orig = bench.consume
def spy(model, out, max_frames):
    masks, gathered = orig(model, out, max_frames)
    seen.append(None if gathered is None else gathered.clone())
    return masks, gathered
bench.consume = spy
flight = bench.ClipsInFlight(FakeModel(), 2)
for s in range(4):
    flight.submit(s)
last = flight.flush()
dist.barrier()
assert flight.pending is None and len(seen) == 4 and int(last[0, rank, 3]) == 1
if rank == 0:
    for s, g in enumerate(seen):
        assert g.shape == (2, 2, 3, 5)
        for r in range(2):
            want = torch.zeros(2, 3, 5, dtype=torch.uint8); want[:, r, s] = 1
            assert torch.equal(g[r], want), (s, r)
    print("PIPELINED_GATHER_OK")
else:
    assert all(g is None for g in seen)
dist.destroy_process_group()
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=240)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "PIPELINED_GATHER_OK" in r.stdout


def test_vos_index_masks_formula_matches_the_evaluator():
    """dist.index_masks with query-frame overrides == the reference evaluator's sequence (vos_eval/eval.py:304-326)."""
    from sam_pt_amd.dist import index_masks
    g = torch.Generator().manual_seed(5)
    M, T, H, W = 3, 5, 24, 40
    logits = torch.randn(M, T, H, W, generator=g) * 3
    qt = torch.tensor([0, 2, 4])
    gt = (torch.rand(M, H, W, generator=g) > 0.6).float()
    lg = torch.stack([torch.zeros(T, H, W)] + [l for l in logits], dim=1)        # (T, M+1, H, W), bg first
    for i, t in enumerate(qt):
        lg[:t, i + 1] = -1e8
    for i, t in enumerate(qt):
        lg[t, i + 1] = torch.where(gt[i].bool(), 1e8, -1e8)
    ref = torch.softmax(lg, dim=1).argmax(dim=1).to(torch.uint8)
    assert torch.equal(ref, index_masks(logits, qt, gt))


def test_shi_tomasi_restatement_properties():
    """Shi-Tomasi point selection without OpenCV (parity unpinned: cv2 is absent): invariants of the restated algorithms —
    the min-eigenvalue map peaks on a corner and vanishes on flat areas and straight edges, erosion matches the square
    structuring element incl. OpenCV's empty-kernel default, selected corners lie inside the mask, are distinct, respect
    the minimum distance, and missing corners are topped up with k-medoid points."""
    import numpy as np
    from sam_pt_amd import query_points as Q
    from sam_pt_amd.synth import synthetic_clip
    img = np.zeros((40, 40), np.uint8)
    img[10:30, 10:30] = 200
    eig = Q.corner_min_eigen_val(img)
    assert eig[20, 20] == 0 and eig[5, 5] == 0                       # flat inside / outside
    assert eig[20, 10] < 1e-6 and eig[10, 20] < 1e-6                  # straight edges: one zero eigenvalue
    y, x = np.unravel_index(eig.argmax(), eig.shape)
    assert min(abs(y - 10), abs(y - 29)) <= 1 and min(abs(x - 10), abs(x - 29)) <= 1
    m = np.zeros((9, 9), np.uint8)
    m[2:7, 2:7] = 1
    assert [int(Q._erode(m, k).sum()) for k in (3, 2, 0, 1, 5)] == [9, 16, 9, 25, 1]
    assert Q._erode(np.ones((6, 6), np.uint8), 3).sum() == 36         # the image border never erodes
    frames, centres = synthetic_clip(T=1, H=128, W=256, seed=3)
    yy, xx = torch.meshgrid(torch.arange(128), torch.arange(256), indexing="ij")
    mask = (((xx - centres[0, 0]) ** 2 + (yy - centres[0, 1]) ** 2) <= 30 ** 2).float()
    torch.manual_seed(0)
    pts = Q.extract_corner_points(frames[0], mask, 8)
    assert pts.shape == (8, 2) and all(mask[int(py), int(px)] == 1 for px, py in pts)
    d = torch.cdist(pts, pts) + torch.eye(8) * 1e9
    eroded = Q.erode_mask_proportional_to_its_furthest_points_distance(mask, 0.06)
    px_ = eroded.nonzero().float()
    assert d.min() >= torch.norm(px_.max(0)[0] - px_.min(0)[0]).item() / 8 - 1e-4
    flat = torch.zeros(3, 128, 256, dtype=torch.uint8)                 # no texture -> no corners -> all k-medoid points
    torch.manual_seed(0)
    assert Q.extract_corner_points(flat, mask, 5).shape == (5, 2)
    mixed = Q.extract_mixed_points([mask, 1 - mask], torch.tensor([0.0, 0.0]), frames, 7)   # 1 + 2 + 4
    assert [tuple(p.shape) for p in mixed] == [(7, 2), (7, 2)]


def test_fused_host_logic_on_cpu_with_a_fake_device_predictor():
    """The device path of SamPt (clip-level encode, ONE ragged batched decode chain, skipped query-mask pass) is host
    logic too: drive it on the CPU with a predictor that implements ``encode_frames`` / ``track_decode`` on top of the
    oracle and compare with the reference call-by-call protocol — ragged prompts (different visible-point counts, an
    empty prompt, two-pass mode with negatives) included."""
    from oracle import sam_ref as R
    from sam_pt_amd.point_tracker import PointTracker
    from sam_pt_amd.sam_pt import SamPt
    from sam_pt_amd.synth import synthetic_clip
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    from tests.util import make_fake_device_predictor
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)

    class NoTracker(PointTracker):
        def forward(self, rgbs, query_points):
            raise AssertionError("not used")

    T, M = 4, 2
    frames, _ = synthetic_clip(T=T, H=128, W=256, seed=3)
    g = torch.Generator().manual_seed(7)
    for neg in (0, 1):
        P = 3 + neg
        traj = torch.rand(T, M, P, 2, generator=g) * torch.tensor([250.0, 120.0]) + 3.0
        vis = torch.ones(T, M, P)
        vis[1, 0, :] = 0                      # object 0 invisible in frame 1 (still gets object 1's positives as negatives)
        vis[2, 1, 1:] = 0                     # a single visible point
        vis[3, :, 0] = 0
        fake = make_fake_device_predictor(sd, cfg)
        fused = SamPt(NoTracker(), fake, sam_iou_threshold=0.0, positive_points_per_mask=3, negative_points_per_mask=neg,
                      iterative_refinement_iterations=2).eval()
        feats = fake.encode_frames(frames)
        _, l_f, s_f = fused._apply_sam_to_trajectories(frames, traj, vis, feats)
        ref = SamPt(NoTracker(), R.SamPredictorRef(sd, cfg), sam_iou_threshold=0.0, positive_points_per_mask=3,
                    negative_points_per_mask=neg, iterative_refinement_iterations=2).eval()
        _, l_s, s_s = ref._apply_sam_to_trajectories(frames, traj, vis, None)
        assert torch.equal(torch.isfinite(l_f), torch.isfinite(l_s))
        fin = torch.isfinite(l_s)
        assert (l_f[fin] - l_s[fin]).abs().max() < 1e-4 and torch.allclose(s_f, s_s, atol=1e-5)
        assert len(fake.calls) == 3 and any(c[3] for c in fake.calls)          # 8 items in chunks of 3, ragged batches


def test_frame_sharded_forward_two_ranks_gloo():
    """dist.sharded_forward (one clip, frame batches dealt over the ranks: BASELINE config #5) with 2 gloo processes on
    the CPU: rank 0's assembled index masks equal the single-process result; nothing but uint8 masks crosses ranks."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from oracle import pips_ref as PO
from sam_pt_amd.dist import init_from_env, sharded_forward, index_masks
from sam_pt_amd.point_tracker import PointTracker
from sam_pt_amd.sam_pt import SamPt
from sam_pt_amd.synth import disc_queries, synthetic_clip
from sam_pt_amd.weights import SAM_CONFIGS, init_pips_state_dict, init_sam_state_dict
from tests.util import make_fake_device_predictor
rank, world, local = init_from_env("gloo")
assert world == 2
torch.set_num_threads(4)
cfg = SAM_CONFIGS["vit_test"]
sd, psd = init_sam_state_dict(cfg, 72), init_pips_state_dict(72)
class OracleTracker(PointTracker):
    def forward(self, rgbs, query_points):
        return PO.PipsTrackerRef(psd).forward(rgbs.cpu(), query_points.cpu())
frames, centres = synthetic_clip(T=6, H=128, W=256, seed=72)
q = disc_queries(centres, n_pos=3, r=9.0)
video = {"image": [f for f in frames], "target_hw": (128, 256), "query_points": q[None]}
def model():
    return SamPt(OracleTracker(), make_fake_device_predictor(sd, cfg, 4), sam_iou_threshold=-1e9, positive_points_per_mask=3,
                 negative_points_per_mask=0, iterative_refinement_iterations=1).eval()
full, own = sharded_forward(model(), video, batch=2)          # batches {0,1},{4,5} -> rank 0 ; {2,3} -> rank 1
assert len(own["logits"][0]) == (4 if rank == 0 else 2) and own["trajectories"].shape[0] == 6
if rank == 0:
    ref = model()(video)
    want = index_masks(torch.stack(ref["logits"], dim=0))
    assert full.shape == want.shape and torch.equal(full, want) and int(want.sum()) > 0
    print("SHARDED_OK")
else:
    assert full is None
dist.barrier(); dist.destroy_process_group()
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=600)
    finally:
        os.unlink(path)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "SHARDED_OK" in r.stdout


def test_erosion_and_min_eigenvalue_map_against_scipy():
    """Independent pins of two pieces of the OpenCV restatement (cv2 itself is absent): ``_erode`` equals
    ``scipy.ndimage.binary_erosion`` with a k x k structuring element and border_value = 1 bit for bit (odd and even k: same anchor
    convention k // 2), and ``corner_min_eigen_val`` equals the textbook formula assembled from ``scipy.ndimage`` filters in fp64
    (Sobel with mode 'mirror' = BORDER_REFLECT_101, 3 x 3 box sum, smaller eigenvalue) to fp32 round-off."""
    import numpy as np
    import scipy.ndimage as ndi
    from sam_pt_amd import query_points as Q
    rng = np.random.default_rng(0)
    for k in (2, 3, 4, 5, 8, 11, 24):
        m = (rng.random((40, 57)) > 0.12).astype(np.uint8)
        m[:, :3] = 1
        assert np.array_equal(Q._erode(m, k), ndi.binary_erosion(m, structure=np.ones((k, k)), border_value=1).astype(np.uint8)), k
    g = rng.integers(0, 256, (50, 70)).astype(np.uint8)
    g[10:30, 20:50] = 180
    gf = g.astype(np.float64)
    scale = 1.0 / (4.0 * 3 * 255.0)
    dx = ndi.sobel(gf, axis=1, mode="mirror") * scale
    dy = ndi.sobel(gf, axis=0, mode="mirror") * scale
    box = lambda a: ndi.uniform_filter(a, size=3, mode="mirror") * 9.0
    a, b, c = box(dx * dx) * 0.5, box(dx * dy), box(dy * dy) * 0.5
    want = (a + c) - np.sqrt((a - c) ** 2 + b * b)
    got = Q.corner_min_eigen_val(g).astype(np.float64)
    assert np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), np.abs(got - want).max()


KMEDOIDS_GOLDEN = [[10, 24, 27], [32, 42, 95, 100, 126, 202, 205, 216], [241, 263, 684, 842, 888, 1301, 1478, 1524],
                   [84, 141, 186, 271, 275, 358, 410, 475, 497, 528, 558, 599, 700, 740, 783, 786]]


def test_kmedoids_host_restatement_golden():
    """the device k-medoids is bit-identical to ``kmedoids_alternate`` by GPU tests only, and that identity leans on
    numpy internals (pairwise summation, argpartition's introselect order).  Fixed point sets with their medoids written down: a
    numpy upgrade that changes either shows up here, on the CPU."""
    import numpy as np
    from sam_pt_amd.query_points import kmedoids_alternate
    rng = np.random.default_rng(1234)
    got = []
    for n, K in ((40, 3), (257, 8), (1800, 8), (900, 16)):
        pts = np.unique(rng.integers(0, 200, (n, 2)), axis=0).astype(np.float32)
        got.append(sorted(int(i) for i in kmedoids_alternate(pts, K)))
    want = KMEDOIDS_GOLDEN
    assert got == want, got


def test_vit_bias_correction_removes_the_token_mean_of_the_weight_rounding_error():
    """pack.vit_bias_correction (the host half of the fp16 ViT mode's static bias correction): with b' = b + (W - fp16(W)) . abar the
    fp16-weight GEMM's output error has ZERO mean over any token set whose column means equal abar — for all four GEMMs of a block,
    algebraically, whatever the tokens are; and the per-token error shrinks when the tokens share a common component."""
    from sam_pt_amd.pack import VIT_GEMM_KINDS, vit_bias_correction
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    D, ld = cfg.embed_dim, cfg.mlp_ratio * cfg.embed_dim
    g = torch.Generator().manual_seed(3)
    abar = torch.zeros(cfg.depth, 4, ld)
    tokens = {}
    for i in range(cfg.depth):
        for kind, mod in enumerate(VIT_GEMM_KINDS):
            K = ld if mod == "mlp.lin2" else D
            common = torch.randn(K, generator=g) * 2.0                       # what every token shares (LayerNorm bias, outlier channels)
            A = (common + 0.3 * torch.randn(200, K, generator=g)).half().float()
            tokens[(i, kind)] = A
            abar[i, kind, :K] = A.double().mean(0).float()
    corr = vit_bias_correction(sd, cfg, abar)
    for i in range(cfg.depth):
        for kind, mod in enumerate(VIT_GEMM_KINDS):
            name = f"image_encoder.blocks.{i}.{mod}"
            W, b = sd[name + ".weight"].double().reshape(-1, tokens[(i, kind)].shape[1]), sd[name + ".bias"].double()
            A = tokens[(i, kind)].double()
            exact = A @ W.t() + b
            plain = A @ W.float().half().double().t() + b
            fixed = A @ W.float().half().double().t() + corr[name + ".bias"].double()
            assert (fixed - exact).mean(0).abs().max() < 1e-6 * exact.abs().max()                 # fp32 rounding of b' only
            assert (plain - exact).mean(0).abs().max() > 20 * (fixed - exact).mean(0).abs().max()
            assert (fixed - exact).pow(2).mean() < 0.5 * (plain - exact).pow(2).mean(), (i, mod)
            assert corr[name + ".bias"].dtype == torch.float32 and corr[name + ".bias"].shape == sd[name + ".bias"].shape


def test_fnet_shard_is_enabled_only_when_every_rank_owns_a_frame_batch():
    """the pyramid all_gather is entered from inside model(...), which a rank without a frame batch never calls.
    ``fnet_shard_usable`` is a pure function of (T, world, batch) — every rank reaches the same verdict — and is False for
    exactly the clip lengths that leave ranks idle (the advisor's list for 8 and 4 ranks)."""
    from sam_pt_amd.dist import fnet_shard_usable, frame_batches

    def usable(T, world):
        batch = max(1, min(8, -(-T // world)))                      # sharded_forward's batch rule
        return fnet_shard_usable(T, world, batch), batch

    idle8 = {1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 17, 18, 19, 20, 21, 25, 26, 27, 28, 33, 34, 35, 41, 42, 49}
    idle4 = {1, 2, 3, 5, 6, 9}
    for world, idle in ((8, idle8), (4, idle4)):
        for T in range(1, 70):
            ok, batch = usable(T, world)
            has_idle = any(not frame_batches(T, world, k, batch) for k in range(world))
            assert ok == (not has_idle)
            assert (T in idle) == has_idle, (T, world)
    assert usable(24, 8)[0] and usable(64, 8)[0] and not usable(9, 8)[0]


def test_frame_sharded_forward_with_an_idle_rank_three_ranks_gloo():
    """T = 2 frames over 3 ranks with ``shard_fnet=True``: rank 2 owns no frame batch and only joins the mask gather.  The job must
    complete (before the fix the other ranks would wait for it in the pyramid all_gather) and no rank may have been handed a
    FnetShard; rank 0's masks equal the single-process result."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from sam_pt_amd.dist import init_from_env, sharded_forward
rank, world, local = init_from_env("gloo")
assert world == 3
torch.set_num_threads(2)
T, H, W = 2, 8, 12
seen = []
class Model:
    device = torch.device("cpu")
    def __call__(self, video):
        seen.append("fnet_shard" in video)
        ids = video["frame_ids"]
        g = torch.Generator().manual_seed(5)
        full = torch.randn(2, T, H, W, generator=g)
        return {"logits": [full[m, ids] for m in range(2)], "trajectories": torch.zeros(T, 2, 1, 2)}
video = {"image": [torch.zeros(3, H, W, dtype=torch.uint8) for _ in range(T)], "target_hw": (H, W)}
full, own = sharded_forward(Model(), video, batch=8, shard_fnet=True)
assert seen == ([False] if rank < 2 else []), seen          # ranks 0 and 1 run one frame each without a FnetShard; rank 2 is idle
if rank == 0:
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(2, T, H, W, generator=g)
    want = torch.cat([torch.zeros(1, T, H, W), lg]).softmax(0).argmax(0).to(torch.uint8)
    assert torch.equal(full, want)
    print("IDLE_RANK_OK")
dist.barrier(); dist.destroy_process_group()
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=300)
    finally:
        os.unlink(path)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "IDLE_RANK_OK" in r.stdout


def test_pil_bilinear_tables_bit_exact_against_pil():
    """The fixed-point tables behind the device resize of SamPredictor.set_image reproduce PIL.Image.resize(BILINEAR)
    bit for bit (numpy evaluation of the same integer arithmetic the HIP kernel runs), up- and down-scaling."""
    from PIL import Image
    from sam_pt_amd.sam_predictor import pil_bilinear_tables

    def axis(img, out, ax):
        img = np.moveaxis(img, ax, 0)
        coef, bounds = pil_bilinear_tables(img.shape[0], out)
        res = np.empty((out,) + img.shape[1:], np.uint8)
        for xx in range(out):
            x0, n = bounds[xx]
            acc = np.full(img.shape[1:], 1 << 21, np.int64)
            for x in range(n):
                acc += img[x0 + x].astype(np.int64) * int(coef[xx, x])
            res[xx] = np.clip(acc >> 22, 0, 255)
        return np.moveaxis(res, 0, ax)

    rng = np.random.default_rng(0)
    for h, w, oh, ow in [(48, 85, 58, 102), (120, 64, 90, 48), (37, 53, 37, 106), (60, 107, 144, 256)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        got = axis(axis(img, ow, 1) if ow != w else img, oh, 0) if oh != h else axis(img, ow, 1)
        assert np.array_equal(ref, got), (h, w, oh, ow)


def test_c_abi_error_behaviour_without_a_gpu():
    """Handle creation only records pointers, so the C ABI's argument / weight-table validation is testable on the CPU
    (no kernel is launched): negative return codes, a message in sampt_last_error(), nothing thrown, no handle leaked."""
    import ctypes as C
    from sam_pt_amd import _lib
    from sam_pt_amd.pack import pack_decoder, pack_pips, pack_pips2
    from sam_pt_amd.weights import SAM_CONFIGS, init_pips2_state_dict, init_pips_state_dict, init_sam_state_dict
    lib = _lib.load()
    assert lib.sampt_version() >= 1

    def last():
        return lib.sampt_last_error().decode()

    w = pack_pips(init_pips_state_dict(72), "cpu")
    names, ptrs, n = _lib.name_table(w)
    h = C.c_void_p()
    assert lib.sampt_pips_create(names, ptrs, n, 4, 8, C.byref(h)) == 0 and h.value
    lib.sampt_pips_destroy(h)
    assert lib.sampt_pips_create(names, ptrs, n, 4, 7, C.byref(h)) < 0 and "S must be 8" in last()
    w.pop("fnet.conv2.weight"), w.pop("vis_predictor.0.bias")
    names, ptrs, n = _lib.name_table(w)
    assert lib.sampt_pips_create(names, ptrs, n, 4, 8, C.byref(h)) < 0 and "fnet.conv2.weight" in last()
    w2 = pack_pips2(init_pips2_state_dict(72), "cpu")
    w2.pop("delta_block.dense.weight")
    names, ptrs, n = _lib.name_table(w2)
    assert lib.sampt_pips2_create(names, ptrs, n, 8, C.byref(h)) < 0 and "delta_block.dense.weight" in last()
    cfg = SAM_CONFIGS["vit_test"]
    wd = pack_decoder(init_sam_state_dict(cfg, 72), cfg, "cpu", 2)           # plain SAM weights ...
    names, ptrs, n = _lib.name_table(wd)
    assert lib.sampt_dec_create(names, ptrs, n, cfg.grid, cfg.img_size, 2, 0, C.byref(h)) == 0
    nb = C.c_size_t()
    assert lib.sampt_dec_workspace_bytes(h, 2, 128, 256, C.byref(nb)) == 0 and nb.value > 0       # dry run: sizes only
    assert lib.sampt_dec_workspace_bytes(h, 3, 128, 256, C.byref(nb)) < 0                          # beyond max_frames
    assert lib.sampt_dec_hq_workspace_bytes(h, 1, C.byref(nb)) < 0 and "HQ-SAM" in last()
    lib.sampt_dec_destroy(h)
    assert lib.sampt_dec_create(names, ptrs, n, cfg.grid, cfg.img_size, 2, cfg.embed_dim, C.byref(h)) < 0   # ... lack HQ keys
    assert "hf_token" in last() or "hf_mlp" in last()
    with pytest.raises(_lib.SamptError):
        _lib.check(-1, "context")


def test_x3_entry_points_refuse_bad_pointers_without_a_gpu():
    """sampt_gemm_x3_rows_epi (epi != 0) and sampt_conv3x3_planes_instnorm_stats dispatch to gemm_x3_wres / conv3x3_halo_x3
    themselves, so they make conv_f16x3's operand checks (x3_args_check) and their own before anything is launched: a NULL or
    misaligned pointer is SAMPT_ERR_ARG with a message, an unsupported shape stays SAMPT_ERR_UNSUPPORTED, a short workspace
    SAMPT_ERR_WORKSPACE.  Nothing is dereferenced before the checks, so made-up addresses stand in for device pointers."""
    from sam_pt_amd import _lib
    lib = _lib.load()
    ARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    base = 0x7F0000000000                      # 16-byte aligned "buffers", 1 MiB apart
    A, WHL, BIAS, RES, C_, EA, EB, MR, WS = (base + (i << 20) for i in range(9))

    def refused(call, good, slot, bad):
        args = list(good)
        args[slot] = bad
        lib.sampt_pips_set_mixer(9, 0)         # (leaves a known message behind: the next one must replace it)
        assert "sampt_pips_set_mixer" in lib.sampt_last_error().decode()
        rc = call(*args)
        msg = lib.sampt_last_error().decode()
        return rc, (msg if "sampt_pips_set_mixer" not in msg else "")

    # A, w_hl, bias, res, res_mod, C, M, N, K, act, shuf_g, epi, epi_a, epi_b, eps, epi_ld, stream: the shapes of
    # test_gemm_x3_rows_fused_upscaling_tails (epi = 1) and test_gemm_x3_rows_fused_layernorm_tail (epi = 3)
    tails = {1: [A, WHL, BIAS, None, 0, C_, 4 * 4096, 256, 256, 2, 64, 1, EA, EB, 1e-6, 0, None],
             3: [A, WHL, BIAS, C_, 0, C_, 5 * 4096 + 5, 256, 128, 0, 0, 3, EA, EB, 1e-5, 0, None]}
    for epi, good in tails.items():
        # A, w_hl and C are read / written 16 bytes at a time: + 4 is misaligned.  The tail vectors are read one float at a time
        # (k_gemm_x3_wres, k_gemm_x3_wres_ln), so a 4-byte aligned epi_a is legal: its bad address has bits 1 and 2 set
        for slot, off in ((0, 4), (1, 4), (5, 4), (12, 6)):
            for bad in (None, good[slot] + off):
                rc, msg = refused(lib.sampt_gemm_x3_rows_epi, good, slot, bad)
                assert rc == ARG and "sampt_gemm_x3_rows_epi" in msg, (epi, slot, bad, rc, msg)
        rc, msg = refused(lib.sampt_gemm_x3_rows_epi, good, 13, None)             # both tails read epi_b too
        assert rc == ARG and msg
        rc, msg = refused(lib.sampt_gemm_x3_rows_epi, good, 7, 128 if epi == 1 else 512)      # N the tail does not take
        assert rc == UNSUPPORTED and "fused tail" in msg, (epi, rc, msg)

    # x_hl, w_hl, bias, y, n, H, W, Cin, Cout, eps, mean_rstd, ws, ws_bytes, stream: test_conv3x3_fused_instnorm_statistics' first shape
    n, H, W, Cin, Cout = 2, 32, 48, 64, 64
    need = n * ((H + 15) // 16) * ((W + 15) // 16) * Cout * 2 * 8
    good = [A, WHL, BIAS, C_, n, H, W, Cin, Cout, 1e-5, MR, WS, need, None]
    for slot in (0, 1, 3, 11):
        for bad in (None, good[slot] + 4):                                         # (ws holds doubles: + 4 is misaligned for it too)
            rc, msg = refused(lib.sampt_conv3x3_planes_instnorm_stats, good, slot, bad)
            assert rc == ARG and "sampt_conv3x3_planes_instnorm_stats" in msg, (slot, bad, rc, msg)
    rc, msg = refused(lib.sampt_conv3x3_planes_instnorm_stats, good, 10, None)
    assert rc == ARG and msg
    assert refused(lib.sampt_conv3x3_planes_instnorm_stats, good, 12, need - 1)[0] == WORKSPACE
    assert refused(lib.sampt_conv3x3_planes_instnorm_stats, good, 7, 48)[0] == UNSUPPORTED      # Cin % 32
    # the stem's statistics workspace, same rule (x, w, bias, y, n, H, W, eps, mean_rstd, ws, ws_bytes, stream)
    stem = [A, WHL, BIAS, C_, 1, 32, 32, 1e-5, MR, WS, 1 << 20, None]
    for bad in (None, WS + 4):
        rc, msg = refused(lib.sampt_conv_stem7x7, stem, 9, bad)
        assert rc == ARG and "sampt_conv_stem7x7" in msg
    assert refused(lib.sampt_conv_stem7x7, stem, 10, 8)[0] == WORKSPACE


def test_device_once_host_program_under_thread_sanitizer(tmp_path):
    """DeviceOnce (csrc/dyn_lds.h: which devices a kernel's dynamic-LDS limit has been raised on) alone, as a host program of its
    own (tests/device_once_main.cpp) built with the host compiler and -fsanitize=thread: 8 threads over 4 ordinals, the callable
    succeeds once per ordinal, a failed first call is tried again, an ordinal outside the table runs it every time."""
    import shutil
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "device_once")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", os.path.join(ROOT, "tests", "device_once_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "device_once: ok" in run.stdout, run.stdout + run.stderr
    assert "ThreadSanitizer" not in run.stderr


def test_split_f16x3_weights_and_per_tracker_default(monkeypatch):
    """Host side of csrc/conv_f16x3.hip: hi + lo reproduces w * 2^8 to fp32 precision (absolute error far below one fp32
    ulp of the layer's largest weight), out-of-range weights are refused, and the split planes are packed for PIPS by
    default, for PIPS++ only on request (SAMPT_FNET_F16X3 overrides both)."""
    from sam_pt_amd.pack import F16X3_WSHIFT, pack_pips, pack_pips2, split_f16x3
    from sam_pt_amd.weights import init_pips2_state_dict, init_pips_state_dict
    g = torch.Generator().manual_seed(3)
    w = torch.randn(96, 864, generator=g) * 0.05
    w[0, 0], w[0, 1], w[0, 2] = 3e-7, 180.0, -1.0
    hl = split_f16x3(w)
    assert hl.dtype == torch.float16 and hl.shape == (2, 96, 864)
    rec = (hl[0].double() + hl[1].double()) / 2 ** F16X3_WSHIFT
    err = (rec - w.double()).abs()
    assert (err <= 2.0 ** -22 * w.double().abs() + 2.0 ** -33).all()
    with pytest.raises(ValueError):
        split_f16x3(torch.full((4, 32), 300.0))
    monkeypatch.delenv("SAMPT_FNET_F16X3", raising=False)
    sd1, sd2 = init_pips_state_dict(72), init_pips2_state_dict(72)
    p1 = pack_pips(sd1, "cpu")
    hl_keys = sorted(k for k in p1 if k.endswith(".weight_hl"))
    assert len(hl_keys) == 21 and "fnet.conv1.weight_hl" not in p1            # every conv but the 3-channel stem
    assert p1["fnet.conv2.weight_hl"].shape == (2, 256, 9 * 416)
    assert not any(k.endswith("_hl") for k in pack_pips2(sd2, "cpu"))
    monkeypatch.setenv("SAMPT_FNET_F16X3", "0")
    assert not any(k.endswith("_hl") for k in pack_pips(sd1, "cpu"))
    monkeypatch.setenv("SAMPT_FNET_F16X3", "1")
    assert sum(k.endswith("_hl") for k in pack_pips2(sd2, "cpu")) == 21


def test_predict_torch_batched_prompts_host_logic(monkeypatch):
    """``SamPredictor.predict_torch`` with upstream's batch dimension (B prompts against the current image, as the
    automatic mask generator issues them): every prompt becomes one C-ABI decode call with its own contiguous buffers and
    its outputs land in row b.  Runs against a recording stand-in for the library (no GPU, no arithmetic)."""
    import types
    from sam_pt_amd import _lib, sam_predictor as SP
    calls = []

    class FakeLib:
        def sampt_sam_decode_multimask(self, dec, feat, p, l, k, bx, mb, ih, iw, oh, ow, lg, io, lw, ws, n, stream):
            calls.append(("multi", tuple(p.shape), tuple(l.shape), k, bx is None, mb is None, tuple(lg.shape)))
            lg.fill_(float(p[0, 0])), io.fill_(float(p[0, 1])), lw.fill_(float(l[0]))
            return 0

        def sampt_sam_decode(self, dec, feat, hq, p, l, k, bx, mb, ih, iw, oh, ow, lg, io, lw, ws, n, stream):
            calls.append(("single", tuple(p.shape), tuple(l.shape), k, None if bx is None else bx.tolist(),
                          None if mb is None else float(mb[0, 0]), tuple(lg.shape)))
            lg.fill_(float(p[-1, 0])), io.fill_(float(p[-1, 1])), lw.fill_(0.0)
            return 0

    def fake_ptr(t):
        assert t is None or t.is_contiguous()
        return t

    monkeypatch.setattr(_lib, "ptr", fake_ptr)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    cfg = types.SimpleNamespace(grid=4, img_size=64, out_chans=256)
    model = types.SimpleNamespace(cfg=cfg, hq=False, mask_threshold=0.0, device=torch.device("cpu"), image_format="RGB")
    pred = SP.SamPredictor(model)
    pred._ensure = lambda: None
    pred._dev, pred._lib, pred._dec = torch.device("cpu"), FakeLib(), object()
    monkeypatch.setattr(pred, "_dec_ws", lambda oh, ow, frames=1, k=0: torch.zeros(16, dtype=torch.uint8))
    pred.set_features(torch.zeros(16, 256), (20, 30), (40, 60))
    assert pred.device == torch.device("cpu")
    B = 5
    pc = torch.arange(B * 2, dtype=torch.float64).reshape(B, 1, 2)            # prompt b = point (2b, 2b+1)
    pl = torch.ones(B, 1, dtype=torch.int64)
    logits, iou, low = pred.predict_torch(pc, pl, multimask_output=True, return_logits=True)
    assert logits.shape == (B, 3, 20, 30) and iou.shape == (B, 3) and low.shape == (B, 3, 16, 16)
    assert len(calls) == B and all(c == ("multi", (1, 2), (1,), 1, True, True, (3, 20, 30)) for c in calls)
    for b in range(B):
        assert bool((logits[b] == 2 * b).all()) and bool((iou[b] == 2 * b + 1).all()) and bool((low[b] == 1).all())
    assert pred.stats["predict"] == B
    calls.clear()
    pc2 = torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0]]])
    boxes = torch.tensor([[[0.0, 1.0, 2.0, 3.0]], [[4.0, 5.0, 6.0, 7.0]]])
    mi = torch.stack([torch.full((1, 16, 16), 0.25), torch.full((1, 16, 16), 0.75)])
    masks, iou, low = pred.predict_torch(pc2, torch.ones(2, 2, dtype=torch.int), boxes=boxes, mask_input=mi,
                                         multimask_output=False, return_logits=False)
    assert masks.dtype == torch.bool and masks.shape == (2, 1, 20, 30) and bool(masks.all())
    assert calls == [("single", (2, 2), (2,), 2, [0.0, 1.0, 2.0, 3.0], 0.25, (1, 20, 30)),
                     ("single", (2, 2), (2,), 2, [4.0, 5.0, 6.0, 7.0], 0.75, (1, 20, 30))]
    assert iou[:, 0].tolist() == [4.0, 8.0]
    calls.clear()                                                              # B = 1 keeps the direct (copy-free) path
    m1, _, _ = pred.predict_torch(pc2[:1], torch.ones(1, 2, dtype=torch.int), boxes=boxes[:1], multimask_output=False,
                                  return_logits=True)
    assert len(calls) == 1 and m1.shape == (1, 1, 20, 30) and bool((m1 == 3.0).all())


def test_f16x3_scheme_is_fp32_grade():
    """The arithmetic behind csrc/conv_f16x3.hip, emulated on the CPU: x = hi + lo in fp16 for both operands (weights
    pre-scaled by 2^8), product = hi*hi + hi*lo + lo*hi with exact products and wide accumulation.  Its distance to the
    fp64 convolution is below that of a plain fp32 convolution, for O(1) post-InstanceNorm activations and Kaiming-sized
    weights (the encoder's regime), including a 416-channel 3x3 layer (K = 3744)."""
    import torch.nn.functional as F
    from sam_pt_amd.pack import F16X3_WSHIFT, split_f16x3
    g = torch.Generator().manual_seed(0)
    for cin, cout, k in ((64, 64, 3), (416, 256, 3), (96, 128, 1)):
        x = torch.relu(torch.randn(1, cin, 24, 24, generator=g)) * 1.3
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5
        ref = F.conv2d(x.double(), w.double(), padding=k // 2)
        f32 = F.conv2d(x, w, padding=k // 2).double()
        xh = x.half()
        xl = (x - xh.float()).half()
        whl = split_f16x3(w.reshape(cout, -1)).reshape(2, cout, cin, k, k)
        conv = lambda a, b: F.conv2d(a.double(), b.double(), padding=k // 2)
        y3 = (conv(xl, whl[0]) + conv(xh, whl[1]) + conv(xh, whl[0])) / 2 ** F16X3_WSHIFT
        err = lambda a: float((a - ref).abs().max() / ref.abs().max())
        assert err(y3) < 2e-7 and err(y3) < err(f32), (cin, err(y3), err(f32))


def test_bench_clips_in_flight_accounting(monkeypatch):
    """bench.py's pipelined step loop: K ``submit`` calls + one ``flush`` begin K clips and collect K clips, each clip is
    collected only after the NEXT one was submitted, and nothing stays in flight after the flush (the contract's "exactly K
    steps inside the timed region")."""
    import importlib
    import sys
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
    bench = importlib.import_module("bench")
    log = []

    class FakeModel:
        def forward_begin(self, video):
            log.append(("begin", video))
            return video

        def forward_end(self, handle):
            log.append(("end", handle))
            return {"id": handle}

    monkeypatch.setattr(bench, "consume", lambda model, out, max_frames: (out["id"], None))
    flight = bench.ClipsInFlight(FakeModel(), 24)
    assert flight.flush() is None and log == []                 # nothing in flight: a no-op
    got = [flight.submit(i) for i in range(4)]
    assert got == [None, 0, 1, 2]                                # submit(i) returns the masks of clip i - 1
    assert flight.flush() == 3 and flight.pending is None
    assert log == [("begin", 0), ("begin", 1), ("end", 0), ("begin", 2), ("end", 1), ("begin", 3), ("end", 2), ("end", 3)]
    assert flight.flush() == 3 and len(log) == 8                 # idempotent


def test_captured_decode_chain_is_kernel_nodes_only():
    """Source-level guard for the round-3 finding: a memset / memcpy NODE of a replayed hipGraph is not
    ordered with the kernel nodes around it on ROCm 7.2, so nothing that sampt_sam_track_decode_graph captures may issue
    one.  DecEngine::track_decode must not call hipMemset* / hipMemcpy* at all; DecEngine::decode only inside its
    multimask branch (never active on the captured path: the flag is set and cleared inside sampt_sam_decode_multimask)."""
    import re
    src = open(os.path.join(ROOT, "sam_pt_amd", "csrc", "engine_dec.hip")).read()
    body = src[src.index("int DecEngine::track_decode("):]
    assert not re.search(r"hipMem(set|cpy)\w*\(", body), "track_decode issues a memset / memcpy: it would become a graph node"
    dec = src[src.index("int DecEngine::decode("):src.index("int DecEngine::track_decode(")]
    calls = [m.start() for m in re.finditer(r"hipMem(set|cpy)\w*\(", dec)]
    assert len(calls) <= 1
    if calls:                                                     # the one copy sits inside `if (multimask) { ... }`
        lo = dec.index("if (multimask) {")
        assert lo < calls[0] < dec.index("hypernetwork MLP of mask token 0", lo)
    cabi = open(os.path.join(ROOT, "sam_pt_amd", "csrc", "c_abi.hip")).read()
    assert cabi.count("h->e.multimask = true") == 1 and cabi.count("h->e.multimask = false") == 1


def test_gelu_polynomial_header_matches_erf_gelu():
    """csrc/gelu_poly.h (the transcendental-free GELU of the fp16 GEMM epilogue) is what tools/gelu_poly_fit.py generates, and
    its fp32 Horner evaluation stays within 4e-6 of the erf GELU (torch.nn.GELU default, the activation of SAM's MLPBlock)
    everywhere — the fp16 rounding of the stored value is 1.2e-4 at |gelu| = 0.25."""
    import importlib.util
    import re
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gelu_poly_fit", os.path.join(root, "tools", "gelu_poly_fit.py"))
    fit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit)
    hdr = open(os.path.join(root, "sam_pt_amd", "csrc", "gelu_poly.h")).read()
    coefs = [float(c.rstrip("f")) for c in re.search(r"GELU_POLY_COEFS \{(.*)\}", hdr).group(1).split(", ")]
    assert len(coefs) == int(re.search(r"GELU_POLY_DEG (\d+)", hdr).group(1)) + 1
    assert float(re.search(r"GELU_POLY_C ([0-9.]+)f", hdr).group(1)) == fit.C
    x = np.concatenate([np.linspace(-12, 12, 240001), np.linspace(-1e-3, 1e-3, 2001)])
    ref = torch.nn.functional.gelu(torch.from_numpy(x)).numpy()
    assert np.abs(fit.gelu_poly_f32(x, np.array(coefs)) - ref).max() < 4e-6
    assert np.allclose(fit.fit(), coefs, rtol=0, atol=5e-7), "gelu_poly.h is stale: regenerate with tools/gelu_poly_fit.py"


def test_fnet_shard_pyramid_all_gather_two_ranks_gloo():
    """dist.FnetShard (the exchange step of the in-clip multi-GPU mode): 2 gloo processes each "encode" their share of a
    5-frame clip (uneven shares: 3 + 2, padded to 3 + 3) into a 4-level pyramid and all_gather it; every rank ends up with the
    pyramid a single process computes, bit for bit.  The emulation mode (one process standing in for rank r of N) fills the
    same buffers through its compute callback."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from sam_pt_amd.dist import FnetShard, frame_shares, init_from_env
rank, world, local = init_from_env("gloo")
assert world == 2
T = 5
def level(l, lo, hi):                     # the "encoder": frame t of level l is a deterministic function of (t, l)
    h, w = 8 >> l, 12 >> l
    t = torch.arange(lo, hi, dtype=torch.float32).view(-1, 1, 1, 1)
    return (t * 1000 + l * 100 + torch.arange(h * w * 4, dtype=torch.float32).view(1, h, w, 4)).contiguous()
want = [level(l, 0, T) for l in range(3)]
fs = FnetShard(rank, world)
assert [list(r) for r in frame_shares(T, world)] == [[0, 1, 2], [3, 4]] and fs.padded_frames(T) == 6
pyr = [torch.full((fs.padded_frames(T), 8 >> l, 12 >> l, 4), -1.0) for l in range(3)]
mine = fs.mine(T)
for l in range(3):
    pyr[l][mine.start:mine.stop] = level(l, mine.start, mine.stop)
fs.exchange(pyr, T)
assert all(torch.equal(p[:T], w) for p, w in zip(pyr, want)), rank
assert fs.bytes_received == sum(w[0].numel() * 4 * (T - len(mine)) for w in want)
dist.barrier(); dist.destroy_process_group()
print("PYRAMID_OK", rank)
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=300)
    finally:
        os.unlink(path)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("PYRAMID_OK") == 2


def test_x3_rows_packing_and_vit_pack_modes():
    """pack.x3_rows (the operand format of the split-fp16 GEMM / attention kernels, csrc/common.h GemmP::x3): hi + lo reproduces the
    fp32 value to 2^-22, blocks of 32 k are laid out hi(32) | lo(32), out-of-range magnitudes saturate into lo; and pack_vit emits
    the per-mode keys the engine looks up (".f16" / ".x3" GEMM weights, the qkv bias as one row of the qkv matrix's format)."""
    from sam_pt_amd.pack import F16X3_WSHIFT, pack_vit, x3_rows, x3_unrows
    from sam_pt_amd.weights import SAM_CONFIGS, init_sam_state_dict
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 96, generator=g) * 3
    x[0, 0], x[1, 33], x[2, 64] = 1.0e5, -1.2e5, 3e-7
    y = x3_rows(x)
    assert y.shape == (7, 192) and y.dtype == torch.float16
    assert torch.equal(y[:, 0:32], x[:, 0:32].clamp(-65504, 65504).half())            # block 0: hi
    assert torch.equal(y[:, 64:96], x[:, 32:64].clamp(-65504, 65504).half())          # block 1 starts at 64
    back = x3_unrows(y)
    # 2^-22 relative for values whose lo piece is a normal fp16 number; an absolute floor of one fp16 subnormal quantum (6e-8) below
    assert bool(((back - x).abs() <= torch.maximum(x.abs() * 2.0 ** -21, torch.tensor(6e-8))).all())
    w = torch.randn(5, 64, generator=g) * 0.02
    werr = (x3_unrows(x3_rows(w, F16X3_WSHIFT), F16X3_WSHIFT) - w).abs()
    assert bool((werr <= torch.maximum(w.abs() * 2.0 ** -21, torch.tensor(6e-8 / 256))).all())
    with pytest.raises(ValueError):
        x3_rows(torch.full((1, 32), 3.0e5))                                            # beyond 2 x 65504: cannot be split
    cfg = SAM_CONFIGS["vit_test"]
    sd = init_sam_state_dict(cfg, 72)
    e = "image_encoder.blocks.0."
    for mode, sfx in ((1, ".f16"), (2, ".x3")):
        p = pack_vit(sd, cfg, "cpu", mode, 2)
        D = cfg.embed_dim
        assert p[e + "attn.qkv.weight" + sfx].shape == (3 * D, D * (2 if mode == 2 else 1))
        assert p[e + "attn.qkv.bias" + sfx].numel() == 3 * D * (2 if mode == 2 else 1) and p[e + "attn.qkv.bias"].dtype == torch.float32
        assert "image_encoder.neck.0.weight_hl" in p and e + "attn.qkv.weight" not in p
    p0 = pack_vit(sd, cfg, "cpu", 0, 2)
    assert e + "attn.qkv.weight" in p0 and e + "attn.qkv.bias.f16" not in p0


def test_eight_ranks_gloo_host_threads_lpt_and_no_packing_in_the_step_loop():
    """`bench.py --gpus 8` as far as it can be exercised without GPUs: 8 gloo processes each cap their host
    threads to an equal share of the cores (dist.host_threads), build their tracker weights ONCE before the step loop (pack.stats
    does not move inside it), own a disjoint LPT share of the 30 DAVIS-17-val-like sequences that together cover all of them, and
    issue their ragged uint8 mask gathers in the same order."""
    code = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from sam_pt_amd import pack
from sam_pt_amd.dist import DAVIS17_VAL_LENGTHS, gather_masks, host_threads, init_from_env, lpt_assign
from sam_pt_amd.weights import init_pips_state_dict
rank, world, local = init_from_env("gloo")
assert world == 8
torch.set_num_threads(host_threads(world))
assert torch.get_num_threads() * world <= max(os.cpu_count() or 8, world), (torch.get_num_threads(), os.cpu_count())
assert host_threads(8, 256) == 32 and host_threads(1, 256) == 32 and host_threads(8, 8) == 1 and host_threads(3, 8) == 2
w = pack.pack_pips(init_pips_state_dict(72 + rank), "cpu")            # model build: before the loop, once
assert any(k.endswith("__x3s16") for k in w)
packs = pack.stats["packs"]
assign = lpt_assign(DAVIS17_VAL_LENGTHS, world)
mine = [DAVIS17_VAL_LENGTHS[i] for i in assign[rank]]
for step in range(2):                                                  # the step loop: only gathers, no packing
    for L in mine[:2]:
        out = gather_masks(torch.full((L, 2, 3), rank + 1, dtype=torch.uint8), max_frames=max(DAVIS17_VAL_LENGTHS))
        if rank == 0:
            assert out.shape[0] == world and all(out[r, 0].eq(r + 1).all() for r in range(world))
assert pack.stats["packs"] == packs
flat = sorted(i for a in assign for i in a)
assert flat == list(range(len(DAVIS17_VAL_LENGTHS)))
loads = [sum(DAVIS17_VAL_LENGTHS[i] for i in a) for a in assign]
assert max(loads) / (sum(loads) / world) < 1.06
if rank == 0:
    print("EIGHT_OK", loads)
dist.barrier(); dist.destroy_process_group()
""" % ROOT
    port = str(_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                            "--master-addr", "127.0.0.1", "--master-port", port, path], env=env, capture_output=True,
                           text=True, timeout=400)
    finally:
        os.unlink(path)
    assert r.returncode == 0, r.stderr[-2500:]
    assert "EIGHT_OK" in r.stdout


def test_stack_frames_takes_consecutive_views_without_a_copy():
    """SamPt accepts the reference's list-of-frames clip; frames that already are consecutive slices of one buffer are stacked as a
    view (no device copy kernel in the fused forward), anything else falls back to torch.stack with the same values."""
    import torch
    from sam_pt_amd.sam_pt import _stack_frames
    clip = torch.randint(0, 256, (5, 3, 6, 7), dtype=torch.uint8)
    v = _stack_frames([f for f in clip])
    assert v.data_ptr() == clip.data_ptr() and torch.equal(v, clip) and v.is_contiguous()
    w = _stack_frames([clip[i] for i in (0, 2, 1, 3, 4)])                       # not in order: a real stack
    assert w.data_ptr() != clip.data_ptr() and torch.equal(w, clip[[0, 2, 1, 3, 4]])
    x = _stack_frames([clip[0], clip[1].clone(), clip[2]])                      # another storage in between
    assert torch.equal(x, clip[:3]) and x.data_ptr() != clip.data_ptr()
    y = _stack_frames([f for f in clip[1:4]])                                   # a sub-range of the buffer is a view too
    assert y.data_ptr() == clip[1].data_ptr() and torch.equal(y, clip[1:4])
    assert torch.equal(_stack_frames([clip[0]]), clip[:1])


def test_rel_pos_operand_images_layout():
    """pack.rel_pos_operand_images: lane l of tile t, k-step ks holds rel_pos[32 t + (l & 31)][16 ks + 8 (l >> 5) .. + 8] as halves,
    zero past the table — what csrc/attention.hip's prologue used to convert per workgroup."""
    import torch
    from sam_pt_amd.pack import rel_pos_operand_images
    for S_, hd in ((14, 80), (64, 80), (14, 64), (6, 32)):
        g = torch.Generator().manual_seed(S_)
        rh, rw = torch.randn(2 * S_ - 1, hd, generator=g), torch.randn(2 * S_ - 1, hd, generator=g)
        o = rel_pos_operand_images(rh, rw)
        nt = -(-(2 * S_ - 1) // 32)
        assert o.shape == (2, nt, hd // 16, 64, 8) and o.dtype == torch.float16
        for tb, tab in enumerate((rh, rw)):
            for t in range(nt):
                for ks in range(hd // 16):
                    for l in (0, 5, 26, 31, 32, 47, 63):
                        row = 32 * t + (l & 31)
                        want = tab[row, 16 * ks + 8 * (l >> 5): 16 * ks + 8 * (l >> 5) + 8].half() if row < 2 * S_ - 1 else torch.zeros(8).half()
                        assert torch.equal(o[tb, t, ks, l], want)
