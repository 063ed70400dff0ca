"""Head-major qkv for the fp16 ViT attention (GemmP::hm_hd, FlashPad::head_major): the qkv GEMM can write [3][heads][rows][hd]
instead of token-major rows [rows][3 D], and the attention kernel can read it.  A change of layout only — every comparison here is
bitwise (torch.equal) against the token-major path on the same values."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def S():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what=""):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


def head_major(rows_tm, heads, hd):
    """token-major [rows][parts * heads * hd] -> [parts][heads][rows][hd]"""
    rows = rows_tm.shape[0]
    return rows_tm.reshape(rows, -1, heads, hd).permute(1, 2, 0, 3).contiguous()


# heads, hd, K, M, destination rows (None: no rowmap)
@pytest.mark.parametrize("heads,hd,K,M,rows", [(4, 64, 128, 512, None),      # base case
                                                (4, 64, 128, 300, 392),       # ragged last row tile + scatter
                                                (16, 80, 128, 256, None),     # 80-column heads across 256-column tiles
                                                (2, 32, 64, 320, None),       # the encoder's reduced geometry: the 128 x 128 tile kernel
                                                (2, 32, 64, 100, 131)])       # ... and the generic tile kernel, scattered
def test_gemm_f16_head_major_output(lib, dev, heads, hd, K, M, rows):
    D, N = heads * hd, 3 * heads * hd
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).half().to(dev)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half().to(dev)
    b = torch.randn(N, generator=g).to(dev)
    rowmap = None
    if rows is not None:
        rm = torch.randperm(rows, generator=g)[:M].to(torch.int32)
        rm[17] = -1                                   # a dropped row
        rowmap = rm.to(dev)
    R = rows if rows is not None else M
    tm = torch.zeros(R, N, device=dev, dtype=torch.float16)
    hm = torch.zeros(3, heads, R, hd, device=dev, dtype=torch.float16)
    ok(lib.sampt_gemm_ex(2, P(A), P(W), P(b), None, P(tm), M, N, K, 0, 1.0, P(rowmap), None, 0, 0, S()), "gemm token-major")
    ok(lib.sampt_gemm_f16_head_major(P(A), P(W), P(b), P(hm), M, N, K, heads, hd, R, P(rowmap), S()), "gemm head-major")
    assert float(tm.float().abs().max()) > 0.5        # (the product ran)
    assert torch.equal(hm, head_major(tm, heads, hd))
    assert D * 3 == N


# S, hd, heads, B, windows per side (0: whole frames), token grid side of the frame
@pytest.mark.parametrize("S_,hd,heads,B,nw,grid", [(14, 80, 2, 4, 2, 20),     # real, edge- and corner-padded windows
                                                   (64, 80, 1, 1, 0, 0),      # global, with the V pad page
                                                   (6, 32, 2, 4, 2, 9),       # the two-wave instantiation
                                                   (16, 32, 2, 1, 0, 0)])     # reduced test geometry
def test_flash_attention_head_major_input(lib, dev, S_, hd, heads, B, nw, grid):
    N, D = S_ * S_, heads * hd
    g = torch.Generator().manual_seed(S_ * hd + B)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).half()
    rel_h = (torch.randn(2 * S_ - 1, hd, generator=g) * 0.3).to(dev)
    rel_w = (torch.randn(2 * S_ - 1, hd, generator=g) * 0.3).to(dev)
    bias_row = None
    if nw:
        bias_row = (torch.randn(3 * D, generator=g) * 0.5).half().to(dev)
        # the qkv rows of padded tokens are never written by the encoder and must never be read: poison them
        t = torch.arange(N)
        for w in range(B):
            wy, wx = divmod(w % (nw * nw), nw)
            pad = (wy * S_ + t // S_ >= grid) | (wx * S_ + t % S_ >= grid)
            qkv[w * N + t[pad]] = float("nan")
        assert bool(torch.isnan(qkv).any())
    tm = qkv.to(dev)
    hm = head_major(qkv, heads, hd).to(dev)
    out_tm = torch.zeros(B * N, D, device=dev, dtype=torch.float16)
    out_hm = torch.zeros(B * N, D, device=dev, dtype=torch.float16)
    if nw:
        ok(lib.sampt_vit_window_attention(1, P(tm), P(rel_h), P(rel_w), P(out_tm), B // (nw * nw), S_, heads, hd, P(bias_row), nw, nw,
                                          grid, grid, S()), "flash token-major (windows)")
    else:
        ok(lib.sampt_vit_attention_f16(P(tm), P(rel_h), P(rel_w), P(out_tm), B, S_, heads, hd, None, 0, S()), "flash token-major")
    ok(lib.sampt_vit_attention_f16_head_major(P(hm), P(rel_h), P(rel_w), P(out_hm), B, S_, heads, hd, P(bias_row), nw, nw, grid, grid,
                                              S()), "flash head-major")
    assert bool(torch.isfinite(out_tm).all()) and float(out_tm.float().abs().max()) > 0.1
    assert torch.equal(out_hm, out_tm)


def _encode(pred, lib, frames, head_major_on):
    """One batch through the encoder engine with the HQ tap, the way SamPredictor.encode_frames drives it."""
    cfg = pred.model.cfg
    B, H, W = frames.shape[0], frames.shape[2], frames.shape[3]
    pred.set_attention_head_major(head_major_on)
    pred._select_bias_set(H, W)
    ws = pred._vit_ws(B)
    dead = pred._dead_rows(frames, True, H, W, ws)
    out = torch.zeros(B, cfg.grid * cfg.grid, cfg.out_chans, device=frames.device)
    tap = torch.zeros(B, cfg.grid * cfg.grid, cfg.embed_dim, device=frames.device)
    if dead is not None:
        ok(lib.sampt_vit_encode_live(pred._vit, P(frames), 1, B, H, W, P(out), P(tap), P(dead), 0, P(ws), ws.numel(), S()), "encode_live")
    else:
        ok(lib.sampt_vit_encode(pred._vit, P(frames), 1, B, H, W, P(out), P(tap), P(ws), ws.numel(), S()), "encode")
    torch.cuda.synchronize()
    return out, tap, dead is not None


@pytest.mark.parametrize("hw,compact", [((100, 256), True),      # landscape: compact live-row stream, padded windows
                                        ((256, 256), False)])    # square: the plain entry point
def test_vit_encoder_head_major_switch_is_exact(lib, dev, hw, compact):
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    g = torch.Generator().manual_seed(hw[0])
    frames = torch.randint(0, 256, (2, 3) + hw, generator=g, dtype=torch.uint8).to(dev)
    pred = SamPredictor(SamHip("vit_test", precision="f16", seed=72, max_batch=2).to(dev))
    pred._ensure()
    off = _encode(pred, lib, frames, False)
    on = _encode(pred, lib, frames, True)
    assert off[2] == compact and on[2] == compact
    assert bool(torch.isfinite(off[0]).all()) and float(off[1].abs().max()) > 0
    assert torch.equal(on[0], off[0]), "embeddings differ"
    assert torch.equal(on[1], off[1]), "HQ intermediate tap differs"
