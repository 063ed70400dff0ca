"""Frames whose area is not a multiple of 4 (an odd height; H % 4 == 2 with an odd width) through everything frame-sized around the
decode: the staging copies of ``SamPt``'s graph-replayed chains (``sampt_move_rows``, ``sampt_fill_f32``) against torch indexing on the
CPU, the staged clip path against the eager one on hand-made tracks, the re-initialisation step on device planes against the host
route, and the output side (``sampt_resize_logits``, the VOS index maps).  The copies are compared bit for bit."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_device_reinit import CONFIGS, VARIANTS, _segment_logits, _stub_model
from tests.test_gpu_kernels import P, S, _vos_resized_prob64, ok
from tests.util import max_abs, synthetic_clip

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SENTINEL = -777.25
ODD = (121, 215)                 # area 26015 = 3 (mod 4)
ODD2 = (126, 215)                # area 27090 = 2 (mod 4)
OUT_HW = (97, 173)               # target_hw of the odd clip: 97 / 121 and 173 / 215 differ by 0.003 (forward's isotropy check: < 0.01)
INDEX_SETS = ((1, 1), (1, 5), (3, 5), (2, 7))                 # (n_objects, n_frames)
ROW_BYTES = (4, 8, 12, 16, 20, 4096, 4100, 16 * 257, 4 * ODD[0] * ODD[1], 4 * ODD2[0] * ODD2[1])


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def embed(rows, words, off, fill):
    """A flat f32 tensor [guard | off | rows * words | guard] filled with ``fill``; each guard is at least one full row and a multiple
    of 4 words, so the region starts 16-byte aligned for off == 0 and one float past alignment for off == 1.
    -> (tensor, first word of the region)."""
    guard = -(-words // 4) * 4
    return torch.full((guard + off + rows * words + guard + 4,), fill, dtype=torch.float32), guard + off


def item_sets(nm, nf, seed):
    """Shuffled proper subsets of the nm * nf items (one item: the item itself), the larger one first, then a single row."""
    n = nm * nf
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    if n == 1:
        return [perm.int()]
    return [perm[:max(1, n - 2)].int(), perm[n // 2:n // 2 + 1].int()]


def run_move(lib, dev, words, nm, nf, idx, scatter, src_off=0, dst_off=0):
    """One ``sampt_move_rows`` call on buffers embedded in guard bands, checked against torch indexing on the CPU."""
    rows = idx.numel()
    n_src, n_dst = (rows, nm * nf) if scatter else (nf, rows)
    src_big, s0 = embed(n_src, words, src_off, float("nan"))
    src_rows = (torch.arange(n_src * words, dtype=torch.float32) + 1.0).view(n_src, words)         # every word its own value
    src_big[s0:s0 + n_src * words] = src_rows.flatten()
    dst_big, d0 = embed(n_dst, words, dst_off, SENTINEL)
    want = dst_big.clone()
    region = want[d0:d0 + n_dst * words].view(n_dst, words)
    li = idx.long()
    if scatter:
        region.view(nm, nf, words)[li % nm, li // nm] = src_rows
    else:
        region[:] = src_rows[li // nm]
    src_d, dst_d, idx_d = src_big.to(dev), dst_big.to(dev), idx.to(dev)
    sp, dp = src_d[s0:], dst_d[d0:]
    assert (sp.data_ptr() % 16 == 0) == (src_off == 0) and (dp.data_ptr() % 16 == 0) == (dst_off == 0)
    rc = lib.sampt_move_rows(P(sp), P(dp), P(idx_d), rows, words * 4, nm, nf, scatter, S())
    what = f"row_bytes {words * 4} nm {nm} nf {nf} rows {rows} scatter {scatter} offsets {src_off} {dst_off}"
    assert rc == 0, (what, rc, lib.sampt_last_error())
    got = dst_d.cpu()
    assert not torch.isnan(got).any(), what                            # nothing of the source's surroundings was read
    assert torch.equal(bits(got), bits(want)), what                    # rows exact; guard bands and unnamed rows keep the sentinel
    assert torch.equal(bits(src_d), bits(src_big)), what               # the source is only read


@pytest.mark.parametrize("scatter", [0, 1])
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_move_rows_equals_torch_indexing(lib, dev, row_bytes, scatter):
    """gather: dst[r] = src[idx[r] // nm] (objects of one frame repeat a source row); scatter: dst.view(nm, nf, -1)[idx % nm, idx // nm] = src.
    16 * 257 bytes is more than one workgroup's 256 units; the last two lengths are frames of 121 x 215 and 126 x 215."""
    for nm, nf in INDEX_SETS:
        for idx in item_sets(nm, nf, row_bytes + 7 * nm + nf):
            run_move(lib, dev, row_bytes // 4, nm, nf, idx, scatter)


@pytest.mark.parametrize("offsets", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("row_bytes", [16, 4096, 16 * 257])
def test_move_rows_off_16_byte_alignment(lib, dev, row_bytes, offsets):
    """A row length made of 16-byte units on buffers one float past alignment moves word by word, exactly."""
    for scatter in (0, 1):
        for idx in item_sets(3, 5, row_bytes + scatter):
            run_move(lib, dev, row_bytes // 4, 3, 5, idx, scatter, *offsets)


def test_move_rows_refusals(lib, dev):
    """Refused with SAMPT_ERR_ARG before anything is launched: the destination keeps its sentinel."""
    src = torch.arange(64, dtype=torch.float32, device=dev)
    dst = torch.full((64,), SENTINEL, device=dev)
    idx = torch.arange(4, dtype=torch.int32, device=dev)
    good = dict(src=P(src), dst=P(dst), idx=P(idx), rows=2, row_bytes=16, nm=1, nf=4, scatter=1)

    def call(**kw):
        a = {**good, **kw}
        return lib.sampt_move_rows(a["src"], a["dst"], a["idx"], a["rows"], a["row_bytes"], a["nm"], a["nf"], a["scatter"], S())

    assert call(row_bytes=6) == ERR_ARG
    msg = lib.sampt_last_error()
    assert b"sampt_move_rows" in msg and b"row_bytes" in msg and b"6" in msg, msg
    assert call(row_bytes=0) == ERR_ARG and b"row_bytes" in lib.sampt_last_error()
    assert call(rows=0) == ERR_ARG and b"rows" in lib.sampt_last_error()
    assert call(nm=0) == ERR_ARG and b"n_objects" in lib.sampt_last_error()
    for name in ("src", "dst", "idx"):
        assert call(**{name: None}) == ERR_ARG and b"null" in lib.sampt_last_error(), name
        assert call(**{name: C.c_void_p(good[name].value + 2)}) == ERR_ARG and b"aligned" in lib.sampt_last_error(), name
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    assert call() == 0                                              # ... and the same arguments unaltered are accepted
    torch.cuda.synchronize()
    assert torch.equal(dst[:8].cpu(), torch.arange(8, dtype=torch.float32))


@pytest.mark.parametrize("value", [-float("inf"), 7.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, ODD[0] * ODD[1]])
def test_fill_f32(lib, dev, n, value):
    for off in (0, 1):
        big, d0 = embed(1, n, off, SENTINEL)
        want = big.clone()
        want[d0:d0 + n] = value
        big_d = big.to(dev)
        ok(lib.sampt_fill_f32(P(big_d[d0:]), n, value, S()), "sampt_fill_f32")
        assert torch.equal(bits(big_d), bits(want)), (n, value, off)


def test_fill_f32_refusals(lib, dev):
    dst = torch.full((16,), SENTINEL, device=dev)
    assert lib.sampt_fill_f32(P(dst), 0, 1.0, S()) == ERR_ARG and b"sampt_fill_f32" in lib.sampt_last_error()
    assert lib.sampt_fill_f32(None, 4, 1.0, S()) == ERR_ARG and b"sampt_fill_f32" in lib.sampt_last_error()
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- the staged clip path
T, M = 5, 2
# visible (1) points of every (frame, object): 4 positives, then 1 negative.  Ragged counts, every decoded item keeps a positive;
# items (1, 0), (3, 1) and (4, 1) have no visible point: they are not decoded and stay -inf
VIS = torch.tensor([[[1, 1, 1, 1, 1], [1, 1, 0, 1, 1]],
                    [[0, 0, 0, 0, 0], [1, 1, 1, 1, 0]],
                    [[1, 0, 1, 0, 1], [0, 1, 0, 0, 0]],
                    [[1, 1, 1, 1, 1], [0, 0, 0, 0, 0]],
                    [[0, 1, 1, 0, 0], [0, 0, 0, 0, 0]]], dtype=torch.float32)
EMPTY = VIS.sum(dim=2) == 0                                            # (T, M)


@pytest.fixture(scope="module")
def pred(dev):
    """7 items with a prompt in chains of at most 3: three chunks a clip, the last one a single row."""
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.weights import SAM_CONFIGS
    return SamPredictor(SamHip(config=SAM_CONFIGS["vit_test"], seed=72, precision="f32", max_batch=4, max_decode_batch=3).to(dev))


def hand_tracks(centres, hw):
    """(T, M, 5, 2) tracks: two objects (on the disc; 0.3 W to its right, 0.1 H above it) that follow the disc centres with a few
    pixels of drift, 4 positives around the object and 1 negative 0.18 W away from it.  All of it stays inside the frame."""
    H, W = hw
    pos = torch.tensor([[5.0, 0.0], [0.0, 4.0], [-5.0, 0.0], [0.0, -4.0], [0.18 * W, 3.0]])
    shift = torch.tensor([[0.0, 0.0], [0.3 * W, -0.1 * H]])
    t = torch.arange(T, dtype=torch.float32)
    drift = torch.stack([0.7 * t, -0.4 * t], dim=1)                    # (T, 2)
    traj = centres.float()[:, None, None, :] + shift[None, :, None, :] + pos[None, None] + drift[:, None, None, :]
    assert bool((traj[..., 0] > 0.01 * W).all() and (traj[..., 0] < 0.99 * W).all())
    assert bool((traj[..., 1] > 0.01 * H).all() and (traj[..., 1] < 0.99 * H).all())
    return traj


def staged_model(pred, tracker=None):
    from sam_pt_amd.sam_pt import SamPt
    return SamPt(tracker if tracker is not None else torch.nn.Module(), pred, sam_iou_threshold=-1e9, positive_points_per_mask=4,
                 negative_points_per_mask=1, add_other_objects_positive_points_as_negative_points=False,
                 iterative_refinement_iterations=2).eval()


@pytest.mark.parametrize("hw", [(120, 214), ODD, ODD2, (215, 121)])
def test_staged_decode_equals_eager_at_odd_frames(dev, pred, hw):
    """``SamPt._apply_sam_to_trajectories`` on the clip's embeddings (without them it takes the call-by-call protocol, which stages
    nothing) and hand-made tracks: the chains replayed from captured graphs through the staging buffers against the same chains launched
    eagerly on torch-indexed tensors, bit for bit — the bar of test_track_decode_graph_replay_is_bitwise_eager; (120, 214) is the control
    whose rows are made of 16-byte units.  The staged side runs on a stream of its own, as in ``forward``: chains on the default stream
    are never captured."""
    frames, centres = synthetic_clip(T=T, H=hw[0], W=hw[1], seed=21)
    images = frames.to(dev)
    traj = hand_tracks(centres, hw)
    model = staged_model(pred)
    feats = pred.encode_frames(images, chw=True)
    side = torch.cuda.Stream(device=dev)
    keep = pred.use_graph
    try:
        pred.use_graph = False
        _, l_e, s_e = model._apply_sam_to_trajectories(images, traj, VIS, feats)
        torch.cuda.synchronize()
        l_e = l_e.cpu()
        assert l_e.shape == (M, T) + tuple(hw) and s_e.shape == (T, M)
        assert bool((s_e[EMPTY] == -float("inf")).all() and torch.isfinite(s_e[~EMPTY]).all())
        assert bool((l_e[EMPTY.T] == -float("inf")).all() and torch.isfinite(l_e[~EMPTY.T]).all())
        pred.use_graph = True
        c0 = pred.graph_stats()
        for rep in range(3):                                           # a signature's first sight is eager, then captured, then replayed
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                _, l_g, s_g = model._apply_sam_to_trajectories(images, traj, VIS, feats)
                side.synchronize()
                l_g = l_g.cpu()
            fin = ~EMPTY.T
            print(f"\n[staged vs eager] {hw} call {rep}: max |logits diff| {max_abs(l_g[fin], l_e[fin]):.3e}, "
                  f"max |score diff| {max_abs(s_g[~EMPTY], s_e[~EMPTY]):.3e}")
            assert torch.equal(l_g, l_e) and torch.equal(s_g, s_e), (hw, rep)
        c1 = pred.graph_stats()
    finally:
        pred.use_graph = keep
    assert c1[2] > c0[2], (c0, c1)                                    # the chains were replayed from their graphs


# ---------------------------------------------------------------------------------------------- around the decode
def test_device_reinit_step_equals_host_step_at_an_odd_frame(dev):
    """tests/test_gpu_device_reinit.py::test_device_step_equals_host_step at 121 x 215 (planes whose rows end inside a word, an area
    that is no multiple of the tile): one variant with per-object frames, every point setting."""
    logits = _segment_logits(*ODD).to(dev)
    frames = torch.randint(0, 256, (5, 3) + ODD, generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(dev)
    variant = VARIANTS[2]
    drew = 0
    for cfg in CONFIGS:
        model = _stub_model(reinit_variant=variant, negative_point_selection_method="mixed", **cfg)
        cur_t = torch.tensor([0, 0, 0, 3], dtype=torch.int32)
        torch.manual_seed(11)
        q_h, inv_h, upd_h = model._reinit_step(frames, logits, cur_t, 0, False)
        state_h = torch.get_rng_state()
        torch.manual_seed(11)
        q_d, inv_d, upd_d = model._reinit_step(frames, logits, cur_t, 0, True)
        state_d = torch.get_rng_state()
        what = f"{variant} {cfg}"
        assert torch.equal(q_h, q_d) and torch.equal(inv_h, inv_d), what
        assert upd_h is not None and upd_d is not None and upd_h.dtype == upd_d.dtype and upd_h.device == upd_d.device, what
        assert torch.equal(upd_h, upd_d), what
        assert torch.equal(state_h, state_d), what
        assert bool((upd_h[..., 1] >= 0).all() and (upd_h[..., 1] < ODD[1]).all() and (upd_h[..., 2] >= 0).all() and (upd_h[..., 2] < ODD[0]).all())
        drew += int((~inv_h).sum())
    assert drew > 0


def test_forward_resizes_odd_frames_to_target_hw(dev, pred):
    """``forward`` on 121 x 215 frames with ``target_hw`` (97, 173), tracks handed in by a stub tracker: the logits that leave the
    decode stage against ``F.interpolate(align_corners=False)`` of them, under the rule of test_resize_logits_and_index_masks (the same
    finite pixels, 1e-5 on those; the items without a prompt are -inf maps)."""
    from sam_pt_amd.point_tracker import PointTracker
    frames, centres = synthetic_clip(T=T, H=ODD[0], W=ODD[1], seed=21)
    traj = hand_tracks(centres, ODD)

    class HandTracker(PointTracker):
        def forward(self, rgbs, query_points):
            return traj.reshape(1, T, M * 5, 2).clone(), VIS.reshape(1, T, M * 5).clone()

    model = staged_model(pred, HandTracker())
    seen = []
    inner = model._resize_logits
    model._resize_logits = lambda logits, target_hw: (seen.append(logits), inner(logits, target_hw))[1]
    q = torch.cat([torch.zeros(M, 5, 1), traj[0]], dim=2)
    out = model({"image": [f.to(dev) for f in frames], "target_hw": OUT_HW, "query_points": q})
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].shape == (M, T) + ODD and seen[0].is_cuda
    got = torch.stack(out["logits"]).cpu()
    ref = F.interpolate(seen[0].cpu(), size=OUT_HW, mode="bilinear", align_corners=False)
    assert got.shape == (M, T) + OUT_HW
    fin = torch.isfinite(ref)
    assert bool((torch.isfinite(got) == fin).all()) and max_abs(got[fin], ref[fin]) < 1e-5
    assert not fin[EMPTY.T].any() and bool(fin[~EMPTY.T].all())
    assert torch.equal(out["visibilities"], VIS)


INDEX_SEED = 9


def index_case():
    """Logits of 3 objects x 4 frames of 121 x 215 with a rejected (-inf) frame, query frames and ground-truth masks."""
    g = torch.Generator().manual_seed(INDEX_SEED)
    logits = torch.randn(3, 4, *ODD, generator=g) * 4
    logits[2, 1] = -float("inf")
    qt = torch.tensor([0, 1, 3])
    gt = (torch.rand(3, *ODD, generator=g) > 0.5).float()
    return logits, qt, gt


def index_statement(logits, qt, gt, candidates):
    """The statement of test_vos_index_masks_resized for ``dist.index_masks(..., out_hw=OUT_HW)``: equal to the float64 argmax wherever
    the two best probabilities differ by more than 1e-5, one of the tied labels elsewhere.  -> (ties, pixels, the decided pixels)."""
    TIE = 1e-5
    p64 = _vos_resized_prob64(logits, qt, gt, OUT_HW)
    top2 = p64.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > TIE
    want = p64.argmax(dim=0)
    for name, idx in candidates:
        idx = idx.long()
        assert idx.shape == (logits.shape[1],) + OUT_HW
        assert torch.equal(idx[decided], want[decided]), (name, int((idx[decided] != want[decided]).sum()))
        p_idx = p64.gather(0, idx[None])[0]
        assert bool((p_idx[~decided] >= top2[0][~decided] - TIE).all()), (name, "a tie resolved to a non-tied label")
    return int((~decided).sum()), decided.numel(), decided


def test_index_maps_at_an_odd_frame(dev):
    """``dist.index_masks`` at 121 x 215 and resized to (97, 173), on the device against the CPU tensor: equal at frame resolution
    (as test_vos_index_masks_overrides), the statement of test_vos_index_masks_resized with its cap on ties for the resized map."""
    from sam_pt_amd.dist import index_masks
    logits, qt, gt = index_case()
    ld, gd = logits.to(dev), gt.to(dev)
    n_tie = n_all = 0
    for q, m in ((None, None), (qt, None), (qt, gt)):
        ref = index_masks(logits, q, m)
        got = index_masks(ld, q, None if m is None else gd).cpu()
        assert got.shape == (4,) + ODD and torch.equal(got, ref), (q, m is None)
        ref_r = index_masks(logits, q, m, out_hw=OUT_HW)
        got_r = index_masks(ld, q, None if m is None else gd, out_hw=OUT_HW).cpu()
        a, b, decided = index_statement(logits, q, m, (("kernel", got_r), ("torch formula", ref_r)))
        assert bool((~decided)[got_r != ref_r].all())                  # where the kernel and the torch formula disagree it is a tie
        n_tie, n_all = n_tie + a, n_all + b
    print(f"\n[odd index maps] {n_tie} of {n_all} output pixels are provable ties")
    assert n_tie < 0.02 * n_all
