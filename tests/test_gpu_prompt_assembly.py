"""Prompt assembly on the HIP device (csrc/prompt_assembly.hip through sam_pt_amd/prompt_assembly.py): count + fill against the host
restatement ``assemble_prompts_host`` with == on every word — coordinates bit for bit, labels, the zeroed padding, k and npos — and
the border rule against ``SamPt._mark_outside_frame``.  The restatement itself is held to ``SamPt._prepare_points`` +
``apply_coords`` by tests/test_prompt_assembly_cpu.py, on the same cases."""
import numpy as np
import pytest
import torch

from sam_pt_amd import _lib
from sam_pt_amd import prompt_assembly as PA
from sam_pt_amd.sam_pt import SamPt
from tests import prompt_assembly_cases as CS

pytestmark = pytest.mark.gpu


def host(M, pp, P, negatives, add_others, ld=None):
    traj, vis, _, _, _, _ = CS.reference(M, pp, P, negatives, add_others)
    return (traj, vis) + PA.assemble_prompts_host(traj, vis, pp, negatives, add_others, *CS.scales(), ld=ld)


def fill(dev, traj_d, vis_d, pp, negatives, add_others, items, ld):
    """One fill call into buffers that hold no zeros beforehand -> numpy (xy words as int32, labels, k_item, npos_item)."""
    F = len(items)
    pts = torch.full((F, ld, 2), float("nan"), dtype=torch.float32, device=dev)
    labels = torch.full((F, ld), 0x7f7f7f7f, dtype=torch.int32, device=dev)
    k_item = torch.full((F,), -7, dtype=torch.int32, device=dev)
    npos_item = torch.full((F,), -7, dtype=torch.int32, device=dev)
    PA.fill_prompts(traj_d, vis_d, pp, negatives, add_others, *CS.scales(), torch.tensor(items, dtype=torch.int32, device=dev), pts,
                    labels, k_item, npos_item)
    return pts.cpu().numpy().view(np.int32), labels.cpu().numpy(), k_item.cpu().numpy(), npos_item.cpu().numpy()


@pytest.mark.parametrize("M,pp,P,negatives,add_others", CS.CASES)
def test_count_and_fill_equal_the_host_restatement(dev, M, pp, P, negatives, add_others):
    traj, vis, xy, lab, k, npos = host(M, pp, P, negatives, add_others)
    traj_d, vis_d = torch.tensor(traj, device=dev), torch.tensor(vis, device=dev)
    counts = PA.count_prompts(vis_d, pp, negatives, add_others).cpu().numpy()
    assert (counts[0] == k).all() and (counts[1] == npos).all()
    n, kmax = len(k), xy.shape[1]
    assert kmax == max(1, int(k.max()))
    everything = list(range(n))
    # a strict subset of the items in non-monotone order: the odd items backwards, then item 0 (T * M >= 3 in every case)
    subset = everything[1::2][::-1] + [0]
    assert len(subset) < n and sorted(subset) != subset
    for ld in sorted({kmax, -(-kmax // 8) * 8}):                   # ld = kmax, and kmax rounded up to 8 as under graphs
        _, _, w_xy, w_lab, _, _ = host(M, pp, P, negatives, add_others, ld=ld)
        for items in (everything, subset):
            g_xy, g_lab, g_k, g_npos = fill(dev, traj_d, vis_d, pp, negatives, add_others, items, ld)
            assert (g_xy == w_xy.view(np.int32)[items]).all(), "coordinates or their padding differ"
            assert (g_lab == w_lab[items]).all(), "labels or their padding differ"
            assert (g_k == k[items]).all() and (g_npos == npos[items]).all()


def test_fill_writes_a_decode_staging_block(dev):
    """The outputs may be the views of ONE int32 block laid out as ``SamPredictor.decode_staging`` lays it out
    [pts | labels | k_item | npos_item | items], the item numbers read from its tail."""
    M, pp, P, negatives, add_others = 9, 8, 9, True, True
    traj, vis, xy, lab, k, npos = host(M, pp, P, negatives, add_others)
    items = [5, 26, 3, 17]
    F, ld = len(items), xy.shape[1]
    block = torch.full((F * ld * 3 + 3 * F,), -1, dtype=torch.int32, device=dev)
    o1, o2, o3, o4 = F * ld * 2, F * ld * 3, F * ld * 3 + F, F * ld * 3 + 2 * F
    block[o4:] = torch.tensor(items, dtype=torch.int32, device=dev)
    PA.fill_prompts(torch.tensor(traj, device=dev), torch.tensor(vis, device=dev), pp, negatives, add_others, *CS.scales(), block[o4:],
                    block[:o1].view(torch.float32).view(F, ld, 2), block[o1:o2].view(F, ld), block[o2:o3], block[o3:o4])
    got = block.cpu().numpy()
    want = np.concatenate([xy.view(np.int32)[items].reshape(-1), lab[items].reshape(-1), k[items], npos[items],
                           np.asarray(items, dtype=np.int32)])
    assert (got == want).all()


def test_item_numbers_outside_the_clip_get_empty_prompts(dev):
    M, pp, P = 2, 3, 5
    traj, vis, xy, lab, k, npos = host(M, pp, P, True, True)
    traj_d, vis_d = torch.tensor(traj, device=dev), torch.tensor(vis, device=dev)
    g_xy, g_lab, g_k, g_npos = fill(dev, traj_d, vis_d, pp, True, True, [-1, 0, CS.T * M, 2 ** 31 - 1], xy.shape[1])
    assert (g_k[[0, 2, 3]] == 0).all() and (g_npos[[0, 2, 3]] == 0).all() and not g_xy[[0, 2, 3]].any() and not g_lab[[0, 2, 3]].any()
    assert g_k[1] == k[0] and (g_xy[1] == xy.view(np.int32)[0]).all()


def test_bad_arguments_are_refused(dev):
    lib = _lib.load()
    v = torch.ones(2, 2, 3, device=dev)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    P, sp = _lib.ptr, _lib.stream_ptr()
    assert lib.sampt_prompt_count(P(v), 0, 2, 3, 2, 0, 1, P(out), P(out), sp) == -1
    assert lib.sampt_prompt_count(P(v), 2, 2, 3, -1, 0, 1, P(out), P(out), sp) == -1
    assert lib.sampt_prompt_count(None, 2, 2, 3, 2, 0, 1, P(out), P(out), sp) == -1
    assert lib.sampt_prompt_count(P(v), 1 << 15, 1 << 15, 3, 2, 0, 1, P(out), P(out), sp) == -1
    assert lib.sampt_prompt_fill(P(v), P(v), 2, 2, 3, 2, 0, 1, 1.0, 1.0, P(out), 1, 0, P(v), P(out), P(out), P(out), sp) == -1
    assert lib.sampt_prompt_fill(P(v), P(v), 2, 2, 3, 2, 0, 1, 1.0, 1.0, None, 1, 4, P(v), P(out), P(out), P(out), sp) == -1
    assert lib.sampt_mark_outside_frame(P(v), P(v), 0, 8, 8, P(v), sp) == -1
    assert lib.sampt_mark_outside_frame(P(v), None, 4, 8, 8, P(v), sp) == -1
    torch.cuda.synchronize()


def test_border_rule_equals_the_host_lines(dev):
    """The four comparisons of ``SamPt._mark_outside_frame`` at and next to their limits, on every visibility code."""
    h, w = 120, 214
    xs = torch.tensor([0.01 * w, 0.99 * w, 2.14, 2.1399999, 2.1400001, 211.86, 211.85999, 211.86001, -3.0, 0.0, 107.0, 500.0])
    ys = torch.tensor([0.01 * h, 0.99 * h, 1.2, 1.1999999, 1.2000001, 118.8, 118.79999, 118.80001, -1.0, 0.0, 60.0, 300.0])
    xs = torch.cat([xs, torch.nextafter(xs, torch.tensor(1e9)), torch.nextafter(xs, torch.tensor(-1e9))])
    ys = torch.cat([ys, torch.nextafter(ys, torch.tensor(1e9)), torch.nextafter(ys, torch.tensor(-1e9))])
    traj = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=-1).reshape(6, -1, 2).contiguous()        # (6, N, 2)
    vis = torch.tensor(CS.CODES)[:, None].repeat(1, traj.shape[1])
    want = vis.clone()
    SamPt._mark_outside_frame(traj, want, h, w)
    got = PA.mark_outside_frame(traj.to(dev), vis.to(dev), h, w)
    assert torch.equal(got.cpu(), want) and (want == -2).any() and (want != -2).any()
    ones = torch.ones(traj.shape[:2])
    SamPt._mark_outside_frame(traj, ones, h, w)
    both = PA.mark_outside_frame(traj.to(dev), torch.ones(traj.shape[:2], dtype=torch.bool, device=dev), h, w)       # a tracker's bools
    assert both.dtype == torch.float32 and torch.equal(both.cpu(), ones)
