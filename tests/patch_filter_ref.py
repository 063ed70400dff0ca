"""What the patch-similarity filter's tests and the fixture's generator (tools/make_patch_filter_golden.py) share.

``similarities`` restates the first half of ``SamPt._patch_similarity_filter`` (sam_pt_amd/sam_pt.py) line by line, returning the
similarities that function thresholds and then drops; in float32 it IS the host path (tests/test_patch_filter_cpu.py pins the two
together through the codes), in float64 it is "the same formulas carried through in float64" that ``bar_sim`` is measured against.
``rgb2lab`` restates skimage.color.rgb2lab, which is absent: that function is parity unpinned, here as everywhere.
"""
import os

import numpy as np
import torch
from torch.nn import functional as F

from sam_pt_amd.sam_pt import PointVisibilityType, SamPt, rgb2lab

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_filter.npz")


def similarities(rgbs, query_points, traj, ps, dtype=torch.float32):
    """rgbs (T,3,H,W) uint8, query_points (N,3), traj (T,N,2), all CPU -> (T,N) similarities in ``dtype``."""
    lab = rgb2lab(rgbs[:, [2, 1, 0], :, :].permute(0, 2, 3, 1)).permute(0, 3, 1, 2).to(dtype)

    def patches(lab_frames, xy):
        _, _, h, w = lab_frames.shape
        tmpl = torch.arange(-(ps // 2), ps // 2 + 1)
        tmpl = torch.stack(torch.meshgrid(tmpl, tmpl, indexing="ij"), dim=-1).reshape(-1, 2)
        grid = ((xy[:, :, None, :] + tmpl[None, None] + 0.5) / torch.tensor([w, h])[None, None, None]) * 2 - 1
        return F.grid_sample(lab_frames, grid.to(dtype), align_corners=False, mode="bilinear").permute(0, 2, 3, 1)

    qt = query_points[:, 0].long()
    qp = patches(lab[qt], query_points[:, None, 1:].to(dtype)).squeeze(1)
    tp = patches(lab, traj.to(dtype))
    diff = tp.flatten(2, 3) - qp[None].flatten(2, 3)
    return torch.exp(-torch.norm(diff, dim=-1) / (2 * ps ** 2))


def host_codes(rgbs, query_points, traj, vis, ps, threshold, border_rule=True):
    """The repository's host path: ``SamPt._patch_similarity_filter`` and then the border lines of ``_track_points``, on CPU tensors."""
    self = type("HostFilter", (), {"patch_size": ps, "patch_similarity_threshold": threshold})()
    out = SamPt._patch_similarity_filter(self, rgbs, query_points, traj, vis.float(), query_points.shape[0], 1)
    if border_rule:
        h, w = rgbs.shape[-2:]
        out[traj[:, :, 0] / w < 0.01] = CODES["OUTSIDE_FRAME"]          # sam_pt.py:684-690
        out[traj[:, :, 1] / h < 0.01] = CODES["OUTSIDE_FRAME"]
        out[traj[:, :, 0] / w > 0.99] = CODES["OUTSIDE_FRAME"]
        out[traj[:, :, 1] / h > 0.99] = CODES["OUTSIDE_FRAME"]
    return out


class StubTracker:
    """What ``_track_points`` (the reference's and this project's) needs of a tracker: eval, to, evaluate_batch.  Hands out the
    prescribed trajectories (T,N,2) and visibilities (T,N) chunk by chunk, on ``device`` if one is given; starts over after N."""

    def __init__(self, traj, vis, device=None):
        self.traj, self.vis, self.device, self.at = traj, vis, device, 0

    def eval(self):
        return self

    def to(self, device):
        return self

    def evaluate_batch(self, rgbs, query_points):
        n = query_points.shape[1]
        sl = slice(self.at, self.at + n)
        self.at = (self.at + n) % self.traj.shape[1]
        t, v = self.traj[None, :, sl].clone(), self.vis[None, :, sl].clone()
        return {"trajectories_pred": t.to(self.device) if self.device else t, "visibilities_pred": v.to(self.device) if self.device else v}


def load_golden():
    g = np.load(GOLDEN)
    return {k: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files}


CODES = {c.name: float(c.value) for c in PointVisibilityType}
