"""TEST INFRASTRUCTURE ONLY: the reference's SuperGlue point tracker run in place on the CPU, and a restatement of it.

``load_reference()`` imports ``sam_pt/point_tracker/superglue`` from the reference tree by path (namespace modules for the
packages whose ``__init__`` files pull absent third-party code, stubs for ``cv2`` / ``matplotlib`` which ``models/utils``
imports, and a stand-in for ``torchvision.transforms`` with exactly what ``tracker.py`` touches: ``rgb_to_grayscale``,
the NEAREST same-size ``resize`` of the masks and ``InterpolationMode``).  torchvision is absent here, so the grey-scale
stand-in is pinned against its documented formula only: parity with torchvision itself is unpinned.  Nothing of the
reference is copied.  ``available()`` is false where the tree is absent.

The rest of the file is SuperPoint + SuperGlue + the tracker's selection loop restated in this project's own words as
functions over state dicts (key names of ``superpoint_v1.pth`` / ``superglue_outdoor.pth``): it stands in for the
reference where the tree does not exist (the GPU tests), and tests/test_superglue_cpu.py pins it to the live reference
and to tests/golden/superglue_ref.npz.  Unlike the reference it runs SuperPoint once per frame; SuperPoint is
deterministic, so no compared number changes.
"""
import contextlib
import importlib
import importlib.machinery
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle.reference_loader import REF, _link_children, _ns

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superglue_ref.npz")
SG_DIR = os.path.join(REF, "sam_pt", "point_tracker", "superglue")

# the golden clip (tools/make_superglue_golden.py): 75 x 109 is no multiple of 8, so the score map covers 72 x 104 only
GOLDEN_T, GOLDEN_H, GOLDEN_W = 3, 75, 109
GOLDEN_POS, GOLDEN_NEG, GOLDEN_MASKS = 4, 2, 2
GOLDEN_SEED = 84            # the clip's seed: the first for which tools/make_superglue_golden.py's assertions hold
GOLDEN_WEIGHT_SEED = 72
GOLDEN_NP_SEED = 1234
GOLDEN_CONFIG = {
    "superpoint": {"nms_radius": 3, "keypoint_threshold": 0.005, "max_keypoints": -1, "descriptor_dim": 256, "remove_borders": 4},
    "superglue": {"sinkhorn_iterations": 20, "match_threshold": 0.2},
}


def available() -> bool:
    return os.path.isfile(os.path.join(SG_DIR, "tracker.py")) and os.path.isfile(os.path.join(SG_DIR, "models", "superglue.py"))


def golden():
    return np.load(GOLDEN)


def golden_clip(seed: int = GOLDEN_SEED):
    """-> frames uint8 (3,3,75,109), masks float (2,75,109) in {0, 1}, query_points (1, 2 * 6, 3).  Frame 1 is frame 0
    shifted by (8, 8) pixels (one SuperPoint cell: interior descriptors repeat), frame 2 another shift with noise and a
    changed patch."""
    g = torch.Generator().manual_seed(seed)
    H, W = GOLDEN_H, GOLDEN_W
    big = F.interpolate(torch.rand(1, 3, 26, 34, generator=g), size=(H + 32, W + 32), mode="bicubic", align_corners=False)[0]
    big = (big + 0.15 * torch.rand(3, H + 32, W + 32, generator=g)).clamp(0, 1)
    f0 = big[:, 16:16 + H, 16:16 + W]
    f1 = big[:, 8:8 + H, 8:8 + W]
    f2 = big[:, 19:19 + H, 5:5 + W] + 0.06 * torch.randn(3, H, W, generator=g)
    f2[:, 20:45, 60:95] = torch.rand(3, 25, 35, generator=g)
    frames = (torch.stack([f0, f1, f2]).clamp(0, 1) * 255).round().to(torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    # mask 0 covers every keypoint row (more positives than asked for, no negatives), mask 1 is a small box (the opposite)
    masks = torch.stack([(yy < 70).float(), ((xx >= 70) & (xx < 80) & (yy >= 30) & (yy < 38)).float()])
    n = GOLDEN_MASKS * (GOLDEN_POS + GOLDEN_NEG)
    q = torch.zeros(1, n, 3)
    q[0, :, 1] = 10 + torch.arange(n) * 7.0
    q[0, :, 2] = 12 + torch.arange(n) * 4.0
    return frames, masks, q


# ---------------------------------------------------------------------------------------------- the live reference
def rgb_to_grayscale(img: torch.Tensor, num_output_channels: int = 1) -> torch.Tensor:
    """torchvision.transforms.functional.rgb_to_grayscale for tensors (..., 3, H, W), as documented:
    ``(0.2989 r + 0.587 g + 0.114 b).to(img.dtype)``, channel dimension kept."""
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def _install_torchvision_standin():
    try:
        import torchvision.transforms.functional  # noqa: F401
        return
    except Exception:
        pass

    class InterpolationMode:
        NEAREST, BILINEAR = "nearest", "bilinear"

    def resize(img, size, interpolation=InterpolationMode.BILINEAR, antialias=None):
        assert interpolation == InterpolationMode.NEAREST and tuple(img.shape[-2:]) == tuple(size), \
            "stand-in: only the tracker's NEAREST same-size resize of the masks"
        return img

    def mod(name):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        sys.modules[name] = m
        return m

    tv, tr, fn = mod("torchvision"), mod("torchvision.transforms"), mod("torchvision.transforms.functional")
    fn.rgb_to_grayscale, fn.resize, fn.InterpolationMode = rgb_to_grayscale, resize, InterpolationMode
    tr.functional, tr.InterpolationMode, tv.transforms = fn, InterpolationMode, tr


def load_reference():
    """-> (SuperGluePointTracker, models.superpoint module, models.superglue module) of the reference, imported in place."""
    assert available(), "reference tree not present"
    sys.dont_write_bytecode = True
    for n, p in [("sam_pt", "/sam_pt"), ("sam_pt.point_tracker", "/sam_pt/point_tracker"),
                 ("sam_pt.point_tracker.superglue", "/sam_pt/point_tracker/superglue"),
                 ("sam_pt.point_tracker.superglue.models", "/sam_pt/point_tracker/superglue/models")]:
        _ns(n, p)

    def stub(name):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        return sys.modules[name]

    stub("cv2")
    try:
        importlib.import_module("matplotlib.pyplot")
    except Exception:
        setattr(stub("matplotlib"), "pyplot", stub("matplotlib.pyplot"))
        if not hasattr(sys.modules["matplotlib"], "use"):
            sys.modules["matplotlib"].use = lambda *a, **k: None
    _install_torchvision_standin()
    T = importlib.import_module("sam_pt.point_tracker.tracker")
    sys.modules["sam_pt.point_tracker"].PointTracker = T.PointTracker
    sp = importlib.import_module("sam_pt.point_tracker.superglue.models.superpoint")
    sg = importlib.import_module("sam_pt.point_tracker.superglue.models.superglue")
    _link_children()
    trk = importlib.import_module("sam_pt.point_tracker.superglue.tracker")
    _link_children()
    return trk.SuperGluePointTracker, sp, sg


def reference_tracker(sp_sd, sg_sd, config=None, pos=GOLDEN_POS, neg=GOLDEN_NEG, dtype=torch.float32):
    """The reference's SuperGluePointTracker with the two state dicts loaded through its own ``torch.load`` of a checkpoint."""
    Tracker, _, _ = load_reference()
    config = config or GOLDEN_CONFIG
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "superpoint.pth"), os.path.join(d, "superglue.pth")
        torch.save({k: v.clone() for k, v in sp_sd.items()}, a)
        torch.save({k: v.clone() for k, v in sg_sd.items()}, b)
        cfg = {"superpoint": {**config["superpoint"], "checkpoint": a}, "superglue": {**config["superglue"], "checkpoint": b}}
        with contextlib.redirect_stdout(io.StringIO()):
            trk = Tracker(pos, neg, [-1, -1], cfg)
    trk.eval()
    if dtype != torch.float32:
        trk.to(dtype)
    return trk


# ---------------------------------------------------------------------------------------------- the restatement
def grey_frames(frames_u8: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """uint8 (T,3,H,W) -> (T,H,W) in [0, 1]: weighted sum in f32, truncated to uint8, divided by 255."""
    f = frames_u8.to(torch.float32)
    l = (0.2989 * f[:, 0] + 0.587 * f[:, 1] + 0.114 * f[:, 2]).to(torch.uint8)
    return l.to(dtype) / 255


def nms(scores: torch.Tensor, radius: int) -> torch.Tensor:
    """simple_nms on one map (H, W): keep a pixel that equals its window maximum, then two rounds in which pixels near a
    kept one are zeroed and the window maxima of what is left are added."""
    def pool(x):
        return F.max_pool2d(x[None, None], kernel_size=2 * radius + 1, stride=1, padding=radius)[0, 0]

    keep = scores == pool(scores)
    for _ in range(2):
        near = pool(keep.to(scores.dtype)) > 0
        rest = torch.where(near, torch.zeros_like(scores), scores)
        keep = keep | ((rest == pool(rest)) & ~near)
    return torch.where(keep, scores, torch.zeros_like(scores))


def keypoints_from_scores(dense: torch.Tensor, radius: int, threshold: float, border: int):
    """dense (Hs, Ws) -> keypoints (n, 2) as (x, y) floats in row-major (y, x) order, their scores (n,)."""
    s = nms(dense, radius)
    yx = torch.nonzero(s > threshold)
    val = s[yx[:, 0], yx[:, 1]]
    Hs, Ws = dense.shape
    ok = (yx[:, 0] >= border) & (yx[:, 0] < Hs - border) & (yx[:, 1] >= border) & (yx[:, 1] < Ws - border)
    return yx[ok].flip(1).to(dense.dtype), val[ok]


def sample_descriptors(dmap: torch.Tensor, kpts: torch.Tensor) -> torch.Tensor:
    """dmap (256, h8, w8) raw, kpts (n, 2) -> (256, n): channel-normalised map sampled bilinearly at the keypoints' cell
    coordinates (align_corners=True, zero padding), normalised again."""
    c, h, w = dmap.shape
    d = F.normalize(dmap[None], p=2, dim=1)
    k = kpts - 8 / 2 + 0.5
    k = k / torch.tensor([w * 8 - 8 / 2 - 0.5, h * 8 - 8 / 2 - 0.5]).to(k)[None]
    k = k * 2 - 1
    out = F.grid_sample(d, k.view(1, 1, -1, 2), mode="bilinear", align_corners=True)
    return F.normalize(out.reshape(1, c, -1), p=2, dim=1)[0]


def superpoint(sd, image: torch.Tensor, cfg) -> dict:
    """image (H, W) in [0, 1] -> dense scores (Hs, Ws), raw descriptor map (256, h8, w8), keypoints, scores, descriptors (256, n)."""
    def conv(name, x, relu=True, pad=1):
        y = F.conv2d(x, sd[name + ".weight"].to(x), sd[name + ".bias"].to(x), padding=pad)
        return F.relu(y) if relu else y

    x = image[None, None]
    for i, name in enumerate(("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")):
        x = conv(name, x)
        if i in (1, 3, 5):
            x = F.max_pool2d(x, 2, 2)
    logits = conv("convPb", conv("convPa", x), relu=False, pad=0)
    prob = F.softmax(logits, 1)[0, :64]
    _, h, w = prob.shape
    dense = prob.reshape(8, 8, h, w).permute(2, 0, 3, 1).reshape(h * 8, w * 8)      # (cell y, dy, cell x, dx)
    dmap = conv("convDb", conv("convDa", x), relu=False, pad=0)[0]
    kpts, scores = keypoints_from_scores(dense, cfg["nms_radius"], cfg["keypoint_threshold"], cfg["remove_borders"])
    return {"dense": dense, "dmap": dmap, "keypoints": kpts, "scores": scores, "descriptors": sample_descriptors(dmap, kpts)}


def fold_bn1d(sd, conv: str, bn: str, dtype=torch.float64):
    """Conv1d(k = 1) + eval-mode BatchNorm1d as one affine map (w [out][in], b [out]) in ``dtype``."""
    w, b = sd[conv + ".weight"][:, :, 0].to(dtype), sd[conv + ".bias"].to(dtype)
    g = sd[bn + ".weight"].to(dtype) / torch.sqrt(sd[bn + ".running_var"].to(dtype) + 1e-5)
    return w * g[:, None], (b - sd[bn + ".running_mean"].to(dtype)) * g + sd[bn + ".bias"].to(dtype)


def _conv1(sd, name: str, x: torch.Tensor) -> torch.Tensor:
    """Conv1d(kernel 1) over columns x (C, n)."""
    return F.conv1d(x[None], sd[name + ".weight"].to(x), sd[name + ".bias"].to(x))[0]


def _mlp(sd, prefix: str, n_conv: int, x: torch.Tensor) -> torch.Tensor:
    """Sequential(Conv1d, BatchNorm1d, ReLU, ..., Conv1d) over columns x (C, n), BatchNorms in eval mode."""
    for i in range(n_conv):
        x = _conv1(sd, f"{prefix}.{3 * i}", x)
        if i < n_conv - 1:
            b = f"{prefix}.{3 * i + 1}"
            x = F.relu(F.batch_norm(x[None], sd[b + ".running_mean"].to(x), sd[b + ".running_var"].to(x), sd[b + ".weight"].to(x),
                                    sd[b + ".bias"].to(x), training=False, eps=1e-5)[0])
    return x


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q (heads, N, d), k / v (heads, M, d) -> (heads, N, d): softmax(q k^T / sqrt(d)) v."""
    p = F.softmax(torch.einsum("hnd,hmd->hnm", q, k) / q.shape[-1] ** 0.5, dim=-1)
    return torch.einsum("hnm,hmd->hnd", p, v)


def _propagate(sd, p: str, x: torch.Tensor, src: torch.Tensor, heads: int = 4) -> torch.Tensor:
    """One AttentionalPropagation on columns x (256, n) with source (256, m) -> the residual delta (256, n)."""
    def proj(j, t):                                        # channel c = d * heads + h (heads interleaved) -> (heads, n, d)
        y = _conv1(sd, f"{p}.attn.proj.{j}", t)
        return y.reshape(-1, heads, y.shape[1]).permute(1, 2, 0)

    o = attention(proj(0, x), proj(1, src), proj(2, src))
    o = o.permute(2, 0, 1).reshape(-1, x.shape[1])         # back to channel d * heads + h
    return _mlp(sd, p + ".mlp", 2, torch.cat([x, _conv1(sd, p + ".attn.merge", o)], 0))


def log_optimal_transport(scores: torch.Tensor, alpha: torch.Tensor, iters: int) -> torch.Tensor:
    """scores (N, M) -> Z (N + 1, M + 1): log-domain Sinkhorn with a dustbin row and column of value alpha."""
    n, m = scores.shape
    Z = torch.full((n + 1, m + 1), float(alpha), dtype=scores.dtype)
    Z[:n, :m] = scores
    fn, fm = scores.new_tensor(float(n)), scores.new_tensor(float(m))
    norm = -(fn + fm).log()
    log_mu = torch.cat([norm.expand(n), (fm.log() + norm)[None]])
    log_nu = torch.cat([norm.expand(m), (fn.log() + norm)[None]])
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None, :], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return Z + u[:, None] + v[None, :] - norm


def matches_from_transport(Z: torch.Tensor, threshold: float):
    """Z (N + 1, M + 1) -> matches0 (N,) int with -1 for none, matching_scores0 (N,)."""
    inner = Z[:-1, :-1]
    m0, m1 = inner.max(1), inner.max(0)
    i0, i1 = m0.indices, m1.indices
    mutual = torch.arange(len(i0)) == i1[i0]
    ms = torch.where(mutual, m0.values.exp(), torch.zeros_like(m0.values))
    valid = mutual & (ms > threshold)
    return torch.where(valid, i0, torch.full_like(i0, -1)).to(torch.int32), ms


def superglue(sd, kp0, sc0, d0, kp1, sc1, d1, H: int, W: int, cfg) -> dict:
    """keypoints (n, 2), scores (n,), descriptors (256, n) of both images -> the GNN output descriptors, the score matrix,
    the transport matrix Z, matches0 and matching_scores0."""
    n0, n1 = kp0.shape[0], kp1.shape[0]
    if n0 == 0 or n1 == 0:
        return {"matches0": torch.full((n0,), -1, dtype=torch.int32), "matching_scores0": torch.zeros(n0, dtype=d0.dtype)}

    def encode(kp, sc, d):
        size = torch.tensor([float(W), float(H)]).to(kp)
        k = (kp - size / 2) / (size.max() * 0.7)
        return d + _mlp(sd, "kenc.encoder", 5, torch.cat([k.t(), sc[None]], 0))

    x0, x1 = encode(kp0, sc0, d0), encode(kp1, sc1, d1)
    for l in range(18):
        p = f"gnn.layers.{l}"
        s0, s1 = (x1, x0) if l % 2 else (x0, x1)           # ['self', 'cross'] * 9
        x0, x1 = x0 + _propagate(sd, p, x0, s0), x1 + _propagate(sd, p, x1, s1)
    m0, m1 = _conv1(sd, "final_proj", x0), _conv1(sd, "final_proj", x1)
    scores = torch.einsum("dn,dm->nm", m0, m1) / 256 ** 0.5
    Z = log_optimal_transport(scores, sd["bin_score"].to(scores), cfg["sinkhorn_iterations"])
    matches0, ms0 = matches_from_transport(Z, cfg["match_threshold"])
    return {"gnn0": x0, "gnn1": x1, "scores": scores, "Z": Z, "matches0": matches0, "matching_scores0": ms0}


def select_points(kp0, kp1, matches0, masks, pos: int, neg: int):
    """The tracker's per-mask draw for one frame (tracker.py:131-186), consuming np.random's global generator exactly as the
    reference does: for every mask, positives then negatives, ``choice(a=len, size=min(len, k))``.  The matched frame-i
    points are split by whether their OWN coordinates lie inside the frame-0 mask (the reference's quirk, kept).
    -> points (n_masks, pos + neg, 2), visibilities (n_masks, pos + neg)."""
    valid = (matches0 > -1).numpy()
    mk1 = kp1.numpy()[matches0.numpy()[valid]]
    pts = np.full((masks.shape[0], pos + neg, 2), -1.0, dtype=np.float32)
    vis = np.zeros((masks.shape[0], pos + neg), dtype=np.float32)
    for mi in range(masks.shape[0]):
        m = (masks[mi] > 0.5).numpy()
        inside = m[mk1[:, 1].astype(int), mk1[:, 0].astype(int)]
        for lst, want, off in ((mk1[inside], pos, 0), (mk1[~inside], neg, pos)):
            idx = np.random.choice(a=len(lst), size=min(len(lst), want))
            pts[mi, off:off + len(idx)] = lst[idx]
            vis[mi, off:off + len(idx)] = 1
    return pts, vis


def track(sp_sd, sg_sd, frames_u8, masks, query_points, config=None, pos=GOLDEN_POS, neg=GOLDEN_NEG, dtype=torch.float32,
          detail: bool = False):
    """The whole tracker on one clip: frames uint8 (T,3,H,W), masks (n_masks,H,W), query_points (1, n_masks * (pos + neg), 3)
    -> trajectories (1,T,n,2), visibilities (1,T,n) [, per-frame SuperPoint results, per-pair SuperGlue results]."""
    config = config or GOLDEN_CONFIG
    T, _, H, W = frames_u8.shape
    nm, P = masks.shape[0], pos + neg
    with torch.no_grad():
        grey = grey_frames(frames_u8, dtype)
        sp = [superpoint(sp_sd, grey[t], config["superpoint"]) for t in range(T)]
        traj = torch.zeros(T, nm, P, 2)
        vis = torch.zeros(T, nm, P)
        traj[0] = query_points[0, :, 1:].reshape(nm, P, 2)
        pairs = []
        for t in range(1, T):
            a, b = sp[0], sp[t]
            r = superglue(sg_sd, a["keypoints"], a["scores"], a["descriptors"], b["keypoints"], b["scores"], b["descriptors"], H, W,
                          config["superglue"])
            pairs.append(r)
            p, v = select_points(a["keypoints"].float(), b["keypoints"].float(), r["matches0"], masks, pos, neg)
            traj[t], vis[t] = torch.from_numpy(p), torch.from_numpy(v)
    out = traj.reshape(1, T, nm * P, 2), vis.reshape(1, T, nm * P)
    return (out + (sp, pairs)) if detail else out
