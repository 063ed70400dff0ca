"""TEST INFRASTRUCTURE ONLY: the reference's RAFT point tracker run in place on the CPU, and a restatement of it.

``load_reference()`` imports ``sam_pt/point_tracker/raft`` from the reference tree by path (namespace modules for the
packages whose ``__init__`` files pull absent third-party code, a stub for ``cv2`` which ``utils/improc`` imports); nothing
of the reference is copied.  ``available()`` is false where the tree is absent.

The rest of the file is RAFT restated in this project's own words as functions over a state dict (key names of
``raft-things.pth`` without ``module.``): it stands in for the reference where the tree does not exist (the GPU tests), and
tests/test_raft_cpu.py pins it to the live reference and to tests/golden/raft_ref.npz.  Unlike the reference it runs each
encoder once per frame and the mask head once per pair; neither changes a number that is compared.
"""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle.reference_loader import REF, _link_children, _ns

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_ref.npz")
RAFT_DIR = os.path.join(REF, "sam_pt", "point_tracker", "raft")


def available() -> bool:
    return os.path.isfile(os.path.join(RAFT_DIR, "tracker.py")) and os.path.isfile(os.path.join(RAFT_DIR, "raft_core", "raft.py"))


def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------- the live reference
def load_reference():
    """-> (Raftnet, RaftPointTracker, raft_core.raft module) of the reference, imported in place."""
    assert available(), "reference tree not present"
    sys.dont_write_bytecode = True
    for n, p in [("sam_pt", "/sam_pt"), ("sam_pt.point_tracker", "/sam_pt/point_tracker"),
                 ("sam_pt.point_tracker.utils", "/sam_pt/point_tracker/utils"),
                 ("sam_pt.point_tracker.raft", "/sam_pt/point_tracker/raft"),
                 ("sam_pt.point_tracker.raft.raft_core", "/sam_pt/point_tracker/raft/raft_core")]:
        _ns(n, p)

    def stub(name):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        return sys.modules[name]

    stub("cv2")
    # utils/improc also wants matplotlib.pyplot and matplotlib.cm for its drawing helpers; another loader of this test suite may
    # have registered an empty ``matplotlib`` already, and the package may be absent altogether
    for sub in ("pyplot", "cm"):
        try:
            importlib.import_module("matplotlib." + sub)
        except Exception:
            setattr(stub("matplotlib"), sub, stub("matplotlib." + sub))
    T = importlib.import_module("sam_pt.point_tracker.tracker")
    sys.modules["sam_pt.point_tracker"].PointTracker = T.PointTracker
    importlib.import_module("sam_pt.point_tracker.utils.basic")
    importlib.import_module("sam_pt.point_tracker.utils.improc")
    importlib.import_module("sam_pt.point_tracker.utils.samp")
    core = importlib.import_module("sam_pt.point_tracker.raft.raft_core.raft")
    net = importlib.import_module("sam_pt.point_tracker.raft.raftnet")
    _link_children()
    trk = importlib.import_module("sam_pt.point_tracker.raft.tracker")
    _link_children()
    return net.Raftnet, trk.RaftPointTracker, core


def reference_tracker(sd, dtype=torch.float32):
    """The reference's RaftPointTracker(checkpoint_path=None) with ``sd`` loaded (strict), in eval mode."""
    import contextlib
    import io
    _, Tracker, _ = load_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        trk = Tracker(None)
    trk.model.model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    trk.eval()
    if dtype != torch.float32:
        trk.to(dtype)
    return trk


def reference_flow(trk, frame1, frame2, iters=32):
    """Raftnet.forward on two uint8 frames (3,H,W) the way the tracker calls it -> (flow_low (2,h8,w8), flow_up (2,H,W))."""
    dt = next(trk.model.parameters()).dtype
    low = {}
    raft = trk.model.model
    orig = raft.forward

    def spy(*a, **k):
        out = orig(*a, **k)
        low["flow"] = out[0]
        return out

    raft.forward = spy
    try:
        with torch.no_grad():
            a = frame1[None].to(dt) * 1. / 255 - 0.5                      # improc.preprocess_color
            b = frame2[None].to(dt) * 1. / 255 - 0.5
            up = trk.model.forward(a, b, iters=iters)[0]
    finally:
        del raft.forward
    return low["flow"][0], up[0]


# ---------------------------------------------------------------------------------------------- the restatement
def padding(H, W):
    """(left, right, top, bottom) of the replicate padding to multiples of 8: half before, the rest after."""
    ph, pw = (-H) % 8, (-W) % 8
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def prepare(frames):
    """uint8 (T,3,H,W) -> padded float frames in [-1, 1]."""
    x = F.pad(frames.float(), padding(*frames.shape[-2:]), mode="replicate")
    return 2 * (x / 255.0) - 1.0


def encoder(sd, enc, x):
    """BasicEncoder: fnet normalises per sample, cnet with its stored batch statistics.  x (N,3,H,W) -> (N,256,H/8,W/8)."""
    def conv(name, t, stride, pad):
        return F.conv2d(t, sd[name + ".weight"].to(t.dtype), sd[name + ".bias"].to(t.dtype), stride=stride, padding=pad)

    def norm(name, t):
        if enc == "fnet":
            return F.instance_norm(t, eps=1e-5)
        g = lambda k: sd[f"{name}.{k}"].to(t.dtype)
        return F.batch_norm(t, g("running_mean"), g("running_var"), g("weight"), g("bias"), False, 0.0, 1e-5)

    x = F.relu(norm(enc + ".norm1", conv(enc + ".conv1", x, 2, 3)))
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        for bi in (0, 1):
            p, st = f"{enc}.layer{li}.{bi}", (stride if bi == 0 else 1)
            y = F.relu(norm(p + ".norm1", conv(p + ".conv1", x, st, 1)))
            y = F.relu(norm(p + ".norm2", conv(p + ".conv2", y, 1, 1)))
            if st != 1:
                x = norm(p + ".norm3", conv(p + ".downsample.0", x, st, 0))
            x = F.relu(x + y)
    return conv(enc + ".conv2", x, 1, 0)


def corr_pyramid(fmap1, fmap2):
    """fmaps (256,h,w) -> 4 levels [(h*w, h_l, w_l)]: all-pairs dot products / 16, then 2 x 2 average pooling (floor sizes)."""
    c, h, w = fmap1.shape
    corr = (fmap1.reshape(c, h * w).t() @ fmap2.reshape(c, h * w)).reshape(h * w, 1, h, w) / (c ** 0.5)
    levels = [corr]
    for _ in range(3):
        levels.append(F.avg_pool2d(levels[-1], 2, stride=2))
    return [lv[:, 0] for lv in levels]


def lookup(levels, coords):
    """levels [(n, h_l, w_l)], coords (n, 2) = (x, y) -> (n, 324).  Channel l*81 + i*9 + j is level l sampled bilinearly at
    (x / 2^l + i - 4, y / 2^l + j - 4); corners outside the level count as zero."""
    n = coords.shape[0]
    d = torch.arange(-4, 5, dtype=coords.dtype)
    rows = torch.arange(n)[:, None, None]
    out = []
    for l, lv in enumerate(levels):
        H, W = lv.shape[-2:]
        x = (coords[:, 0, None, None] / 2 ** l + d[None, :, None]).expand(n, 9, 9)
        y = (coords[:, 1, None, None] / 2 ** l + d[None, None, :]).expand(n, 9, 9)
        x0, y0 = x.floor(), y.floor()

        def tap(yy, xx):
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = lv[rows, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()]
            return torch.where(ok, v, torch.zeros_like(v))

        wx1, wy1 = x - x0, y - y0
        wx0, wy0 = (x0 + 1) - x, (y0 + 1) - y
        v = tap(y0, x0) * (wx0 * wy0) + tap(y0, x0 + 1) * (wx1 * wy0) + tap(y0 + 1, x0) * (wx0 * wy1) \
            + tap(y0 + 1, x0 + 1) * (wx1 * wy1)
        out.append(v.reshape(n, 81))
    return torch.cat(out, dim=1)


def update_step(sd, net, inp, corr, flow):
    """One BasicUpdateBlock step without its mask head: (net', delta_flow); tensors (1,C,h,w)."""
    u = "update_block."

    def conv(name, t, pad):
        return F.conv2d(t, sd[u + name + ".weight"].to(t.dtype), sd[u + name + ".bias"].to(t.dtype), padding=pad)

    cor = F.relu(conv("encoder.convc2", F.relu(conv("encoder.convc1", corr, 0)), 1))
    flo = F.relu(conv("encoder.convf2", F.relu(conv("encoder.convf1", flow, 3)), 1))
    motion = torch.cat([F.relu(conv("encoder.conv", torch.cat([cor, flo], 1), 1)), flow], 1)
    x = torch.cat([inp, motion], 1)
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([net, x], 1)
        z = torch.sigmoid(conv("gru.convz" + n, hx, pad))
        r = torch.sigmoid(conv("gru.convr" + n, hx, pad))
        q = torch.tanh(conv("gru.convq" + n, torch.cat([r * net, x], 1), pad))
        net = (1 - z) * net + z * q
    delta = conv("flow_head.conv2", F.relu(conv("flow_head.conv1", net, 1)), 1)
    return net, delta


def mask_head(sd, net):
    u = "update_block.mask."
    t = F.relu(F.conv2d(net, sd[u + "0.weight"].to(net.dtype), sd[u + "0.bias"].to(net.dtype), padding=1))
    return 0.25 * F.conv2d(t, sd[u + "2.weight"].to(net.dtype), sd[u + "2.bias"].to(net.dtype))


def upsample(flow, mask):
    """flow (2,h,w), mask (576,h,w) -> (2,8h,8w): per fine pixel a softmax-weighted mean of the 3 x 3 coarse neighbours of 8*flow."""
    _, h, w = flow.shape
    wgt = torch.softmax(mask.reshape(9, 8, 8, h, w), dim=0)
    fl = F.pad(8 * flow, (1, 1, 1, 1))
    taps = torch.stack([fl[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)])      # (9,2,h,w)
    up = (wgt[:, None] * taps[:, :, None, None]).sum(0)                                            # (2,8,8,h,w)
    return up.permute(0, 3, 1, 4, 2).reshape(2, 8 * h, 8 * w)


def unpad(x, H, W):
    l, _, t, _ = padding(H, W)
    return x[..., t:t + H, l:l + W]


def grid(h, w, dtype=torch.float32):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return torch.stack([xx, yy])


def features(sd, frames, dtype=torch.float32):
    """Per frame: fmap (T,256,h,w), tanh(net) (T,128,h,w), relu(inp) (T,128,h,w)."""
    x = prepare(frames).to(dtype)
    fmap = torch.cat([encoder(sd, "fnet", x[t:t + 1]) for t in range(x.shape[0])])
    ctx = torch.cat([encoder(sd, "cnet", x[t:t + 1]) for t in range(x.shape[0])])
    return fmap, torch.tanh(ctx[:, :128]), torch.relu(ctx[:, 128:])


def pair_flow(sd, fmap1, fmap2, net, inp, iters, record=None):
    """-> flow_low (2,h,w), mask (576,h,w).  record (dict, optional): {"iter": k} asks for the state of iteration k."""
    _, h, w = fmap1.shape
    levels = corr_pyramid(fmap1, fmap2)
    c0 = grid(h, w, fmap1.dtype)
    c1 = c0.clone()
    net, inp = net[None], inp[None]
    for it in range(iters):
        corr = lookup(levels, c1.reshape(2, -1).t()).t().reshape(1, 324, h, w)
        flow = (c1 - c0)[None]
        net, delta = update_step(sd, net, inp, corr, flow)
        if record is not None and record.get("iter") == it:
            record.update(levels=levels, coords=c1.clone(), lookup=corr[0].clone(), net=net[0].clone())
        c1 = c1 + delta[0]
    return c1 - c0, mask_head(sd, net)[0]


def flows(sd, frames, iters=32, dtype=torch.float32):
    """uint8 (T,3,H,W) -> flows_forward, flows_backward (T-1,2,H,W) and the 1/8-resolution flows (2,T-1,2,h,w)."""
    with torch.no_grad():
        sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
        T, _, H, W = frames.shape
        fmap, net, inp = features(sd, frames, dtype)
        out = [[], []]
        low = [[], []]
        for t in range(T - 1):
            for d, (a, b) in enumerate(((t, t + 1), (t + 1, t))):
                fl, mask = pair_flow(sd, fmap[a], fmap[b], net[a], inp[a], iters)
                low[d].append(fl)
                out[d].append(unpad(upsample(fl, mask), H, W))
        return torch.stack(out[0]), torch.stack(out[1]), torch.stack([torch.stack(low[0]), torch.stack(low[1])])


def sample(flow, xy):
    """flow (2,H,W) at points xy (N,2): bilinear with indices clamped to the frame and weights from the un-clamped floor."""
    _, H, W = flow.shape
    x, y = xy[:, 0], xy[:, 1]
    x0, y0 = x.floor().int(), y.floor().int()
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1, cy0, cy1 = x0.clamp(0, W - 1).long(), x1.clamp(0, W - 1).long(), y0.clamp(0, H - 1).long(), y1.clamp(0, H - 1).long()
    w00 = ((x1.float() - x) * (y1.float() - y))[:, None]
    w01 = ((x - x0.float()) * (y1.float() - y))[:, None]
    w10 = ((x1.float() - x) * (y - y0.float()))[:, None]
    w11 = ((x - x0.float()) * (y - y0.float()))[:, None]
    f = flow.permute(1, 2, 0)
    return w00 * f[cy0, cx0] + w01 * f[cy0, cx1] + w10 * f[cy1, cx0] + w11 * f[cy1, cx1]


def chain(fwd, bwd, q):
    """flows (T-1,2,H,W), q (N,3) = (t, x, y) -> trajectories (T,N,2), visibilities (T,N) bool."""
    T, (H, W) = fwd.shape[0] + 1, fwd.shape[-2:]
    q = q.float()
    coords = []
    for t in range(T):
        c = torch.zeros_like(q[:, 1:]) if t == 0 else coords[t - 1] + sample(fwd[t - 1], coords[t - 1])
        coords.append(torch.where((q[:, 0] == t)[:, None], q[:, 1:], c))
    for t in range(T - 2, -1, -1):
        back = coords[t + 1] + sample(bwd[t], coords[t + 1])
        coords[t] = torch.where((t < q[:, 0])[:, None], back, coords[t])
    traj = torch.stack(coords)
    vis = (traj[..., 0] >= 0) & (traj[..., 1] >= 0) & (traj[..., 0] < W) & (traj[..., 1] < H)
    return traj, vis


def track(sd, frames, q, iters=32):
    fwd, bwd, _ = flows(sd, frames, iters)
    return chain(fwd, bwd, q)
