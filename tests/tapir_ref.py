"""TEST INFRASTRUCTURE ONLY: TAPIR (sam_pt/point_tracker/tapir/) restated in this project's own words, in plain PyTorch.

STATUS: PARITY UNPINNED.  The reference model is JAX / Haiku code and needs a checkpoint; none of the three exists where this
project is built, so the model half of this file cannot be run against the reference.  It is written from
``tapir_model.py`` (heads :349-417, refinement :419-567, features :569-771, iterations :773-1053), ``models/resnet.py``
(:153-258, :306-472) and ``utils/model_utils.py`` (:69-206) by reading.  What can be pinned is pinned by
tests/test_tapir_cpu.py: the coordinate conversion against the reference's NumPy-only ``utils/transforms.py``, the two bilinear
reads against scipy, TensorFlow's "SAME" padding against its closed formula, and the adapter (``tracker.py:72-108``) against the
reference's own ``TapirPointTracker.forward`` run in place over small stand-in modules.

Everything is a function over a flat state dict (names: sam_pt_amd.weights.init_tapir_state_dict).  ``dtype`` switches the whole
computation between float32 and float64.  Conventions of the reference that matter:

  * one resolution: the adapter always hands the model 256 x 256 frames, so one ResNet pass serves the heads and the four
    refinements, and the result is the fourth refinement alone;
  * Haiku convolutions have no bias in the ResNet and pad "SAME" the TensorFlow way (more padding after than before);
  * ``jax.nn.gelu`` is the tanh approximation; depthwise output channel c * 4 + m belongs to input channel c;
  * ``map_coordinates(order=1, mode='constant')`` in JAX zeroes every CORNER that lies outside the map (scipy calls this
    'grid-constant'; scipy's own 'constant' returns 0 for every sample outside the map's extent).
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle.reference_loader import REF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tapir_ref.npz")
TAPIR_DIR = os.path.join(REF, "sam_pt", "point_tracker", "tapir")
SIZE = 256                                     # the adapter's resize_height / resize_width
GROUPS = ((64, 1), (128, 2), (256, 2), (256, 1))   # channels, stride of the four block groups
N_BLOCKS, DIM, PATCH, ITERS, TEMPERATURE = 12, 512, 7, 4, 20.0


def available() -> bool:
    return os.path.isfile(os.path.join(TAPIR_DIR, "tracker.py")) and os.path.isfile(os.path.join(TAPIR_DIR, "utils", "transforms.py"))


def golden():
    return np.load(GOLDEN)


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------- small pieces
def convert_grid_coordinates(coords, input_grid_size, output_grid_size):
    """utils/transforms.py:25-79 — a plain ratio, no half-pixel shift."""
    return coords * torch.as_tensor(output_grid_size, dtype=coords.dtype) / torch.as_tensor(input_grid_size, dtype=coords.dtype)


def same_padding(side: int, k: int, stride: int):
    """TensorFlow 'SAME': output ceil(side / stride); the padding that needs is split floor / ceil (before, after)."""
    out = -(-side // stride)
    total = max((out - 1) * stride + k - side, 0)
    return total // 2, total - total // 2


def conv_same(x, w, stride=1, bias=None):
    """x (B,C,H,W), w (O,I,k,k)."""
    pt, pb = same_padding(x.shape[2], w.shape[2], stride)
    pl, pr = same_padding(x.shape[3], w.shape[3], stride)
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, bias, stride=stride)


def instance_norm(x, scale, offset, eps=1e-5):
    mean = x.mean((2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((2, 3), keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * scale[None, :, None, None] + offset[None, :, None, None]


def layer_norm(x, scale, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * scale


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def bilinear(grid, yx, mode):
    """grid (H,W,C); yx (...,2) in index coordinates (the caller has subtracted the half pixel) -> (...,C).
    mode 'nearest': corner indices are clamped to the map; 'constant': a corner outside the map contributes zero."""
    H, W = grid.shape[:2]
    y, x = yx[..., 0], yx[..., 1]
    y0, x0 = torch.floor(y), torch.floor(x)
    wy1, wx1 = y - y0, x - x0
    wy0, wx0 = 1 - wy1, 1 - wx1
    y0, x0 = y0.long(), x0.long()
    out = 0
    for yi, wy in ((y0, wy0), (y0 + 1, wy1)):
        for xi, wx in ((x0, wx0), (x0 + 1, wx1)):
            v = grid[yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
            if mode == "constant":
                inside = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)
                v = v * inside[..., None].to(v.dtype)
            out = out + (wy * wx)[..., None] * v
    return out


# ---------------------------------------------------------------------------------------------- backbone
def backbone(sd, video):
    """video (T,256,256,3) in [-1, 1] -> hires (T,64,64,128), lowres (T,32,32,256), each divided by its channel norm."""
    x = conv_same(video.permute(0, 3, 1, 2), sd["resnet.initial_conv.weight"], 2)
    units = []
    for g, (_, stride) in enumerate(GROUPS):
        for b in range(2):
            p = f"resnet.g{g}.b{b}."
            st = stride if b == 0 else 1
            shortcut = x
            y = F.relu(instance_norm(x, sd[p + "norm0.scale"], sd[p + "norm0.offset"]))
            if b == 0:
                shortcut = conv_same(y, sd[p + "shortcut.weight"], st)           # the projection reads the normalised map
            y = conv_same(y, sd[p + "conv0.weight"], st)
            y = F.relu(instance_norm(y, sd[p + "norm1.scale"], sd[p + "norm1.offset"]))
            x = conv_same(y, sd[p + "conv1.weight"], 1) + shortcut
        units.append(x)

    def unit(v):
        v = v.permute(0, 2, 3, 1)
        return v / torch.sqrt(torch.clamp((v * v).sum(-1, keepdim=True), min=1e-12))

    return unit(units[1]), unit(units[3])


def query_features(hires, lowres, q_tyx):
    """q_tyx (N,3) in frame / 256-pixel coordinates -> (N,384) = hires (128) | lowres (256), edge-clamped bilinear reads."""
    t = torch.round(q_tyx[:, 0]).long()
    out = []
    for grid in (hires, lowres):
        scale = grid.shape[1] / SIZE
        rows = [bilinear(grid[t[i]], q_tyx[i, 1:] * scale - 0.5, "nearest") for i in range(q_tyx.shape[0])]
        out.append(torch.stack(rows))
    return torch.cat(out, -1)


# ---------------------------------------------------------------------------------------------- cost-volume heads
def soft_argmax(sm, threshold=5.0):
    """sm (...,h,w) softmax maps -> (...,2) = (x, y) in grid cells: the softmax-weighted mean of the cell centres closer than
    `threshold` to the centre of the first maximal cell in row-major order."""
    h, w = sm.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=sm.dtype), torch.arange(w, dtype=sm.dtype), indexing="ij")
    coords = torch.stack([xs + 0.5, ys + 0.5], -1)                                  # (h,w,2)
    flat = sm.reshape(-1, h * w)
    best = torch.argmax(flat, -1)                                                  # the first maximum
    pos = coords.reshape(-1, 2)[best].reshape(sm.shape[:-2] + (1, 1, 2))
    valid = (((coords - pos) ** 2).sum(-1, keepdim=True) < threshold ** 2).to(sm.dtype)
    wsum = (coords * valid * sm[..., None]).sum((-3, -2))
    norm = torch.clamp((valid * sm[..., None]).sum((-3, -2)), min=1e-12)
    return wsum / norm


def heads(sd, qlow, lowres, q_tyx, return_logits=False):
    """qlow (N,256), lowres (T,32,32,256), q_tyx (N,3) -> points (N,T,2) px, occlusion (N,T), expected_dist (N,T)."""
    T, gh, gw, _ = lowres.shape
    N = qlow.shape[0]
    cost = torch.einsum("nc,thwc->tnhw", qlow, lowres).reshape(T * N, 1, gh, gw)
    hid = F.relu(conv_same(cost, sd["heads.hid1.weight"], 1, sd["heads.hid1.bias"]))
    logits = conv_same(hid, sd["heads.hid2.weight"], 1, sd["heads.hid2.bias"]).reshape(T, N, gh, gw).permute(1, 0, 2, 3)
    sm = torch.softmax((logits * TEMPERATURE).reshape(N, T, -1), -1).reshape(N, T, gh, gw)
    points = convert_grid_coordinates(soft_argmax(sm), (gw, gh), (SIZE, SIZE))
    is_query = (torch.round(q_tyx[:, 0]).long()[:, None] == torch.arange(T)[None]).to(points.dtype)[..., None]
    points = points * (1 - is_query) + q_tyx[:, None, [2, 1]] * is_query
    occ = F.relu(conv_same(hid, sd["heads.hid3.weight"], 2, sd["heads.hid3.bias"])).mean((2, 3))
    occ = F.relu(occ @ sd["heads.hid4.weight"].t() + sd["heads.hid4.bias"])
    occ = (occ @ sd["heads.occ_out.weight"].t() + sd["heads.occ_out.bias"]).reshape(T, N, 2).permute(1, 0, 2)
    if return_logits:
        return points, occ[..., 0], occ[..., 1], logits
    return points, occ[..., 0], occ[..., 1]


# ---------------------------------------------------------------------------------------------- refinement
def patch_correlation(grid, pos, vec):
    """grid (T,H,W,C), pos (N,T,2) = (x, y) in 256 px, vec (N,C) or (N,T,C) -> (N,T,49): sample s = i * 7 + j sits at
    (y + i - 3, x + j - 3) grid cells, read bilinearly with zero outside, dotted with vec."""
    T, gh, gw, _ = grid.shape
    yx = convert_grid_coordinates(pos, (SIZE, SIZE), (gw, gh)).flip(-1)
    r = torch.arange(-(PATCH // 2), PATCH // 2 + 1, dtype=pos.dtype)
    off = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2)               # (49,2) = (dy, dx)
    at = yx[:, :, None, :] + off[None, None] - 0.5                                         # (N,T,49,2)
    if vec.dim() == 2:
        vec = vec[:, None].expand(-1, T, -1)
    out = [torch.einsum("nsc,nc->ns", bilinear(grid[t], at[:, t], "constant"), vec[:, t]) for t in range(T)]
    return torch.stack(out, 1)


def temporal_half(sd, p, x):
    """x (N,T,512) -> x + fours(dw2(gelu(dw1(LN(x))))): depthwise k = 3 convolutions over time, zero padding at the clip ends."""
    N, T, D = x.shape
    y = layer_norm(x, sd[p + "ln1.scale"]).repeat_interleave(4, -1)                          # channel c feeds outputs 4c .. 4c+3
    w1, w2 = sd[p + "dw1.weight"], sd[p + "dw2.weight"]                                      # (3, 2048): tap, channel
    yp = F.pad(y, (0, 0, 1, 1))
    g = gelu_tanh(yp[:, 0:T] * w1[0] + yp[:, 1:T + 1] * w1[1] + yp[:, 2:T + 2] * w1[2] + sd[p + "dw1.bias"])
    gp = F.pad(g, (0, 0, 1, 1))
    z = gp[:, 0:T] * w2[0] + gp[:, 1:T + 1] * w2[1] + gp[:, 2:T + 2] * w2[2] + sd[p + "dw2.bias"]
    z = z.reshape(N, T, D, 4)
    return z[..., 0] + z[..., 1] + z[..., 2] + z[..., 3] + x


def channel_half(sd, p, x):
    y = layer_norm(x, sd[p + "ln2.scale"])
    y = gelu_tanh(y @ sd[p + "up.weight"].t() + sd[p + "up.bias"])
    return y @ sd[p + "down.weight"].t() + sd[p + "down.bias"] + x


def mixer_block(sd, i, x):
    p = f"mixer.blocks.{i}."
    return channel_half(sd, p, temporal_half(sd, p, x))


def mixer(sd, x):
    x = x @ sd["mixer.in.weight"].t() + sd["mixer.in.bias"]
    for i in range(N_BLOCKS):
        x = mixer_block(sd, i, x)
    return layer_norm(x, sd["mixer.ln_out.scale"]) @ sd["mixer.out.weight"].t() + sd["mixer.out.bias"]


def mixer_input(hires, lowres, qf, pos, occ, expd, feats):
    """The 486 columns of a (query, frame) row: 0, 0, occlusion, expected_dist, features (384), 49 + 49 correlations."""
    N, T = occ.shape
    base = qf[:, None].expand(-1, T, -1) if feats is None else feats
    vh, vl = (qf[:, :128], qf[:, 128:]) if feats is None else (feats[..., :128], feats[..., 128:])
    corr = torch.cat([patch_correlation(hires, pos, vh), patch_correlation(lowres, pos, vl)], -1)
    return torch.cat([torch.zeros_like(pos), occ[..., None], expd[..., None], base, corr], -1), base


def refine(sd, hires, lowres, qf, pos, occ, expd, feats):
    """One refinement: feats None on the first iteration (the query features stand in).  -> pos, occ, expd, feats."""
    x, base = mixer_input(hires, lowres, qf, pos, occ, expd, feats)
    res = mixer(sd, x)
    return pos + res[..., :2], occ + res[..., 2], expd + res[..., 3], base + res[..., 4:]


def forward(sd, video, q_tyx, iters=ITERS, dtype=torch.float32, stages=False):
    """video (T,256,256,3) in [-1, 1], q_tyx (N,3) -> dict: tracks (N,T,2), occlusion, expected_dist (N,T) = the last iteration, and
    iter_tracks / iter_occlusion / iter_expected_dist lists over iterations 0 .. iters."""
    sd = cast(sd, dtype)
    video, q_tyx = video.to(dtype), q_tyx.to(dtype)
    with torch.no_grad():
        hires, lowres = backbone(sd, video)
        qf = query_features(hires, lowres, q_tyx)
        pos, occ, expd, logits = heads(sd, qf[:, 128:], lowres, q_tyx, return_logits=True)
        its = [(pos, occ, expd)]
        feats = None
        for _ in range(iters):
            pos, occ, expd, feats = refine(sd, hires, lowres, qf, pos, occ, expd, feats)
            its.append((pos, occ, expd))
    out = dict(tracks=pos, occlusion=occ, expected_dist=expd, iter_tracks=[i[0] for i in its], iter_occlusion=[i[1] for i in its],
               iter_expected_dist=[i[2] for i in its])
    if stages:
        out.update(hires=hires, lowres=lowres, qf=qf, logits=logits, feats=feats)
    return out


def model_fn(sd, dtype=torch.float32):
    """The callable the reference adapter calls ``jitted_forward``: (video (B,T,256,256,3) numpy, query (B,N,3) = (t, y, x) numpy) ->
    dict of numpy tracks (B,N,T,2), occlusion and expected_dist (B,N,T)."""
    def run(video, query):
        outs = [forward(sd, torch.as_tensor(np.asarray(video[b])), torch.as_tensor(np.asarray(query[b])), dtype=dtype)
                for b in range(len(video))]
        return {k: np.stack([o[k].float().numpy() for o in outs]) for k in ("tracks", "occlusion", "expected_dist")}
    return run


def visibility_probability(occ, expd):
    return (1 - torch.sigmoid(occ)) * (1 - torch.sigmoid(expd))


# ---------------------------------------------------------------------------------------------- the live reference adapter
def load_transforms():
    """The reference's utils/transforms.py (NumPy only), loaded by file path."""
    spec = importlib.util.spec_from_file_location("_tapir_transforms_ref", os.path.join(TAPIR_DIR, "utils", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def reference_tracker(model, visibility_threshold=0.1):
    """The reference's TapirPointTracker, imported in place, whose model is ``model`` (see ``model_fn``).  ``tensorflow``,
    ``jaxline.base_config`` and ``ml_collections.config_dict`` are small stand-ins registered only while it is built; ``haiku`` and
    ``jax`` are never imported because ``_create_jitted_forward`` is replaced before the constructor calls it."""
    assert available(), "reference tree not present"

    class ConfigDict(dict):
        def __init__(self, d=None):
            super().__init__()
            for k, v in (d or {}).items():
                self[k] = ConfigDict(v) if isinstance(v, dict) and not isinstance(v, ConfigDict) else v
        __getattr__ = dict.__getitem__

        def __setattr__(self, k, v):
            self[k] = v

        def lock(self):
            return self

        def get_oneway_ref(self, key):
            return self[key]

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    tf = mod("tensorflow")
    tf.config = types.SimpleNamespace(experimental=types.SimpleNamespace(set_visible_devices=lambda *a, **k: None))
    base_config = mod("jaxline.base_config", get_base_config=lambda: ConfigDict())
    config_dict = mod("ml_collections.config_dict", ConfigDict=ConfigDict)
    stand_ins = {"tensorflow": tf, "jaxline": mod("jaxline", base_config=base_config), "jaxline.base_config": base_config,
                 "ml_collections": mod("ml_collections", config_dict=config_dict, ConfigDict=ConfigDict),
                 "ml_collections.config_dict": config_dict}
    pkgs = {n: mod(n) for n in ("sam_pt", "sam_pt.point_tracker", "sam_pt.point_tracker.tapir", "sam_pt.point_tracker.tapir.configs")}
    pkgs["sam_pt.point_tracker.tapir"].__path__ = [TAPIR_DIR]
    pkgs["sam_pt.point_tracker.tapir.configs"].__path__ = [os.path.join(TAPIR_DIR, "configs")]

    class PointTracker(torch.nn.Module):
        pass

    pkgs["sam_pt.point_tracker"].PointTracker = PointTracker
    saved = {k: sys.modules.get(k) for k in list(stand_ins) + list(pkgs) + ["sam_pt.point_tracker.tapir.tracker",
                                                                          "sam_pt.point_tracker.tapir.configs.tapir_config"]}
    sys.dont_write_bytecode = True
    try:
        sys.modules.update(stand_ins)
        sys.modules.update(pkgs)
        spec = importlib.util.spec_from_file_location("sam_pt.point_tracker.tapir.tracker", os.path.join(TAPIR_DIR, "tracker.py"))
        trk = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = trk
        spec.loader.exec_module(trk)
        trk.TapirPointTracker._create_jitted_forward = lambda self: model
        return trk.TapirPointTracker(checkpoint_path="unused", visibility_threshold=visibility_threshold)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
