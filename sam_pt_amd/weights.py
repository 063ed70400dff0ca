"""Seeded random-init state dicts in the *upstream checkpoint key layout*.

No checkpoints exist in this environment, so every model on the hot path is
driven by deterministic random weights.  The key names / shapes follow the real checkpoints so
that a genuine ``.pth`` drops in unchanged:

* PIPS   – ``model-*.pth['model_state_dict']`` of aharley/pips (module tree at
  /root/reference/sam_pt/point_tracker/pips/pips.py:191-287, 290-317, 410-437).
* SAM    – ``sam_vit_{b,l,h}.pth`` of facebookresearch/segment-anything @ aac76a1
  (hyper-parameters at /root/reference/configs/model/sam/**.yaml; key list in SURVEY.md App. C).

The generator is plain tensor code (CPU ``torch.Generator``), identical on every machine with the
same torch build, so the oracle and the HIP path always see the same numbers.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch


# --------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------
class _Init:
    def __init__(self, seed: int):
        self.g = torch.Generator(device="cpu")
        self.g.manual_seed(seed)
        self.sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()

    def uniform(self, name, shape, bound):
        self.sd[name] = (torch.rand(shape, generator=self.g, dtype=torch.float32) * 2 - 1) * bound

    def normal(self, name, shape, std, mean=0.0):
        self.sd[name] = torch.randn(shape, generator=self.g, dtype=torch.float32) * std + mean

    def linear(self, prefix, out_f, in_f, bias=True):
        b = 1.0 / math.sqrt(in_f)
        self.uniform(prefix + ".weight", (out_f, in_f), b)
        if bias:
            self.uniform(prefix + ".bias", (out_f,), b)

    def conv(self, prefix, out_c, in_c, kh, kw, bias=True, kaiming_fan_out=False):
        fan_in = in_c * kh * kw
        if kaiming_fan_out:  # pips.py:237-239 (kaiming_normal_, fan_out, relu)
            self.normal(prefix + ".weight", (out_c, in_c, kh, kw), math.sqrt(2.0 / (out_c * kh * kw)))
        else:
            self.uniform(prefix + ".weight", (out_c, in_c, kh, kw), 1.0 / math.sqrt(fan_in))
        if bias:
            self.uniform(prefix + ".bias", (out_c,), 1.0 / math.sqrt(fan_in))

    def norm(self, prefix, dim):
        # affine parameters perturbed away from (1, 0) so that parity tests exercise them
        self.normal(prefix + ".weight", (dim,), 0.05, mean=1.0)
        self.normal(prefix + ".bias", (dim,), 0.05)


# --------------------------------------------------------------------------------------
# PIPS
# --------------------------------------------------------------------------------------
PIPS_S = 8
PIPS_LATENT = 128
PIPS_CORR_LEVELS = 4
PIPS_CORR_RADIUS = 3
PIPS_MIXER_DIM = 512
PIPS_MIXER_DEPTH = 12
PIPS_KITCHEN_DIM = PIPS_CORR_LEVELS * (2 * PIPS_CORR_RADIUS + 1) ** 2 + PIPS_LATENT + 64 * 3 + 3  # 519


def init_pips_state_dict(seed: int = 72, S: int = PIPS_S, delta_scale: float = 0.05,
                         vis_bias: float = 2.0) -> "OrderedDict[str, torch.Tensor]":
    """Random PIPS weights, keys as in the reference module tree (pips.py:410-437).

    ``delta_scale`` shrinks the mixer's output head so that the 6-iteration update is contractive,
    like the trained model's.  With an unscaled random head every iteration moves points by several
    pixels and the 968-rad/px sin/cos flow embedding (utils/misc.py:30-55) amplifies fp32 round-off
    ~10x per iteration — even the reference run twice with a different op order diverges by 0.1 px
    after 6 iterations — which would make trajectory parity meaningless.  ``vis_bias`` centres the
    visibility head near the 0.9 linking threshold (pips/tracker.py:111-148) so both linking branches
    are exercised.  Pass ``delta_scale=1.0, vis_bias=0.0`` for an untouched default-style init.
    """
    w = _Init(seed)
    # --- fnet: BasicEncoder (pips.py:191-287), instance norm => no norm parameters
    w.conv("fnet.conv1", 64, 3, 7, 7, kaiming_fan_out=True)
    in_planes = 64
    for li, (dim, stride) in enumerate([(64, 1), (96, 2), (128, 2), (128, 2)], start=1):
        for bi in range(2):
            cin = in_planes if bi == 0 else dim
            p = f"fnet.layer{li}.{bi}"
            w.conv(p + ".conv1", dim, cin, 3, 3, kaiming_fan_out=True)
            w.conv(p + ".conv2", dim, dim, 3, 3, kaiming_fan_out=True)
            if bi == 0 and stride != 1:
                w.conv(p + ".downsample.0", dim, cin, 1, 1, kaiming_fan_out=True)
        in_planes = dim
    w.conv("fnet.conv2", 2 * PIPS_LATENT, 128 + 128 + 96 + 64, 3, 3, kaiming_fan_out=True)
    w.conv("fnet.conv3", PIPS_LATENT, 2 * PIPS_LATENT, 1, 1, kaiming_fan_out=True)
    # --- delta block: MLP-Mixer (pips.py:115-128, 290-317)
    d = PIPS_MIXER_DIM
    w.linear("delta_block.to_delta.0", d, PIPS_KITCHEN_DIM)
    for i in range(1, PIPS_MIXER_DEPTH + 1):
        p = f"delta_block.to_delta.{i}"
        w.norm(p + ".0.norm", d)
        w.conv(p + ".0.fn.0", 4 * S, S, 1, 1)  # Conv1d(k=1): squeeze last dim below
        w.conv(p + ".0.fn.3", S, 4 * S, 1, 1)
        for k in (".0.fn.0.weight", ".0.fn.3.weight"):
            w.sd[p + k] = w.sd[p + k].squeeze(-1)
        w.norm(p + ".1.norm", d)
        w.linear(p + ".1.fn.0", 4 * d, d)
        w.linear(p + ".1.fn.3", d, 4 * d)
    w.norm(f"delta_block.to_delta.{PIPS_MIXER_DEPTH + 1}", d)
    w.linear(f"delta_block.to_delta.{PIPS_MIXER_DEPTH + 3}", S * (PIPS_LATENT + 2), d)
    # --- heads (pips.py:427-437)
    w.norm("norm", PIPS_LATENT)
    w.linear("ffeat_updater.0", PIPS_LATENT, PIPS_LATENT)
    w.linear("vis_predictor.0", 1, PIPS_LATENT)
    head = f"delta_block.to_delta.{PIPS_MIXER_DEPTH + 3}"
    w.sd[head + ".weight"] *= delta_scale
    w.sd[head + ".bias"] *= delta_scale
    w.sd["vis_predictor.0.bias"] += vis_bias
    return w.sd


# --------------------------------------------------------------------------------------
# RAFT (princeton-vl/RAFT @ aac9dd5, vendored by the reference under sam_pt/point_tracker/raft/raft_core)
# --------------------------------------------------------------------------------------
def init_raft_state_dict(seed: int = 72) -> "OrderedDict[str, torch.Tensor]":
    """Random RAFT weights under the key names of ``raft-things.pth`` without the ``module.`` prefix (the module tree of
    raft_core/raft.py:57-59: ``fnet`` with InstanceNorm — no parameters —, ``cnet`` with BatchNorm, ``update_block``).

    The encoders keep their own kaiming fan-out init (extractor.py:149-151) and the update block PyTorch's default, which
    already gives flows of several pixels that converge over the 32 iterations (figures: DESIGN.md §4).  ``cnet``'s
    BatchNorms get non-trivial running statistics and affine terms, so that folding them into the convolutions
    (pack.pack_raft) is exercised.  ``norm3`` and ``downsample.1`` of a strided block are one module registered twice, as
    in the checkpoint."""
    w = _Init(seed)

    def bn(prefix, dim):
        w.normal(prefix + ".weight", (dim,), 0.1, mean=1.0)
        w.normal(prefix + ".bias", (dim,), 0.1)
        w.normal(prefix + ".running_mean", (dim,), 0.2)
        w.uniform(prefix + ".running_var", (dim,), 0.5)
        w.sd[prefix + ".running_var"] = w.sd[prefix + ".running_var"] + 1.0          # in [0.5, 1.5]
        w.sd[prefix + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    for enc, out_dim, batch in (("fnet", 256, False), ("cnet", 256, True)):
        if batch:
            bn(enc + ".norm1", 64)
        w.conv(enc + ".conv1", 64, 3, 7, 7, kaiming_fan_out=True)
        in_planes = 64
        for li, (dim, stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
            for bi in range(2):
                cin = in_planes if bi == 0 else dim
                p = f"{enc}.layer{li}.{bi}"
                w.conv(p + ".conv1", dim, cin, 3, 3, kaiming_fan_out=True)
                w.conv(p + ".conv2", dim, dim, 3, 3, kaiming_fan_out=True)
                if batch:
                    bn(p + ".norm1", dim)
                    bn(p + ".norm2", dim)
                if bi == 0 and stride != 1:
                    if batch:
                        bn(p + ".norm3", dim)
                    w.conv(p + ".downsample.0", dim, cin, 1, 1, kaiming_fan_out=True)
                    if batch:
                        for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                            w.sd[f"{p}.downsample.1.{k}"] = w.sd[f"{p}.norm3.{k}"]
            in_planes = dim
        w.conv(enc + ".conv2", out_dim, 128, 1, 1, kaiming_fan_out=True)
    u = "update_block."
    w.conv(u + "encoder.convc1", 256, 324, 1, 1)
    w.conv(u + "encoder.convc2", 192, 256, 3, 3)
    w.conv(u + "encoder.convf1", 128, 2, 7, 7)
    w.conv(u + "encoder.convf2", 64, 128, 3, 3)
    w.conv(u + "encoder.conv", 126, 256, 3, 3)
    for n, (kh, kw) in (("1", (1, 5)), ("2", (5, 1))):
        for g in ("z", "r", "q"):
            w.conv(f"{u}gru.conv{g}{n}", 128, 384, kh, kw)
    w.conv(u + "flow_head.conv1", 256, 128, 3, 3)
    w.conv(u + "flow_head.conv2", 2, 256, 3, 3)
    w.conv(u + "mask.0", 256, 128, 3, 3)
    w.conv(u + "mask.2", 576, 256, 1, 1)
    return w.sd


# --------------------------------------------------------------------------------------
# CoTracker v1 (facebookresearch/co-tracker @ 4f297a9, requirements.txt:29 — third-party, absent from the reference tree)
# --------------------------------------------------------------------------------------
COTRACKER_HIDDEN = 384
COTRACKER_HEADS = 8
COTRACKER_DEPTH = 6          # time_depth = space_depth = 6 (build_cotracker: cotracker_stride_4_wind_8.pth)
COTRACKER_INPUT_DIM = 456    # 130 flow embedding + 196 correlation + 128 track feature + 2 (track mask, visibility)


def init_cotracker_state_dict(seed: int = 72, delta_scale: float = 0.003, vis_bias: float = 0.0,
                              hidden: int = COTRACKER_HIDDEN, depth: int = COTRACKER_DEPTH) -> "OrderedDict[str, torch.Tensor]":
    """Random CoTracker weights with the key layout of ``cotracker_stride_4_wind_8.pth``: ``fnet.*`` =
    the same BasicEncoder tree as PIPS (instance norm: no norm parameters), ``updateformer.input_transform``,
    ``updateformer.{time,space}_blocks.{i}.{attn.qkv, attn.proj, mlp.fc1, mlp.fc2}`` (timm ``Attention`` / ``Mlp``; the
    blocks' LayerNorms are affine-free), ``updateformer.flow_head``, ``norm`` (GroupNorm), ``ffeat_updater.0``,
    ``vis_predictor.0``.  UpdateFormer linears are xavier-uniform with zero bias as upstream's ``initialize_weights``.
    ``delta_scale``: see ``init_pips_state_dict`` — with xavier weights and 12 residual blocks the unscaled random
    head moves points by pixels per iteration and the 968-rad/px flow embedding makes the model chaotic (a 1e-7 relative
    weight perturbation moves trajectories by 2.3 px at 0.05, 0.34 px at 0.01, 6e-4 px at 0.003), so 0.003 is the
    default.  The random visibility head already straddles the 0.7 threshold of configs/model/point_tracker/
    cotracker.yaml:7 (logits 1.6 +- 0.8 vs logit(0.7) = 0.85: ~80 % visible), so ``vis_bias`` defaults to 0."""
    w = _Init(seed)
    w.conv("fnet.conv1", 64, 3, 7, 7, kaiming_fan_out=True)
    in_planes = 64
    for li, (dim, stride) in enumerate([(64, 1), (96, 2), (128, 2), (128, 2)], start=1):
        for bi in range(2):
            cin = in_planes if bi == 0 else dim
            p = f"fnet.layer{li}.{bi}"
            w.conv(p + ".conv1", dim, cin, 3, 3, kaiming_fan_out=True)
            w.conv(p + ".conv2", dim, dim, 3, 3, kaiming_fan_out=True)
            if bi == 0 and stride != 1:
                w.conv(p + ".downsample.0", dim, cin, 1, 1, kaiming_fan_out=True)
        in_planes = dim
    w.conv("fnet.conv2", 2 * PIPS_LATENT, 128 + 128 + 96 + 64, 3, 3, kaiming_fan_out=True)
    w.conv("fnet.conv3", PIPS_LATENT, 2 * PIPS_LATENT, 1, 1, kaiming_fan_out=True)

    def xavier(prefix, out_f, in_f):
        w.uniform(prefix + ".weight", (out_f, in_f), math.sqrt(6.0 / (in_f + out_f)))
        w.sd[prefix + ".bias"] = torch.zeros(out_f)

    xavier("updateformer.input_transform", hidden, COTRACKER_INPUT_DIM)
    xavier("updateformer.flow_head", PIPS_LATENT + 2, hidden)
    for kind in ("time_blocks", "space_blocks"):
        for i in range(depth):
            p = f"updateformer.{kind}.{i}"
            xavier(p + ".attn.qkv", 3 * hidden, hidden)
            xavier(p + ".attn.proj", hidden, hidden)
            xavier(p + ".mlp.fc1", 4 * hidden, hidden)
            xavier(p + ".mlp.fc2", hidden, 4 * hidden)
    w.norm("norm", PIPS_LATENT)
    w.linear("ffeat_updater.0", PIPS_LATENT, PIPS_LATENT)
    w.linear("vis_predictor.0", 1, PIPS_LATENT)
    w.sd["updateformer.flow_head.weight"] *= delta_scale
    w.sd["updateformer.flow_head.bias"] *= delta_scale
    w.sd["vis_predictor.0.bias"] += vis_bias
    return w.sd


PIPS2_KITCHEN = 3 * PIPS_CORR_LEVELS * (2 * PIPS_CORR_RADIUS + 1) ** 2 + PIPS_LATENT + 2      # 718
PIPS2_BLOCKS = [(128, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024)]


def init_pips2_state_dict(seed: int = 72, delta_scale: float = 0.05) -> "OrderedDict[str, torch.Tensor]":
    """Random PIPS++ weights, keys as in the reference module tree (pips_plus_plus.py:420-434: ``fnet`` BasicEncoder
    (:180-260, instance norm -> no norm parameters), ``delta_block`` 1-D ResNet (:263-342) and the unused ``norm``).
    ``delta_scale`` shrinks the final dense layer so that the 16-iteration update is contractive (see
    ``init_pips_state_dict``).  Unused-but-present modules of the reference (``first_block_norm``, ``final_norm``,
    InstanceNorm without affine) have no parameters; ``norm`` (GroupNorm) has and is kept so the dict strict-loads."""
    w = _Init(seed)
    w.conv("fnet.conv1", 64, 3, 7, 7, kaiming_fan_out=True)
    in_planes = 64
    for li, (dim, stride) in enumerate([(64, 1), (96, 2), (128, 2), (128, 2)], start=1):
        for bi in range(2):
            cin = in_planes if bi == 0 else dim
            p = f"fnet.layer{li}.{bi}"
            w.conv(p + ".conv1", dim, cin, 3, 3, kaiming_fan_out=True)
            w.conv(p + ".conv2", dim, dim, 3, 3, kaiming_fan_out=True)
            if bi == 0 and stride != 1:
                w.conv(p + ".downsample.0", dim, cin, 1, 1, kaiming_fan_out=True)
        in_planes = dim
    w.conv("fnet.conv2", 2 * PIPS_LATENT, 128 + 128 + 96 + 64, 3, 3, kaiming_fan_out=True)
    w.conv("fnet.conv3", PIPS_LATENT, 2 * PIPS_LATENT, 1, 1, kaiming_fan_out=True)

    def conv1d(name, cout, cin):
        w.conv(name, cout, cin, 3, 1)
        w.sd[name + ".weight"] = w.sd[name + ".weight"].squeeze(-1)          # (cout, cin, 3)

    conv1d("delta_block.first_block_conv.conv", 128, PIPS2_KITCHEN)
    for i, (cin, cout) in enumerate(PIPS2_BLOCKS):
        conv1d(f"delta_block.basicblock_list.{i}.conv1.conv", cout, cin)
        conv1d(f"delta_block.basicblock_list.{i}.conv2.conv", cout, cout)
    w.linear("delta_block.dense", 2, 1024)
    w.sd["delta_block.dense.weight"] *= delta_scale
    w.sd["delta_block.dense.bias"] *= delta_scale
    w.norm("norm", PIPS_LATENT)
    return w.sd


# --------------------------------------------------------------------------------------
# SAM
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SamConfig:
    """Hyper-parameters of one SAM variant (configs/model/sam/image_encoder/vit_*.yaml,
    configs/model/sam/{mask_decoder,prompt_encoder}/sam.yaml, sam_vit_base.yaml:10-16)."""
    name: str
    embed_dim: int
    depth: int
    num_heads: int
    global_attn_indexes: Tuple[int, ...]
    img_size: int = 1024
    patch_size: int = 16
    window_size: int = 14
    mlp_ratio: int = 4
    out_chans: int = 256          # prompt_embed_dim
    mask_in_chans: int = 16
    dec_depth: int = 2
    dec_heads: int = 8
    dec_mlp_dim: int = 2048
    num_multimask_outputs: int = 3
    iou_head_depth: int = 3
    iou_head_hidden_dim: int = 256
    pixel_mean: Tuple[float, float, float] = (123.675, 116.28, 103.53)
    pixel_std: Tuple[float, float, float] = (58.395, 57.12, 57.375)

    @property
    def grid(self) -> int:
        return self.img_size // self.patch_size

    @property
    def head_dim(self) -> int:
        return self.embed_dim // self.num_heads

    @property
    def hq_dim(self) -> int:
        """Width of the token map HQ-SAM's decoder taps (``MaskDecoderHQ(vit_dim=...)``)."""
        return self.embed_dim


@dataclass(frozen=True)
class TinyVitConfig:
    """Hyper-parameters of a SAM whose image encoder is TinyViT (ChaoningZhang/MobileSAM tiny_vit_sam.py): MobileSAM
    (configs/model/sam/sam_mobile_vit_tiny.yaml) and Light HQ-SAM (samhq_light_vit_tiny.yaml).  Entry 0 of ``num_heads`` /
    ``window_sizes`` belongs to the convolutional stage and is unused, as upstream.  The prompt encoder / mask decoder fields are
    ``SamConfig``'s; ``patch_size`` is the encoder's total stride (patch embed 4, two stride-2 PatchMergings)."""
    name: str
    embed_dims: Tuple[int, int, int, int]
    depths: Tuple[int, int, int, int]
    num_heads: Tuple[int, int, int, int]
    window_sizes: Tuple[int, int, int, int]
    img_size: int = 1024
    patch_size: int = 16
    mlp_ratio: int = 4
    mbconv_expand_ratio: int = 4
    local_conv_size: int = 3
    out_chans: int = 256
    mask_in_chans: int = 16
    dec_depth: int = 2
    dec_heads: int = 8
    dec_mlp_dim: int = 2048
    num_multimask_outputs: int = 3
    iou_head_depth: int = 3
    iou_head_hidden_dim: int = 256
    pixel_mean: Tuple[float, float, float] = (123.675, 116.28, 103.53)
    pixel_std: Tuple[float, float, float] = (58.395, 57.12, 57.375)

    @property
    def grid(self) -> int:
        return self.img_size // self.patch_size

    @property
    def merge_strides(self) -> Tuple[int, int, int]:
        """Stride of the PatchMerging after layers 0..2: upstream's rule is by VALUE of the merged width."""
        return tuple(1 if d in (320, 448, 576) else 2 for d in self.embed_dims[1:])

    @property
    def resolutions(self) -> Tuple[int, int, int, int]:
        """Side of the map each layer works on (img/4, then divided by the merge strides)."""
        r = [self.img_size // 4]
        for st in self.merge_strides:
            r.append(r[-1] // st)
        return tuple(r)

    @property
    def hq_dim(self) -> int:
        """Width of the token map Light HQ-SAM's decoder taps: the input of ``layers.2``."""
        return self.embed_dims[2]


SAM_CONFIGS: Dict[str, SamConfig] = {
    "vit_b": SamConfig("vit_b", 768, 12, 12, (2, 5, 8, 11)),
    "vit_l": SamConfig("vit_l", 1024, 24, 16, (5, 11, 17, 23)),
    "vit_h": SamConfig("vit_h", 1280, 32, 16, (7, 15, 23, 31)),
    # reduced geometry for fast CPU tests only (same code paths: windows, padding, global blocks)
    "vit_test": SamConfig("vit_test", 64, 2, 2, (1,), img_size=256, patch_size=16, window_size=6,
                          out_chans=256),
    # TinyViT-5M as MobileSAM / Light HQ-SAM ship it
    "vit_t": TinyVitConfig("vit_t", (64, 128, 160, 320), (2, 2, 6, 2), (2, 4, 5, 10), (7, 7, 14, 7)),
    # reduced TinyViT for tests: resolutions 64 / 32 / 16 / 16, grid 16 as vit_test; every layer pads its windows (32 -> 35,
    # 16 -> 28, 16 -> 21); the last width stays 320 so that upstream's stride rule holds literally
    "vit_t_test": TinyVitConfig("vit_t_test", (32, 64, 96, 320), (2, 1, 2, 1), (1, 2, 3, 10), (7, 7, 14, 7), img_size=256),
}


def _init_vit_encoder(w: _Init, cfg: SamConfig) -> None:
    D, g, hd = cfg.embed_dim, cfg.grid, cfg.head_dim
    C = cfg.out_chans
    w.conv("image_encoder.patch_embed.proj", D, 3, cfg.patch_size, cfg.patch_size)
    w.normal("image_encoder.pos_embed", (1, g, g, D), 0.02)
    for i in range(cfg.depth):
        p = f"image_encoder.blocks.{i}"
        s = g if i in cfg.global_attn_indexes else cfg.window_size
        w.norm(p + ".norm1", D)
        w.linear(p + ".attn.qkv", 3 * D, D)
        w.linear(p + ".attn.proj", D, D)
        w.normal(p + ".attn.rel_pos_h", (2 * s - 1, hd), 0.05)
        w.normal(p + ".attn.rel_pos_w", (2 * s - 1, hd), 0.05)
        w.norm(p + ".norm2", D)
        w.linear(p + ".mlp.lin1", cfg.mlp_ratio * D, D)
        w.linear(p + ".mlp.lin2", D, cfg.mlp_ratio * D)
    w.conv("image_encoder.neck.0", C, D, 1, 1, bias=False)
    w.norm("image_encoder.neck.1", C)
    w.conv("image_encoder.neck.2", C, C, 3, 3, bias=False)
    w.norm("image_encoder.neck.3", C)


def _init_tinyvit_encoder(w: _Init, cfg: TinyVitConfig) -> None:
    """TinyViT in upstream's key layout (tiny_vit_sam.py): ``Conv2d_BN`` = children ``c`` (bias-free Conv2d) and ``bn``.  The
    BatchNorm statistics are off their defaults (running variance in [0.5, 1.5], non-zero means) and ``conv3.bn.weight`` is not
    the zero upstream initialises it to, so that folding them is exercised; ``attention_biases`` get a spread that matters to the
    softmax (std 0.5).  ``norm_head`` / ``head`` are in the checkpoints (TinyViT is built with its 1000-class head) and unused."""
    e = "image_encoder."

    def conv_bn(prefix, cin, cout, k, groups=1):
        w.conv(prefix + ".c", cout, cin // groups, k, k, bias=False)
        w.normal(prefix + ".bn.weight", (cout,), 0.1, mean=1.0)
        w.normal(prefix + ".bn.bias", (cout,), 0.1)
        w.normal(prefix + ".bn.running_mean", (cout,), 0.2)
        w.uniform(prefix + ".bn.running_var", (cout,), 0.5)
        w.sd[prefix + ".bn.running_var"] = w.sd[prefix + ".bn.running_var"] + 1.0          # in [0.5, 1.5]
        w.sd[prefix + ".bn.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    def merging(prefix, cin, cout, stride):
        conv_bn(prefix + ".conv1", cin, cout, 1)
        conv_bn(prefix + ".conv2", cout, cout, 3, groups=cout)
        conv_bn(prefix + ".conv3", cout, cout, 1)

    dims, C = cfg.embed_dims, cfg.out_chans
    conv_bn(e + "patch_embed.seq.0", 3, dims[0] // 2, 3)
    conv_bn(e + "patch_embed.seq.2", dims[0] // 2, dims[0], 3)
    hid = dims[0] * cfg.mbconv_expand_ratio
    for b in range(cfg.depths[0]):
        p = f"{e}layers.0.blocks.{b}"
        conv_bn(p + ".conv1", dims[0], hid, 1)
        conv_bn(p + ".conv2", hid, hid, 3, groups=hid)
        conv_bn(p + ".conv3", hid, dims[0], 1)
    merging(e + "layers.0.downsample", dims[0], dims[1], cfg.merge_strides[0])
    for i in range(1, 4):
        D, ws = dims[i], cfg.window_sizes[i]
        for b in range(cfg.depths[i]):
            p = f"{e}layers.{i}.blocks.{b}"
            w.normal(p + ".attn.attention_biases", (cfg.num_heads[i], ws * ws), 0.5)
            w.norm(p + ".attn.norm", D)
            w.linear(p + ".attn.qkv", 3 * D, D)
            w.linear(p + ".attn.proj", D, D)
            w.norm(p + ".mlp.norm", D)
            w.linear(p + ".mlp.fc1", cfg.mlp_ratio * D, D)
            w.linear(p + ".mlp.fc2", D, cfg.mlp_ratio * D)
            conv_bn(p + ".local_conv", D, D, cfg.local_conv_size, groups=D)
        if i < 3:
            merging(f"{e}layers.{i}.downsample", D, dims[i + 1], cfg.merge_strides[i])
    w.norm(e + "norm_head", dims[3])
    w.linear(e + "head", 1000, dims[3])
    w.conv(e + "neck.0", C, dims[3], 1, 1, bias=False)
    w.norm(e + "neck.1", C)
    w.conv(e + "neck.2", C, C, 3, 3, bias=False)
    w.norm(e + "neck.3", C)


def init_sam_state_dict(cfg, seed: int = 72, hq: bool = False) -> "OrderedDict[str, torch.Tensor]":
    """Random SAM weights with the upstream ``sam_vit_*.pth`` key layout; ``hq=True`` adds the HQ-SAM decoder extras of
    ``sam_hq_vit_*.pth`` (m43/sam-hq @ 75c73fa, MaskDecoderHQ: SURVEY.md App. A-5).  A ``TinyVitConfig`` gives the layout of
    ``mobile_sam.pt`` / ``sam_hq_vit_tiny.pth``: the TinyViT encoder's keys (``_init_tinyvit_encoder``), the same prompt encoder
    and decoder, the HQ extras at ``vit_dim = embed_dims[2]``.  That key map is restated from upstream's module tree and is
    UNVERIFIED against a real checkpoint (none is available here)."""
    w = _Init(seed)
    C = cfg.out_chans
    if isinstance(cfg, TinyVitConfig):
        _init_tinyvit_encoder(w, cfg)
    else:
        _init_vit_encoder(w, cfg)
    D = cfg.hq_dim
    # ---- prompt encoder
    w.normal("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (2, C // 2), 1.0)
    for i in range(4):
        w.normal(f"prompt_encoder.point_embeddings.{i}.weight", (1, C), 1.0)
    w.normal("prompt_encoder.not_a_point_embed.weight", (1, C), 1.0)
    w.normal("prompt_encoder.no_mask_embed.weight", (1, C), 1.0)
    m = cfg.mask_in_chans
    w.conv("prompt_encoder.mask_downscaling.0", m // 4, 1, 2, 2)
    w.norm("prompt_encoder.mask_downscaling.1", m // 4)
    w.conv("prompt_encoder.mask_downscaling.3", m, m // 4, 2, 2)
    w.norm("prompt_encoder.mask_downscaling.4", m)
    w.conv("prompt_encoder.mask_downscaling.6", C, m, 1, 1)
    # ---- mask decoder
    T = "mask_decoder.transformer"

    def attn(prefix, downsample):
        inner = C // downsample
        w.linear(prefix + ".q_proj", inner, C)
        w.linear(prefix + ".k_proj", inner, C)
        w.linear(prefix + ".v_proj", inner, C)
        w.linear(prefix + ".out_proj", C, inner)

    for i in range(cfg.dec_depth):
        p = f"{T}.layers.{i}"
        attn(p + ".self_attn", 1)
        w.norm(p + ".norm1", C)
        attn(p + ".cross_attn_token_to_image", 2)
        w.norm(p + ".norm2", C)
        w.linear(p + ".mlp.lin1", cfg.dec_mlp_dim, C)
        w.linear(p + ".mlp.lin2", C, cfg.dec_mlp_dim)
        w.norm(p + ".norm3", C)
        w.norm(p + ".norm4", C)
        attn(p + ".cross_attn_image_to_token", 2)
    attn(T + ".final_attn_token_to_image", 2)
    w.norm(T + ".norm_final_attn", C)
    nmt = cfg.num_multimask_outputs + 1
    w.normal("mask_decoder.iou_token.weight", (1, C), 1.0)
    w.normal("mask_decoder.mask_tokens.weight", (nmt, C), 1.0)
    # ConvTranspose2d weights are (in, out, kh, kw)
    w.uniform("mask_decoder.output_upscaling.0.weight", (C, C // 4, 2, 2), 1.0 / math.sqrt(C))
    w.uniform("mask_decoder.output_upscaling.0.bias", (C // 4,), 1.0 / math.sqrt(C))
    w.norm("mask_decoder.output_upscaling.1", C // 4)
    w.uniform("mask_decoder.output_upscaling.3.weight", (C // 4, C // 8, 2, 2), 1.0 / math.sqrt(C // 4))
    w.uniform("mask_decoder.output_upscaling.3.bias", (C // 8,), 1.0 / math.sqrt(C // 4))
    for i in range(nmt):
        p = f"mask_decoder.output_hypernetworks_mlps.{i}.layers"
        w.linear(p + ".0", C, C)
        w.linear(p + ".1", C, C)
        w.linear(p + ".2", C // 8, C)
    p = "mask_decoder.iou_prediction_head.layers"
    h = cfg.iou_head_hidden_dim
    dims = [C] + [h] * (cfg.iou_head_depth - 1) + [nmt]
    for i in range(cfg.iou_head_depth):
        w.linear(f"{p}.{i}", dims[i + 1], dims[i])
    if hq:
        M = "mask_decoder."
        w.normal(M + "hf_token.weight", (1, C), 1.0)
        w.linear(M + "hf_mlp.layers.0", C, C)
        w.linear(M + "hf_mlp.layers.1", C, C)
        w.linear(M + "hf_mlp.layers.2", C // 8, C)

        def convt(name, cin, cout):
            w.uniform(name + ".weight", (cin, cout, 2, 2), 1.0 / math.sqrt(cin))
            w.uniform(name + ".bias", (cout,), 1.0 / math.sqrt(cin))

        convt(M + "compress_vit_feat.0", D, C)
        w.norm(M + "compress_vit_feat.1", C)
        convt(M + "compress_vit_feat.3", C, C // 8)
        convt(M + "embedding_encoder.0", C, C // 4)
        w.norm(M + "embedding_encoder.1", C // 4)
        convt(M + "embedding_encoder.3", C // 4, C // 8)
        w.conv(M + "embedding_maskfeature.0", C // 4, C // 8, 3, 3)
        w.norm(M + "embedding_maskfeature.1", C // 4)
        w.conv(M + "embedding_maskfeature.3", C // 8, C // 4, 3, 3)
    return w.sd


# --------------------------------------------------------------------------------------
# SuperPoint + SuperGlue (sam_pt/point_tracker/superglue/models/{superpoint,superglue}.py)
# --------------------------------------------------------------------------------------
SUPERGLUE_KENC_DIMS = (3, 32, 64, 128, 256, 256)
SUPERGLUE_GNN_LAYERS = 18
SUPERGLUE_HEADS = 4


def init_superpoint_state_dict(seed: int = 72) -> "OrderedDict[str, torch.Tensor]":
    """Random SuperPoint weights under the key names of ``superpoint_v1.pth`` (superpoint.py:123-138): eight 3 x 3
    convolutions of the shared encoder, the detector head (convPa, convPb -> 65) and the descriptor head (convDa, convDb).

    Kaiming (fan-in, ReLU) weights keep the activations' scale through the eight layers; the detector's last layer is
    scaled by 1.25 so that the softmax over the 65 channels is uneven enough for the local maxima of the score map to lie on
    both sides of the shipped ``keypoint_threshold`` of 0.005 while no score reaches 0.5 (figures: DESIGN.md §4)."""
    w = _Init(seed)
    c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
    for name, cout, cin, k in (("conv1a", c1, 1, 3), ("conv1b", c1, c1, 3), ("conv2a", c2, c1, 3), ("conv2b", c2, c2, 3),
                               ("conv3a", c3, c2, 3), ("conv3b", c3, c3, 3), ("conv4a", c4, c3, 3), ("conv4b", c4, c4, 3),
                               ("convPa", c5, c4, 3), ("convPb", 65, c5, 1), ("convDa", c5, c4, 3), ("convDb", 256, c5, 1)):
        w.normal(name + ".weight", (cout, cin, k, k), math.sqrt(2.0 / (cin * k * k)))
        w.uniform(name + ".bias", (cout,), 0.1)
    w.sd["convPb.weight"] = w.sd["convPb.weight"] * 1.25
    return w.sd


def init_superglue_state_dict(seed: int = 72, gnn_scale: float = 0.1, proj_gain: float = 40.0,
                              bin_score: float = 125.0) -> "OrderedDict[str, torch.Tensor]":
    """Random SuperGlue weights under the key names of ``superglue_outdoor.pth`` (superglue.py:208-223): ``kenc.encoder``
    (Conv1d / BatchNorm1d / ReLU x 4, Conv1d), 18 x ``gnn.layers.<l>.{attn.proj.<0..2>, attn.merge, mlp.<0, 1, 3>}``,
    ``final_proj`` and ``bin_score``.  Every BatchNorm1d gets non-trivial running statistics and affine terms, so that
    folding them (pack.pack_superglue) is exercised.

    DAMPED init, as for CoTracker's flow head: with PyTorch's default init the 18 residual layers swamp the unit-norm
    SuperPoint descriptors, the rows of the score matrix differ mostly by their norms and almost nothing passes the
    mutual check.  The last convolution of every layer's MLP and of the keypoint encoder is therefore scaled by
    ``gnn_scale``: the residual stream stays dominated by the descriptors while every layer still contributes.
    ``final_proj`` is a random projection of gain ``proj_gain`` (scores of about ``proj_gain ** 2 / 16``, peaked enough
    for assignments above the shipped ``match_threshold`` of 0.2) and ``bin_score`` sits at the median score, where the
    golden clip yields about 30 matches, 175 unmatched keypoints, mutual-check failures and matching scores on both sides
    of the threshold (figures: DESIGN.md §4)."""
    w = _Init(seed)

    def bn(prefix, dim):
        w.normal(prefix + ".weight", (dim,), 0.1, mean=1.0)
        w.normal(prefix + ".bias", (dim,), 0.1)
        w.normal(prefix + ".running_mean", (dim,), 0.2)
        w.uniform(prefix + ".running_var", (dim,), 0.5)
        w.sd[prefix + ".running_var"] = w.sd[prefix + ".running_var"] + 1.0          # in [0.5, 1.5]
        w.sd[prefix + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    def conv1d(prefix, cout, cin, gain=1.0, zero_bias=False):
        b = 1.0 / math.sqrt(cin)
        w.uniform(prefix + ".weight", (cout, cin, 1), b * gain)
        w.uniform(prefix + ".bias", (cout,), b * gain)
        if zero_bias:                                                                # nn.init.constant_(..., 0.0)
            w.sd[prefix + ".bias"] = torch.zeros(cout)

    d = SUPERGLUE_KENC_DIMS
    for i in range(1, len(d)):
        last = i == len(d) - 1
        conv1d(f"kenc.encoder.{3 * (i - 1)}", d[i], d[i - 1], gain=gnn_scale if last else 1.0, zero_bias=last)
        if not last:
            bn(f"kenc.encoder.{3 * (i - 1) + 1}", d[i])
    for l in range(SUPERGLUE_GNN_LAYERS):
        p = f"gnn.layers.{l}"
        conv1d(p + ".attn.merge", 256, 256)
        for j in range(3):
            conv1d(f"{p}.attn.proj.{j}", 256, 256, gain=2.0 if j < 2 else 1.0)
        conv1d(p + ".mlp.0", 512, 512)
        bn(p + ".mlp.1", 512)
        conv1d(p + ".mlp.3", 256, 512, gain=gnn_scale, zero_bias=True)
    w.normal("final_proj.weight", (256, 256, 1), proj_gain / 16.0)
    w.uniform("final_proj.bias", (256,), 0.05)
    w.sd["bin_score"] = torch.tensor(float(bin_score))
    return w.sd


# --------------------------------------------------------------------------------------
# TAPIR (deepmind/tapnet @ ba1a8c8, vendored by the reference under sam_pt/point_tracker/tapir)
# --------------------------------------------------------------------------------------
TAPIR_GROUPS = ((64, 1), (128, 2), (256, 2), (256, 1))     # channels, stride of the four ResNet block groups
TAPIR_MIXER_BLOCKS = 12
TAPIR_MIXER_DIM = 512
TAPIR_MIXER_IN = 4 + 384 + 2 * 49                          # 486
TAPIR_MIXER_OUT = 4 + 384                                  # 388


def init_tapir_state_dict(seed: int = 72, delta_scale: float = 0.02, logit_gain: float = 0.5, occ_gain: float = 1500.0,
                          occ_centre: Tuple[float, float] = (0.2575, -0.2712)) -> "OrderedDict[str, torch.Tensor]":
    """Random TAPIR weights under flat names of this project's choosing, in PyTorch layouts (``load_tapir_checkpoint`` maps a
    Haiku checkpoint onto them):

      resnet.initial_conv.weight (64,3,7,7); resnet.g<G>.b<B>.{norm0,norm1}.{scale,offset}, .{conv0,conv1}.weight (O,I,3,3) and,
      for B = 0, .shortcut.weight (O,I,1,1) — no convolution of the ResNet has a bias;
      heads.{hid1,hid2,hid3}.{weight,bias} (O,I,3,3), heads.{hid4,occ_out}.{weight,bias} (out,in);
      mixer.in / mixer.out.{weight,bias} (out,in); mixer.blocks.<i>.{ln1,ln2}.scale, .{dw1,dw2}.weight (3,2048) = (tap, channel) with
      channel 4 c + m of dw1 reading input channel c, .{dw1,dw2}.bias, .{up,down}.{weight,bias}; mixer.ln_out.scale.

    CONDITIONED init, as for the other trackers.  The ResNet keeps a fan-out normal init.  The cost-volume heads of a
    trained model turn a correlation peak into a heat-map peak; random ones do not, so ``hid1`` / ``hid2`` get a positive centre
    tap on top of their random weights and ``hid2`` the gain ``logit_gain``: the 20 x softmax then has one clear maximum near the
    best-correlated cell while its neighbours keep some weight, and the runner-up cell lies well below it in the logits.  The
    occlusion head averages a ReLU map over 256 cells, so with random weights its two outputs barely move between items
    (0.2575 +- 0.001 and -0.2712 +- 0.0005 on the golden clip): ``occlusion_out`` is re-centred on ``occ_centre`` and scaled by
    ``occ_gain``, which spreads the logits over about +- 2 and the visibility probabilities over both sides of the 0.1 threshold.  ``delta_scale`` shrinks the mixer's output
    head: four refinements then move a point by fractions of a pixel to a few pixels, like the trained model's, instead of
    throwing it out of the frame, where every patch correlation is zero."""
    w = _Init(seed)
    w.conv("resnet.initial_conv", 64, 3, 7, 7, bias=False, kaiming_fan_out=True)
    cin = 64
    for g, (c, _) in enumerate(TAPIR_GROUPS):
        for b in range(2):
            p = f"resnet.g{g}.b{b}"
            bc = cin if b == 0 else c
            for n, dim in (("norm0", bc), ("norm1", c)):
                w.normal(f"{p}.{n}.scale", (dim,), 0.05, mean=1.0)
                w.normal(f"{p}.{n}.offset", (dim,), 0.05)
            w.conv(p + ".conv0", c, bc, 3, 3, bias=False, kaiming_fan_out=True)
            w.conv(p + ".conv1", c, c, 3, 3, bias=False, kaiming_fan_out=True)
            if b == 0:
                w.conv(p + ".shortcut", c, bc, 1, 1, bias=False, kaiming_fan_out=True)
        cin = c
    w.conv("heads.hid1", 16, 1, 3, 3)
    w.conv("heads.hid2", 1, 16, 3, 3)
    w.conv("heads.hid3", 32, 16, 3, 3)
    w.linear("heads.hid4", 16, 32)
    w.linear("heads.occ_out", 2, 16)
    w.sd["heads.hid1.weight"][:, 0, 1, 1] += 1.0
    w.sd["heads.hid2.weight"][0, :, 1, 1] += 0.5
    w.sd["heads.hid2.weight"] *= logit_gain
    w.sd["heads.occ_out.weight"] *= occ_gain
    w.sd["heads.occ_out.bias"] = (w.sd["heads.occ_out.bias"] - torch.tensor(occ_centre)) * occ_gain
    d = TAPIR_MIXER_DIM
    w.linear("mixer.in", d, TAPIR_MIXER_IN)
    for i in range(TAPIR_MIXER_BLOCKS):
        p = f"mixer.blocks.{i}"
        w.normal(p + ".ln1.scale", (d,), 0.05, mean=1.0)
        w.uniform(p + ".dw1.weight", (3, 4 * d), 1.0 / math.sqrt(3.0))
        w.uniform(p + ".dw1.bias", (4 * d,), 1.0 / math.sqrt(3.0))
        w.uniform(p + ".dw2.weight", (3, 4 * d), 1.0 / math.sqrt(3.0))
        w.uniform(p + ".dw2.bias", (4 * d,), 1.0 / math.sqrt(3.0))
        w.normal(p + ".ln2.scale", (d,), 0.05, mean=1.0)
        w.linear(p + ".up", 4 * d, d)
        w.linear(p + ".down", d, 4 * d)
    w.normal("mixer.ln_out.scale", (d,), 0.05, mean=1.0)
    w.linear("mixer.out", TAPIR_MIXER_OUT, d)
    w.sd["mixer.out.weight"] *= delta_scale
    w.sd["mixer.out.bias"] *= delta_scale
    return w.sd


def tapir_haiku_key_map() -> "OrderedDict[str, Tuple[str, str, str]]":
    """our name -> (Haiku module path, parameter name, layout) for every tensor the forward pass uses.

    UNVERIFIED AGAINST A REAL CHECKPOINT: no TAPIR checkpoint exists where this project is built.  The paths are derived by reading
    from Haiku's naming rules applied to tapir_model.py and models/resnet.py: a module created in its parent's ``__init__`` is
    ``parent/~/child``, one created inside another method is ``parent/child``; repeated names get ``_1``, ``_2``, ...  So the
    ResNet and the heads (built in ``TAPIR.__init__``) sit under ``tapir/~/``, the mixer's layers (built in its ``__call__``) under
    ``tapir/~/pips_mlp_mixer/``, and the two depthwise convolutions of a block, both named ``mlp1_up``, are ``mlp1_up`` and
    ``mlp1_up_1``.  Layouts: conv2d = Haiku (kh, kw, cin, cout) -> (cout, cin, kh, kw); linear = (in, out) -> (out, in);
    dw = DepthwiseConv1D (k, 1, C * mult) -> (k, C * mult); vec = unchanged."""
    m: "OrderedDict[str, Tuple[str, str, str]]" = OrderedDict()
    r = "tapir/~/resnet/~/"
    m["resnet.initial_conv.weight"] = (r + "initial_conv", "w", "conv2d")
    for g in range(4):
        for b in range(2):
            hp, p = f"{r}block_group_{g}/~/block_{b}/~/", f"resnet.g{g}.b{b}."
            for j in range(2):
                m[f"{p}norm{j}.scale"] = (f"{hp}instancenorm_{j}", "scale", "vec")
                m[f"{p}norm{j}.offset"] = (f"{hp}instancenorm_{j}", "offset", "vec")
                m[f"{p}conv{j}.weight"] = (f"{hp}conv_{j}", "w", "conv2d")
            if b == 0:
                m[p + "shortcut.weight"] = (hp + "shortcut_conv", "w", "conv2d")
    for ours, theirs, kind in (("hid1", "cost_volume_regression_1", "conv2d"), ("hid2", "cost_volume_regression_2", "conv2d"),
                               ("hid3", "cost_volume_occlusion_1", "conv2d"), ("hid4", "cost_volume_occlusion_2", "linear"),
                               ("occ_out", "occlusion_out", "linear")):
        m[f"heads.{ours}.weight"] = ("tapir/~/" + theirs, "w", kind)
        m[f"heads.{ours}.bias"] = ("tapir/~/" + theirs, "b", "vec")
    x = "tapir/~/pips_mlp_mixer/"
    for ours, theirs in (("mixer.in", "linear"), ("mixer.out", "linear_1")):
        m[ours + ".weight"] = (x + theirs, "w", "linear")
        m[ours + ".bias"] = (x + theirs, "b", "vec")
    m["mixer.ln_out.scale"] = (x + "layer_norm", "scale", "vec")
    for i in range(TAPIR_MIXER_BLOCKS):
        hb, p = x + ("block" if i == 0 else f"block_{i}") + "/", f"mixer.blocks.{i}."
        m[p + "ln1.scale"] = (hb + "layer_norm", "scale", "vec")
        m[p + "ln2.scale"] = (hb + "layer_norm_1", "scale", "vec")
        for ours, theirs, kind in (("dw1", "mlp1_up", "dw"), ("dw2", "mlp1_up_1", "dw"), ("up", "mlp2_up", "linear"),
                                   ("down", "mlp2_down", "linear")):
            m[f"{p}{ours}.weight"] = (hb + theirs, "w", kind)
            m[f"{p}{ours}.bias"] = (hb + theirs, "b", "vec")
    return m


def load_tapir_checkpoint(path: str) -> "OrderedDict[str, torch.Tensor]":
    """The reference's checkpoint format (tapir/tracker.py:44-45): ``np.load(path, allow_pickle=True).item()`` is
    ``{"params": {module path: {name: array}}, "state": ...}``.  -> a state dict under this project's names and layouts
    (``tapir_haiku_key_map``, UNVERIFIED AGAINST A REAL CHECKPOINT).  Modules the forward pass never calls (``regression_*``,
    ``conv_stats_*``) are ignored; a tensor the map expects and the file lacks is named in the error."""
    import numpy as np
    ck = np.load(path, allow_pickle=True).item()
    params = ck["params"]
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    missing = []
    for ours, (module, name, kind) in tapir_haiku_key_map().items():
        if module not in params or name not in params[module]:
            missing.append(f"{module}:{name}")
            continue
        a = torch.from_numpy(np.asarray(params[module][name], dtype=np.float32).copy())
        if kind == "conv2d":
            a = a.permute(3, 2, 0, 1)
        elif kind == "linear":
            a = a.t()
        elif kind == "dw":
            a = a.reshape(a.shape[0], a.shape[-1])
        sd[ours] = a.contiguous()
    if missing:
        raise KeyError(f"TAPIR checkpoint {path} lacks {len(missing)} tensors: " + ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else ""))
    return sd


def tapir_state_dict_to_haiku(sd: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, "object"]]:
    """The inverse of ``load_tapir_checkpoint``'s mapping: the ``params`` tree of a checkpoint file holding ``sd`` (round-trip tests)."""
    params: Dict[str, Dict[str, object]] = {}
    for ours, (module, name, kind) in tapir_haiku_key_map().items():
        a = sd[ours]
        if kind == "conv2d":
            a = a.permute(2, 3, 1, 0)
        elif kind == "linear":
            a = a.t()
        elif kind == "dw":
            a = a.reshape(a.shape[0], 1, a.shape[1])
        params.setdefault(module, {})[name] = a.contiguous().numpy()
    return params


# --------------------------------------------------------------------------------------
# TapNet (deepmind/tapnet @ ba1a8c8, vendored by the reference under sam_pt/point_tracker/tapnet)
# --------------------------------------------------------------------------------------
TAPNET_UNITS = ((64, 1, 0.125), (128, 2, 0.125), (256, 1, 0.0))     # channels, stride, shifted fraction of units 0 .. 2
TAPNET_BN_EPS = 1e-5                                                # hk.BatchNorm's default


def init_tapnet_state_dict(seed: int = 72, logit_gain: float = 0.5, occ_gain: float = 2000.0,
                           occ_centre: float = 0.18545) -> "OrderedDict[str, torch.Tensor]":
    """Random TapNet weights under flat names of this project's choosing, in PyTorch layouts (``load_tapnet_checkpoint`` maps a
    Haiku checkpoint onto them):

      tsm.stem.weight (64,3,7,7); tsm.u<U>.b<B>.{bn0,bn1}.{scale,offset,mean,var} — BatchNorm's parameters and its moving
      statistics —, .{conv0,conv2}.weight (O,I,3,3) and, for B = 0, .shortcut.weight (O,I,1,1) — no convolution of the backbone has a
      bias, and at depth 18 a block has no conv_1;
      heads.{hid1,hid2,hid3}.{weight,bias} (O,I,3,3), heads.hid4.{weight,bias} (16,32), heads.occ_out.{weight,bias} (1,16).

    CONDITIONED init, as for TAPIR.  The moving means and variances are drawn away from (0, 1), so the host's fold
    into a per-channel affine is exercised.  ``hid1`` / ``hid2`` get a positive centre tap on top of their random weights and ``hid2``
    the gain ``logit_gain``: the 10 x softmax then has one clear maximum near the best-correlated cell.  The occlusion head averages a
    map over 256 cells, so with random weights its output barely moves between items (0.1850 .. 0.1859 on the golden clip):
    ``occlusion_out`` is re-centred on ``occ_centre`` and scaled by ``occ_gain``, which spreads the logits over about +- 1, i.e. the
    visibilities over both sides of the yaml's threshold 0.5."""
    w = _Init(seed)
    w.conv("tsm.stem", 64, 3, 7, 7, bias=False, kaiming_fan_out=True)
    cin = 64
    for u, (c, _, _) in enumerate(TAPNET_UNITS):
        for b in range(2):
            p = f"tsm.u{u}.b{b}"
            bc = cin if b == 0 else c
            for n, dim in (("bn0", bc), ("bn1", c)):
                w.normal(f"{p}.{n}.scale", (dim,), 0.05, mean=1.0)
                w.normal(f"{p}.{n}.offset", (dim,), 0.05)
                w.normal(f"{p}.{n}.mean", (dim,), 0.2)
                w.uniform(f"{p}.{n}.var", (dim,), 0.5)
                w.sd[f"{p}.{n}.var"] += 1.25                      # in [0.75, 1.75]
            w.conv(p + ".conv0", c, bc, 3, 3, bias=False, kaiming_fan_out=True)
            w.conv(p + ".conv2", c, c, 3, 3, bias=False, kaiming_fan_out=True)
            if b == 0:
                w.conv(p + ".shortcut", c, bc, 1, 1, bias=False, kaiming_fan_out=True)
        cin = c
    w.conv("heads.hid1", 16, 1, 3, 3)
    w.conv("heads.hid2", 1, 16, 3, 3)
    w.conv("heads.hid3", 32, 16, 3, 3)
    w.linear("heads.hid4", 16, 32)
    w.linear("heads.occ_out", 1, 16)
    w.sd["heads.hid1.weight"][:, 0, 1, 1] += 1.0
    w.sd["heads.hid2.weight"][0, :, 1, 1] += 0.5
    w.sd["heads.hid2.weight"] *= logit_gain
    w.sd["heads.occ_out.weight"] *= occ_gain
    w.sd["heads.occ_out.bias"] = (w.sd["heads.occ_out.bias"] - occ_centre) * occ_gain
    return w.sd


def tapnet_haiku_key_map() -> "OrderedDict[str, Tuple[str, str, str, str]]":
    """our name -> (tree, Haiku module path, entry name, layout) for every tensor the forward pass uses; tree is "params" or "state".

    UNVERIFIED AGAINST A REAL CHECKPOINT: no TapNet checkpoint exists where this project is built.  The paths are derived by reading
    from Haiku's naming rules applied to tapnet_model.py and models/tsm_resnet.py: a module created in its parent's ``__init__`` is
    ``parent/~/child``, one created inside another method is ``parent/child``; repeated names get ``_1``.  ``TAPNet`` names itself
    ``tap_net`` (Haiku's snake case of the class name); the backbone (built in ``TAPNet.__init__``, name ``tsm_resnet_video``) and the
    heads sit under ``tap_net/~/``; stem, units, blocks and their convolutions are built in ``__call__`` methods, so no ``~``; the two
    ``hk.BatchNorm`` of a block, created through ``normalize_fn`` inside the block's ``__call__``, are ``batch_norm`` and
    ``batch_norm_1``; the moving statistics are the ``average`` of the ExponentialMovingAverage children ``~/mean_ema`` / ``~/var_ema``
    (built in ``BatchNorm.__init__``) in the state tree.  Layouts: conv2d = (kh, kw, cin, cout) -> (cout, cin, kh, kw); conv3d = the
    heads' Conv3D (1, kh, kw, cin, cout) -> (cout, cin, kh, kw); linear = (in, out) -> (out, in); vec = unchanged; stat = (1, 1, 1, C) -> (C)."""
    m: "OrderedDict[str, Tuple[str, str, str, str]]" = OrderedDict()
    r = "tap_net/~/tsm_resnet_video/"
    m["tsm.stem.weight"] = ("params", r + "tsm_resnet_stem", "w", "conv2d")
    for u in range(3):
        for b in range(2):
            hp, p = f"{r}tsm_resnet_unit_{u}/block_{b}/", f"tsm.u{u}.b{b}."
            for j, bn in enumerate(("batch_norm", "batch_norm_1")):
                m[f"{p}bn{j}.scale"] = ("params", hp + bn, "scale", "stat")
                m[f"{p}bn{j}.offset"] = ("params", hp + bn, "offset", "stat")
                m[f"{p}bn{j}.mean"] = ("state", hp + bn + "/~/mean_ema", "average", "stat")
                m[f"{p}bn{j}.var"] = ("state", hp + bn + "/~/var_ema", "average", "stat")
            m[p + "conv0.weight"] = ("params", hp + "conv_0", "w", "conv2d")
            m[p + "conv2.weight"] = ("params", hp + "conv_2", "w", "conv2d")
            if b == 0:
                m[p + "shortcut.weight"] = ("params", hp + "shortcut_conv", "w", "conv2d")
    for ours, theirs, kind in (("hid1", "cost_volume_regression_1", "conv3d"), ("hid2", "cost_volume_regression_2", "conv3d"),
                               ("hid3", "cost_volume_occlusion_1", "conv3d"), ("hid4", "cost_volume_occlusion_2", "linear"),
                               ("occ_out", "occlusion_out", "linear")):
        m[f"heads.{ours}.weight"] = ("params", "tap_net/~/" + theirs, "w", kind)
        m[f"heads.{ours}.bias"] = ("params", "tap_net/~/" + theirs, "b", "vec")
    return m


def load_tapnet_checkpoint(path: str) -> "OrderedDict[str, torch.Tensor]":
    """The reference's checkpoint format (tapnet/tracker.py:43-44): ``np.load(path, allow_pickle=True).item()`` of
    ``checkpoint_wo_optstate.npy`` is ``{"params": {module path: {name: array}}, "state": {module path: {name: array}}}``.  -> a state
    dict under this project's names and layouts (``tapnet_haiku_key_map``, UNVERIFIED AGAINST A REAL CHECKPOINT: none exists where
    this project is built).  Modules the forward pass never calls (``regression_hid``, ``regression_out``, unit 3 of the backbone) and
    the moving averages' ``hidden`` / ``counter`` are ignored; a tensor the map expects and the file lacks is named in the error."""
    import numpy as np
    ck = np.load(path, allow_pickle=True).item()
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    missing = []
    for ours, (tree, module, name, kind) in tapnet_haiku_key_map().items():
        src = ck[tree]
        if module not in src or name not in src[module]:
            missing.append(f"{tree}:{module}:{name}")
            continue
        a = torch.from_numpy(np.asarray(src[module][name], dtype=np.float32).copy())
        if kind == "conv2d":
            a = a.permute(3, 2, 0, 1)
        elif kind == "conv3d":
            a = a[0].permute(3, 2, 0, 1)
        elif kind == "linear":
            a = a.t()
        elif kind == "stat":
            a = a.reshape(-1)
        sd[ours] = a.contiguous()
    if missing:
        raise KeyError(f"TapNet checkpoint {path} lacks {len(missing)} tensors: " + ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else ""))
    return sd


def tapnet_state_dict_to_haiku(sd: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, Dict[str, "object"]]]:
    """The inverse of ``load_tapnet_checkpoint``'s mapping: ``{"params": ..., "state": ...}`` of a checkpoint file holding ``sd``
    (round-trip tests)."""
    ck: Dict[str, Dict[str, Dict[str, object]]] = {"params": {}, "state": {}}
    for ours, (tree, module, name, kind) in tapnet_haiku_key_map().items():
        a = sd[ours]
        if kind == "conv2d":
            a = a.permute(2, 3, 1, 0)
        elif kind == "conv3d":
            a = a.permute(2, 3, 1, 0)[None]
        elif kind == "linear":
            a = a.t()
        elif kind == "stat":
            a = a.reshape(1, 1, 1, -1)
        ck[tree].setdefault(module, {})[name] = a.contiguous().numpy()
    return ck
