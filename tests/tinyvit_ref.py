"""TinyViT as MobileSAM / Light HQ-SAM use it for their image encoder — a literal restatement of upstream's
``tiny_vit_sam.py`` (ChaoningZhang/MobileSAM @ 01ea8d0, m43/sam-hq @ 75c73fa) in plain PyTorch, TEST INFRASTRUCTURE ONLY.

The third-party source is not available here, so **parity with upstream is unpinned**: this file follows the written description
of the model (module tree, attribute names, the order of operations inside a block, the PatchMerging stride rule, the
first-appearance numbering of the attention offsets) and is the authority the device path is held to.  The modules carry
upstream's attribute names (``c``, ``bn``, ``seq``, ``conv1`` .., ``attn.norm``, ``local_conv``, ``mlp.fc1``, ``neck``), so a
``strict=True`` ``load_state_dict`` of ``init_sam_state_dict``'s encoder keys pins the key layout on this class structure.

Everything runs in the dtype of the module (``.float()`` / ``.double()``); ``forward`` returns the stages.
"""
from __future__ import annotations

import itertools
import os
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tinyvit_ref.npz")
STAGES = ("patch_embed", "layer0", "layer1", "layer2", "layer3", "neck")


class Conv2d_BN(nn.Sequential):
    def __init__(self, a, b, ks=1, stride=1, pad=0, groups=1):
        super().__init__()
        self.add_module("c", nn.Conv2d(a, b, ks, stride, pad, groups=groups, bias=False))
        self.add_module("bn", nn.BatchNorm2d(b, eps=1e-5))


class PatchEmbed(nn.Module):
    def __init__(self, in_chans, embed_dim):
        super().__init__()
        self.seq = nn.Sequential(Conv2d_BN(in_chans, embed_dim // 2, 3, 2, 1), nn.GELU(), Conv2d_BN(embed_dim // 2, embed_dim, 3, 2, 1))

    def forward(self, x):
        return self.seq(x)


class MBConv(nn.Module):
    def __init__(self, in_chans, out_chans, expand_ratio):
        super().__init__()
        hidden = int(in_chans * expand_ratio)
        self.conv1 = Conv2d_BN(in_chans, hidden, 1)
        self.act1 = nn.GELU()
        self.conv2 = Conv2d_BN(hidden, hidden, 3, 1, 1, groups=hidden)
        self.act2 = nn.GELU()
        self.conv3 = Conv2d_BN(hidden, out_chans, 1)
        self.act3 = nn.GELU()

    def forward(self, x):
        shortcut = x
        x = self.act1(self.conv1(x))
        x = self.act2(self.conv2(x))
        x = self.conv3(x)
        x = x + shortcut
        return self.act3(x)


class PatchMerging(nn.Module):
    def __init__(self, input_resolution, dim, out_dim):
        super().__init__()
        self.input_resolution, self.dim, self.out_dim = input_resolution, dim, out_dim
        self.act = nn.GELU()
        self.conv1 = Conv2d_BN(dim, out_dim, 1, 1, 0)
        stride_c = 2
        if out_dim == 320 or out_dim == 448 or out_dim == 576:          # upstream's rule is by VALUE
            stride_c = 1
        self.stride = stride_c
        self.conv2 = Conv2d_BN(out_dim, out_dim, 3, stride_c, 1, groups=out_dim)
        self.conv3 = Conv2d_BN(out_dim, out_dim, 1, 1, 0)

    def forward(self, x):
        if x.ndim == 3:
            H, W = self.input_resolution
            B = len(x)
            x = x.view(B, H, W, -1).permute(0, 3, 1, 2)
        x = self.act(self.conv1(x))
        x = self.act(self.conv2(x))
        x = self.conv3(x)
        return x.flatten(2).transpose(1, 2)


class ConvLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, out_dim, expand_ratio):
        super().__init__()
        self.blocks = nn.ModuleList([MBConv(dim, dim, expand_ratio) for _ in range(depth)])
        self.downsample = PatchMerging(input_resolution, dim, out_dim)

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return self.downsample(x)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.norm = nn.LayerNorm(in_features, eps=1e-5)
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.act = nn.GELU()

    def forward(self, x):
        return self.fc2(self.act(self.fc1(self.norm(x))))


def first_appearance_index(ws: int) -> torch.Tensor:
    """``attention_bias_idxs`` as upstream builds it: offsets (|dy|, |dx|) numbered by first appearance over
    ``itertools.product(range(ws), range(ws))`` squared."""
    points = list(itertools.product(range(ws), range(ws)))
    offsets: Dict[tuple, int] = {}
    idxs = []
    for p1 in points:
        for p2 in points:
            off = (abs(p1[0] - p2[0]), abs(p1[1] - p2[1]))
            if off not in offsets:
                offsets[off] = len(offsets)
            idxs.append(offsets[off])
    return torch.tensor(idxs, dtype=torch.long).view(len(points), len(points))


class Attention(nn.Module):
    def __init__(self, dim, key_dim, num_heads, resolution):
        super().__init__()
        self.num_heads, self.key_dim, self.scale = num_heads, key_dim, key_dim ** -0.5
        self.d = key_dim                                                  # attn_ratio 1
        self.norm = nn.LayerNorm(dim, eps=1e-5)
        self.qkv = nn.Linear(dim, 3 * key_dim * num_heads)
        self.proj = nn.Linear(key_dim * num_heads, dim)
        idxs = first_appearance_index(resolution[0])
        self.attention_biases = nn.Parameter(torch.zeros(num_heads, int(idxs.max()) + 1))
        self.register_buffer("attention_bias_idxs", idxs, persistent=False)

    def forward(self, x):                                                 # (B, N, C)
        B, N, _ = x.shape
        x = self.norm(x)
        qkv = self.qkv(x)
        q, k, v = qkv.view(B, N, self.num_heads, -1).split([self.key_dim, self.key_dim, self.d], dim=3)   # interleaved per head
        q, k, v = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        attn = (q @ k.transpose(-2, -1)) * self.scale + self.attention_biases[:, self.attention_bias_idxs]
        attn = attn.softmax(dim=-1)
        x = (attn @ v).transpose(1, 2).reshape(B, N, self.num_heads * self.d)
        return self.proj(x)


class TinyViTBlock(nn.Module):
    def __init__(self, dim, input_resolution, num_heads, window_size, mlp_ratio, local_conv_size):
        super().__init__()
        self.dim, self.input_resolution, self.window_size = dim, input_resolution, window_size
        self.attn = Attention(dim, dim // num_heads, num_heads, (window_size, window_size))
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.local_conv = Conv2d_BN(dim, dim, local_conv_size, 1, local_conv_size // 2, groups=dim)

    def forward(self, x):
        H, W = self.input_resolution
        B, L, C = x.shape
        ws = self.window_size
        res_x = x
        if H == ws and W == ws:
            x = self.attn(x)
        else:
            x = x.view(B, H, W, C)
            pad_b, pad_r = (ws - H % ws) % ws, (ws - W % ws) % ws
            if pad_b > 0 or pad_r > 0:
                x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
            pH, pW = H + pad_b, W + pad_r
            nH, nW = pH // ws, pW // ws
            x = x.view(B, nH, ws, nW, ws, C).transpose(2, 3).reshape(B * nH * nW, ws * ws, C)
            x = self.attn(x)                                              # over ALL ws^2 positions, padded ones included, no mask
            x = x.view(B, nH, nW, ws, ws, C).transpose(2, 3).reshape(B, pH, pW, C)
            if pad_b > 0 or pad_r > 0:
                x = x[:, :H, :W].contiguous()
            x = x.view(B, L, C)
        x = res_x + x
        x = x.transpose(1, 2).reshape(B, C, H, W)
        x = self.local_conv(x)                                            # no residual, no activation
        x = x.view(B, C, L).transpose(1, 2)
        return x + self.mlp(x)


class BasicLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, local_conv_size, out_dim):
        super().__init__()
        self.blocks = nn.ModuleList([TinyViTBlock(dim, input_resolution, num_heads, window_size, mlp_ratio, local_conv_size)
                                     for _ in range(depth)])
        self.downsample = PatchMerging(input_resolution, dim, out_dim) if out_dim is not None else None

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return x if self.downsample is None else self.downsample(x)


class LayerNorm2d(nn.Module):
    def __init__(self, num_channels, eps=1e-6):
        super().__init__()
        self.weight, self.bias, self.eps = nn.Parameter(torch.ones(num_channels)), nn.Parameter(torch.zeros(num_channels)), eps

    def forward(self, x):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + self.eps)
        return self.weight[:, None, None] * x + self.bias[:, None, None]


class TinyViT(nn.Module):
    def __init__(self, img_size=1024, in_chans=3, num_classes=1000, embed_dims=(64, 128, 160, 320), depths=(2, 2, 6, 2),
                 num_heads=(2, 4, 5, 10), window_sizes=(7, 7, 14, 7), mlp_ratio=4.0, mbconv_expand_ratio=4.0, local_conv_size=3,
                 out_chans=256):
        super().__init__()
        self.img_size = img_size
        self.patch_embed = PatchEmbed(in_chans, embed_dims[0])
        r = img_size // 4
        self.layers = nn.ModuleList()
        for i in range(4):
            out_dim = embed_dims[i + 1] if i < 3 else None
            if i == 0:
                layer = ConvLayer(embed_dims[0], (r, r), depths[0], out_dim, mbconv_expand_ratio)
            else:
                layer = BasicLayer(embed_dims[i], (r, r), depths[i], num_heads[i], window_sizes[i], mlp_ratio, local_conv_size, out_dim)
            self.layers.append(layer)
            if i < 3:
                r //= layer.downsample.stride
        self.grid = r
        self.norm_head = nn.LayerNorm(embed_dims[-1])                     # in the checkpoints, unused by SAM
        self.head = nn.Linear(embed_dims[-1], num_classes)
        self.neck = nn.Sequential(nn.Conv2d(embed_dims[-1], out_chans, 1, bias=False), LayerNorm2d(out_chans),
                                  nn.Conv2d(out_chans, out_chans, 3, padding=1, bias=False), LayerNorm2d(out_chans))

    def forward(self, x):
        """x: (B, 3, img, img) preprocessed -> dict of the stages: ``patch_embed`` (B, C0, R0, R0), ``layer0..3`` token maps
        (B, L, C) after each layer's downsample, ``interm`` (B, g, g, C2) = the input of layers.2, ``neck`` (B, 256, g, g)."""
        out = {}
        x = self.patch_embed(x)
        out["patch_embed"] = x
        for i, layer in enumerate(self.layers):
            if i == 2:
                B, L, C = x.shape
                out["interm"] = x.view(B, int(L ** 0.5), int(L ** 0.5), C)
            x = layer(x)
            out[f"layer{i}"] = x
        B, _, C = x.shape
        x = x.view(B, self.grid, self.grid, C).permute(0, 3, 1, 2)
        out["neck"] = self.neck(x)
        return out


def build(cfg, sd, dtype=torch.float32) -> TinyViT:
    """The restatement for a ``TinyVitConfig`` with the ``image_encoder.*`` keys of ``sd`` loaded strictly."""
    m = TinyViT(cfg.img_size, 3, 1000, cfg.embed_dims, cfg.depths, cfg.num_heads, cfg.window_sizes, cfg.mlp_ratio,
                cfg.mbconv_expand_ratio, cfg.local_conv_size, cfg.out_chans)
    enc = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
    m.load_state_dict(enc, strict=True)
    return m.to(dtype).eval()


def preprocess(cfg, frames_u8: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """Sam.preprocess: uint8 (B, 3, H, W) -> (x - mean) / std, zero-padded bottom / right to img_size^2."""
    mean = torch.tensor(cfg.pixel_mean, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(cfg.pixel_std, dtype=torch.float32).view(1, 3, 1, 1)
    x = (frames_u8.float() - mean) / std
    H, W = x.shape[-2:]
    return F.pad(x, (0, cfg.img_size - W, 0, cfg.img_size - H)).to(dtype)


@torch.no_grad()
def run(cfg, sd, frames_u8, dtype=torch.float32, model=None):
    m = build(cfg, sd, dtype) if model is None else model
    return m(preprocess(cfg, frames_u8, dtype))


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
