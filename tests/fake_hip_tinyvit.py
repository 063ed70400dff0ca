"""The recording fake of tests/fake_hip.py extended by the TinyViT seam (TEST INFRASTRUCTURE ONLY).

``install(monkeypatch, sam_sd, cfg, pips_sd, hq)`` is ``fake_hip.install`` with a ``FakeHip`` that also models the four calls a
``SamPredictor`` over a ``TinyVitConfig`` makes (include/sampt_hip.h, seam 2a'): ``sampt_tinyvit_create``,
``sampt_tinyvit_encode_workspace_bytes``, ``sampt_tinyvit_encode`` and ``sampt_tinyvit_destroy``.  The model is the restatement of
tests/tinyvit_ref.py on the CPU tensors the call receives.  Every ``sampt_vit_*`` entry point of the base fake is taken away: a
predictor over a TinyViT may not make one.
"""
from __future__ import annotations

import contextlib

import torch

from tests import fake_hip
from tests import tinyvit_ref as R

WORKSPACE_BYTES = 4096


class FakeHipTinyVit(fake_hip.FakeHip):
    def __init__(self, sam_sd, cfg, pips_sd=None, hq=False):
        super().__init__(sam_sd, cfg, pips_sd, hq)
        self.tinyvit_names = None
        self._model = None

    def __getattribute__(self, name):
        if name.startswith("sampt_vit_"):
            raise AttributeError(f"FakeHipTinyVit: {name} called on a TinyViT predictor")
        return super().__getattribute__(name)

    def sampt_tinyvit_create(self, cfg_ref, names, ptrs, n, max_batch, out):
        self.calls["tinyvit_create"] += 1
        c = cfg_ref._obj
        assert (tuple(c.embed_dims), tuple(c.depths), tuple(c.num_heads), tuple(c.window_sizes)) == \
            (tuple(self.cfg.embed_dims), tuple(self.cfg.depths), tuple(self.cfg.num_heads), tuple(self.cfg.window_sizes))
        assert (c.img_size, c.out_chans, c.mlp_ratio, c.mbconv_expand_ratio) == (self.cfg.img_size, self.cfg.out_chans, 4, 4) and max_batch >= 1
        self.tinyvit_names = dict(names)     # the packed weights (name_table is patched to hand the dict itself over)
        e = "image_encoder."
        assert e + "patch_embed.seq.0.weight" in names and e + "layers.1.blocks.0.attn.pad_qkv" in names and e + "neck.2.weight_khwc_hl" in names
        assert not any(".bn." in k or ".c.weight" in k or "head" in k for k in names)        # folded, and the classifier head left out
        return self._handle(out)

    def sampt_tinyvit_destroy(self, h):
        self.calls["tinyvit_destroy"] += 1

    def sampt_tinyvit_encode_workspace_bytes(self, h, B, out):
        self.calls["tinyvit_workspace_bytes"] += 1
        fake_hip._set(out, WORKSPACE_BYTES)
        return 0

    def sampt_tinyvit_encode(self, h, frames, chw, B, H, W, out, interm, ws, nbytes, stream):
        self.calls["tinyvit_encode"] += 1
        self.calls["tinyvit_encode_frames"] += B
        x = (frames if chw else frames.permute(0, 3, 1, 2)).contiguous()     # (one memory layout: one convolution algorithm)
        assert x.dtype == torch.uint8 and tuple(x.shape) == (B, 3, H, W) and max(H, W) == self.cfg.img_size
        assert ws.dtype == torch.uint8 and nbytes == ws.numel() == WORKSPACE_BYTES
        g = self.cfg.grid
        assert tuple(out.shape) == (B, g * g, self.cfg.out_chans)
        assert (interm is not None) == self.hq and (interm is None or tuple(interm.shape)[1:] == (g * g, self.cfg.embed_dims[2]))
        if self._model is None:
            self._model = R.build(self.cfg, self.sam_sd)
        st = R.run(self.cfg, self.sam_sd, x, model=self._model)
        out.copy_(st["neck"].permute(0, 2, 3, 1).reshape(B, g * g, -1))
        if interm is not None:
            interm[:B] = st["interm"].reshape(B, g * g, -1)
        return 0


def install(monkeypatch, sam_sd, cfg, pips_sd=None, hq=False) -> FakeHipTinyVit:
    from sam_pt_amd import _lib
    fake = FakeHipTinyVit(sam_sd, cfg, pips_sd, hq)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "ptr_array", lambda ts: list(ts))
    monkeypatch.setattr(_lib, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(_lib, "name_table", lambda named: (named, None, len(named)))
    monkeypatch.setattr(_lib, "require_hip", lambda device, who: None)
    monkeypatch.setattr(_lib, "device_guard", lambda device: contextlib.nullcontext())
    return fake
