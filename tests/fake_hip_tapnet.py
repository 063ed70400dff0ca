"""The recording fake of tests/fake_hip.py extended by the TapNet seam (TEST INFRASTRUCTURE ONLY).

``install(monkeypatch, tapnet_sd, sam_sd, cfg)`` is ``fake_hip.install`` with a ``FakeHip`` that also models the five calls
``TapnetPointTracker`` makes (include/sampt_hip.h, seam 1g): ``sampt_tapnet_create``, ``sampt_tapnet_workspace_bytes``,
``sampt_tapnet_track_f32``, ``sampt_tapnet_launches`` and ``sampt_tapnet_destroy``.  The model is the restatement of
tests/tapnet_ref.py on the CPU tensors the call receives; the arguments of every call are kept in ``fake.tapnet_calls``.
"""
from __future__ import annotations

import contextlib

import torch

from tests import fake_hip
from tests import tapnet_ref as R

WORKSPACE_BYTES = 4096
STEM_CHUNK = 8                          # the engine's default (csrc/engine.h)


def nominal_launches(T: int) -> int:
    """csrc/engine_tapnet.hip: 3 per stem chunk + 27 for the six blocks + 1 channel normalisation + 2 (query features, heads)."""
    return 3 * -(-T // STEM_CHUNK) + 30


class FakeHipTapnet(fake_hip.FakeHip):
    def __init__(self, tapnet_sd, sam_sd=None, cfg=None):
        super().__init__(sam_sd, cfg, None)
        self.tapnet_sd = tapnet_sd
        self.tapnet_calls = []              # (name, arguments that are not tensors)
        self.tapnet_names = None
        self._tapnet_launches = 0

    def sampt_tapnet_create(self, names, ptrs, n, out):
        self.calls["tapnet_create"] += 1
        self.tapnet_calls.append(("create", n))
        self.tapnet_names = dict(names)     # the packed weights (name_table is patched to hand the dict itself over)
        assert n == len(self.tapnet_names) and "tsm.stem.weight" in names and "tsm.u2.b1.bn1.b" in names and "tsm.u0.b0.bn0.mean" not in names
        return self._handle(out)

    def sampt_tapnet_destroy(self, h):
        self.calls["tapnet_destroy"] += 1
        self.tapnet_calls.append(("destroy",))

    def sampt_tapnet_workspace_bytes(self, h, T, n, out):
        self.calls["tapnet_workspace_bytes"] += 1
        self.tapnet_calls.append(("workspace_bytes", T, n))
        assert T >= 1 and n >= 1
        fake_hip._set(out, WORKSPACE_BYTES)
        return 0

    def sampt_tapnet_track_f32(self, h, frames, T, q, n, tracks, occ, ws, nbytes, stream):
        self.calls["tapnet_track"] += 1
        self.calls["tapnet_track_frames"] += T
        self.tapnet_calls.append(("track_f32", T, n))
        assert frames.dtype == torch.float32 and tuple(frames.shape) == (T, 3, 256, 256) and frames.is_contiguous()
        assert 0 <= float(frames.min()) and float(frames.max()) <= 1          # the * 2 - 1 is the device's
        assert q.dtype == torch.float32 and tuple(q.shape) == (n, 3) and q.is_contiguous()      # (t, x, y) in 256 x 256 pixels
        assert tuple(tracks.shape) == (n, T, 2) and tuple(occ.shape) == (n, T)
        assert ws.dtype == torch.uint8 and nbytes == ws.numel() == WORKSPACE_BYTES
        o = R.forward(self.tapnet_sd, (frames * 2 - 1).permute(0, 2, 3, 1), q[:, [0, 2, 1]])
        tracks.copy_(o["tracks"]), occ.copy_(o["occlusion"])
        self._tapnet_launches = nominal_launches(T)
        return 0

    def sampt_tapnet_launches(self, h):
        self.calls["tapnet_launches"] += 1
        self.tapnet_calls.append(("launches",))
        return self._tapnet_launches


def install(monkeypatch, tapnet_sd, sam_sd=None, cfg=None) -> FakeHipTapnet:
    from sam_pt_amd import _lib
    fake = FakeHipTapnet(tapnet_sd, sam_sd, cfg)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "ptr_array", lambda ts: list(ts))
    monkeypatch.setattr(_lib, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(_lib, "name_table", lambda named: (named, None, len(named)))
    monkeypatch.setattr(_lib, "require_hip", lambda device, who: None)
    monkeypatch.setattr(_lib, "device_guard", lambda device: contextlib.nullcontext())
    return fake
