"""The recording fake of tests/fake_hip.py extended by the TAPIR seam (TEST INFRASTRUCTURE ONLY).

``install(monkeypatch, tapir_sd, sam_sd, cfg)`` is ``fake_hip.install`` with a ``FakeHip`` that also models the six calls
``TapirPointTracker`` makes (include/sampt_hip.h, seam 1f): ``sampt_tapir_create``, ``sampt_tapir_workspace_bytes``,
``sampt_tapir_set_max_queries``, ``sampt_tapir_track_f32``, ``sampt_tapir_launches`` and ``sampt_tapir_destroy``.  The model is the
restatement of tests/tapir_ref.py on the CPU tensors the call receives; the arguments of every call are kept in ``fake.tapir_calls``.
"""
from __future__ import annotations

import contextlib

import torch

from tests import fake_hip
from tests import tapir_ref as R

WORKSPACE_BYTES = 4096


class FakeHipTapir(fake_hip.FakeHip):
    def __init__(self, tapir_sd, sam_sd=None, cfg=None):
        super().__init__(sam_sd, cfg, None)
        self.tapir_sd = tapir_sd
        self.tapir_calls = []               # (name, arguments that are not tensors)
        self.tapir_names = None
        self._tapir_max_queries = 0
        self._tapir_launches = 0

    def sampt_tapir_create(self, names, ptrs, n, out):
        self.calls["tapir_create"] += 1
        self.tapir_calls.append(("create", n))
        self.tapir_names = dict(names)      # the packed weights (name_table is patched to hand the dict itself over)
        assert n == len(self.tapir_names) and "resnet.initial_conv.weight" in names and "mixer.blocks.11.down.weight" in names
        return self._handle(out)

    def sampt_tapir_destroy(self, h):
        self.calls["tapir_destroy"] += 1
        self.tapir_calls.append(("destroy",))

    def sampt_tapir_workspace_bytes(self, h, T, n, max_queries_in_flight, out):
        self.calls["tapir_workspace_bytes"] += 1
        self.tapir_calls.append(("workspace_bytes", T, n, max_queries_in_flight))
        assert T >= 1 and n >= 1 and 1 <= max_queries_in_flight <= n
        fake_hip._set(out, WORKSPACE_BYTES)
        return 0

    def sampt_tapir_set_max_queries(self, h, max_queries):
        self.calls["tapir_set_max_queries"] += 1
        self.tapir_calls.append(("set_max_queries", max_queries))
        self._tapir_max_queries = max_queries
        return 0

    def sampt_tapir_track_f32(self, h, frames, T, q, n, iters, tracks, occ, expd, iter_out, ws, nbytes, stream):
        self.calls["tapir_track"] += 1
        self.calls["tapir_track_frames"] += T
        self.tapir_calls.append(("track_f32", T, n, iters))
        assert frames.dtype == torch.float32 and tuple(frames.shape) == (T, 3, 256, 256) and frames.is_contiguous()
        assert 0 <= float(frames.min()) and float(frames.max()) <= 1          # the * 2 - 1 is the device's
        assert q.dtype == torch.float32 and tuple(q.shape) == (n, 3) and q.is_contiguous()      # (t, x, y) in 256 x 256 pixels
        assert tuple(tracks.shape) == (n, T, 2) and tuple(occ.shape) == (n, T) and tuple(expd.shape) == (n, T)
        assert ws.dtype == torch.uint8 and nbytes == ws.numel() == WORKSPACE_BYTES
        o = R.forward(self.tapir_sd, (frames * 2 - 1).permute(0, 2, 3, 1), q[:, [0, 2, 1]], iters=iters)
        tracks.copy_(o["tracks"]), occ.copy_(o["occlusion"]), expd.copy_(o["expected_dist"])
        if iter_out is not None:
            assert tuple(iter_out.shape) == (iters + 1, n, T, 4)
            for i in range(iters + 1):
                iter_out[i, ..., :2] = o["iter_tracks"][i]
                iter_out[i, ..., 2], iter_out[i, ..., 3] = o["iter_occlusion"][i], o["iter_expected_dist"][i]
        chunks = -(-n // max(1, min(n, self._tapir_max_queries or n)))
        self._tapir_launches = 72 * T + 2 + chunks * iters * 53       # the engine's nominal count (csrc/engine_tapir.hip)
        return 0

    def sampt_tapir_launches(self, h):
        self.calls["tapir_launches"] += 1
        self.tapir_calls.append(("launches",))
        return self._tapir_launches


def install(monkeypatch, tapir_sd, sam_sd=None, cfg=None) -> FakeHipTapir:
    from sam_pt_amd import _lib
    fake = FakeHipTapir(tapir_sd, sam_sd, cfg)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "ptr_array", lambda ts: list(ts))
    monkeypatch.setattr(_lib, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(_lib, "name_table", lambda named: (named, None, len(named)))
    monkeypatch.setattr(_lib, "require_hip", lambda device, who: None)
    monkeypatch.setattr(_lib, "device_guard", lambda device: contextlib.nullcontext())
    return fake
