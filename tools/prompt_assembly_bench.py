#!/usr/bin/env python
"""Prompt assembly of ``SamPt``: the host path against ``device_tracks`` (sam_pt_amd/prompt_assembly.py, csrc/prompt_assembly.hip).

  python tools/prompt_assembly_bench.py [--repeats 7] [--model vit_b] [--frames 24] [--objects 3] [--log profiles/prompt_assembly_bench.log]

Part 1, the assembly alone, at 36 frames x 100 objects x 9 points (the VIS configuration's tracker batch) and 24 x 3 x 17.  Host:
what ``SamPt._enqueue_sam_fused`` does with CPU tracks — the ``_prepare_points`` + ``apply_coords`` loop, the padded float32 / int32
arrays, the counts — by a host clock; the download of the tracks and the upload of the blocks, which the host path adds on the
device-resident pipeline, are timed apart.  Device: count, the copy of 2 * T * M ints into pinned memory, a synchronise, then one fill
of every item, by a host clock that ends in a synchronise.  The two alternate, ``--repeats`` times after a warm-up; median, min, max and
spread are printed.  Before anything is timed the device's words are compared with the host's.

Part 2, one ``SamPt.forward`` per mode with ``use_patch_matching_filtering=True`` on the bench clip (PIPS, the ``--model`` ViT in fp16):
the default mode (host filter, host assembly — the same tree's unchanged path) against ``device_tracks=True``, alternating.

Everything printed also goes to ``--log``."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_pt_amd import prompt_assembly as PA  # noqa: E402
from sam_pt_amd.sam_predictor import ResizeLongestSide  # noqa: E402
from sam_pt_amd.sam_pt import SamPt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--model", default="vit_b")
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--objects", type=int, default=3)
ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "prompt_assembly_bench.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
SIZE = (480, 854)
_lines = []


def say(msg=""):
    print(msg, flush=True)
    _lines.append(msg)


def stats(ts, unit="ms"):
    return f"median {statistics.median(ts):.3f} {unit}, min {min(ts):.3f}, max {max(ts):.3f} (spread {max(ts) - min(ts):.3f})"


def tracks(T, M, P, seed=72):
    rng = np.random.default_rng(seed)
    traj = (rng.random((T, M, P, 2)) * np.array([SIZE[1], SIZE[0]])).astype(np.float32)
    vis = (rng.random((T, M, P)) < 0.9).astype(np.float32)
    return torch.from_numpy(traj), torch.from_numpy(vis)


def host_assembly(me, tf, traj, vis):
    """The host half of ``SamPt._enqueue_sam_fused`` up to the padded arrays and the counts."""
    T, M = vis.shape[:2]
    traj_np, vis_np = traj.numpy(), (vis == 1).numpy()
    prompts = []
    for t in range(T):
        for m in range(M):
            c, l = SamPt._prepare_points(me, traj_np, vis_np, t, m, M)
            if len(c):
                c = tf.apply_coords(c, SIZE)
            prompts.append((c, l))
    k_all = np.array([len(c) for c, _ in prompts], dtype=np.int32)
    npos_all = np.array([int((l == 1).sum()) for _, l in prompts], dtype=np.int32)
    kmax = max(1, int(k_all.max()))
    xy = np.zeros((len(prompts), kmax, 2), dtype=np.float32)
    lab = np.zeros((len(prompts), kmax), dtype=np.int32)
    for i, (c, l) in enumerate(prompts):
        xy[i, :len(c)] = c
        lab[i, :len(c)] = l
    return xy, lab, k_all, npos_all


def assembly_part(T, M, P, pp):
    from types import SimpleNamespace
    me = SimpleNamespace(positive_points_per_mask=pp, negative_points_per_mask=1, add_other_objects_positive_points_as_negative_points=True,
                         max_other_objects_positive_points=None)
    tf = ResizeLongestSide(1024)
    new_h, new_w = tf.get_preprocess_shape(SIZE[0], SIZE[1], 1024)
    sx, sy = new_w / SIZE[1], new_h / SIZE[0]
    traj, vis = tracks(T, M, P)
    traj_d, vis_d = traj.to(dev), vis.to(dev)
    n = T * M
    items = torch.arange(n, dtype=torch.int32, device=dev)
    pinned = torch.empty((2, n), dtype=torch.int32, pin_memory=True)

    def device_assembly():
        counts = PA.count_prompts(vis_d, pp, True, True)
        pinned.copy_(counts, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        kmax = max(1, int(pinned[0].max()))
        xy = torch.empty((n, kmax, 2), dtype=torch.float32, device=dev)
        lab = torch.empty((n, kmax), dtype=torch.int32, device=dev)
        k, npos = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        PA.fill_prompts(traj_d, vis_d, pp, True, True, sx, sy, items, xy, lab, k, npos)
        torch.cuda.synchronize()
        return xy, lab, k, npos

    want = host_assembly(me, tf, traj, vis)
    got = device_assembly()
    same = all((g.cpu().numpy().view(np.int32) == w.view(np.int32)).all() for g, w in zip(got, want))
    say(f"{T} frames x {M} objects x {P} points (pp = {pp}, negatives, other objects' positives appended): {n} items, longest prompt "
        f"{want[0].shape[1]} points; device words equal the host's: {same}")
    assert same
    t_host, t_dev = [], []
    for i in range(1 + args.repeats):                              # alternating, the first round is the warm-up
        t0 = time.perf_counter()
        host_assembly(me, tf, traj, vis)
        t1 = time.perf_counter()
        device_assembly()
        t2 = time.perf_counter()
        if i:
            t_host.append((t1 - t0) * 1e3)
            t_dev.append((t2 - t1) * 1e3)
    say(f"  host assembly (loop + padded arrays + counts), host clock:            {stats(t_host)}")
    say(f"  device: count + 2 * T * M ints home + synchronise + one fill + synchronise: {stats(t_dev)}")
    xy, lab, k, npos = got                                         # the two launches alone, between device events
    t_count, t_fill = [], []
    for i in range(3 + 20):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        PA.count_prompts(vis_d, pp, True, True)
        e[1].record()
        PA.fill_prompts(traj_d, vis_d, pp, True, True, sx, sy, items, xy, lab, k, npos)
        e[2].record()
        torch.cuda.synchronize()
        if i >= 3:
            t_count.append(e[0].elapsed_time(e[1]) * 1e3)
            t_fill.append(e[1].elapsed_time(e[2]) * 1e3)
    say(f"    count alone (wrapper + launch), events, 20 repeats after 3: {stats(t_count, 'us')}")
    say(f"    fill of all {n} items alone (wrapper + launch), events:      {stats(t_fill, 'us')}")
    t_move = []
    for i in range(1 + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        traj_d.cpu(), vis_d.cpu()
        torch.from_numpy(want[0]).to(dev), torch.from_numpy(want[1]).to(dev)
        torch.cuda.synchronize()
        if i:
            t_move.append((time.perf_counter() - t0) * 1e3)
    say(f"  the host path's copies on top (tracks down, padded arrays up, pageable):  {stats(t_move)}")
    say(f"  host / device = {statistics.median(t_host) / statistics.median(t_dev):.1f} x (medians, without the copies)")


def forward_part():
    from sam_pt_amd.point_tracker import PipsPointTracker
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    from sam_pt_amd.synth import bench_clip
    from sam_pt_amd.weights import init_pips_state_dict
    frames, qp = bench_clip(T=args.frames, seed=72, n_pos=8, n_objects=args.objects, n_neg=1)
    video = {"image": frames.to(dev), "target_hw": tuple(frames.shape[-2:]), "query_points": qp}
    pred = SamPredictor(SamHip(args.model, precision="f16", seed=72, max_batch=8, max_decode_batch=32).to(dev))
    trk = PipsPointTracker(state_dict=init_pips_state_dict(72), fnet_chunk=8)
    kw = dict(sam_iou_threshold=-1e9, positive_points_per_mask=8, negative_points_per_mask=1, iterative_refinement_iterations=12,
              use_patch_matching_filtering=True)
    modes = {"default (host filter, host assembly)": SamPt(trk, pred, **kw).eval(),
             "device_tracks=True": SamPt(trk, pred, device_tracks=True, **kw).eval()}
    say(f"SamPt.forward, {args.model} fp16 + PIPS, {args.frames} frames of {frames.shape[-2]} x {frames.shape[-1]}, {args.objects} objects x 9 "
        f"points, patch filter on, {args.repeats} alternating repeats after 2 warm-ups (eager, graph capture):")
    times = {name: [] for name in modes}
    vis = {}
    for i in range(2 + args.repeats):
        for name, model in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model(video)
            torch.cuda.synchronize()
            if i >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            vis[name] = out["visibilities"]
    for name in modes:
        say(f"  {name}: {stats(times[name])}")
    a, b = vis.values()
    say(f"  visibility codes that differ between the modes (the host filter's similarities differ from the device's by an ulp): "
        f"{int((a != b).sum())} of {a.numel()}")
    med = [statistics.median(t) for t in times.values()]
    say(f"  default / device_tracks = {med[0] / med[1]:.2f} x (medians)")


def main():
    assert torch.cuda.is_available(), "prompt_assembly_bench needs a GPU"
    say(f"prompt_assembly_bench on {torch.cuda.get_device_name(0)}, torch.get_num_threads() = {torch.get_num_threads()}")
    assembly_part(36, 100, 9, 8)
    assembly_part(24, 3, 17, 16)
    if not args.skip_forward:
        forward_part()
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
