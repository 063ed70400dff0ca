"""``SamPtInteractive`` — the interactive point-correction simulator (reference: sam_pt/modeling/sam_pt_interactive.py), with the
reference's constructor parameters and ``forward(video)`` contract: ``gt_masks``, a single mask, ``query_masks`` or
``query_points``, ``target_hw``; it returns ``logits`` and ``None`` for the other four entries.

The loop is the reference's: thresholds 0.10 .. 0.95 offline or the single online one; a click budget that the query points count
against; at most ``interactions_max_per_frame`` clicks per frame; first remove an incorrect negative point, then an incorrect
positive one, otherwise add a positive point on the false negatives if FN > FP, else a negative one on the false positives
(``interactive.extract_largest_cluster_points``); the added point is tracked from its frame on with ``_track_points``;
``disable_point_tracking`` is kept; a checkpoint is kept at each threshold reached and the best one wins at the end.

What differs from the reference:

* **Written against the interfaces.**  The loop uses the ``SamPredictor`` interface (``set_image`` / ``features`` or
  ``encode_frames`` / ``set_features``, ``transform``, ``predict_torch``) and ``_track_points`` only, so it runs over any predictor,
  the oracle's CPU one included (that is how tests/test_interactive_cpu.py pins the control flow on the reference's own
  ``forward``).
* **Device work on a ``SamHip`` predictor.**  The clip is encoded once with ``encode_frames`` (the reference's feature cache), masks
  stay on the device, IoU and boundary F come from the J&F counts (``vos_metrics.jf_device``: the float64 formulas the host
  functions share), the click rule reads ``interactive.frame_state_device`` and the click comes from
  ``extract_largest_cluster_points(device=...)``.  Per decision a handful of integers reach the host.  ``device_primitives=False``
  keeps the predictor but downloads the masks and uses the host functions (the comparison the GPU test makes).
* **``full_pass`` is incremental.**  A click at frame f changes no input of a frame before f (visibilities are cleared from f on,
  added points are invisible before f), so only frames >= f are decoded again and the logits, J and F of the others are reused;
  the "after" figures of frame f are that frame's entry of the same pass, and the "before" figures the entry of the previous one.
  ``incremental=False`` decodes as often as the reference does (tests prove the two agree with ``==``).
* **One decode path.**  ``predict_mask`` of one frame is the only decode path, for single frames and passes alike, so the loop's
  "before" and "after" figures agree with its cache bit for bit.  It keeps the reference's point order and pass structure (the
  second pass only with a visible negative point).  A prompt without a visible positive point gives zero logits and score 0 (not
  ``SamPt``'s ``-inf``), and there is no ``sam_iou_threshold`` gate.  ``decode_batch`` (default 1) above 1 decodes up to that many
  frames of a pass as one ``track_decode`` chain instead (a predictor with ``track_decode`` only): positives first, as that call wants
  them, frames with a visible negative point (two-pass chains) and without (single-pass chains) in separate chains, every frame of
  the loop — single ones too — through the same call.  The decoder's token side is not batch-invariant, so such logits are a few 1e-7
  off the ``decode_batch=1`` ones (tests/test_gpu_interactive.py holds them to 8 x 1.9e-7) and a history may differ from the default's.
* **No side effects by default.**  The reference always writes ``interactions/<video_id>/history.json``, two pickles and a plot into
  the working directory.  Here ``output_dir=None`` writes nothing: the history, the threshold checkpoints and the final state are on
  ``self.last_run``.  With ``output_dir`` set, ``history.json`` and ``overall_iou_history.json`` are written there under
  ``<video_id>/`` with the reference's field names (one object per interaction; the reference's ``json.dump`` of named tuples
  writes the same values as bare arrays).  The pickles, the plot and the visualisation switches
  (``visualize_all_interactions_separately``, ``visualize_all_interactions_as_mp4``, ``font_path``) are not built: the arguments
  are accepted and raise ``NotImplementedError`` by name when set.
* The query masks of ``query_points`` mode, which the reference computes and only checks the shape of, are not computed; the
  threshold list is copied per video (the reference pops from the instance's list, so a second video would start where the first
  stopped).
"""
from __future__ import annotations

import json
import os
from collections import namedtuple
from typing import List

import numpy as np
import torch

from . import interactive as I
from . import vos_metrics as VM
from .sam_pt import SamPt, _stack_frames

HistoryEntry = namedtuple("HistoryEntry",
                          "action type frame_idx point_idx iou_before iou_after interaction_idx current_iou_threshold "
                          "overall_iou_before overall_iou_after boundary_score_before boundary_score_after "
                          "overall_boundary_score_before overall_boundary_score_after jf_score_before jf_score_after")

OFFLINE_THRESHOLDS = (0.10, 0.20, 0.30, 0.40, 0.50, 0.60, 0.65, 0.70, 0.75, 0.80, 0.85, 0.88, 0.90, 0.92, 0.95)


class SamPtInteractive(SamPt):
    def __init__(self, interactions_max=300, interactions_max_per_frame=3, online_interactive_iou_threshold=0.9,
                 disable_point_tracking=False, online=False, font_path=None, visualize_all_interactions_separately=False,
                 visualize_all_interactions_as_mp4=False, incremental=True, decode_batch=1, output_dir=None,
                 device_primitives=True, **kwargs):
        super().__init__(**kwargs)
        for name, value in (("visualize_all_interactions_separately", visualize_all_interactions_separately),
                            ("visualize_all_interactions_as_mp4", visualize_all_interactions_as_mp4), ("font_path", font_path)):
            if value:
                raise NotImplementedError(f"SamPtInteractive: {name} is not built (the history is on self.last_run)")
        if int(decode_batch) < 1:
            raise ValueError(f"SamPtInteractive: decode_batch must be at least 1; got {decode_batch}")
        self.disable_point_tracking = disable_point_tracking
        self.interactions_max = interactions_max
        self.interactions_max_per_frame = interactions_max_per_frame
        self.online = online
        self.online_interactive_iou_threshold = online_interactive_iou_threshold
        self.offline_interactive_iou_thresholds = list(OFFLINE_THRESHOLDS)
        self.incremental = bool(incremental)
        self.decode_batch = int(decode_batch)
        self.output_dir = output_dir
        self.device_primitives = bool(device_primitives)
        self.last_run = None

    # ------------------------------------------------------------------------------------------------------------------------------
    def decode_state(self, video, trajectories, visibilities, point_labels):
        """Logits (T, H, W) of ONE pass over the clip for a given point state (trajectories (T, 1, P, 2), visibilities (T, 1, P),
        labels (P,)), through the decode path the loop uses: what ``last_run`` holds can be decoded again, by another
        ``decode_batch`` for instance."""
        from . import _lib
        with _lib.device_guard(self.device):
            return self._forward_impl(video, state=(trajectories.cpu(), visibilities.cpu(), point_labels.cpu()))

    def _forward_impl(self, video, defer=False, state=None):
        images = _stack_frames(video["image"]) if isinstance(video["image"], (list, tuple)) else video["image"]
        n_frames, channels, height, width = images.shape
        assert images.dtype == torch.uint8, "Input images must be in uint8 format (0-255)"
        if state is not None:
            query_points = torch.zeros((1, 0, 3))
        elif video.get("query_masks") is not None:
            assert video.get("query_points") is None
            query_points = self.extract_query_points(images, video["query_masks"].float(), video["query_point_timestep"])
        elif video.get("query_points") is not None:
            query_points = video["query_points"]
        else:
            raise ValueError("No query points or masks provided")
        query_points = query_points.cpu()
        n_masks, n_points_per_mask, _ = query_points.shape
        assert n_masks == 1, "Interactive point correction only works with a single mask"
        assert "gt_masks" in video, "Ground truth masks must be provided for interactive point correction"
        gt_masks = torch.stack(list(video["gt_masks"])).squeeze(1).bool()
        assert gt_masks.shape == (n_frames, height, width)

        thresholds = [self.online_interactive_iou_threshold] if self.online else list(self.offline_interactive_iou_thresholds)
        interactions_max = self.interactions_max
        interactions_left = interactions_max
        if self.disable_point_tracking:
            thresholds = [1.0]
            interactions_max = self.interactions_max_per_frame * n_frames

        pred = self.sam_predictor
        pdev = self.device
        on_hip = getattr(pdev, "type", None) == "cuda"
        use_dev = on_hip and self.device_primitives
        gt_dev = gt_masks.to(pdev).to(torch.uint8).contiguous() if use_dev else None
        gt_np = gt_masks.cpu().numpy()
        stats = {"decoder_calls": 0, "decoder_chains": 0, "tracker_calls": 0, "device_clicks": 0, "host_clicks": 0}
        batched = self.decode_batch > 1
        if batched and not (hasattr(pred, "encode_frames") and hasattr(pred, "track_decode")):
            raise NotImplementedError("SamPtInteractive: decode_batch > 1 needs a predictor with encode_frames and track_decode")

        # 1. the clip's embeddings, once
        if hasattr(pred, "encode_frames") and hasattr(pred, "set_features"):
            feats = pred.encode_frames(images.to(pdev))
            in_size = pred.transform.get_preprocess_shape(height, width, pred.transform.target_length)

            def select_frame(f):
                pred.set_features(feats[f], (height, width), in_size)
        else:
            cache = []
            for f in range(n_frames):
                pred.set_image(images[f].permute(1, 2, 0).cpu().numpy())
                cache.append((pred.features, getattr(pred, "hq_feat", None)))

            def select_frame(f):
                pred.features = cache[f][0]
                if cache[f][1] is not None:
                    pred.hq_feat = cache[f][1]

        def to_input_frame(coords):
            if hasattr(pred.transform, "apply_coords_torch"):
                return pred.transform.apply_coords_torch(coords=coords, original_size=pred.original_size)
            return torch.as_tensor(pred.transform.apply_coords(coords.numpy(), pred.original_size), dtype=torch.float)

        def keep(x):
            return x if use_dev else x.cpu()

        def predict_mask(f, point_coords, point_labels):
            """One frame's logits (H, W) and score: the reference's predict_mask, point order and pass structure included."""
            if len(point_coords) == 0 or point_labels.sum() == 0:
                dev = pdev if use_dev else "cpu"
                return torch.zeros((height, width), dtype=torch.float32, device=dev), torch.tensor(0, dtype=torch.float32, device=dev)
            stats["decoder_calls"] += 1
            select_frame(f)
            pc = to_input_frame(point_coords)
            pos = point_labels == 1
            kw = dict(multimask_output=False, return_logits=True)
            ml, iou, low = pred.predict_torch(point_coords=pc[pos][None].to(pdev), point_labels=point_labels[pos][None].to(pdev),
                                              boxes=None, mask_input=None, **kw)
            if int((point_labels == 0).sum()) > 0:
                ml, iou, low = pred.predict_torch(point_coords=pc[None].to(pdev), point_labels=point_labels[None].to(pdev), boxes=None,
                                                  mask_input=low, **kw)
            for _ in range(int(self.iterative_refinement_iterations)):
                m = ml[0, 0] > 0
                if m.sum() < 2:
                    break
                yx = m.nonzero()
                box = torch.tensor([yx[:, 1].min(), yx[:, 0].min(), yx[:, 1].max(), yx[:, 0].max()], dtype=torch.float, device=pdev)
                ml, iou, low = pred.predict_torch(point_coords=pc[None].to(pdev), point_labels=point_labels[None].to(pdev),
                                                  boxes=box[None, None, :], mask_input=low, **kw)
            return keep(ml[0, 0]), keep(iou[0, 0])

        # per-frame cache of the current state's prediction: logits, score, IoU and boundary F (float32 scalars, as the reference's
        # torch.tensor(float) makes them)
        c_logits, c_score = [None] * n_frames, [None] * n_frames
        c_iou, c_bnd = [None] * n_frames, [None] * n_frames

        def predict_masks_batched(frames, trajectories, visibilities, point_labels):
            """``predict_mask`` of several frames as ``track_decode`` chains of up to ``decode_batch`` items: positives first, frames
            with and without a visible negative point in separate chains (two passes / one pass, as the reference decides per
            frame)."""
            groups = {False: [], True: []}
            for f in frames:
                vis = visibilities[f, 0, :] == 1
                lab = point_labels[vis]
                if int(vis.sum()) == 0 or int(lab.sum()) == 0:
                    dev = pdev if use_dev else "cpu"
                    c_logits[f] = torch.zeros((height, width), dtype=torch.float32, device=dev)
                    c_score[f] = torch.tensor(0, dtype=torch.float32, device=dev)
                    continue
                order = torch.argsort((lab != 1).int(), stable=True)                       # positives first, each class in track order
                xy = pred.transform.apply_coords_torch(trajectories[f, 0, :, :][vis][order], (height, width)).numpy()   # (as predict_mask)
                groups[bool((lab == 0).any())].append((f, xy, lab[order].numpy(), int((lab == 1).sum())))
            chunk_max = min(self.decode_batch, int(getattr(pred.model, "max_decode_batch", self.decode_batch)))
            for two_pass, items in groups.items():
                for c0 in range(0, len(items), chunk_max):
                    chunk = items[c0:c0 + chunk_max]
                    F_ = len(chunk)
                    ks = np.array([len(it[2]) for it in chunk], dtype=np.int32)
                    ps = np.array([it[3] for it in chunk], dtype=np.int32)
                    xy = np.zeros((F_, int(ks.max()), 2), dtype=np.float32)
                    lab = np.zeros((F_, int(ks.max())), dtype=np.int32)
                    for i, it in enumerate(chunk):
                        xy[i, :ks[i]], lab[i, :ks[i]] = it[1], it[2]
                    ragged = bool((ks != ks[0]).any() or (two_pass and (ps != ps[0]).any()))
                    out_l = torch.empty((F_, height, width), dtype=torch.float32, device=pdev)
                    out_s = torch.empty((F_,), dtype=torch.float32, device=pdev)
                    idx = torch.tensor([it[0] for it in chunk], dtype=torch.long, device=pdev)
                    pred.track_decode(feats.index_select(0, idx), torch.from_numpy(xy).to(pdev), torch.from_numpy(lab).to(pdev),
                                      int(ks.max()), int(ps.max()) if two_pass else -1, int(self.iterative_refinement_iterations),
                                      -3.0e38, (height, width), out_l, out_s,           # (no sam_iou_threshold gate in this class)
                                      k_item=torch.from_numpy(ks).to(pdev) if ragged else None,
                                      npos_item=torch.from_numpy(ps).to(pdev) if (ragged and two_pass) else None)
                    stats["decoder_calls"] += F_
                    stats["decoder_chains"] += 1
                    for i, it in enumerate(chunk):
                        c_logits[it[0]], c_score[it[0]] = keep(out_l[i]), keep(out_s[i])

        def evaluate(frames, trajectories, visibilities, point_labels):
            """Decode ``frames`` with the given state and score them against the ground truth, into the cache."""
            if batched:
                predict_masks_batched(frames, trajectories, visibilities, point_labels)
            else:
                for f in frames:
                    vis = visibilities[f, 0, :] == 1
                    c_logits[f], c_score[f] = predict_mask(f, trajectories[f, 0, :, :][vis], point_labels[vis])
            if use_dev:
                J, Fb = VM.jf_device(gt_dev[list(frames)] != 0, torch.stack([c_logits[f] for f in frames]), threshold=0.0)
                for k, f in enumerate(frames):
                    c_iou[f], c_bnd[f] = torch.tensor(float(J[k])), torch.tensor(float(Fb[k]))
            else:
                for f in frames:
                    m = (c_logits[f] > 0).cpu().numpy()
                    c_iou[f] = torch.tensor(VM.db_eval_iou(m, gt_np[f]))
                    c_bnd[f] = torch.tensor(VM.db_eval_boundary(m, gt_np[f]))

        def full_pass(trajectories, visibilities, point_labels, start=0):
            evaluate(range(start, n_frames), trajectories, visibilities, point_labels)
            return np.mean(c_iou), np.mean(c_bnd)

        def track(rgbs, qp):
            stats["tracker_calls"] += 1
            t, v = self._track_points(rgbs, qp)
            return t.cpu(), v.cpu()

        if state is not None:
            evaluate(range(n_frames), *state)
            return torch.stack(c_logits)

        # 2. initial tracking
        if self.disable_point_tracking:
            trajectories = torch.zeros((n_frames, 1, 1, 2), dtype=torch.float32)
            visibilities = torch.zeros((n_frames, 1, 1), dtype=torch.float32)
            point_labels = torch.ones((1,), dtype=torch.int)
            interactions_left = interactions_max
        else:
            trajectories, visibilities = track(images, query_points)
            point_labels = torch.ones((n_points_per_mask,), dtype=torch.int)
            point_labels[self.positive_points_per_mask:] = 0
            interactions_left -= len(query_points[0])

        # 3. correct until the budget is gone
        checkpoints = []
        current_threshold = thresholds.pop(0)
        history: List[HistoryEntry] = []
        pass_ious, pass_bnds = [], []
        frame_idx = frame_interactions = 0
        prev_iou, prev_bnd = full_pass(trajectories, visibilities, point_labels)
        while interactions_left > 0:
            if frame_idx == n_frames:
                assert len(pass_ious) == n_frames
                checkpoints.append({
                    "current_threshold": current_threshold, "trajectories": trajectories.clone(), "visibilities": visibilities.clone(),
                    "point_labels": point_labels.clone(), "interaction_history": [h._asdict() for h in history],
                    "interactions_left": interactions_left, "average_iou": np.mean(pass_ious),
                    "average_boundary_score": np.mean(pass_bnds), "current_pass_ious": pass_ious,
                    "current_pass_boundary_scores": pass_bnds})
                if len(thresholds) == 0:
                    break
                current_threshold = thresholds.pop(0)
                frame_idx = frame_interactions = 0
                pass_ious, pass_bnds = [], []

            if not self.incremental:                   # (the reference decodes the frame again; the cache holds the same)
                evaluate([frame_idx], trajectories, visibilities, point_labels)
            logits, iou_score, bnd_score = c_logits[frame_idx], c_iou[frame_idx], c_bnd[frame_idx]
            if iou_score >= current_threshold:
                frame_idx += 1
                frame_interactions = 0
                pass_ious.append(iou_score)
                pass_bnds.append(bnd_score)
                continue

            # the click
            if use_dev:
                st = I.frame_state_device(logits, gt_dev[frame_idx], trajectories[frame_idx, 0], visibilities[frame_idx, 0], point_labels)
            else:
                st = I.frame_state(logits, gt_masks[frame_idx], trajectories[frame_idx, 0], visibilities[frame_idx, 0], point_labels)
            if st.first_bad_negative >= 0:
                visibilities[frame_idx:, 0, st.first_bad_negative] = 0
                action_name, action_type, action_point_idx = "remove", "negative", st.first_bad_negative
            elif st.first_bad_positive >= 0:
                visibilities[frame_idx:, 0, st.first_bad_positive] = 0
                action_name, action_type, action_point_idx = "remove", "positive", st.first_bad_positive
            else:
                action_name, action_point_idx = "add", trajectories.shape[2]
                if st.fn > st.fp:
                    mask, mask_sum, label, action_type = st.fn_mask, st.fn, 1, "positive"
                else:
                    mask, mask_sum, label, action_type = st.fp_mask, st.fp, 0, "negative"
                assert mask_sum > 0
                stats["device_clicks" if use_dev else "host_clicks"] += 1
                x, y = I.extract_largest_cluster_points(mask, n_points_to_select=min(3, mask_sum),
                                                        device=pdev if use_dev else None)[0, :].tolist()
                if self.disable_point_tracking:
                    new_t = torch.zeros((n_frames, 1, 1, 2), dtype=torch.float32)
                    new_v = torch.zeros((n_frames, 1, 1), dtype=torch.float32)
                    new_t[frame_idx, 0, 0, :] = torch.tensor([x, y], dtype=torch.float32)
                    new_v[frame_idx, 0, 0] = 1
                else:
                    new_t, new_v = track(images[frame_idx:], torch.tensor([0, x, y], dtype=torch.int)[None, None, :])
                    new_t[0, 0, 0, :] = torch.tensor([x, y], dtype=torch.float32)
                    new_v[0, 0, 0] = 1
                    new_t = torch.cat([torch.zeros((frame_idx, 1, 1, 2), dtype=torch.float32), new_t])
                    new_v = torch.cat([torch.zeros((frame_idx, 1, 1), dtype=torch.float32), new_v])
                trajectories = torch.cat([trajectories, new_t], dim=2)
                visibilities = torch.cat([visibilities, new_v], dim=2)
                point_labels = torch.cat([point_labels, torch.tensor([label], dtype=torch.int)], dim=0)

            # the frame after the click, and the whole clip
            if self.disable_point_tracking:
                evaluate([frame_idx], trajectories, visibilities, point_labels)
                next_iou, next_bnd = prev_iou, prev_bnd
            else:
                if not self.incremental:
                    evaluate([frame_idx], trajectories, visibilities, point_labels)
                next_iou, next_bnd = full_pass(trajectories, visibilities, point_labels, start=frame_idx if self.incremental else 0)
            iou_after, bnd_after = c_iou[frame_idx], c_bnd[frame_idx]
            history.append(HistoryEntry(
                action=action_name, type=action_type, frame_idx=frame_idx, point_idx=action_point_idx,
                iou_before=iou_score.item(), iou_after=iou_after.item(), interaction_idx=interactions_left,
                current_iou_threshold=current_threshold, overall_iou_before=prev_iou.item(), overall_iou_after=next_iou.item(),
                boundary_score_before=bnd_score.item(), boundary_score_after=bnd_after.item(),
                overall_boundary_score_before=prev_bnd.item(), overall_boundary_score_after=next_bnd.item(),
                jf_score_before=(prev_iou.item() + prev_bnd.item()) / 2, jf_score_after=(next_iou.item() + next_bnd.item()) / 2))
            interactions_left -= 1
            frame_interactions += 1
            prev_iou, prev_bnd = next_iou, next_bnd
            if iou_after >= current_threshold or frame_interactions >= self.interactions_max_per_frame:
                frame_idx += 1
                frame_interactions = 0
                pass_ious.append(iou_after)
                pass_bnds.append(bnd_after)

        # 8. the final masks: the cache is the current state's pass
        if not self.incremental:
            full_pass(trajectories, visibilities, point_labels)
        final_iou = np.mean(c_iou)
        used_checkpoint = None
        if len(checkpoints) > 0:
            best = checkpoints[int(np.argmax([c["average_iou"] for c in checkpoints]))]
            if best["average_iou"] > final_iou:
                trajectories, visibilities, point_labels = best["trajectories"], best["visibilities"], best["point_labels"]
                full_pass(trajectories, visibilities, point_labels)
                assert np.isclose(np.mean(c_iou), best["average_iou"], atol=0.001)
                assert np.isclose(np.mean(c_bnd), best["average_boundary_score"], atol=0.001)
                used_checkpoint = best["current_threshold"]
        logits = torch.stack(c_logits)[None]                                   # (1, T, H, W)
        scores_per_frame = torch.stack([s.reshape(()) for s in c_score])[:, None]

        thr_list = [h.current_iou_threshold for h in history]
        overall = {"threshold": thr_list,
                   "achieved_threshold": [max([0] + [t for t in thr_list[:i + 1] if t < thr_list[i]]) for i in range(len(thr_list))],
                   "before": [h.overall_iou_before for h in history], "after": [h.overall_iou_after for h in history]}
        self.last_run = {"interaction_history": history, "achieved_iou_thresholds_cache": checkpoints, "overall_iou_history": overall,
                         "trajectories": trajectories, "visibilities": visibilities, "point_labels": point_labels,
                         "scores_per_frame": scores_per_frame, "interactions_left": interactions_left,
                         "used_checkpoint": used_checkpoint, "final_ious": [t.item() for t in c_iou], **stats}
        if self.output_dir is not None:
            root = os.path.join(self.output_dir, str(video.get("video_id", "video")))
            os.makedirs(root, exist_ok=True)
            with open(os.path.join(root, "history.json"), "w") as fh:
                json.dump([h._asdict() for h in history], fh, indent=4)
            with open(os.path.join(root, "overall_iou_history.json"), "w") as fh:
                json.dump(overall, fh, indent=4)

        target_hw = tuple(video["target_hw"])
        resize_factor = torch.tensor(target_hw) / torch.tensor(logits.shape[-2:])
        assert (resize_factor[0] - resize_factor[1]).abs().item() < 0.01, "The resizing should have been isotropic"
        if tuple(logits.shape[-2:]) != target_hw:
            logits = self._resize_logits(logits, target_hw)
        assert logits.shape == (n_masks, n_frames, target_hw[0], target_hw[1])
        return {"logits": [m for m in logits], "scores": None, "scores_per_frame": None, "trajectories": None, "visibilities": None}
