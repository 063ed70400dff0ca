/* sampt_hip.h — C ABI of libsampt_hip.so, the MI355X (gfx950) HIP implementation of the SAM-PT hot path.
 *
 * The reference (SysCV/sam-pt) has no native code and no FFI: its "plugin boundary" is duck typing through Hydra
 * `_target_`s.  This header is therefore the binding a maintainer of the reference would add
 * underneath the two Python seams — see INTEGRATION.md for the ctypes stub:
 *
 *   seam 1  sam_pt.point_tracker.PointTracker.forward(rgbs, query_points)        sam_pt/point_tracker/tracker.py:26-51
 *           as implemented by PipsPointTracker                                   sam_pt/point_tracker/pips/tracker.py:42-201
 *   seam 2  SamPredictor.set_image / predict_torch as driven by SamPt            sam_pt/modeling/sam_pt.py:771, 783-828, 849
 *
 * Conventions: every function returns 0 (SAMPT_OK) or a negative error code and never throws; all pointers named
 * `*_dev` / documented "device" are HIP device pointers owned by the caller; kernels never allocate; work is
 * enqueued on the given hipStream_t (passed as void*) and no function synchronises unless documented.  Activation
 * scratch comes from a caller-provided workspace: call the *_workspace_bytes query first.
 */
#ifndef SAMPT_HIP_H
#define SAMPT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAMPT_OK 0
#define SAMPT_ERR_ARG (-1)
#define SAMPT_ERR_HIP (-2)
#define SAMPT_ERR_UNSUPPORTED (-3)
#define SAMPT_ERR_WORKSPACE (-4)
#define SAMPT_ERR_CAPACITY (-5)   /* more results than the capacity the caller gave (nothing is truncated silently) */

typedef void* sampt_stream_t; /* hipStream_t */
typedef struct sampt_pips* sampt_pips_t;
typedef struct sampt_pips2* sampt_pips2_t;
typedef struct sampt_cotracker* sampt_cotracker_t;
typedef struct sampt_raft* sampt_raft_t;
typedef struct sampt_sg* sampt_sg_t;
typedef struct sampt_vit* sampt_vit_t;
typedef struct sampt_dec* sampt_dec_t;

int sampt_version(void);
/* Last error message of the calling thread's most recent failing call ("" if none). */
const char* sampt_last_error(void);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1 — PIPS point tracker.  Weights: `n` (name, device pointer) pairs keyed by the upstream checkpoint keys
 * (model-*.pth['model_state_dict'], module tree pips.py:191-287, 290-317, 410-437) after the host-side repack
 * documented in sam_pt_amd/pack.py (conv weights -> [Cout][KH][KW][Cin], stem Cin padded to 4, mixer input
 * weight K padded 519 -> 520, "ffeat_updater.0.weight_t", "__times").
 * --------------------------------------------------------------------------------------------------------- */
int sampt_pips_create(const char* const* names, const void* const* ptrs, int n, int stride, int S, sampt_pips_t* out);
void sampt_pips_destroy(sampt_pips_t h);

/* Pips.fnet (BasicEncoder, pips.py:254-287) + CorrBlock pyramid (pips.py:355-361) for `nf` frames.
 * frames_dev: uint8 (nf,3,H,W) as handed to PointTracker.forward.  pyr_dev[l]: float32 [nf][H_l][W_l][128] (NHWC),
 * H_0 = H/stride, H_{l+1} = H_l/2.  Replaces `self.fnet(rgbs_)` at pips.py:453-455 and CorrBlock.__init__. */
int sampt_pips_fnet_workspace_bytes(sampt_pips_t h, int nf, int H, int W, size_t* bytes);
int sampt_pips_fnet_f32(sampt_pips_t h, const uint8_t* frames_dev, int nf, int H, int W, float* const pyr_dev[4],
                        void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);

/* Initial point features: bilinear_sample2d(fmaps[:,0], xy/stride) (pips.py:469-475, utils/samp.py:6-80).
 * fmap_dev: level-0 maps [frames][H0][W0][128]; frame_idx_dev: int32 [n] frame of each point (NULL: frame 0);
 * xy_dev: [n][2] in feature-map pixels; out_dev: [n][128]. */
int sampt_pips_sample_feat_f32(const float* fmap_dev, int H0, int W0, const int32_t* frame_idx_dev, const float* xy_dev,
                               int n, float* out_dev, sampt_stream_t stream);

/* All chained 8-frame windows of PipsPointTracker._forward (sam_pt/point_tracker/pips/tracker.py:42-153) for n point CHAINS
 * (one point in one temporal direction) over a T-frame pyramid, with the per-window bookkeeping — window frames, write-back
 * of frames 1..7, visibility-threshold linking (tracker.py:111-148) — on the device.  q_* [n][3] = (t, x, y) of each chain's
 * query in ITS OWN time axis (the same values on the device and on the host), flip_* [n] bytes: chain frame d reads pyramid
 * frame T-1-d (tracker.py:162-167).  vis_threshold = initial_next_frame_visibility_threshold (pips.yaml:5).  chunk_events
 * (hipEvent_t[nchunks], may be NULL with nchunks = 0): pyramid frames [chunk_lo[c], chunk_hi[c]) are valid once event c has
 * fired; each round waits only for the chunks it can reach.  traj_dev [T][n][2] px and vis_dev [T][n] (sigmoid; 0 where
 * never written) are complete when the call returns: the number of rounds is data dependent, so this entry point
 * SYNCHRONISES with `stream` (rounds are enqueued one ahead of the device; at most one idle round is spent). */
int sampt_pips_track_workspace_bytes(sampt_pips_t h, int n, size_t* bytes);
int sampt_pips_track_f32(sampt_pips_t h, const float* const pyr_dev[4], int H0, int W0, int T, int n, const float* q_dev,
                         const uint8_t* flip_dev, const float* q_host, const uint8_t* flip_host, float vis_threshold, int iters,
                         void* const* chunk_events, const int32_t* chunk_lo, const int32_t* chunk_hi, int nchunks,
                         float* traj_dev, float* vis_dev, void* ws, size_t ws_bytes, sampt_stream_t stream, int32_t* rounds);
/* One 8-frame window of Pips.forward's iterative update (pips.py:458-476, 507-568) + sigmoid (pips/tracker.py:102).
 * frame_idx_dev: int32 [n][S] — per POINT, the indices of its window frames in the pyramid (tail repeated as
 * tracker.py:73-78).  Points are independent in PIPS, so points anchored at different frames share one call;
 * xys_dev: [n][2] pixels at the window's first frame; feat_init_dev: [n][128].
 * traj_out_dev: [S][n][2] pixels (last iteration); vis_out_dev: [S][n] in (0,1). */
/* Kernel launches of one ROUND of the last sampt_pips_track_f32 call (one window of every chain: round begin, the window's
 * iterations as counted at their launch sites, round end); 0 before the first call. */
int sampt_pips_round_launches(sampt_pips_t h);
int sampt_pips_update_workspace_bytes(sampt_pips_t h, int n, size_t* bytes);
int sampt_pips_update_f32(sampt_pips_t h, const float* const pyr_dev[4], int H0, int W0, const int32_t* frame_idx_dev,
                          int n, const float* xys_dev, const float* feat_init_dev, int iters, float* traj_out_dev,
                          float* vis_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1b — PIPS++ point tracker (sam_pt/point_tracker/pips_plus_plus/{pips_plus_plus.py:420-546, tracker.py:25-134}).
 * Weights keyed by the checkpoint names after sam_pt_amd.pack.pack_pips2 (fnet convs as for PIPS; Conv1d weights
 * (Cout, Cin, 3) -> [Cout][3][Cin] with the first conv's 718 input channels zero-padded to 720; "__omega" [32]).
 * fnet_f32 = PipsPlusPlus.fnet on every frame + the 4-level average-pool pyramid of CorrBlock.__init__ (:366-379),
 * stride 8.  update_f32 = one PipsPlusPlus.forward after the encoder for n points over a chunk of S frames
 * (frame_idx_dev int32 [n][S] selects each point's pyramid frames, so sub-clips and time-reversed clips are index
 * maps): trajs0_dev [S][n][2] px is `trajs_e0`, feats_dev[3] = (feats1, feats2, feats4) [n][S][128] are read as
 * `feat_init` when have_feat_init != 0 and always written back (tracker.py:49-54), trajs_out_dev [S][n][2] px =
 * coord_predictions1[-1].
 * --------------------------------------------------------------------------------------------------------- */
int sampt_pips2_create(const char* const* names, const void* const* ptrs, int n, int stride, sampt_pips2_t* out);
void sampt_pips2_destroy(sampt_pips2_t h);
int sampt_pips2_fnet_workspace_bytes(sampt_pips2_t h, int nf, int H, int W, size_t* bytes);
/* frames_dev: (nf,3,H,W) uint8, or float32 in [0, 255] when frames_are_f32 != 0 (the bilinearly pre-resized video of
 * PipsPlusPlusPointTracker(image_size=...), tracker.py:69-76). */
int sampt_pips2_fnet_f32(sampt_pips2_t h, const void* frames_dev, int frames_are_f32, int nf, int H, int W,
                         float* const pyr_dev[4], void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_pips2_update_workspace_bytes(sampt_pips2_t h, int n, int S, size_t* bytes);
int sampt_pips2_update_f32(sampt_pips2_t h, const float* const pyr_dev[4], int H0, int W0, const int32_t* frame_idx_dev,
                           int n, int S, const float* trajs0_dev, int have_feat_init, float* const feats_dev[3],
                           int iters, float* trajs_out_dev, void* workspace_dev, size_t workspace_bytes,
                           sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1c — CoTracker = what sam_pt.point_tracker.cotracker.CoTrackerPointTracker.forward (cotracker/tracker.py:72-170)
 * asks of the third-party model (facebookresearch/co-tracker @ 4f297a9, built by build_cotracker from
 * cotracker_stride_4_wind_8.pth: CoTracker(stride=4, S=8, space_depth=6, time_depth=6)).
 * Weight names: the checkpoint's keys ("fnet.*" packed like PIPS' encoder, "updateformer.input_transform",
 * "updateformer.{time,space}_blocks.{i}.{attn.qkv,attn.proj,mlp.fc1,mlp.fc2}", "updateformer.flow_head", "norm",
 * "ffeat_updater.0" (+ ".weight_t"), "vis_predictor.0") plus "__times_embed" [8][456], "__ln_ones"/"__ln_zeros" [384]
 * (sam_pt_amd/pack.py::pack_cotracker).
 *   resize_frames_f32 : the adapter's F.interpolate(rgbs, interp_shape, mode="bilinear") (tracker.py:90-92) over `planes`
 *                       = T*3 single-channel planes, uint8 (src_u8 != 0) or float32 input, float32 output in [0, 255].
 *                       Source positions are exact integer fractions (not torch's f32 product); every size <= 16384.  Also the
 *                       entry point of the resize_planes kernel test.
 *   fnet_f32          : CoTracker.fnet (the BasicEncoder of PIPS, stride 4) on every float frame + the 4-level average-pool
 *                       pyramid of CorrBlock; each frame once per clip (InstanceNorm is per-sample), both directions share it.
 *   track_f32         : one CoTracker.forward (one temporal direction) over T >= 8 model frames: sliding windows of 8 frames
 *                       with step 4, `iters` UpdateFormer iterations each, the carry-over between windows on the device, no
 *                       host synchronisation.  frame_map_dev int32 [T]: pyramid frame of model frame t (identity; T-1-t for
 *                       the time-flipped pass of tracker.py:154-161; clamped to the last real frame for clips shorter than 8,
 *                       tracker.py:17-21).  Points SORTED by query frame as CoTracker.forward sorts them: query_t_host /
 *                       query_t_dev int32 [n] (same values; window membership is host control flow), query_xy_dev [n][2] px
 *                       of the model frame size.  pos_x_dev [W0][228] / pos_y_dev [H0][228]: the 1-D tables of
 *                       get_2d_sincos_pos_embed(456, (H0, W0)).  traj_out_dev [T][n][2] px — exact zeros where no window
 *                       wrote (what the adapter's `== 0` back-fill keys on, tracker.py:166) — vis_out_dev [T][n] =
 *                       sigmoid(visibility logit), 0.5 where no window wrote.
 * --------------------------------------------------------------------------------------------------------- */
int sampt_cotracker_create(const char* const* names, const void* const* ptrs, int n, int stride, int S,
                           sampt_cotracker_t* out);
void sampt_cotracker_destroy(sampt_cotracker_t h);
int sampt_resize_frames_f32(const void* frames_dev, int src_u8, long planes, int H, int W, float* out_dev, int out_h,
                            int out_w, sampt_stream_t stream);
int sampt_cotracker_fnet_workspace_bytes(sampt_cotracker_t h, int nf, int H, int W, size_t* bytes);
int sampt_cotracker_fnet_f32(sampt_cotracker_t h, const float* frames_dev, int nf, int H, int W, float* const pyr_dev[4],
                             void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_cotracker_track_workspace_bytes(sampt_cotracker_t h, int n, size_t* bytes);
int sampt_cotracker_track_f32(sampt_cotracker_t h, const float* const pyr_dev[4], int H0, int W0, int T,
                              const int32_t* frame_map_dev, int n, const int32_t* query_t_host,
                              const int32_t* query_t_dev, const float* query_xy_dev, const float* pos_x_dev,
                              const float* pos_y_dev, int iters, float* traj_out_dev, float* vis_out_dev,
                              void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1d — RAFT point tracker (sam_pt/point_tracker/raft/{tracker.py:29-88, raftnet.py:29-43, raft_core/}).
 * Weights keyed by the names of raft-things.pth without "module." after sam_pt_amd.pack.pack_raft: convolutions
 * [Cout][KH][KW][Cin] (both stems' Cin zero-padded 3 -> 4), cnet's eval-mode BatchNorms folded into the convolution in
 * front of them, "update_block.encoder.convc1" K-padded 324 -> 352, "update_block.encoder.convf1.weight" as [98][128],
 * "update_block.gru.convzr{1,2}" = [convz; convr], "update_block.flow_head.conv2" N-padded 2 -> 4.
 *   flows_f32 : frames_dev uint8 (T,3,H,W) -> flows_fwd_dev / flows_bwd_dev [T-1][2][H][W] = Raftnet.forward(rgb[t],
 *               rgb[t+1], iters)[0] and its reverse, un-padded; flow_low_dev (optional) [2][T-1][2][Hp/8][Wp/8] = the 1/8
 *               resolution flows (forward stack, then backward).  fnet and cnet run once per frame; pair-directions go
 *               through the correlation pyramid and the update block in chunks of as many pairs as the workspace holds
 *               (workspace_bytes sizes it for max_pairs_in_flight; a smaller workspace means more chunks, same result).
 *               Frames whose size padded to multiples of 8 is below 128 on either side are refused with
 *               SAMPT_ERR_UNSUPPORTED: the coarsest correlation level would be a single cell, where the reference
 *               divides by zero and returns NaN.
 *   chain     : tracker.py:46-88 — query_points_dev [n][3] = (t, x, y); traj_out_dev [T][n][2] f32, vis_out_dev [T][n]
 *               bytes (0 / 1).
 * Test entry points: corr_pyramid (fmap1, fmap2 [hw][256] NHWC -> the 4 levels [hw][h_l w_l]; ws of
 * sampt_raft_corr_pyramid_workspace_bytes), lookup (levels [M][h_l w_l] = one plane per row, coords [M][2] -> [M][352], any M >= 1),
 * upsample (flow_low [P][h8][w8][2],
 * mask [P][h8][w8][576] -> [P][2][H][W]).
 * --------------------------------------------------------------------------------------------------------- */
int sampt_raft_create(const char* const* names, const void* const* ptrs, int n, sampt_raft_t* out);
void sampt_raft_destroy(sampt_raft_t h);
int sampt_raft_workspace_bytes(sampt_raft_t h, int T, int H, int W, int max_pairs_in_flight, size_t* bytes);
int sampt_raft_flows_f32(sampt_raft_t h, const uint8_t* frames_dev, int T, int H, int W, int iters, float* flows_fwd_dev,
                         float* flows_bwd_dev, float* flow_low_dev, void* workspace_dev, size_t workspace_bytes,
                         sampt_stream_t stream);
int sampt_raft_chain(const float* flows_fwd_dev, const float* flows_bwd_dev, int T, int H, int W,
                     const float* query_points_dev, int n, float* traj_out_dev, uint8_t* vis_out_dev, sampt_stream_t stream);
size_t sampt_raft_corr_pyramid_workspace_bytes(int h8, int w8);
int sampt_raft_corr_pyramid(const float* fmap1_dev, const float* fmap2_dev, int h8, int w8, float* const levels_dev[4],
                            void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_raft_lookup(const float* const levels_dev[4], int h8, int w8, const float* coords_dev, long m, float* out_dev,
                      sampt_stream_t stream);
int sampt_raft_upsample(const float* flow_low_dev, const float* mask_dev, float mask_scale, int pairs, int h8, int w8, int H,
                        int W, float* out_dev, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1f — TAPIR point tracker (sam_pt/point_tracker/tapir/{tracker.py:72-108, tapir_model.py, models/resnet.py,
 * utils/model_utils.py}).  Weights under the flat names of sam_pt_amd.weights.init_tapir_state_dict after
 * sam_pt_amd.pack.pack_tapir: convolutions [Cout][KH][KW][Cin] (the stem's Cin zero-padded 3 -> 4) with ".weight_hl" split-fp16
 * planes where Cin % 32 == 0, "mixer.in.weight" K-padded 486 -> 496, the depthwise weights as [3][2048].
 * The model's geometry is fixed: 256 x 256 frames, hires 64 x 64 x 128, lowres 32 x 32 x 256.  Rows are (query, frame): q * T + t.
 *   track_f32 : frames_dev f32 (T,3,256,256) in [0, 1] (the adapter's antialiased resize of the clip / 255), query_points_dev
 *               [n][3] = (t, x, y) in 256 x 256 pixels -> tracks_dev [n][T][2] (x, y) px, occlusion_dev / expected_dist_dev [n][T]
 *               logits after `iters` refinements (iters >= 0; 0 = the cost-volume heads alone).  iter_out_dev (optional)
 *               [iters + 1][n][T][4] = (x, y, occlusion, expected_dist) after the heads and after every refinement.  One call per
 *               clip, no host synchronisation.  The refinement runs in chunks of as many queries as the workspace holds
 *               (workspace_bytes sizes it for max_queries_in_flight; a smaller workspace means more chunks, same values).
 *   backbone_f32 : the feature maps alone: hires_dev [nf][64][64][128], lowres_dev [nf][32][32][256], channel-normalised.
 * Kernel-level entry points (no handle): query_feats (bilinear edge-clamped read of both maps -> [n][384] = hires | lowres),
 * heads (one workgroup per (query, frame): weights[10] = w1 [16][9], b1, w2 [16][9], b2, w3 [16][9][32], b3, w4 [16][32], b4,
 * w5 [2][16], b5; the 256 lowres channels of a query start at qf[q * ldq + qoff]), patch_corr (mixer input rows [n T][ldx >= 486]),
 * temporal_mix (the mixer's time half-block; x, xo [n][T][512], ln [512], w1 / b1 / w2 / b2 [3][2048] / [2048]), gemm (act: 0 none,
 * 1 ReLU, 3 tanh-GELU; K % 16 == 0, N % 4 == 0; every row's K order is the same whatever M is), conv2d_same_nhwc (bias-free, TensorFlow
 * "SAME" padding — asymmetric under stride 2; dtype as for sampt_conv2d_nhwc: 0, 3 or 4) and instance_norm_affine_nhwc (scale and
 * offset, optional ReLU; y_dev and / or y_hl_dev [2][n][hw][C] halves = the split-fp16 planes; ws of sampt_instance_norm_workspace_bytes).
 * Every entry returns SAMPT_ERR_ARG for null pointers or non-positive counts before any launch.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct sampt_tapir* sampt_tapir_t;
int sampt_tapir_create(const char* const* names, const void* const* ptrs, int n, sampt_tapir_t* out);
void sampt_tapir_destroy(sampt_tapir_t h);
int sampt_tapir_workspace_bytes(sampt_tapir_t h, int T, int n, int max_queries_in_flight, size_t* bytes);
int sampt_tapir_track_f32(sampt_tapir_t h, const float* frames_dev, int T, const float* query_points_dev, int n, int iters,
                          float* tracks_dev, float* occlusion_dev, float* expected_dist_dev, float* iter_out_dev, void* workspace_dev,
                          size_t workspace_bytes, sampt_stream_t stream);
/* NOMINAL kernel launches of the last track_f32 call: the engine adds, per stage that really ran, the number of kernels that stage
 * is written as (an InstanceNorm = 3: partial sums, statistics, apply; every convolution, GEMM and TAPIR kernel = 1).  It is not
 * measured at the launch sites, so a dispatcher that splits a launch does not show.  0 for a null handle or before the first call. */
int sampt_tapir_launches(sampt_tapir_t h);
/* at most max_queries queries per refinement chunk even where the workspace holds more (0: no bound).  At few frames the workspace is
 * bounded by one frame's backbone scratch, not by the chunk, so this is how a caller (or a test) asks for smaller chunks. */
int sampt_tapir_set_max_queries(sampt_tapir_t h, int max_queries);
int sampt_tapir_backbone_workspace_bytes(sampt_tapir_t h, int nf, size_t* bytes);
int sampt_tapir_backbone_f32(sampt_tapir_t h, const float* frames_dev, int nf, float* hires_dev, float* lowres_dev, void* workspace_dev,
                             size_t workspace_bytes, sampt_stream_t stream);
int sampt_tapir_query_feats_f32(const float* hires_dev, const float* lowres_dev, int T, const float* query_points_dev, int n,
                                float* qf_dev, sampt_stream_t stream);
int sampt_tapir_heads_f32(const float* lowres_dev, int T, const float* qf_dev, int ldq, int qoff, const float* query_points_dev, int n,
                          const float* const weights_dev[10], float* points_dev, float* occlusion_dev, float* expected_dist_dev,
                          sampt_stream_t stream);
int sampt_tapir_patch_corr_f32(const float* hires_dev, const float* lowres_dev, int T, int n, const float* pos_dev, const float* occ_dev,
                               const float* expd_dev, const float* feat_dev, int feat_per_row, float* x_dev, int ldx, sampt_stream_t stream);
int sampt_tapir_temporal_mix_f32(const float* x_dev, float* xo_dev, const float* ln_dev, const float* w1_dev, const float* b1_dev,
                                 const float* w2_dev, const float* b2_dev, int n, int T, sampt_stream_t stream);
int sampt_tapir_gemm_f32(const float* A_dev, const float* W_dev, const float* bias_dev, const float* res_dev, float* C_dev, int M, int N,
                         int K, int act, sampt_stream_t stream);
int sampt_conv2d_same_nhwc(int dtype, const void* x_dev, const void* w_dev, float* y_dev, int n, int H, int W, int Cin, int Cout, int K,
                           int stride, sampt_stream_t stream);
int sampt_instance_norm_affine_nhwc(const float* x_dev, const float* scale_dev, const float* offset_dev, float* y_dev, void* y_hl_dev,
                                    int n, int hw, int C, float eps, int relu, void* workspace_dev, size_t workspace_bytes,
                                    sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1g — TapNet point tracker (sam_pt/point_tracker/tapnet/{tracker.py:67-103, tapnet_model.py, models/tsm_resnet.py,
 * models/tsm_utils.py}).  Weights under the flat names of sam_pt_amd.weights.init_tapnet_state_dict after
 * sam_pt_amd.pack.pack_tapnet: convolutions [Cout][KH][KW][Cin] (the stem's Cin zero-padded 3 -> 4) with ".weight_hl" split-fp16
 * planes where Cin % 32 == 0, every BatchNorm folded into "<norm>.a" / "<norm>.b", the heads as for TAPIR with occ_out [1][16].
 * The model's geometry is fixed: 256 x 256 frames, a 32 x 32 x 256 grid per frame.  Rows are (query, frame): q * T + t.
 *   track_f32 : frames_dev f32 (T,3,256,256) in [0, 1] (the adapter's antialiased resize of the clip / 255), query_points_dev
 *               [n][3] = (t, x, y) in 256 x 256 pixels -> tracks_dev [n][T][2] (x, y) px, occlusion_dev [n][T] logits.  One call
 *               per clip for any T >= 1 (at most 4096), no host synchronisation; every block of the backbone takes all T frames in
 *               one launch per kernel, the stem and the max-pool run in chunks of frames (set_stem_chunk, default 8; same values).
 *   backbone_f32 : the grid alone, grid_dev [nf][32][32][256], channel-normalised.  stages_dev (optional, each entry optional):
 *               the max-pooled stem [nf][64][64][64] and the raw outputs of units 0, 1, 2 ([nf][64][64][64], [nf][32][32][128],
 *               [nf][32][32][256]).  The nf frames are ONE clip: the temporal shift couples neighbours.
 * Kernel-level entry points (no handle): bn_shift (relu(a[c] x + b[c]) of x [T][hw][C], shifted in time by n_shift channels each
 * way -> shifted_dev f32 and / or shifted_hl_dev [2][T][hw][C] halves = the split-fp16 planes; the same map unshifted -> unshifted_dev
 * / unshifted_hl_dev where given), maxpool_nhwc (3 x 3, stride 2, "SAME"; y [n][ceil(H/2)][ceil(W/2)][C]), query_feats (trilinear,
 * every index clamped -> [n][256]), heads (weights[10] as for sampt_tapir_heads_f32 with w5 [1][16]; temperature 10, no ReLU after w3).
 * Every entry returns SAMPT_ERR_ARG for null pointers or non-positive counts before any launch.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct sampt_tapnet* sampt_tapnet_t;
int sampt_tapnet_create(const char* const* names, const void* const* ptrs, int n, sampt_tapnet_t* out);
void sampt_tapnet_destroy(sampt_tapnet_t h);
int sampt_tapnet_workspace_bytes(sampt_tapnet_t h, int T, int n, size_t* bytes);
int sampt_tapnet_track_f32(sampt_tapnet_t h, const float* frames_dev, int T, const float* query_points_dev, int n, float* tracks_dev,
                           float* occlusion_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* NOMINAL kernel launches of the last track_f32 / backbone_f32 call: 3 per stem chunk + 27 for the six blocks + 1 channel
 * normalisation (+ 2: query features, heads).  Not measured at the launch sites.  0 for a null handle or before the first call. */
int sampt_tapnet_launches(sampt_tapnet_t h);
int sampt_tapnet_set_stem_chunk(sampt_tapnet_t h, int frames);
int sampt_tapnet_backbone_workspace_bytes(sampt_tapnet_t h, int nf, size_t* bytes);
int sampt_tapnet_backbone_f32(sampt_tapnet_t h, const float* frames_dev, int nf, float* grid_dev, float* const stages_dev[4],
                              void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_tapnet_bn_shift_f32(const float* x_dev, const float* a_dev, const float* b_dev, int T, int hw, int C, int n_shift,
                              float* shifted_dev, void* shifted_hl_dev, float* unshifted_dev, void* unshifted_hl_dev, sampt_stream_t stream);
int sampt_tapnet_maxpool_nhwc(const float* x_dev, float* y_dev, int n, int H, int W, int C, sampt_stream_t stream);
int sampt_tapnet_query_feats_f32(const float* grid_dev, int T, const float* query_points_dev, int n, float* qf_dev, sampt_stream_t stream);
int sampt_tapnet_heads_f32(const float* grid_dev, int T, const float* qf_dev, const float* query_points_dev, int n,
                           const float* const weights_dev[10], float* points_dev, float* occlusion_dev, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 1e — SuperGlue point tracker (sam_pt/point_tracker/superglue/{tracker.py, models/superpoint.py, models/superglue.py}).
 * Weights after sam_pt_amd.pack.pack_superglue: "superpoint.<conv>.{weight,bias}" as [Cout][KH][KW][Cin] (conv1a's Cin
 * zero-padded 1 -> 4, convPb's Cout 65 -> 68), "superglue.kenc.<0..4>", "superglue.gnn.<l>.{qkv,merge,mlp0,mlp1}",
 * "superglue.final_proj" as [N][K] with every eval-mode BatchNorm1d folded in and the attention heads permuted from the
 * reference's interleaved channels (d * 4 + h) to blocked ones (h * 64 + d); "superglue.bin_score" [1].
 *   detect : frames_dev uint8 (T,3,H,W) -> per frame the keypoints (x, y) [T][cap][2] in torch.nonzero's order, their scores
 *            [T][cap], sampled descriptors [T][cap][256] (rows, not channels-first) and counts [T] on the device AND on the host
 *            (one stream synchronisation).  dense_dev (optional) receives the score maps [T][8 (H/8)][8 (W/8)].  A frame with
 *            more than cap keypoints makes the call return SAMPT_ERR_CAPACITY (counts_host then holds the true counts; no
 *            descriptor has been sampled).
 *   match  : SuperGlue on one pair -> matches0_dev int32 [n0] (-1 = none), mscores0_dev [n0].  n0 == 0 or n1 == 0: all -1 / 0.
 *            Optional copies for tests: gnn_out_dev [n0 + n1][256] (descriptors after the last GNN layer, blocked-head
 *            independent), scores_out_dev [n0][n1] (the matrix Sinkhorn starts from), uv_out_dev [n0 + 1 + n1 + 1].
 * Test / building-block entry points: nms (dense score maps -> keypoints, as inside detect), sample_descriptors (raw dense
 * descriptor map [h8 * w8][256] NHWC + n keypoints -> [n][256]), attention (q [N][heads * 64], k / v [M][heads * 64], blocked
 * heads, scale 1 / 8), sinkhorn (S [N][M] -> u [N + 1], v [M + 1]), mutual_match (S, u, v -> matches0, mscores0; ws of
 * (2 N + M) * 4 bytes), select (per-mask ordered lists of matched keypoint-1 indices inside / outside the mask) and gather.
 * --------------------------------------------------------------------------------------------------------- */
int sampt_sg_create(const char* const* names, const void* const* ptrs, int n, sampt_sg_t* out);
void sampt_sg_destroy(sampt_sg_t h);
int sampt_sg_workspace_bytes(sampt_sg_t h, int T, int H, int W, int n0, int n1, size_t* detect_bytes, size_t* match_bytes);
int sampt_sg_detect(sampt_sg_t h, const uint8_t* frames_dev, int T, int H, int W, int nms_radius, float keypoint_threshold,
                    int remove_borders, int cap, float* kpts_dev, float* kscores_dev, float* desc_dev, int32_t* counts_dev,
                    int32_t* counts_host, float* dense_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_sg_match(sampt_sg_t h, const float* kpts0_dev, const float* kscores0_dev, const float* desc0_dev, int n0,
                   const float* kpts1_dev, const float* kscores1_dev, const float* desc1_dev, int n1, int H, int W,
                   int sinkhorn_iterations, float match_threshold, int32_t* matches0_dev, float* mscores0_dev, float* gnn_out_dev,
                   float* scores_out_dev, float* uv_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
size_t sampt_sg_nms_workspace_bytes(int nimg, int Hs, int Ws);
int sampt_sg_nms(const float* scores_dev, int nimg, int Hs, int Ws, int nms_radius, float keypoint_threshold, int remove_borders,
                 int cap, float* kpts_dev, float* kscores_dev, int32_t* counts_dev, int32_t* counts_host, void* workspace_dev,
                 size_t workspace_bytes, sampt_stream_t stream);
int sampt_sg_sample_descriptors(const float* dmap_dev, int h8, int w8, const float* kpts_dev, int n, float* out_dev,
                                sampt_stream_t stream);
int sampt_sg_attention(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int N, int M, int heads,
                       sampt_stream_t stream);
int sampt_sg_sinkhorn(const float* scores_dev, int N, int M, const float* bin_score_dev, int iters, float* u_dev, float* v_dev,
                      sampt_stream_t stream);
int sampt_sg_mutual_match(const float* scores_dev, int N, int M, const float* u_dev, const float* v_dev, float match_threshold,
                          int32_t* matches0_dev, float* mscores0_dev, void* workspace_dev, size_t workspace_bytes,
                          sampt_stream_t stream);
int sampt_sg_select(const int32_t* matches0_dev, int n0, const float* kpts1_dev, const float* masks_dev, int n_masks, int H, int W,
                    int cap, int32_t* lists_dev, int32_t* counts_dev, sampt_stream_t stream);
int sampt_sg_gather(const float* query_xy_dev, const float* kpts_dev, int kp_cap, const int32_t* lists_dev, int list_cap,
                    const int32_t* counts_dev, const int32_t* draw_dev, int T, int n_masks, int n_pos, int n_neg, float* traj_dev,
                    float* vis_dev, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 2a — SAM image encoder = SamPredictor.set_image (Sam.preprocess + ImageEncoderViT, Appendix A-1..A-3).
 * cfg: see sampt_vit_config.  Weight names: upstream sam_vit_*.pth keys; GEMM weights as ".f16" copies when
 * cfg.f16 == 1, as ".x3" copies (x3 rows of w * 2^8, see sampt_gemm_ex) when cfg.f16 == 2;
 * "image_encoder.neck.2.weight_khwc"; "__win_rows" (window-partition row map for win_batches frames).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct sampt_vit_config {
  int embed_dim, depth, num_heads, grid, window, patch, out_chans, mlp_ratio, img_size;
  int global_mask; /* bit i: block i uses global attention (configs/model/sam/image_encoder/vit_*.yaml) */
  int f16;         /* 1: fp16 MFMA + flash attention (fp32 accumulate/softmax/LN/residual); 0: exact fp32 (f32 MFMA,
                      materialised scores); 2: "f16x3" — the fp16 graph with every product rebuilt from split-fp16 pieces
                      (hi.hi + hi.lo + lo.hi, fp32 accumulate): fp32-grade results on the fp16 matrix pipe */
  float pixel_mean[3], pixel_std[3];
} sampt_vit_config;

int sampt_vit_create(const sampt_vit_config* cfg, const char* const* names, const void* const* ptrs, int n,
                     int win_batches, sampt_vit_t* out);
void sampt_vit_destroy(sampt_vit_t h);
int sampt_vit_encode_workspace_bytes(sampt_vit_t h, int B, size_t* bytes);
/* Persistent workgroups per XCD (of 32 CUs) for the encoder's fp16 GEMMs from now on; 0 = one per CU (the default).  A
 * GEMM workgroup (512 threads, 128 KiB of LDS, 256 VGPRs) owns its CU: a caller that runs latency-bound kernels on another
 * stream beside the encoder (the point tracker's window rounds) leaves them a few CUs per XCD this way. */
int sampt_vit_set_gemm_workgroups(sampt_vit_t h, int per_xcd);
/* The same per launch kind — the qkv, proj, fc1 and fc2 GEMM of a block — each 0 .. 32, 0 = whatever
 * sampt_vit_set_gemm_workgroups says.  The four shapes have different tile counts (N / 256 = 15, 5, 20, 5 column tiles for
 * ViT-H), so the number of workgroups that wastes least of the last round of tiles differs per kind. */
int sampt_vit_set_gemm_workgroups_kind(sampt_vit_t h, int qkv, int proj, int fc1, int fc2);
/* Per handle, fp16 mode (cfg.f16 == 1; ignored by the other two): on = 1 (default) — the qkv GEMM of every block writes the head-major
 * matrix [3][heads][rows][hd] and the attention kernel reads it (sampt_gemm_f16_head_major, sampt_vit_attention_f16_head_major)
 * instead of token-major rows.  Bitwise the same embeddings.  A new handle has it ON (the measured default: DESIGN.md section 4, k_flash_f16); 0 = token-major. */
int sampt_vit_set_attention_head_major(sampt_vit_t h, int on);
/* Process-wide experiment knob of the 8-phase fp16 GEMM (csrc/gemm_f16_p8.hip): G > 1 phase groups — persistent workgroup w of an
 * XCD belongs to group w % G and starts (w % G) / G of a tile's K-loop late, so that the groups' epilogue bursts interleave with
 * the other groups' K-loops.  0 / 1 = off (the default). */
int sampt_gemm_set_stagger(int groups);
/* Process-wide A / B switch of the same kernel's stage schedule: 0 (default) = the LDS-DMA instructions of a phase are issued in
 * its read segment, two phases after the half tile's last read; 1 = behind the first MFMAs of its multiply segment, one phase
 * after the last read (the round-3 / round-4 schedule).  Results are bitwise identical. */
int sampt_gemm_set_schedule(int sched);
/* Process-wide switch of the persistent fp16 GEMM's launcher: 1 (default) = a launch uses the FEWEST workgroups per XCD that need the
 * same number of tile rounds as the allowed count (sampt_vit_set_gemm_workgroups, or 32) — same finishing time, whole CUs left to the
 * streams beside it; 0 = always the allowed count.  Results are bitwise identical. */
int sampt_gemm_set_trim(int on);
/* Process-wide knob of the thin f32 GEMM (csrc/gemm.hip gemm_thin_f32: the tracker mixers' token-side products): the launcher grows
 * the (16 * FM) x 16 tile only while at least n workgroups remain (default 256 = one per CU). */
int sampt_gemm_set_thin_min_wgs(int n);
/* Process-wide A / B switch: 1 (default) = 3 x 3 stride-1 split-fp16 convolutions over pre-split planes (the tracker encoder's) run on
 * the halo-tiled kernel of csrc/conv_halo_x3.hip; 0 = on the implicit-GEMM LDS-DMA kernel of rounds 3 - 5 (csrc/conv_f16x3.hip);
 * 2 = halo-tiled with 4-wave workgroups at every tile width (1 uses 8 waves from 96 output channels up); 3 = as 1, but the tracker
 * encoder's InstanceNorms sum their statistics in a pass of their own instead of in the convolution's epilogue. */
int sampt_conv_set_halo(int on);
/* Staging of SamPt's per-frame decode (sam_pt.py:690-757 _apply_sam_to_trajectories: one predict_mask per (frame, object) item,
 * item = frame * n_objects + object) for a batched chain that reads and writes fixed buffers.  idx: rows int32 item numbers (device).
 *   scatter = 0: dst[r] = src[idx[r] / n_objects]                                   (item r's frame embedding into the chain's input)
 *   scatter = 1: dst[(idx[r] % n_objects) * n_frames + idx[r] / n_objects] = src[r]  (masks into logits [n_objects][n_frames][H * W];
 *                scores with n_objects = 1: dst[idx[r]] = src[r])
 * row_bytes: any positive multiple of 4, src and dst 4-byte aligned (frames of every size: H * W floats).  Rows that are a multiple
 * of 16 bytes on 16-byte aligned src and dst move in 16-byte units, all others word by word.  A row_bytes that is no multiple of 4, a
 * pointer off 4-byte alignment, a null pointer, or rows, n_objects (n_frames of a scatter) <= 0: SAMPT_ERR_ARG with the argument
 * named in sampt_last_error, nothing launched.  sampt_fill_f32: dst[0 .. n) = value, dst 4-byte aligned, n > 0 (the -inf of items
 * without a prompt, sam_pt.py:766-767). */
int sampt_move_rows(const void* src, void* dst, const int* idx, int rows, size_t row_bytes, int n_objects, int n_frames, int scatter,
                    sampt_stream_t stream);
int sampt_fill_f32(float* dst, size_t n, float value, sampt_stream_t stream);
/* The tracker encoder's stem (pips.py:200 BasicEncoder.conv1: Conv2d(3, 64, 7, stride 2, padding 3)) over normalised NHWC4 frames
 * x [n][H][W][4] (fourth channel 0) with w f32 [64][7][7][4], as 3-term split-fp16 MFMA products — fp32-grade.  y [n][OH][OW][64].
 * mean_rstd non-null: also the statistics of the InstanceNorm2d that follows ([n][64][2], as sampt_conv3x3_planes_instnorm_stats);
 * ws then holds n * ceil(OH / 16) * ceil(OW / 16) * 64 * 16 bytes. */
int sampt_conv_stem7x7(const float* x_nhwc4, const float* w, const float* bias, float* y, int n, int H, int W, float eps,
                       float* mean_rstd, void* ws, size_t ws_bytes, sampt_stream_t stream);
/* 3 x 3 stride-1 pad-1 split-fp16 convolution over pre-split planes (sampt_conv2d_nhwc dtype 4) that ALSO produces the statistics of
 * the InstanceNorm2d that follows it in the tracker's encoder (pips.py:191-287 BasicEncoder: every convolution is followed by
 * norm_fn = "instance"): mean_rstd [n][Cout][2] = (mean, 1 / sqrt(biased var + eps)) of y over H x W, summed from the convolution's
 * registers per 16 x 16 tile (fp32 over 64 pixels, fp64 beyond).  ws: n * ceil(H / 16) * ceil(W / 16) * Cout * 16 bytes, 8-byte aligned
 * (doubles); x_hl, w_hl, y (bias where given): 16-byte aligned — else SAMPT_ERR_ARG. */
int sampt_conv3x3_planes_instnorm_stats(const void* x_hl, const void* w_hl, const float* bias, float* y, int n, int H, int W, int Cin,
                                        int Cout, float eps, float* mean_rstd, void* ws, size_t ws_bytes, sampt_stream_t stream);
/* The mask decoder's image-side projection as an operator: C [M][N] = act(A W^T + bias) + res[row % res_mod (0: row)] with f32 A
 * [M][K] (K % 32 == 0) and W as split-fp16 planes [2][N][K] scaled by 2^8 (pack.split_f16x3) — 3-term fp16 MFMA products, fp32-grade
 * (reference: segment_anything/modeling/transformer.py:185-232 q / k / v / out projections over the image tokens).  shuf_g > 0: the
 * ConvTranspose2d(k = 2, s = 2) form (mask_decoder.py:53-61): N = 4 * cout columns ordered (dy, dx, channel), GEMM row f g^2 + y g + x
 * goes to pixel row f 4 g^2 + (2 y + dy) 2 g + 2 x + dx of C [.][cout]; bias has cout entries; res must be null.  act: 0 none, 1 ReLU,
 * 2 GELU (erf). */
int sampt_gemm_x3_rows(const float* A, const void* w_hl, const float* bias, const float* res, int res_mod, float* C, int M, int N,
                       int K, int act, int shuf_g, sampt_stream_t stream);
/* sampt_gemm_x3_rows with the NEXT operator of the mask decoder's output_upscaling (mask_decoder.py:53-61, 118-126) done on the rows
 * while they are in registers (weights-resident kernel only: M >= 16384, shuf_g > 0, act = 2, res null — anything else is refused):
 *   epi = 1 (K = 256, N = 4 x 64): LayerNorm2d over the 64 channels of every output pixel (epi_a / epi_b = weight / bias [64],
 *            epi_eps), then GELU: C as sampt_gemm_x3_rows;
 *   epi = 2 (K = 64, N = 4 x 32): GELU, then <pixel's 32 channels, epi_a[frame * epi_ld + 0 .. 31]> with frame = row / shuf_g^2:
 *            C [M * 4] holds one float per output pixel (the low-resolution mask logits of predict_masks);
 *   epi = 3 (K = 128, N = 256, shuf_g = 0, act = 0, res [M][256] non-null): C = LayerNorm(res + A W^T + bias) over the row, weights
 *            epi_a / epi_b [256] (transformer.py:145-150: keys = norm4(keys + attn_out)); C may be res (in place).
 * Bit for bit what sampt_gemm_x3_rows followed by sampt_layernorm (D = 64, act 2 / D = 256) / sampt_sam_mask_dot computes.
 * A, w_hl, C (bias, res where given): 16-byte aligned; epi_a / epi_b: floats, non-null where the tail reads them — else SAMPT_ERR_ARG. */
int sampt_gemm_x3_rows_epi(const float* A, const void* w_hl, const float* bias, const float* res, int res_mod, float* C, int M, int N,
                           int K, int act, int shuf_g, int epi, const float* epi_a, const float* epi_b, float epi_eps, int epi_ld,
                           sampt_stream_t stream);
/* low [frames][npix] = <up [frames][npix][C], hyper [frames][ld_hyper]> over C channels (MaskDecoder.predict_masks: hyper_in @ upscaled). */
int sampt_sam_mask_dot(const float* up, const float* hyper, int ld_hyper, float* low, int frames, int npix, int C, sampt_stream_t stream);
/* Process-wide A / B switch: 1 (default) = 1 x 1 split-fp16 "convolutions" over f32 activations with M >= 16384 rows and K = 64 /
 * 128 / 256 (the mask decoder's image-side projections and transposed convolutions) run on the weights-resident-in-LDS kernel of
 * csrc/gemm_x3_wres.hip; 0 = on the tiled kernel of rounds 2 - 5 (csrc/conv_f16x3.hip k_conv_f16x3); 2 = weights-resident, but the
 * decoder's LayerNorm2d + GELU and mask dot product stay kernels of their own.  Results are bitwise identical in all three. */
int sampt_gemm_set_wres(int on);
/* Process-wide knob of the PIPS window's MLP-Mixer (csrc/pips_mixer.hip).  fused = 1 (default): two launches per mixer block —
 * [sum of the previous channel MLP's slabs + residual -> token mixing] and [LayerNorm -> fc1 -> GELU -> fc2 over hidden slices];
 * fused = 0: the four-launch blocks of rounds 1 - 5 (token mixing, LayerNorm, two thin GEMMs); fused = 2: the two-launch blocks with
 * the channel MLP as 3-term split-fp16 MFMA products at fp32 grade (csrc/pips_mixer_x3.hip; needs the packed operand streams
 * "delta_block.to_delta.<i>.__x3s16" / "__x3s32" among the weights, else it falls back to fused = 1).  workgroups = how many
 * workgroups a channel-MLP launch should reach (it uses 8, 16 or 32 hidden slices per group of two point chains; default 32 =
 * the CUs the ViT encoder's persistent GEMMs leave free beside the tracker). */
int sampt_pips_set_mixer(int fused, int workgroups);
/* A HIP stream confined to the CUs [cu_lo, cu_hi) of EVERY XCD (hipExtStreamCreateWithCUMask; MI355X: 8 XCDs of 32 CUs, mask bit i
 * = CU i / 8 of XCD i % 8 — tools/probes/cu_mask_probe.hip, profiles/r6_c3_cu_mask_probe.log; an XCD left without any CU gets all of
 * them back, so every XCD keeps at least one).  The host orchestration uses two of them to split the chip in space between the ViT
 * encoder and the latency-bound side work (tracker window rounds, decoder chains): kernels of one never wait for CUs of the other.
 * priority: 0 normal, -1 high (the runtime's mask call has no priority argument: recorded for the caller, currently unused).
 * Destroy with sampt_stream_destroy after the stream is idle. */
int sampt_stream_create_cu_range(int cu_lo, int cu_hi, sampt_stream_t* out);
int sampt_stream_destroy(sampt_stream_t stream);
/* Calibration hook of the fp16 mode's static bias correction (sam_pt_amd/sam_predictor.py: the rounding of a weight matrix to
 * fp16 adds A.(W - fp16(W))^T to a GEMM's output; its token-mean part mean(A).(W - fp16(W))^T is a per-column constant that the
 * packer folds into the bias once per frame geometry).  While colmeans_dev is set, every block GEMM of sampt_vit_encode (fp16 mode,
 * plain entry point, one frame) also writes the column means of its A operand over the frame's real tokens to
 * colmeans_dev[(block * 4 + kind) * ld + k], kind = 0 qkv, 1 proj, 2 fc1, 3 fc2; ld >= mlp_ratio * embed_dim.  NULL ends it. */
int sampt_vit_calibrate(sampt_vit_t h, float* colmeans_dev, int ld);
/* Measurement hook: between begin and end every fp16 GEMM launch of sampt_vit_encode is bracketed by HIP events on the
 * launching stream; end waits for them and returns the summed algorithmic FLOP (2*M*N*K), the summed kernel time and the
 * number of launches — the in-situ figures behind bench.py's `roofline`. */
int sampt_vit_profile_begin(sampt_vit_t h);
int sampt_vit_profile_end(sampt_vit_t h, double* flop, double* ms, int* launches);
/* frames_dev: uint8, (B,3,H,W) if chw else (B,H,W,3), H,W <= img_size with the longest side == img_size already
 * (the reference pipelines resize before SamPt: configs/demo.yaml:20, configs/vos_eval_root.yaml:28).
 * features_dev: float32 [B][grid*grid][out_chans] — the (B,256,64,64) embedding in NHWC / token-major order.
 * interm_out_dev: NULL, or float32 [B][grid*grid][embed_dim] receiving the token stream after the first
 * global-attention block — HQ-SAM's interm_embeddings[0] (configs/model/sam/samhq_vit_*.yaml, MaskDecoderHQ). */
int sampt_vit_encode(sampt_vit_t h, const uint8_t* frames_dev, int chw, int B, int H, int W, float* features_dev,
                     float* interm_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* The same result (bit for bit) with the frame-independent part of the work done once per frame geometry.  Sam.preprocess
 * (sam.py: normalise, then zero-pad to img_size^2) leaves the token rows below a landscape frame — 28 of 64 rows for 16:9
 * video — without any pixel; until the first global-attention block such a token only ever meets tokens of its own
 * window, so whole window rows of them evolve identically in every frame.
 *   sampt_vit_live_rows: *live_rows = the token rows that can depend on the frame before the first global block
 *     (ceil(H/patch) completed to whole windows), == grid when nothing can be skipped (portrait / square frames, a
 *     global block first); *cache_bytes = size of the dead-row cache [(grid - live_rows) * grid][embed_dim] f32.
 *   sampt_vit_encode_live(build=1): fills dead_cache_dev from ONE frame of that geometry (frames_dev[0]; features_dev /
 *     interm_out_dev unused).  build=0: encodes B frames, running the blocks before the first global one on the live
 *     rows only and taking the other rows from dead_cache_dev.  Workspace: sampt_vit_encode_workspace_bytes. */
int sampt_vit_live_rows(sampt_vit_t h, int H, int W, int* live_rows, size_t* cache_bytes);
int sampt_vit_encode_live(sampt_vit_t h, const uint8_t* frames_dev, int chw, int B, int H, int W, float* features_dev,
                          float* interm_out_dev, float* dead_cache_dev, int build, void* workspace_dev,
                          size_t workspace_bytes, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 2a' — TinyViT image encoder = SamPredictor.set_image of MobileSAM and Light HQ-SAM (configs/model/sam/
 * sam_mobile_vit_tiny.yaml, samhq_light_vit_tiny.yaml: Sam.preprocess + TinyViT of ChaoningZhang/MobileSAM tiny_vit_sam.py).
 * Weight names: upstream's state-dict keys under `image_encoder.` after sam_pt_amd.pack.pack_tinyvit — every Conv2d_BN folded into
 * `<conv>.weight` ([Cout][KH][KW][Cin], the stem's Cin zero-padded to 4; depthwise: [3][3][C]) and `<conv>.bias`, `.weight_hl`
 * split-fp16 planes for the dense layers, `attn.attention_biases` [heads][ws^2], `attn.pad_qkv` [3 C] per block (the qkv of a
 * zero-padded window position), the neck as for seam 2a (`neck.0.weight_hl`, `neck.2.weight_khwc_hl`).  One arithmetic, fp32
 * grade.  embed_dims[i] / num_heads[i] must be 32 and window_sizes at most 14 for i >= 1; entry 0 of num_heads / window_sizes
 * belongs to the convolutional stage and is not used.  PatchMerging strides follow upstream's rule: 1 where the merged width is
 * 320, 448 or 576, else 2; the grid is img_size / 4 divided by those strides (img_size / 16 for every published model).
 * encode: frames, chw, B <= max_batch, H, W, features_dev, workspace as for sampt_vit_encode (here H, W <= img_size is all that is
 * asked); interm_out_dev: NULL, or float32 [B][grid*grid][embed_dims[2]] receiving the token map that enters layers.2 — Light
 * HQ-SAM's interm_embeddings[0].  No host synchronisation.
 * encode_stages (tests, measurement): additionally copies out the outputs of patch_embed and of layers 0..3, each after its
 * downsample (stages_dev[5], NULL entries skipped; NHWC), and, with stage_ms (HOST float[6]) non-NULL, times patch_embed, the four
 * layers and the neck with HIP events and synchronises with the stream before it returns. */
typedef struct sampt_tinyvit* sampt_tinyvit_t;
typedef struct sampt_tinyvit_config {
  int img_size, out_chans, mlp_ratio, mbconv_expand_ratio;
  int embed_dims[4], depths[4], num_heads[4], window_sizes[4];
  float pixel_mean[3], pixel_std[3];
} sampt_tinyvit_config;
int sampt_tinyvit_create(const sampt_tinyvit_config* cfg, const char* const* names, const void* const* ptrs, int n, int max_batch,
                         sampt_tinyvit_t* out);
void sampt_tinyvit_destroy(sampt_tinyvit_t h);
int sampt_tinyvit_encode_workspace_bytes(sampt_tinyvit_t h, int B, size_t* bytes);
int sampt_tinyvit_encode(sampt_tinyvit_t h, const uint8_t* frames_dev, int chw, int B, int H, int W, float* features_dev,
                         float* interm_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_tinyvit_encode_stages(sampt_tinyvit_t h, const uint8_t* frames_dev, int chw, int B, int H, int W, float* features_dev,
                                float* interm_out_dev, float* const stages_dev[5], float* stage_ms, void* workspace_dev,
                                size_t workspace_bytes, sampt_stream_t stream);
/* Kernel-level entry points (no handle; the kernels the engine launches, csrc/tinyvit.hip):
 *   preprocess: uint8 frames (B,3,H,W) [chw] or (B,H,W,3) -> float32 [B][img][img][4] = (x - mean[c]) / std[c] inside the picture,
 *     zeros outside it and in the 4th channel; mean / std: HOST float[3].
 *   dwconv3x3: depthwise 3 x 3, pad 1, stride 1 or 2 over NHWC float32, weights [3][3][C], bias [C], optional erf-GELU; C % 32 == 0.
 *   window_attention: qkv [B][H][W][96 heads] (per head q | k | v of 32), bias table [heads][ws^2] read at |dy| ws + |dx|, pad_qkv
 *     [96 heads] = the qkv of a zero-padded position (padded keys take part in every softmax) -> out [B][H][W][32 heads]; ws <= 14. */
int sampt_tinyvit_preprocess(const uint8_t* frames_dev, int chw, int B, int H, int W, int img_size, const float* mean, const float* std,
                             float* out_dev, sampt_stream_t stream);
int sampt_tinyvit_dwconv3x3_nhwc(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int n, int H, int W, int C,
                                 int stride, int gelu, sampt_stream_t stream);
int sampt_tinyvit_window_attention_f32(const float* qkv_dev, const float* table_dev, const float* pad_qkv_dev, float* out_dev, int B,
                                       int H, int W, int heads, int ws, sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * seam 2b — prompt encoder + mask decoder + postprocess = SamPredictor.predict_torch(multimask_output=False,
 * return_logits=True) as called at sam_pt.py:783-828.
 * --------------------------------------------------------------------------------------------------------- */
/* max_frames: capacity of the frame batch of sampt_sam_track_decode (the packed pixel-shuffle row maps
 * "mask_decoder.__up0_map" / "__up1_map" must cover it, see sam_pt_amd/pack.py).
 * vit_dim: 0 = SAM MaskDecoder (configs/model/sam/mask_decoder/sam.yaml); > 0 = HQ-SAM MaskDecoderHQ
 * (configs/model/sam/samhq_vit_huge.yaml:8-10, vit_dim = image encoder embed_dim), which needs the extra
 * "mask_decoder.{hf_token,hf_mlp,compress_vit_feat,embedding_encoder,embedding_maskfeature}" weights. */
int sampt_dec_create(const char* const* names, const void* const* ptrs, int n, int grid, int img_size, int max_frames,
                     int vit_dim, sampt_dec_t* out);
void sampt_dec_destroy(sampt_dec_t h);
/* Workspace for prompts of up to 120 points (every shipped SAM-PT config with <= 7 objects per batch); for larger
 * prompts (k <= SAMPT_DEC_MAX_POINTS: the reference accepts any k — 16 points x M objects fed to each other as
 * negatives, sam_pt.py:737-756, or the VIS adapter's 100-mask batches) size it with the _k variant. */
#define SAMPT_DEC_MAX_POINTS 4000
int sampt_dec_workspace_bytes(sampt_dec_t h, int frames, int out_h, int out_w, size_t* bytes);
int sampt_dec_workspace_bytes_k(sampt_dec_t h, int frames, int k, int out_h, int out_w, size_t* bytes);
/* HQ-SAM only: hq_features_dev [frames][16*grid*grid][32] = embedding_encoder(features) +
 * compress_vit_feat(interm) (MaskDecoderHQ.forward), computed once per frame from sampt_vit_encode's two outputs
 * and passed to every decode pass of that frame. */
int sampt_dec_hq_workspace_bytes(sampt_dec_t h, int frames, size_t* bytes);
int sampt_dec_hq_features(sampt_dec_t h, int frames, const float* features_dev, const float* interm_dev,
                          float* hq_features_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* One pass, one frame.  features_dev [grid*grid][256]; hq_features_dev: sampt_dec_hq_features output for the frame
 * (HQ-SAM handles) or NULL (SAM handles); pts_dev [k][2] (input-frame pixels), labels_dev int32 [k];
 * box_dev 4 floats or NULL; mask_in_dev [4*grid][4*grid] low-res logits or NULL.  Limit: k <= SAMPT_DEC_MAX_POINTS prompt
 * points (tokens-as-keys attention is tiled over the tokens; SAMPT_ERR_UNSUPPORTED beyond), workspace sized for k.  Outputs: logits_out_dev
 * [out_h][out_w], iou_out_dev [1], low_res_out_dev [4*grid][4*grid]. */
int sampt_sam_decode(sampt_dec_t h, const float* features_dev, const float* hq_features_dev, const float* pts_dev,
                     const int32_t* labels_dev, int k, const float* box_dev, const float* mask_in_dev, int in_h, int in_w, int out_h, int out_w,
                     float* logits_out_dev, float* iou_out_dev, float* low_res_out_dev, void* workspace_dev,
                     size_t workspace_bytes, sampt_stream_t stream);
/* The same pass with multimask_output=True (SAM decoder only): the 3 masks / IoU predictions of mask tokens 1..3, in
 * that order (MaskDecoder.forward mask_slice = slice(1, None)).  logits_out_dev [3][out_h][out_w], iou_out_dev [3],
 * low_res_out_dev [3][4*grid][4*grid].  Not on the SAM-PT path (sam_pt.py always passes False); part of the
 * SamPredictor.predict_torch surface. */
int sampt_sam_decode_multimask(sampt_dec_t h, const float* features_dev, const float* pts_dev, const int32_t* labels_dev,
                               int k, const float* box_dev, const float* mask_in_dev, int in_h, int in_w, int out_h,
                               int out_w, float* logits_out_dev, float* iou_out_dev, float* low_res_out_dev,
                               void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* n point prompts against ONE image in one batched launch sequence (the automatic mask generator's inner step).
 * features_dev [grid*grid][256] of that image (not n copies), hq_features_dev [16*grid*grid][32] (HQ-SAM handles) or NULL;
 * pts_dev [n][k][2] (input-frame pixels), labels_dev int32 [n][k], k >= 1; no box, no mask input.  n <= max_frames of the handle.
 * Outputs: low_res_out_dev [n][m][4*grid][4*grid], iou_out_dev [n][m]; nothing at full resolution (see the amg functions below).
 * m = 3 for a SAM handle with multimask != 0 (mask tokens 1..3 in that order, as the multimask entry point above), m = 1
 * otherwise.  HQ-SAM with multimask != 0 follows MaskDecoderHQ.forward with hq_token_only=False: of mask tokens 1..3 the one with
 * the largest predicted IoU is chosen ON THE DEVICE, the output is its SAM mask + the HQ mask and that IoU.  Image-side work
 * that does not depend on the prompt (features + no_mask_embed, the layer-0 K | V | Q' projection) runs once per call. */
int sampt_sam_decode_points_workspace_bytes(sampt_dec_t h, int n, int k, size_t* bytes);
int sampt_sam_decode_points(sampt_dec_t h, int n, const float* features_dev, const float* hq_features_dev, const float* pts_dev,
                            const int32_t* labels_dev, int k, int multimask, float* low_res_out_dev, float* iou_out_dev,
                            void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* Scoring tail of the automatic mask generator on low-res masks low_res_dev [n_masks][L][L].  With v = Sam.postprocess_masks of a
 * mask, evaluated on the fly with the arithmetic of the postprocess entry point below (no logits are written):
 * score: out8_dev int32 [n_masks][8] = { #(v > thr + offset), #(v > thr - offset), #(v > thr), x0, y0, x1, y1, 0 } with the
 *   inclusive XYXY box of v > thr (zeros for an empty mask); thresholds are formed in double and rounded to float once, as a
 *   float tensor compared with a Python scalar.  Integer partial sums + a final reducer: bitwise reproducible.
 * binarize: out_dev bytes [n_rows][out_h][out_w] = (v(low_res[rows_dev[r]]) > thr) as 0 / 1, any out_h x out_w. */
size_t sampt_amg_score_workspace_bytes(int n_masks);
int sampt_amg_score(const float* low_res_dev, int n_masks, int L, int img_size, int in_h, int in_w, int out_h, int out_w,
                    double mask_threshold, double offset, int32_t* out8_dev, void* workspace_dev, size_t workspace_bytes,
                    sampt_stream_t stream);
int sampt_amg_binarize(const float* low_res_dev, int n_masks, const int32_t* rows_dev, int n_rows, int L, int img_size, int in_h,
                       int in_w, int out_h, int out_w, double mask_threshold, uint8_t* out_dev, sampt_stream_t stream);
/* Tail of the automatic mask generator on the device; both equal the host functions of sam_pt_amd/automatic_mask_generator.py
 * exactly (integer / threshold logic, no tolerance).
 * regions: remove_small_regions(m, min_area, "holes") then (., min_area, "islands") of masks_in_dev bytes [n][h][w] (0 / non-0):
 *   8-connected components; a component is small when it has fewer than min_area pixels; small background components are
 *   filled, then small foreground components are removed — the largest survives when all are small, among equals the one
 *   whose first pixel comes first in raster order.  masks_out_dev bytes [n][h][w] (0 / 1; may alias masks_in_dev),
 *   changed_out_dev bytes [n] (either pass found a small component), area_out_dev int32 [n], boxes_out_dev int32 [n][4]
 *   inclusive XYXY (zeros for an empty mask).  Labels are the smallest linear pixel index of a component and all sums are
 *   integer: bitwise reproducible.  h * w < 2^31.  The workspace (16-byte aligned) holds 8 bytes per pixel + 1040 bytes per
 *   mask in flight; with less than n masks' worth the stack is processed in chunks, with less than one mask's the call fails.
 * nms: boxes_dev f32 [n][4] XYXY (16-byte aligned), scores_dev f32 [n], n <= 65535.  Sweep in stable decreasing score order;
 *   a box is dropped when inter / ((area_i + area_j) - inter) > iou_thr with an already kept box, every operation rounded
 *   to f32 separately (0 / 0 = nan never suppresses).  keep_out_dev int64 [n]: the kept input indices in sweep order, the
 *   first *count_out_dev (int32 [1]) entries are valid. */
size_t sampt_amg_regions_workspace_bytes(int n_masks, int h, int w);
int sampt_amg_regions(const uint8_t* masks_in_dev, int n, int h, int w, int min_area, uint8_t* masks_out_dev,
                      uint8_t* changed_out_dev, int32_t* area_out_dev, int32_t* boxes_out_dev, void* workspace_dev,
                      size_t workspace_bytes, sampt_stream_t stream);
size_t sampt_amg_nms_workspace_bytes(int n);
int sampt_amg_nms(const float* boxes_dev, const float* scores_dev, int n, float iou_thr, int64_t* keep_out_dev,
                  int32_t* count_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* COCO run-length encoding of a contiguous stack x_dev [n][h][w] on the device, h * w < 2^31: bytes (non-zero = set; is_f32 = 0)
 * or f32 values with a threshold (is_f32 = 1: set iff x > thr; NaN and x == thr are clear).  Runs go over the column-major
 * flattening p = x * h + y and the first run counts zeros (a mask whose first pixel is set starts with a 0 count): exactly
 * mask_to_rle of sam_pt_amd/automatic_mask_generator.py.  All integer, no atomics: bitwise repeatable.  Between the phases the
 * host reads one total.
 * count: offsets_out_dev int64 [n + 1] = the number of runs of the masks before m ([n] = the stack's total, the length of the
 *   counts array), area_out_dev int32 [n] = set pixels (the sum of the odd runs).  The pixels are read once, here; rows that are
 *   4-byte (f32: 16-byte) aligned (w % 4 == 0 and an aligned x_dev) are read with one vector load per 4 pixels, others element by
 *   element with the same result.  The workspace (16-byte aligned, sampt_rle_workspace_bytes(n, h, w) = 16 bytes per 64 pixels of
 *   a column + 16 per mask; 0 for a bad shape) keeps the transition words for emit; with less the call fails with
 *   SAMPT_ERR_WORKSPACE and the caller splits the stack by masks.
 * emit: the same n, h, w, workspace and the offsets of count -> counts_out_dev uint32 [offsets[n]], mask m at [offsets[m], offsets[m + 1]).
 * string_sizes / string_emit: the COCO string of every mask's counts (maskApi rleToString: c[i] - c[i - 2] for i > 2, 5 bits at a
 *   time from the low end with an arithmetic shift, bit 5 = more to come, chr(chunk + 48)), concatenated.  sizes writes
 *   str_offsets_dev [n] (int64 [n + 1]) = the total bytes; emit writes chars_out_dev uint8 [that total] and str_offsets_dev [0 .. n).
 *   total_counts = offsets[n]; workspace (8-byte aligned) of sampt_rle_string_workspace_bytes(total_counts), the same for both. */
size_t sampt_rle_workspace_bytes(int n, int h, int w);
int sampt_rle_count(const void* x_dev, int is_f32, float thr, int n, int h, int w, int64_t* offsets_out_dev, int32_t* area_out_dev,
                    void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_rle_emit(int n, int h, int w, const int64_t* offsets_dev, uint32_t* counts_out_dev, const void* workspace_dev,
                   size_t workspace_bytes, sampt_stream_t stream);
size_t sampt_rle_string_workspace_bytes(int64_t total_counts);
int sampt_rle_string_sizes(const uint32_t* counts_dev, const int64_t* offsets_dev, int n, int64_t total_counts,
                           int64_t* str_offsets_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_rle_string_emit(const uint32_t* counts_dev, const int64_t* offsets_dev, int n, int64_t total_counts,
                          int64_t* str_offsets_dev, uint8_t* chars_out_dev, const void* workspace_dev, size_t workspace_bytes,
                          sampt_stream_t stream);
/* DAVIS J and F on the device: six integer counts per item i of n, an item being a pair of binary images (h, w) — seg (the
 * prediction) and ann (the ground truth):
 *   counts_out_dev int32 [n][6] = inter |seg & ann|, union |seg | ann|, n_seg |B(seg)|, n_ann |B(ann)|,
 *                                 seg_match |B(seg) & dil(B(ann))|, ann_match |B(ann) & dil(B(seg))|
 * B = the boundary map of sam_pt_amd/vos_metrics.py seg2bmap, dil = binary dilation with the disk dy^2 + dx^2 <= radius^2
 * (0 <= radius <= 64; the host derives it from bound_th), everything outside the image 0.  h * w < 2^31.
 * An image is a plane of a contiguous stack [.][h][w]: kind 0 = bytes (set iff non-zero), kind 1 = f32 (set iff x > thr; NaN
 * and x == thr are clear), kind 2 = a uint8 index map (set iff x == values_dev[i], int32 [n], required for this kind only).
 * planes_dev int32 [n] names the plane of every item, so that several items share one plane (the objects of one frame of an index
 * map); NULL: item i reads plane i.  The plane numbers are not checked on the device: the caller validates them.
 * void_dev: optional bytes [.][h][w] with their own optional plane numbers; non-zero pixels are cleared from seg and ann first.
 * Every pixel is read once, 4 pixels per load from any pixel address (rows of a width that is no multiple of 4 are not aligned;
 * images narrower than 4 are read element by element, with the same result); the workspace (16-byte aligned, sampt_jf_workspace_bytes = 2 bits per pixel rounded up to 64 rows; 0 for
 * a bad shape or radius) holds the two boundary bit-planes, the dilated maps are never written.  Integer sums: bitwise repeatable.
 * With too small a workspace the call fails with SAMPT_ERR_WORKSPACE and the caller splits the stack by items. */
size_t sampt_jf_workspace_bytes(int n, int h, int w, int radius);
int sampt_jf_counts(const void* seg_dev, int seg_kind, float seg_thr, const int32_t* seg_values_dev, const int32_t* seg_planes_dev,
                    const void* ann_dev, int ann_kind, float ann_thr, const int32_t* ann_values_dev, const int32_t* ann_planes_dev,
                    const uint8_t* void_dev, const int32_t* void_planes_dev, int n, int h, int w, int radius,
                    int32_t* counts_out_dev, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* The J / F counts of every (seg mask p, ann mask k) pair of every frame (csrc/vos_pairs.hip): what the DAVIS unsupervised protocol needs
 * before its assignment.  Every mask is read once and its boundary dilated once, whatever the number of its partners; the pair pass is
 * a popcount GEMM over bit words.  The two sources are described as for sampt_jf_counts (kind, threshold, values_dev, planes_dev, now
 * int32 [n_frames * n_seg] and [n_frames * n_ann]); seg mask (p, t) is item t * n_seg + p, ann mask (k, t) item t * n_ann + k.
 * void_dev: optional bytes, one plane per frame (void_planes_dev int32 [n_frames] or NULL: frame t reads plane t), cleared from both
 * sides.  Boundary map, disk, 0 <= radius <= 64 and "outside the image is 0" are those of sampt_jf_counts.  Outputs, int32:
 *   pair_out_dev [n_frames][n_seg][n_ann][3] = inter, seg_match = |B(seg) & dil(B(ann))|, ann_match = |B(ann) & dil(B(seg))|;
 *   seg_stat_out_dev [n_frames][n_seg][2] and ann_stat_out_dev [n_frames][n_ann][2] = area, |B|  (union = area + area - inter).
 * The workspace (16-byte aligned, sampt_jf_pairs_workspace_bytes = 3 bits per pixel of every mask, rounded up to 64 rows; 0 for a bad
 * shape or radius) holds the mask, boundary and dilated-boundary bit-planes.  Integer sums: bitwise repeatable.  With too small a
 * workspace the call fails with SAMPT_ERR_WORKSPACE and the caller splits by frames.  3 * n_seg * n_ann * n_frames < 2^31. */
size_t sampt_jf_pairs_workspace_bytes(int n_seg, int n_ann, int n_frames, int h, int w, int radius);
int sampt_jf_pairs_counts(const void* seg_dev, int seg_kind, float seg_thr, const int32_t* seg_values_dev, const int32_t* seg_planes_dev,
                          int n_seg, const void* ann_dev, int ann_kind, float ann_thr, const int32_t* ann_values_dev,
                          const int32_t* ann_planes_dev, int n_ann, const uint8_t* void_dev, const int32_t* void_planes_dev, int n_frames,
                          int h, int w, int radius, int32_t* pair_out_dev, int32_t* seg_stat_out_dev, int32_t* ann_stat_out_dev,
                          void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* YouTube-VIS AP / AR on the device (csrc/vis_eval.hip): bit-planes of mask stacks, spatio-temporal intersection / union of all
 * (detection, ground truth) pairs of a video, and the greedy matching of the reference's YTVOSeval.evaluateVid.  Integer work and
 * one IEEE float64 division per IoU: bitwise repeatable and equal to the host restatement of sam_pt_amd/vis_metrics.py.
 * Bit-plane format: a stack [n][h][w] is uint64 [n][ceil(h / 64)][w]; bit j of word (band b, column x) is pixel (64 b + j, x), and the
 *   bits of rows >= h are 0 (every popcount below relies on it).  h * w < 2^31.
 * bits_pack: x_dev is a contiguous stack [.][h][w] of kind 0 = bytes (set iff non-zero), kind 1 = f32 (set iff x > thr; NaN and
 *   x == thr are clear) or kind 2 = a uint8 index map (set iff x == values_dev[i], int32 [n], this kind only).  planes_dev int32 [n]
 *   names the plane of every item (NULL: item i reads plane i; not checked on the device).  bits_out_dev (16-byte aligned) receives the
 *   n bit-planes, area_out_dev int32 [n] the set pixels.  Every pixel is read once, 4 pixels per load from any pixel address (images
 *   narrower than 4: element by element, with the same result).  n = 0 is a no-op.
 * rle_decode_bits: the inverse of sampt_rle_count / sampt_rle_emit.  counts_dev uint32 [total_counts] and offsets_dev int64 [n + 1]
 *   hold column-major runs, the first run of a mask counting zeros; zero-length runs are legal.  status_out_dev int32 [n]: 0 = decoded;
 *   1 = the runs do not sum to h * w; 2 = the mask's offsets are not ordered inside [0, total_counts].  A mask with a non-zero status
 *   gets an all-zero plane and area 0, and nothing is read or written out of bounds for it.  The workspace (8-byte aligned,
 *   sampt_rle_decode_workspace_bytes(total_counts) = 8 bytes per run + 16) holds the prefix sums of the runs.
 * bits_unpack: n bit-planes -> bytes_out_dev [n][h][w] (0 / 1).
 * seq_iou_counts: dt_planes_dev int32 [n_dt][n_frames] and gt_planes_dev int32 [n_gt][n_frames] name the bit-plane (of dt_bits_dev /
 *   gt_bits_dev, with their areas int32 per plane) of every item on every frame; -1 (or a number >= the plane count given) means "no
 *   mask on this frame"; several entries may name one plane.  counts_out_dev int64 [n_dt][n_gt][2] = inter = sum_t popc(d_t & g_t) and
 *   union = sum_t (|d_t| + |g_t|) - inter, an absent frame contributing nothing of its own: an absent and an empty mask behave alike,
 *   as in the reference's iou_seq.  The workspace (8-byte aligned, sampt_seq_iou_workspace_bytes; 0 for a bad shape) holds partial
 *   sums that are added in a fixed order: no atomics.
 * vis_match: one (video, category) group.  counts_dev as above with the detections in score order, cut to the last maxDets.  Per area
 *   range a of n_ranges: gt_order_dev int32 [n_ranges][n_gt] (the stable sort of the ground truths by their ignore flag),
 *   gt_ignore_dev bytes [n_ranges][n_gt] in that order, dt_out_dev bytes [n_ranges][n_dt] (the detection's average area is outside the
 *   range); iscrowd_dev bytes [n_gt] in the original order; thrs_dev float64 [n_thr], n_thr <= 64; n_gt <= 960.  IoU = (double) inter /
 *   (double) union, 0 for an empty union.  Outputs per (range, threshold): dt_match_out_dev int32 [n_ranges][n_thr][n_dt] = 1 + the
 *   matched ground truth's original index, or 0; gt_match_out_dev int32 [n_ranges][n_thr][n_gt] = 1 + the matching detection's
 *   position, or 0, in the range's order; dt_ignore_out_dev bytes [n_ranges][n_thr][n_dt]. */
int sampt_bits_pack(const void* x_dev, int kind, float thr, const int32_t* values_dev, const int32_t* planes_dev, int n, int h, int w,
                    uint64_t* bits_out_dev, int32_t* area_out_dev, sampt_stream_t stream);
size_t sampt_rle_decode_workspace_bytes(int64_t total_counts);
int sampt_rle_decode_bits(const uint32_t* counts_dev, const int64_t* offsets_dev, int n, int64_t total_counts, int h, int w,
                          uint64_t* bits_out_dev, int32_t* area_out_dev, int32_t* status_out_dev, void* workspace_dev,
                          size_t workspace_bytes, sampt_stream_t stream);
int sampt_bits_unpack(const uint64_t* bits_dev, int n, int h, int w, uint8_t* bytes_out_dev, sampt_stream_t stream);
/* Rank -> pixel on bit-planes (csrc/mask_points.hip): "the r-th set pixel of this mask, in nonzero() order", so that a host that knows
 * only a mask's area can draw ranks and the pixels stay on the device (query-point selection, sam_pt_amd/query_points.py).  Integer
 * work only, no atomics, stream-ordered; equal to the host restatement of sam_pt_amd/mask_points.py.
 * bits_row_prefix: bits_dev holds n planes in the format of sampt_bits_pack (8-byte aligned).  prefix_out_dev int32 [n][h + 1]:
 *   prefix[i][y] = the set pixels of plane i in rows < y, so prefix[i][0] = 0 and prefix[i][h] = the plane's area.  The complement's
 *   prefix is not stored: it is y * w - prefix[i][y].  n = 0 is a no-op.
 * bits_select: prefix_dev as written by bits_row_prefix for the same planes.  queries_dev int32 [nq][3] = (plane, invert, rank);
 *   yx_out_dev f32 [nq][2] receives ((float) y, (float) x) of the rank-th pixel, 0-based, in row-major order - mask.nonzero()[rank] -
 *   counting set pixels, or with invert != 0 the clear pixels inside the image (rows >= h and columns >= w never count).  A query whose
 *   plane is outside [0, n) or whose rank is outside [0, area) (inverted: [0, h * w - area)) gives (-1, -1) and reads nothing out of
 *   bounds.  Queries are independent: any order, any mix of planes and polarities in one launch.  nq = 0 and n = 0 are no-ops. */
int sampt_bits_row_prefix(const uint64_t* bits_dev, int n, int h, int w, int32_t* prefix_out_dev, sampt_stream_t stream);
int sampt_bits_select(const uint64_t* bits_dev, const int32_t* prefix_dev, int n, int h, int w, const int32_t* queries_dev, int nq,
                      float* yx_out_dev, sampt_stream_t stream);
size_t sampt_seq_iou_workspace_bytes(int n_dt, int n_gt, int n_frames, int h, int w);
int sampt_seq_iou_counts(const uint64_t* dt_bits_dev, const int32_t* dt_area_dev, const int32_t* dt_planes_dev, int n_dt, int dt_n_planes,
                         const uint64_t* gt_bits_dev, const int32_t* gt_area_dev, const int32_t* gt_planes_dev, int n_gt, int gt_n_planes,
                         int n_frames, int h, int w, int64_t* counts_out_dev, void* workspace_dev, size_t workspace_bytes,
                         sampt_stream_t stream);
int sampt_vis_match(const int64_t* counts_dev, int n_dt, int n_gt, int n_ranges, int n_thr, const double* thrs_dev,
                    const int32_t* gt_order_dev, const uint8_t* gt_ignore_dev, const uint8_t* iscrowd_dev, const uint8_t* dt_out_dev,
                    int32_t* dt_match_out_dev, int32_t* gt_match_out_dev, uint8_t* dt_ignore_out_dev, sampt_stream_t stream);
/* Prediction overlays on the device (csrc/viz.hip; the definitions are those of sam_pt_amd/visualize.py, whose host restatement
 * the results equal byte for byte).  No scratch memory, no atomics, integer work only: bitwise repeatable, stream-ordered.
 * viz_band: bits_dev holds n bit-planes in the format of sampt_bits_pack (8-byte aligned); band_out_dev receives, in the same layout,
 *   dil(m) & dil(~m): dil = binary dilation with the disk dy^2 + dx^2 <= radius^2 (0 <= radius <= 64), ~m the complement inside the
 *   image only, everything outside the image 0 for both, the bits of rows >= h 0.  An empty mask, a full mask and radius 0 give zeros.
 * viz_compose: frames_dev uint8 [n_frames][3][h][w], or [n_frames][h][w][3] with interleaved != 0; out_dev uint8 interleaved
 *   [n_frames][h][w][3] for panel 1 (input: the frame and the markers) and panel 2 (predictions: the frame, then every mask's tint and
 *   band, then the markers), [n_frames][2 h][w][3] for panel 3 (input above predictions, one pass).  bits_dev / band_dev: mask m of frame
 *   t is plane m * n_frames + t (required when n_masks > 0 and the panel has predictions).  lut_dev uint8 [62][256], 4-byte aligned: a
 *   pixel of mask m goes, channel by channel, through table (min(m, 9) * 3 + channel) * 2 + band if its mask bit is set and through table
 *   60 + band if not, mask after mask; the host builds the tables.  markers_dev int32 [n_frames][n_markers][8] = centre x, centre y, kind
 *   (0 = ring, 1 = cross), size (ring radius R / cross arm L), line width, reach (every covered pixel is within reach of the centre in
 *   both axes), colour on the predictions panel, colour on the input panel (r | g << 8 | b << 16).  Markers are drawn in table order,
 *   the last one that covers a pixel wins; centres may lie off the frame.  Pixels are read 4 per load from any byte address (widths
 *   under 4: element by element, with the same result); out_dev 4-byte aligned and w % 4 == 0 gets 12-byte stores. */
int sampt_viz_band(const uint64_t* bits_dev, int n, int h, int w, int radius, uint64_t* band_out_dev, sampt_stream_t stream);
int sampt_viz_compose(const uint8_t* frames_dev, int interleaved, int n_frames, int h, int w, const uint64_t* bits_dev,
                      const uint64_t* band_dev, int n_masks, const uint8_t* lut_dev, const int32_t* markers_dev, int n_markers, int panel,
                      uint8_t* out_dev, sampt_stream_t stream);
/* Patch-similarity filter of SamPt._track_points (csrc/patch_filter.hip; the definitions are those of sam_pt_amd/sam_pt.py:
 * rgb2lab and SamPt._patch_similarity_filter, reference sam_pt.py:597-690).  One launch, no scratch memory, stream-ordered, bitwise
 * repeatable.  rgb_dev uint8 [T][3][H][W]; query_dev f32 [N][3] = (t, x, y); traj_dev f32 [T][N][2]; vis_in_dev f32 [T][N];
 * companding_dev float64 [256]: the sRGB companding of byte / 255 as the host's rgb2lab computes it (sam_pt_amd/patch_filter.py
 * builds it); vis_out_dev f32 [T][N], a buffer of its own; sim_out_dev f32 [T][N] or null.
 * Per item: the CIELAB patch (taps -(ps/2) .. ps/2 on both axes, i.e. ps + 1 per side for an even ps; bilinear, corners outside the
 * frame 0) around the trajectory point against the patch around the query point on the query frame,
 * sim = exp(-||difference||_2 / (2 ps^2)); vis == 1 and not sim > threshold -> -3.  Per point: everything after the first -3 after
 * the query frame and everything before the first -3 before it -> -4.  border_rule != 0: then x / W < 0.01, y / H < 0.01,
 * x / W > 0.99 or y / H > 0.99 (f32, IEEE division) -> -2.  With sim_out_dev the similarity of EVERY item is written; without it the
 * items with vis != 1 are not sampled.  An item with a non-finite coordinate, and every item of a point whose query is non-finite or
 * names a frame outside 0 .. T - 1, is non-similar (similarity 0).
 * SAMPT_ERR_ARG: a null pointer other than sim_out_dev; T, N, H or W <= 0; patch_size outside 1 .. 15. */
#define SAMPT_PATCH_FILTER_MAX_PATCH_SIZE 15
int sampt_patch_filter(const uint8_t* rgb_dev, int T, int H, int W, const float* query_dev, const float* traj_dev,
                       const float* vis_in_dev, int N, int patch_size, float threshold, const double* companding_dev, int border_rule,
                       float* vis_out_dev, float* sim_out_dev, sampt_stream_t stream);
/* Prompt assembly of SamPt on the device (csrc/prompt_assembly.hip; the specification is assemble_prompts_host of
 * sam_pt_amd/prompt_assembly.py, i.e. SamPt._prepare_points followed by ResizeLongestSide.apply_coords, reference sam_pt.py:726-758).
 * No handle, no scratch memory, no atomics, stream-ordered, bitwise repeatable; inputs are finite.
 * traj_dev f32 [T][M][P][2]; vis_dev f32 [T][M][P] visibility codes: a point is visible iff its code == 1.0f (0, -1 .. -4 are not).
 * pp = positive_points_per_mask; negatives != 0 <=> negative_points_per_mask > 0; add_others != 0 <=> other objects' positives are
 * appended.  Item i = t * M + m.  Its prompt: the object's own visible points in index order — label 1 for index < pp, label 0 for
 * index >= pp when `negatives`, label 1 throughout otherwise —, then, when M > 1 and `add_others`, the visible points among the first
 * min(pp, P) of every other object, object-major, label 0.  A coordinate is (float)((double)x * sx) resp. (float)((double)y * sy).
 * k = prompt length, npos = number of label-1 entries.
 * sampt_prompt_count: k_all_dev / npos_all_dev int32 [T * M] of every item (the caller downloads them and decides which items run,
 *   with how many point slots, in which chunks).
 * sampt_prompt_fill: the n_items items named by items_dev (int32, any subset in any order; a number outside 0 .. T * M - 1 yields an
 *   empty prompt) -> pts_dev f32 [n_items][ld][2], labels_dev int32 [n_items][ld], both zero from an item's k on; k_item_dev /
 *   npos_item_dev int32 [n_items].  ld must be at least the largest k of the chunk (entries from slot ld on are dropped, k_item keeps
 *   the full length).  The outputs are the layout of sampt_sam_track_decode's pts_dev / labels_dev / k_item_dev / npos_item_dev.
 * sampt_mark_outside_frame: the four border comparisons of SamPt._track_points (sam_pt.py:684-690) over n points: traj_dev f32
 *   [n][2], vis_out_dev[i] = -2 where x / W < 0.01, y / H < 0.01, x / W > 0.99 or y / H > 0.99 (f32, IEEE division), else
 *   vis_in_dev[i]; vis_out_dev may be vis_in_dev.
 * SAMPT_ERR_ARG: a null pointer; T, M, P, n_items, ld, n, H or W <= 0; pp < 0; T * M * P * 2 or n_items * ld * 2 above 2^31 - 1. */
int sampt_prompt_count(const float* vis_dev, int T, int M, int P, int pp, int negatives, int add_others, int32_t* k_all_dev,
                       int32_t* npos_all_dev, sampt_stream_t stream);
int sampt_prompt_fill(const float* traj_dev, const float* vis_dev, int T, int M, int P, int pp, int negatives, int add_others, double sx,
                      double sy, const int32_t* items_dev, int n_items, int ld, float* pts_dev, int32_t* labels_dev, int32_t* k_item_dev,
                      int32_t* npos_item_dev, sampt_stream_t stream);
int sampt_mark_outside_frame(const float* traj_dev, const float* vis_in_dev, long n, int H, int W, float* vis_out_dev,
                             sampt_stream_t stream);
/* Whole SamPt.predict_mask chain (sam_pt.py:760-837) for `frames` independent (frame, object) items that share the
 * visible-point count k, batched into one launch sequence and without host synchronisation:
 * [positives-only pass over the first n_pos_first points when n_pos_first >= 0, i.e. negative_points_per_mask > 0;
 * pass -1 for the single-pass case] -> all-points pass -> `refine_iters` box+mask refinement passes
 * (bbox of logits>0 and the `sum < 2 -> stop` rule evaluated per item on device) -> logits = -inf if iou < iou_thr.
 * Ragged batches: k_item_dev / npos_item_dev (int32 [frames], or NULL for uniform) give each item's own point count
 * (<= k) and leading-positive count (<= n_pos_first); an item's prompt tokens are packed in front of its token matrix
 * and the padding rows are masked out of every attention, so each item's result equals its un-batched one.
 * features_dev [frames][grid*grid][256]; hq_features_dev [frames][16*grid*grid][32] (HQ-SAM) or NULL;
 * pts_dev [frames][ld_pts][2]; labels_dev int32 [frames][ld_pts];
 * final_logits_dev [frames][out_h][out_w]; score_out_dev [frames] = predicted IoU. */
int sampt_sam_track_decode(sampt_dec_t h, int frames, const float* features_dev, const float* hq_features_dev,
                           const float* pts_dev, const int32_t* labels_dev, int k, const int32_t* k_item_dev,
                           const int32_t* npos_item_dev, int ld_pts, int n_pos_first, int refine_iters, float iou_thr,
                           int in_h, int in_w, int out_h, int out_w, float* final_logits_dev, float* score_out_dev,
                           void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* The same chain replayed from a hipGraph.  The launch sequence of sampt_sam_track_decode depends only on its arguments, so
 * it is stream-captured once per distinct argument tuple — every scalar AND every pointer: the caller keeps the inputs,
 * outputs and workspace of a prompt bucket in persistent buffers (sam_pt_amd.SamPredictor.track_decode(graph=True)) — and
 * replayed with one hipGraphLaunch afterwards.  First call of a tuple: plain launches; second: capture + instantiate +
 * launch; then: launch only.  At most 64 instantiated graphs are cached per handle (least recently used one dropped).
 * `stream` must not be the NULL stream (not capturable: falls back to plain launches).  Results are those of
 * sampt_sam_track_decode bit for bit (same kernels, same order).  sampt_dec_graph_stats: cache size / captures / replays. */
int sampt_sam_track_decode_graph(sampt_dec_t h, int frames, const float* features_dev, const float* hq_features_dev,
                                 const float* pts_dev, const int32_t* labels_dev, int k, const int32_t* k_item_dev,
                                 const int32_t* npos_item_dev, int ld_pts, int n_pos_first, int refine_iters, float iou_thr,
                                 int in_h, int in_w, int out_h, int out_w, float* final_logits_dev, float* score_out_dev,
                                 void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
int sampt_dec_graph_stats(sampt_dec_t h, long* cached, long* captures, long* launches);
/* Batch-invariant decoding (on = 1; a new handle has it off).  Off, the decoder's latency-bound f32 products choose their kernel by
 * total row count and the token -> image attention splits its keys by the number of workgroups, so an item's logits depend — in the
 * last bits — on how many items share its call.  On, every item of sampt_sam_decode / _decode_multimask / _decode_points /
 * _track_decode / _track_decode_graph gets the bits it gets alone: the plain f32 products take the row-invariant route
 * (sampt_gemm_f32_route, invariant = 1), the attention's key split is that of sampt_attn_t2i_plan(invariant = 1), and the image
 * side is told from the token side by the rows of one item.  The workspace sizes the handle reports hold in either mode; captured
 * graphs are keyed by the mode.  The results of the two modes differ from each other by rounding (a few 1e-7 relative). */
int sampt_dec_set_batch_invariant(sampt_dec_t h, int on);
int sampt_postprocess_masks(const float* low_res_dev, int L, int img_size, int in_h, int in_w, float* out_dev, int out_h,
                            int out_w, sampt_stream_t stream);
/* bbox_state_dev: int32[5] = {xmin, ymin, xmax, ymax, count} over logits > 0 (sam_pt.py:809-820). */
size_t sampt_bbox_workspace_bytes(int h, int w);
int sampt_bbox_from_logits(const float* logits_dev, int h, int w, int32_t* bbox_state_dev, void* workspace_dev,
                           size_t workspace_bytes, sampt_stream_t stream);

/* One axis of PIL's 8-bit separable resampler (Image.resize, the arithmetic behind ResizeLongestSide.apply_image =
 * torchvision resize(to_pil_image(.)) in SamPredictor.set_image, App. A-1): src_dev [outer][in_len][inner] uint8 ->
 * dst_dev [outer][out_len][inner], dst = clip8((2^21 + sum_x src[xmin+x]*coef[xx][x]) >> 22).  coef_dev int32
 * [out_len][ksize] / bounds_dev int32 [out_len][2] = PIL's precompute_coeffs + normalize_coeffs_8bpc tables, built by the
 * host (sam_pt_amd/sam_predictor.py); horizontal pass first, then vertical, each rounded to uint8 as PIL does. */
int sampt_pil_resample_u8(const uint8_t* src_dev, uint8_t* dst_dev, long outer, int in_len, int out_len, int inner,
                          const int32_t* coef_dev, const int32_t* bounds_dev, int ksize, sampt_stream_t stream);

/* VOS post-processing.  sampt_resize_logits: F.interpolate(logits, target_hw, bilinear, align_corners=False) of
 * sam_pt.py:205-206 for n single-channel maps.  sampt_index_masks: uint8 object index per pixel = argmax over
 * {background logit 0, logits_dev[M][npix]}, i.e. the bg-stack + softmax + argmax of vos_eval/eval.py:304, 326, 355. */
int sampt_resize_logits(const float* src_dev, int n, int sh, int sw, float* dst_dev, int dh, int dw, sampt_stream_t stream);
int sampt_index_masks(const float* logits_dev, int M, long npix, uint8_t* out_dev, sampt_stream_t stream);
/* The same for logits_dev [M][T][hw] with the evaluator's overrides (vos_eval/eval.py:318-326): object m is -1e8 on
 * frames before query_t_dev[m] (int32 [M]) and, when gt_masks_dev (uint8 [M][hw], already at this resolution) is given,
 * +-1e8 from its ground-truth mask on the query frame.  out_dev uint8 [T][hw]. */
int sampt_vos_index_masks(const float* logits_dev, int M, int T, long hw, const int32_t* query_t_dev,
                          const uint8_t* gt_masks_dev, uint8_t* out_dev, sampt_stream_t stream);
/* ... and for frames processed at (h, w) but wanted at (out_h, out_w) (eval.py:326, 340-356: softmax, bilinear resize of
 * the probabilities with align_corners=False, argmax).  logits_dev [M][T][h][w], gt_masks_dev [M][h][w] or NULL,
 * out_dev uint8 [T][out_h][out_w]; M <= 32. */
int sampt_vos_index_masks_resized(const float* logits_dev, int M, int T, int h, int w, const int32_t* query_t_dev,
                                  const uint8_t* gt_masks_dev, int out_h, int out_w, uint8_t* out_dev,
                                  sampt_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Kernel-level entry points (used by the parity tests and the roofline bench; same kernels the engines launch).
 * --------------------------------------------------------------------------------------------------------- */
/* C[M][N] = act(alpha * A[M][K] . W[N][K]^T + bias) (+ res).  dtype: 0 = f32 (exact f32 MFMA), 1 = f16 in / f32 out,
 * 2 = f16 in / f16 out.  act: 0 none, 1 relu, 2 gelu(erf). */
int sampt_gemm(int dtype, const void* A_dev, const void* W_dev, const float* bias_dev, const float* res_dev,
               void* C_dev, int M, int N, int K, int act, float alpha, sampt_stream_t stream);
/* The same GEMM with the row maps the ViT engine uses: rowmap[m] = destination row of C / res for GEMM row m (-1 drops the
 * row; C must hold max(rowmap)+1 rows), a_rowmap[m] = row of A read by GEMM row m (gather), res_mod > 0: the residual row
 * is (destination row) % res_mod (broadcast over the batch, e.g. a positional embedding), ldr = row stride of res (0: N). */
/* The plain f32 product as the mask decoder issues it: C[m][n] = act(A[m * lda ..] . W[n][K] + bias[n]) (+ res[(m % res_mod)][n],
 * res_mod = 0: res[m][n]); lda / ldc = 0: K / N; workspace_dev: optional split-K workspace of the default routes.
 * invariant = 1: the row-invariant route — row m's bits are a function of its K inputs, K, N, the leading dimensions and the
 * pointers' alignment alone, whatever M is and wherever the row sits.
 * sampt_gemm_f32_route (host only): the kernel that call takes for 16-byte aligned operands and the decoder's split-K workspace —
 * route 0 skinny, 1 thin, 2 tiled, 3 row-invariant thin, 4 row-invariant one-wave-per-element — and the number of K partitions whose
 * partial sums are added at the end (lanes, waves or split-K slices). */
int sampt_gemm_f32_rows(const float* A_dev, int lda, const float* W_dev, const float* bias_dev, const float* res_dev, int res_mod,
                        float* C_dev, int ldc, int M, int N, int K, int act, int invariant, void* workspace_dev,
                        size_t workspace_bytes, sampt_stream_t stream);
int sampt_gemm_f32_route(int M, int N, int K, int lda, int ldc, int invariant, int* route, int* kparts);
int sampt_gemm_ex(int dtype, const void* A_dev, const void* W_dev, const float* bias_dev, const float* res_dev,
                  void* C_dev, int M, int N, int K, int act, float alpha, const int32_t* rowmap_dev,
                  const int32_t* a_rowmap_dev, int res_mod, int ldr, sampt_stream_t stream);
/* sampt_gemm_ex for dtype 1 .. 4 on the persistent 256 x 256 fp16 kernel (csrc/gemm_f16_p8.hip) and on no other: a shape or an
 * alignment that kernel does not take (M < 256, N % 256, stored K % 128, operands not 16-byte aligned, an x3 product with fp16
 * output, ...) returns SAMPT_ERR_UNSUPPORTED and nothing is computed.  heads, hd, rows: the head-major destination of
 * sampt_gemm_f16_head_major (dtype 2; all 0 = off).  wgs_per_xcd: persistent workgroups per XCD for this call, 0 = one per CU (32);
 * stagger: phase groups for this call, 0 = the process setting (sampt_gemm_set_stagger), 1 = off.  Reads sampt_gemm_set_trim /
 * _schedule / _stagger like every launch of the kernel and writes no process-wide state.  Whatever the workgroup count, the trim
 * rule, the schedule and the phase groups, the bits of C are the same.
 * sampt_gemm_f16_p8_plan (host only): what the launcher of that kernel does with an M x N product (M >= 256, N % 256 == 0) allowed
 * wgs_per_xcd workgroups per XCD (0 = 32) — the workgroups per XCD it launches (8 XCDs), the tile rounds (the longest tile list of a
 * workgroup) and the strip height in 256-row panels of the tile order.  trim: 0 / 1, -1 = the process setting (sampt_gemm_set_trim). */
int sampt_gemm_f16_p8(int dtype, const void* A_dev, const void* W_dev, const float* bias_dev, const float* res_dev, void* C_dev,
                      int M, int N, int K, int act, float alpha, const int32_t* rowmap_dev, const int32_t* a_rowmap_dev,
                      int res_mod, int ldr, int heads, int hd, int rows, int wgs_per_xcd, int stagger, sampt_stream_t stream);
int sampt_gemm_f16_p8_plan(int M, int N, int wgs_per_xcd, int trim, int* workgroups_per_xcd, int* rounds, int* strip_rows);
/* dtype 3 / 4 of sampt_gemm_ex: fp32-grade product on the fp16 matrix pipe.  A [M][2K] and W [N][2K] are "x3 rows": every
 * block of 32 consecutive k of a logical row is stored as 64 halves hi(32) | lo(32), v = hi + lo with hi = fp16(v),
 * lo = fp16(v - hi) (sampt_split_rows_x3; weights are split after scaling by 2^8 — sam_pt_amd/pack.py:x3_rows — and the
 * caller passes alpha = 2^-8).  K is the LOGICAL K (K % 64 == 0).  dtype 3: C f32 [M][N]; dtype 4: C x3 rows [M][2N]. */
int sampt_split_rows_x3(const float* x_dev, void* y_dev, int M, int K, sampt_stream_t stream);
/* NHWC convolution as implicit GEMM: x [n][H][W][Cin], w [Cout][KH][KW][Cin], y [n][OH][OW][Cout] (f32 out).
 * dtype 3 = fp32-grade result on the fp16 matrix pipe: x is f32, w_dev is half [2][Cout][KH*KW*Cin] = the weights times
 * 2^8 split as hi = fp16(w), lo = fp16(w - hi) (sam_pt_amd/pack.py:split_f16x3); Cin % 32 == 0, Cout % 4 == 0.
 * dtype 4 = the same with PRE-SPLIT activations: x_dev is half [2][n][H][W][Cin] = hi plane fp16(x), lo plane fp16(x - hi)
 * (what the tracker encoder's InstanceNorm writes); all four operand planes then reach LDS by LDS-DMA. */
int sampt_conv2d_nhwc(int dtype, const void* x_dev, const void* w_dev, const float* bias_dev, float* y_dev, int n,
                      int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, sampt_stream_t stream);
int sampt_instance_norm_nhwc(float* x_dev, int n, int hw, int C, float eps, int relu, const float* skip_dev,
                             void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
size_t sampt_instance_norm_workspace_bytes(int n, int hw, int C);
/* out_f16: 0 = f32 rows, 1 = fp16 rows, 2 = x3 rows [M][2D] (see sampt_split_rows_x3; D % 32 == 0) */
int sampt_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, void* y_dev, int M, int D, float eps,
                    int out_f16, int act, sampt_stream_t stream);
int sampt_resize_bilinear_nhwc(const float* src_dev, int n, int sh, int sw, int C, float* dst_dev, int dh, int dw,
                               int dstC, int c_off, int align_corners, sampt_stream_t stream);
int sampt_avgpool2x2_nhwc(const float* src_dev, int n, int h, int w, int C, float* dst_dev, sampt_stream_t stream);
/* Fused correlation + 7x7x4-level window sampler (CorrBlock.corr + .sample, pips.py:364-407).
 * ffeats_dev [n][S][128]; coords_dev [S][n][2] (level-0 feature-map pixels); out_dev [n][S][196]. */
int sampt_corr_sample_f32(const float* const pyr_dev[4], int H0, int W0, const int32_t* frame_idx_dev, int S, int n,
                          const float* ffeats_dev, const float* coords_dev, float* out_dev, sampt_stream_t stream);
/* The trackers' window kernels one by one (csrc/pips.hip, pips2.hip, cotracker.hip; layouts in those files' headers), exported for
 * tests/test_gpu_tracker_kernels.py.  Every one returns SAMPT_ERR_ARG for a null pointer or a non-positive count before any launch.
 * corr_sample_ex: sampt_corr_sample_f32 writing columns [xoff, xoff + 196) of rows of ldx floats; times (device [S], may be NULL)
 *   additionally writes the rest of the PIPS mixer input (needs xoff == 128, 519 <= ldx <= 580), as build_input does. */
int sampt_pips_corr_sample_ex(const float* const pyr[4], int H0, int W0, const int32_t* frame_idx, int S, int n, const float* ffeats,
                              const float* coords, float* x, int ldx, int xoff, const float* times, sampt_stream_t stream);
/* x [n][S][ldx]: columns [0, 128) = ffeats, [324, 519) = sin/cos embedding of (flow, time) and the three values, [519, ldx) = 0 */
int sampt_pips_build_input_f32(const float* ffeats, const float* coords, const float* times, int S, int n, float* x, int ldx,
                               sampt_stream_t stream);
/* coords [S][n][2] = coords0 [n][2] = xys / stride; ffeats [n][S][128] = feat_init [n][128] on every frame */
int sampt_pips_init_state_f32(const float* xys, const float* feat_init, float stride, int S, int n, float* coords, float* coords0,
                              float* ffeats, sampt_stream_t stream);
/* delta [n][S][130] = (dx, dy, 128 feature deltas): ffeats += gelu(Linear(GroupNorm(1, 128)(delta[2:]))), coords += delta[:2];
 * coords0 (may be NULL) locks frame 0 to it.  up_wT: the Linear weight transposed to [in][out]. */
int sampt_pips_apply_update_f32(const float* delta, const float* gn_w, const float* gn_b, const float* up_wT, const float* up_b,
                                float* ffeats, float* coords, const float* coords0, int S, int n, sampt_stream_t stream);
/* vis [S][n] = sigmoid(<ffeats, vis_w> + vis_b); traj [S][n][2] = coords * stride */
int sampt_pips_finalize_f32(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride, int S,
                            int n, float* traj, float* vis, sampt_stream_t stream);
/* Bookkeeping of the chained PIPS windows: q [n][3] = (t, x, y); cur int32 [n]; traj [T][n][2]; vis [T][n]; flip bytes [n];
 * fidx int32 [n][S]; xys [n][2]; xy_feat [n][2] and f0 int32 [n] come together or are both NULL; tr [S][n][2] and vi [S][n] are a
 * window's results; n_active int32 [1]. */
int sampt_pips_chain_init(const float* q, int n, int T, int32_t* cur, float* traj, float* vis, sampt_stream_t stream);
int sampt_pips_round_begin(const int32_t* cur, const uint8_t* flip, const float* traj, int T, int n, int S, int32_t* fidx, float* xys,
                           float* xy_feat, int32_t* f0, float stride, sampt_stream_t stream);
int sampt_pips_round_end(int32_t* cur, const float* tr, const float* vi, int T, int n, int S, float thr0, float* traj, float* vis,
                         int32_t* n_active, sampt_stream_t stream);
/* PIPS++: trajs0 [S][n][2] px; fmap [frames][H][W][128]; frame_idx int32 [n][S]; coords [S][n][2]; bak [n][2]; templates f1 / f2 /
 * f4 [n][S][128] (written only when have_init == 0); x [n][S][720]; omega [32]; delta [n][S][2]. */
int sampt_pips2_init_f32(const float* trajs0, const float* fmap, int H, int W, const int32_t* frame_idx, float stride, int S, int n,
                         int have_init, float* coords, float* bak, float* f1, float* f2, float* f4, sampt_stream_t stream);
int sampt_pips2_templates_f32(const float* fmap, int H, int W, const int32_t* frame_idx, const float* coords, int S, int n, float* f2,
                              float* f4, sampt_stream_t stream);
int sampt_pips2_build_input_f32(const float* coords, const float* omega, int S, int n, float* x, int ldx, sampt_stream_t stream);
/* y [n][S][C] = relu(InstanceNorm1d over S of x); y may be x */
int sampt_instnorm1d_relu_f32(const float* x, float* y, int n, int S, int C, sampt_stream_t stream);
/* out [rows][cout] += identity [rows][cin] placed at channel (cout - cin) / 2; relu != 0: max(., 0) of the sum */
int sampt_add_chanpad_f32(float* out, const float* identity, long rows, int cin, int cout, int relu, sampt_stream_t stream);
int sampt_pips2_apply_delta_f32(const float* delta, const float* bak, float stride, int S, int n, int last, float* coords, float* trajs,
                                sampt_stream_t stream);
/* CoTracker windows: qxy [n][2] px, qt int32 [n], frame_map int32 [T]; xy0 [n][2]; fidx_pt int32 [n]; traj_out [T][n_total][2];
 * vis_out [T][n_total]; window state coords [S][na][2], visin / mask [S][na], fidx int32 [na][S], ffeats [na][S][128]; carries
 * coords_prev [S][prev][2], vis_prev [S][prev] (needed when prev > 0); pos [na][E] from the tables pos_x [W][E / 2], pos_y [H][E / 2];
 * x [na][S][456] with the correlation columns [130, 326) already in place; times [S][456]. */
int sampt_cot_prepare(const float* qxy, const int32_t* qt, const int32_t* frame_map, float stride, int n, int T, float* xy0,
                      int32_t* fidx_pt, float* traj_out, float* vis_out, sampt_stream_t stream);
int sampt_cot_window_init(int ind, int S_local, int prev, int na, int S, const int32_t* qt, const float* xy0, const int32_t* frame_map,
                          const float* coords_prev, const float* vis_prev, const float* feat_init, float* coords, float* visin,
                          float* mask, int32_t* fidx, float* ffeats, sampt_stream_t stream);
int sampt_cot_pos_embed_f32(const float* coords, const float* pos_x, const float* pos_y, int H, int W, int E, int na, float* pos,
                            sampt_stream_t stream);
int sampt_cot_build_input_f32(const float* ffeats, const float* coords, const float* visin, const float* mask, const float* pos,
                              const float* times, int S, int na, float* x, sampt_stream_t stream);
int sampt_cot_window_store_f32(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride, int S,
                               int na, int ind, int S_local, int n_total, float* coords_prev, float* vis_prev, float* traj_out,
                               float* vis_out, sampt_stream_t stream);
/* The two kernels of a fused MLP-Mixer block (csrc/pips_mixer.hip; pips.py:96-128), exported for the kernel tests.
 * mlp: part_dev[slice][nseq*8][512] = fc2 over the slice's hidden units of gelu(fc1(LayerNorm(x)) + b1); x_dev [nseq*8][512],
 *      w1 [2048][512], b1 [2048], w2 [512][2048]; slices = 8, 16 or 32 (what sampt_pips_set_mixer's workgroup target selects).
 * reduce: x' = res + (sum of the `slices` slabs in order + bias) (slices = 0: x' = res, part / bias unused);
 *      mode 0: out_dev [nseq*8][512] = x' + token-mix(LayerNorm(x')) with tw1 [32][8], tb1 [32], tw2 [8][32], tb2 [8];
 *      mode 1: out_dev [nseq][512] = mean over the 8 tokens of LayerNorm(x') (token weights unused).  out_dev != res_dev. */
int sampt_pips_mix_mlp_f32(const float* x_dev, const float* lnw_dev, const float* lnb_dev, const float* w1_dev,
                           const float* b1_dev, const float* w2_dev, float* part_dev, int nseq, int slices,
                           sampt_stream_t stream);
int sampt_pips_mix_reduce_f32(const float* part_dev, int slices, const float* bias_dev, const float* res_dev, int nseq, int mode,
                              const float* lnw_dev, const float* lnb_dev, const float* tw1_dev, const float* tb1_dev,
                              const float* tw2_dev, const float* tb2_dev, float* out_dev, sampt_stream_t stream);
/* The split-fp16 generation of the same block (csrc/pips_mixer_x3.hip), exported for the kernel tests.
 * pre: x' = res + (slab sum + bias) (slices = 0: x' = res); xout_dev [nseq*8][512] = x' + token-mix(LayerNorm1(x')); xop_dev = the
 *      operand images of 2^6 LayerNorm2(xout) split into fp16 hi / lo, sampt_pips_mix_xop_halves(nseq) halves.
 * mlp_x3: part_dev[slice][nseq*8][512] from xop_dev and the block's packed weight stream wstream_dev [slices][(2048/slices/16)*64*512]
 *      halves (sam_pt_amd/pack.py pips_mixer_x3_stream; slices = 16 or 32) and the fc1 bias b1_dev [2048]. */
size_t sampt_pips_mix_xop_halves(int nseq);
int sampt_pips_mix_pre_f32(const float* part_dev, int slices, const float* bias_dev, const float* res_dev, int nseq,
                           const float* ln1w_dev, const float* ln1b_dev, const float* tw1_dev, const float* tb1_dev,
                           const float* tw2_dev, const float* tb2_dev, const float* ln2w_dev, const float* ln2b_dev,
                           float* xout_dev, void* xop_dev, sampt_stream_t stream);
int sampt_pips_mix_mlp_x3(const void* xop_dev, const void* wstream_dev, const float* b1_dev, float* part_dev, int nseq, int slices,
                          sampt_stream_t stream);
/* ViT attention on a packed qkv matrix [B*S*S][3*heads*hd] (f16), decomposed rel-pos tables (2S-1, hd) f32.
 * out_dev f16 [B*S*S][heads*hd].  The bias tables are built inside the kernel; the workspace arguments are kept for
 * ABI stability and ignored (may be NULL / 0). */
/* The mask decoder's two small fp32 attention kernels: q [F][Nq][heads*hd], k / v [F][Nk][heads*hd], out like q;
 * nk_item_dev (int32 [F] or NULL): per-item number of valid keys of a ragged batch.  kind 0 = few queries against up to
 * 4096 keys: hd 32 (token self-attention) runs wave = (64 queries, head) with scalar-loaded key rows split over 4 waves,
 * hd 16 one workgroup per (4 queries, head, item) — the engine's token->image attention is sampt_attention_t2i_f32 below;
 * kind 1 = many queries against few keys (image->token, hd 16, any Nk): with 8 heads wave = head, lane = query and the
 * K / V rows are scalar loads, otherwise one thread per (query, head) with keys staged through LDS in chunks of 128. */
int sampt_attention_f32(int kind, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int F, int Nq,
                        int Nk, int heads, int hd, const int32_t* nk_item_dev, sampt_stream_t stream);
/* The decoder's token -> image attention (8 heads x 16 channels: q [F][Nq][128], k / v [F][Nk][128]) as the engine runs
 * it: the keys of a frame are split over workgroups that each read their K / V rows once, fully coalesced, for all heads
 * and up to 8 queries (running softmax), and a second launch merges the splits.  Same result as kind 0 above up to fp32
 * re-association. */
int sampt_attention_t2i_workspace_bytes(int F, int Nq, int Nk, size_t* bytes);
int sampt_attention_t2i_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int F, int Nq, int Nk,
                            void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* The key split of that attention (host only): KS workgroups of kper keys per (item, 8 queries), one partial softmax state of
 * 144 floats per (item, query, split).  invariant = 0: chosen to fill the chip, so it shrinks as F * ceil(Nq / 8) grows;
 * invariant = 1 (sampt_dec_set_batch_invariant): a function of Nk alone.  sampt_attention_t2i_workspace_bytes covers both. */
int sampt_attn_t2i_plan(int F, int Nq, int Nk, int invariant, int* KS, int* kper);
/* CoTracker's UpdateFormer attention straight from packed qkv rows [rows][3*heads*hd] (timm Attention): token t of group b
 * is row b*batch_stride_rows + t*token_stride_rows (time attention: S, 1; space attention: 1, S); out [rows][heads*hd]. */
int sampt_cotracker_attention_f32(const float* qkv_dev, float* out_dev, int nbatch, int L, int batch_stride_rows,
                                  int token_stride_rows, int heads, int hd, sampt_stream_t stream);
/* SAM's ViT attention (sam/modeling/image_encoder.py Attention.forward with use_rel_pos: third-party segment-anything, absent
 * from /root/reference; restated in oracle/sam_ref.py) for B windows (or whole frames) of S x S tokens straight from the
 * packed fp16 qkv rows [B*S*S][3*heads*hd]; rel_h / rel_w: the block's rel_pos tables f32 [2S-1][hd] (the decomposed bias
 * is computed inside the kernel); out fp16 [B*S*S][heads*hd].  Supported geometries: (S, hd) = (64, 80), (64, 64),
 * (14, 80), (14, 64), (16, 32), (6, 32); anything else returns SAMPT_ERR_UNSUPPORTED.  workspace_dev / workspace_bytes
 * are unused (kept for ABI stability: K / V tiles are staged by LDS-DMA, nothing goes through HBM scratch). */
int sampt_vit_attention_f16(const void* qkv_dev, const float* rel_h_dev, const float* rel_w_dev, void* out_dev, int B,
                            int S, int heads, int hd, void* workspace_dev, size_t workspace_bytes, sampt_stream_t stream);
/* The same attention from the HEAD-MAJOR fp16 qkv matrix [3][heads][B*S*S][hd] (what sampt_gemm_f16_head_major writes with
 * rows = B*S*S): the K / V rows of one (window | frame, head) are one contiguous run, a key tile is a linear copy.  bias_row_dev
 * non-null: the B = frames * nwx * nwy launches are SAM's windows as in sampt_vit_window_attention (bias_row_dev: the qkv bias as
 * ONE TOKEN-MAJOR row of 3*heads*hd halves); null: whole frames, nwx .. grid_w ignored.  out fp16 token-major [B*S*S][heads*hd],
 * bitwise what sampt_vit_attention_f16 / sampt_vit_window_attention(precision 1) give on the token-major rows of the same values. */
int sampt_vit_attention_f16_head_major(const void* qkv_dev, const float* rel_h_dev, const float* rel_w_dev, void* out_dev, int B,
                                       int S, int heads, int hd, const void* bias_row_dev, int nwx, int nwy, int grid_h, int grid_w,
                                       sampt_stream_t stream);
/* fp16 product with the head-major destination: C[((part * heads + h) * rows + r) * hd + c] = A[m] . W[part * heads * hd + h * hd + c]
 * + bias, r = rowmap_dev[m] (null: m; -1 drops the row), fp32 accumulate, fp16 A [M][K], W [N][K] and C; N % (heads * hd) == 0,
 * hd % 4 == 0, rows > every destination row.  Element for element the values sampt_gemm_ex(dtype 2) writes to C[r][col]. */
int sampt_gemm_f16_head_major(const void* A_dev, const void* W_dev, const float* bias_dev, void* C_dev, int M, int N, int K,
                              int heads, int hd, int rows, const int32_t* rowmap_dev, sampt_stream_t stream);
/* K-medoids query-point selection (SamPt in query_masks mode / point re-initialisation: sam_pt/utils/query_points.py:62-99,
 * third-party sklearn_extra KMedoids(method="alternate", init="heuristic") restated in sam_pt_amd/query_points.py) on the
 * device, bit-identical to that host restatement: fp64 distances, numpy's pairwise summation order, first-index ties.
 * xy_dev: [n][2] f32 pixel coordinates (integers), n <= 2048.
 *   rowsums:   out_dev[i] = sum_j |xy_i - xy_j|  (the heuristic initialisation partitions these on the host: np.argpartition)
 *   alternate: medoids_dev int32 [K] holds the initial medoids on entry and the converged ones on return (K <= 64);
 *              iters_dev (int32, may be NULL) receives the number of iterations run (<= max_iter). */
int sampt_kmedoids_rowsums_f64(const float* xy_dev, int n, double* out_dev, sampt_stream_t stream);
int sampt_kmedoids_alternate(const float* xy_dev, int n, int K, int32_t* medoids_dev, int max_iter, int32_t* iters_dev,
                             sampt_stream_t stream);
/* Interactive point correction (sam_pt/modeling/sam_pt_interactive.py: the click simulator's DBSCAN and click rule) on the device.
 *   dbscan_labels:  labels_out_dev int32 [n] equal to sklearn.cluster.DBSCAN(eps, min_samples).fit(X).labels_ element for element,
 *                   by the order-free restatement in sam_pt_amd/interactive.py:dbscan_labels.  xy_dev: [n][2] f32 (row, col) pairs of
 *                   INTEGER pixel coordinates in 0 .. 32767 (what mask.nonzero().float() yields), 1 <= n <= 2^20.  A pair is a
 *                   neighbour iff its exact int32 squared distance is <= r2; the host passes r2 = floor(eps * eps) computed in
 *                   float64, which equals scikit-learn's dist <= eps unless eps^2 is within rounding of an integer (the Python
 *                   wrapper refuses such an eps).  The result does not depend on scheduling.  ws_dev: 16-byte aligned,
 *                   sampt_dbscan_workspace_bytes(n) bytes (0 for an n out of range); stream-ordered, no host synchronisation, so
 *                   what only the device can know comes back in the workspace: after the call its int32 word 0 is a status (0 = good;
 *                   bit 0: a pointer chase of the union-find hit its hard cap of n + 8 steps, which a forest over n nodes cannot
 *                   need - the kernels never spin; bit 1: a coordinate was no integer pixel in range) and word 1 the number of
 *                   clusters.  A C caller must read word 0 after it has synchronised with the stream and treat a non-zero value as
 *                   a failed call (the labels are then not valid): sampt_last_error cannot report what only the device knows
 *                   without a synchronisation inside the call.  The Python wrapper does exactly that and raises.
 *   dbscan_largest: Counter(labels).most_common(1) after -1 is removed: the largest cluster, on equal size the one whose first
 *                   member has the smallest index.  members_out_dev int32 [n]: its member indices in ascending order (the order of
 *                   mask_pixels[labels == id]).  info_out_dev int32 [4] = {id, size, number of clusters, id of the largest cluster};
 *                   with no cluster, or a largest one below min_points, id is -1 ("use the whole mask") and no member is written.
 *                   Same workspace size; it may be the one dbscan_labels used (words 0 .. 3 are left alone).
 *   int_frame_state: one frame of the click rule (lines 330 - 361 of the reference).  logits_dev f32 [h][w] (mask = logits > 0),
 *                   gt_dev bytes [h][w] (non-zero = object), points xy_dev f32 [n_points][2] (x, y), vis_dev f32 [n_points]
 *                   (visible iff == 1), label_dev int32 [n_points] (1 = positive).  info_out_dev int32 [8] = {|TP|, |FN|, |FP|, first
 *                   incorrect visible negative point or -1, first incorrect visible positive point or -1, 1 if a visible point's
 *                   rounded coordinate is off the frame, 0, 0}; cat_out_dev bytes [n_points]: bit 0 visible, 1 positive, 2 correct,
 *                   3 tp, 4 tn, 5 fp, 6 fn at the rounded coordinate (round half to even, as torch.round; -1 .. -size wraps as Python's
 *                   indexing does, nothing is clamped); fn_out_dev / fp_out_dev: the FN and FP masks as byte planes [h][w]. */
size_t sampt_dbscan_workspace_bytes(int n);
int sampt_dbscan_labels(const float* xy_dev, int n, int r2, int min_samples, int32_t* labels_out_dev, void* ws_dev, size_t ws_bytes,
                        sampt_stream_t stream);
int sampt_dbscan_largest(const int32_t* labels_dev, int n, int min_points, int32_t* members_out_dev, int32_t* info_out_dev, void* ws_dev,
                         size_t ws_bytes, sampt_stream_t stream);
int sampt_int_frame_state(const float* logits_dev, const uint8_t* gt_dev, int h, int w, const float* xy_dev, const float* vis_dev,
                          const int32_t* label_dev, int n_points, int32_t* info_out_dev, uint8_t* cat_out_dev, uint8_t* fn_out_dev,
                          uint8_t* fp_out_dev, sampt_stream_t stream);
/* Shi-Tomasi query points and mask erosion on the device (replaces the cv2 calls of
 * sam_pt/utils/query_points.py:102-162 extract_corner_points and :165-194 erode_mask_proportional_to_its_furthest_points_distance;
 * bit-identical to the numpy restatement of OpenCV's algorithms in sam_pt_amd/query_points.py).
 *   erode:      out = cv2.erode(mask, ones((k, k))) of a {0, 1} byte mask [H][W]; k = 0 means the default 3 x 3, k = 1 a copy;
 *               tmp_dev: H*W scratch bytes.
 *   shi_tomasi: image_dev u8 [3][H][W] RGB, mask_dev u8 {0, 1} [H][W].  Gray conversion, the 6 % / 2 % / 1 % / no erosion cascade
 *               (>= 10 surviving pixels), cornerMinEigenVal(3, 3), threshold at quality_level x the maximum inside the eroded
 *               mask, 3 x 3 local maxima, greedy selection of up to n_points (<= 64) corners at minDistance = the eroded mask's
 *               bounding-box diagonal / n_points — one launch sequence without a host round trip.  out_xy_dev f32 [n_points][2]
 *               (x, y); out_info_dev int32 [16]: [12] corners found, [10] k of the erosion kept (-1: the mask itself), [9] pixels
 *               of the eroded mask, [5..8] its bounding box (ymin, ymax, xmin, xmax), [0..4] the mask's bounding box and count. */
int sampt_qp_corners_workspace_bytes(int H, int W, size_t* bytes);
int sampt_qp_erode_u8(const uint8_t* mask_dev, int H, int W, int k, uint8_t* tmp_dev, uint8_t* out_dev, sampt_stream_t stream);
int sampt_qp_shi_tomasi(const uint8_t* image_dev, const uint8_t* mask_dev, int H, int W, int n_points, float quality_level,
                        float* out_xy_dev, int32_t* out_info_dev, void* ws_dev, size_t ws_bytes, sampt_stream_t stream);
/* The same attention at fp32 grade (precision "f16x3": three split-fp16 MFMAs per product in Q.K^T, the bias tables and
 * P.V; fp32 softmax).  qkv_dev: x3 rows [B*S*S][2*3*heads*hd] halves (what the dtype-4 qkv GEMM writes), out_dev: x3 rows
 * [B*S*S][2*heads*hd].  Same geometries as sampt_vit_attention_f16; heads*hd % 32 == 0. */
int sampt_vit_attention_x3(const void* qkv_dev, const float* rel_h_dev, const float* rel_w_dev, void* out_dev, int B, int S,
                           int heads, int hd, sampt_stream_t stream);
/* The windowed blocks as the encoder runs them (SAM's window_partition, App. A-3): qkv_dev holds frames x nwy x nwx windows of
 * S x S tokens in window order; token (iy, ix) of window (wy, wx) is zero PADDING when wy*S + iy >= grid_h or wx*S + ix >=
 * grid_w.  SAM pads after norm1, so a padded token's qkv is the bias alone: the kernels take its K / V from bias_row_dev (the
 * qkv bias as ONE row in the matrix's format: 3*heads*hd halves for precision 1, an x3 row of twice that for precision 2) and
 * never read the qkv rows of padded tokens (they may be uninitialised; the output rows of padded queries are meaningless). */
int sampt_vit_window_attention(int precision, const void* qkv_dev, const float* rel_h_dev, const float* rel_w_dev, void* out_dev,
                               int frames, int S, int heads, int hd, const void* bias_row_dev, int nwx, int nwy, int grid_h,
                               int grid_w, sampt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMPT_HIP_H */
