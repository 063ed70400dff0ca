// Internal C++ launcher API of the HIP library (one function per kernel family).
// All tensors are device pointers owned by the caller; every launcher is stream-ordered, allocation-free and
// returns SAMPT_OK or a negative SAMPT_ERR_* code.
#pragma once
#include "common.h"

namespace sampt {

// ---- elementwise.hip ------------------------------------------------------------------------
// uint8 CHW frames (T,3,H,W) -> f32 NHWC4 (T,H,W,4) = 2*(x/255)-1, 4th channel 0      (pips.py:446)
int rgb_u8chw_to_nhwc4(const void* src, int src_f32, float* dst, int T, int H, int W, hipStream_t s);
// per-(image, channel) mean / rstd over H*W of an NHWC f32 tensor (InstanceNorm2d, eps, biased variance)
// partials: workspace of at least instnorm_partial_floats(nimg, hw, C) doubles
size_t instnorm_partial_doubles(int nimg, long hw, int C);
// elementwise.hip: row gather / scatter by (frame, object) item numbers and a plain fill (SamPt's decode staging)
int move_rows(const void* src, void* dst, const int* idx, int rows, long row_bytes, int nm, int nf, int scatter, hipStream_t s);
int fill_f32(float* dst, long n, float v, hipStream_t s);
// conv_stem_x3.hip: the tracker encoder's 7 x 7 stride-2 stem over NHWC4 frames as 3-term split-fp16 products (+ InstanceNorm partial sums)
int conv_stem_tiles(int H, int W);
int conv_stem7x7_x3(const float* x, const float* w, const float* bias, float* y, int nimg, int H, int W, double* in_part, hipStream_t s);
int instnorm_finalize(const double* partials, int nimg, int nchunks, long hw, int C, float eps, float* mean_rstd, hipStream_t s);
int instnorm_stats(const float* x, int nimg, long hw, int C, float eps, double* partials, float* mean_rstd,
                   hipStream_t s);
// y = (x-mean)*rstd ; if relu1: y = max(y,0) ; if skip: y = max(y + skip, 0)
// y_hi / y_lo (optional, both or none): y additionally split into two fp16 planes (hi = fp16(y), lo = fp16(y - hi)), the
// operand format of conv_f16x3's pre-split path.  y == nullptr (planes given): the f32 result is not written at all
int instnorm_apply(const float* x, const float* mean_rstd, const float* skip, float* y, int nimg, long hw, int C,
                   int relu1, hipStream_t s, half_t* y_hi = nullptr, half_t* y_lo = nullptr);
// bilinear resize of an NHWC f32 tensor into channels [c_off, c_off+C) of a dstC-channel NHWC tensor
// dst_hi / dst_lo (optional, both or none): write the result as two fp16 planes (hi, lo = the split-fp16 convolution's
// operand format) INSTEAD of the f32 dst
int resize_bilinear_nhwc(const float* src, int n, int sh, int sw, int C, float* dst, int dh, int dw, int dstC,
                         int c_off, int align_corners, hipStream_t s, half_t* dst_hi = nullptr, half_t* dst_lo = nullptr);
int avgpool2x2_nhwc(const float* src, int n, int h, int w, int C, float* dst, hipStream_t s);
// LayerNorm over the last dim of rows. src_rows: optional gather (row index into x, or -1 -> output row = 0).
// out_f16: 1 = y is half; 2 = y is half "x3 rows" [M][2D] (common.h GemmP::x3; D % 32 == 0). act: applied after the affine transform (ACT_GELU for LayerNorm2d+GELU).
// column means of an fp16 matrix over M (optionally gathered) rows; calibration of the fp16 ViT mode's bias correction
int colmean_rows_f16(const half_t* A, long M, int K, int lda, const int* rowmap, float* out, hipStream_t s);
int layernorm_rows(const float* x, const float* w, const float* b, void* y, long M, int D, float eps,
                   const int* src_rows, int out_f16, int act, hipStream_t s);
// out[i] = a[i] + b[i % bmod] (f32).  n, bmod in elements.
int add_bcast(const float* a, const float* b, float* out, long n, long bmod, hipStream_t s);
int cast_f32_f16(const float* x, half_t* y, long n, hipStream_t s);
// f32 rows [M][K] -> x3 rows [M][2K] halves (common.h GemmP::x3: per 32-block hi(32) | lo(32), saturating split)
int split_rows_x3(const float* x, half_t* y, long M, int K, hipStream_t s);
// SAM preprocess + patch im2col: frames u8 HWC (B,H,W,3) -> A[B*g*g][3*P*P] with k = c*P*P + ky*P + kx,
// value = (x-mean[c])/std[c] inside the h x w image, 0 in the padded region (Sam.preprocess, App. A-2)
// chw: frames are (B,3,H,W) planar instead of (B,H,W,3).  mean/stdv are HOST pointers (3 floats each).
int sam_patchify(const uint8_t* frames, int chw, int B, int H, int W, int img, int P, const float* mean,
                 const float* stdv, void* A, int out_f16, hipStream_t s);

// single-channel bilinear resize (align_corners=False) of n maps: the target_hw resize of sam_pt.py:205-206
int resize_logits(const float* src, int n, int sh, int sw, float* dst, int dh, int dw, hipStream_t s);
// uint8 index mask = argmax over {background 0, object logits [M][npix]} (vos_eval/eval.py:304-355)
int index_masks(const float* logits, int M, long npix, uint8_t* out, hipStream_t s);

// ---- attention.hip --------------------------------------------------------------------------
// Decomposed relative-position terms of SAM's ViT attention (App. A-3):
//   relh[bh][q][kh] = <q_vec, rel_pos_h[qh - kh + S-1]>, relw likewise.  qkv: [B*S*S][3*D] (f32 or f16),
//   outputs f32 [B*heads][S*S][S].
int vit_rel_bias(const void* qkv, int qkv_f16, const float* rel_h, const float* rel_w, int B, int S, int heads,
                 int hd, float* relh, float* relw, hipStream_t s);
// scores[bh][q][k] (already scaled) += relh[bh][q][k/S] + relw[bh][q][k%S]; softmax over k, in place (f32).
int softmax_rel_rows(float* scores, const float* relh, const float* relw, long BH, int Nq, int S, hipStream_t s);
// Window padding of SAM's window_partition inside the attention kernels: the B launches of S x S tokens are frames x nwin
// windows, window w % nwin = (wy, wx) in row-major order over nwx windows per row; token (iy, ix) of it is PADDING when
// wy*S + iy >= gh or wx*S + ix >= gw.  Padded tokens enter attention as keys with qkv = bias (zero padding comes after norm1,
// App. A-3): the kernels fetch their K / V from ``bias_row`` (the qkv bias as one row in the qkv matrix's own format: 3D halves,
// or an x3 row of 6D halves) and never read the qkv rows of padded tokens.  bias_row == nullptr: no padding anywhere.
struct FlashPad {
  const half_t* bias_row = nullptr;
  int nwx = 0, nwin = 0, gh = 0, gw = 0;
  // vit_flash_attention_f16 only, optional: the block's rel-pos tables as fp16 MFMA operand images (pack.rel_pos_operand_images:
  // [2][ceil((2 S - 1) / 32)][hd / 16][64][8] halves) — the prologue then loads 16 bytes per lane and k-step instead of converting
  // the f32 tables in every workgroup.  Same halves, same results.
  const half_t* rel_ops = nullptr;
  // vit_flash_attention_f16 only: qkv is the head-major matrix [3][heads][B * S * S][hd] (GemmP::hm_hd with hm_rows = B * S * S)
  // instead of token-major rows.  bias_row stays a token-major row of 3 D halves; the output stays token-major.  Same results.
  int head_major = 0;
};
// Fused flash-style attention, f16 operands, fp32 softmax/accumulate.  qkv f16 [B*S*S][3*D]; out f16 [B*S*S][D];
// rel_h / rel_w: rel_pos tables f32 [2S-1][hd] (the decomposed bias is computed inside the kernel).
int vit_flash_attention_f16(const half_t* qkv, const float* rel_h, const float* rel_w, half_t* out, int B, int S,
                            int heads, int hd, hipStream_t s, FlashPad pad = FlashPad());

// attention_x3.hip: the same attention at fp32 grade (3-term split-fp16 products).  qkv: x3 rows [B*S*S][2*3D] halves (common.h
// GemmP::x3), out: x3 rows [B*S*S][2*D]
int vit_flash_attention_x3(const half_t* qkv, const float* rel_h, const float* rel_w, half_t* out, int B, int S, int heads,
                           int hd, hipStream_t s, FlashPad pad = FlashPad());

// ---- kmedoids.hip (query-point selection, sam_pt/utils/query_points.py:62-99; bit-identical to query_points.kmedoids_alternate)
// xy: device [n][2] f32 pixel coordinates (integers), n <= 2048.  rowsums: out[i] = sum_j dist(i, j) (fp64, numpy's pairwise order)
int kmedoids_rowsums(const float* xy, int n, double* out, hipStream_t s);
// medoids: device int [K], in = the initial medoids, out = the converged ones; iters_out (device int, optional) = iterations run
int kmedoids_alternate(const float* xy, int n, int K, int* medoids, int max_iter, int* iters_out, hipStream_t s);

// ---- dbscan.hip (interactive point correction, sam_pt/modeling/sam_pt_interactive.py:330-395, 678-729; labels equal to
// sklearn.cluster.DBSCAN's element for element, restated in sam_pt_amd/interactive.py)
// xy: device [n][2] f32 integer pixel coordinates (row, col) in 0 .. 32767, n <= 2^20; neighbours: d^2 <= r2.  labels int32 [n].
// ws (16-byte aligned, dbscan_workspace_bytes(n)): word 0 = status after the call (0 = good), word 1 = number of clusters
size_t dbscan_workspace_bytes(int n);
int dbscan_labels(const float* xy, int n, int r2, int min_samples, int* labels, void* ws, size_t ws_bytes, hipStream_t s);
// members int32 [n] (ascending indices of the chosen cluster), info int32 [4] = chosen id or -1, its size, clusters, largest id
int dbscan_largest(const int* labels, int n, int min_points, int* members, int* info, void* ws, size_t ws_bytes, hipStream_t s);
// frame state of the click rule: info int32 [8], cat u8 [n_points], fn / fp byte planes [h][w]
int int_frame_state(const float* logits, const unsigned char* gt, int h, int w, const float* xy, const float* vis, const int* label,
                    int n_points, int* info, unsigned char* cat, unsigned char* fn_out, unsigned char* fp_out, hipStream_t s);

// ---- corners.hip (Shi-Tomasi query points + mask erosion, sam_pt/utils/query_points.py:102-194; bit-identical to the numpy
// restatement in sam_pt_amd/query_points.py)
size_t qp_corners_workspace_bytes(int H, int W);
// out = cv2.erode(mask, ones((k, k))) for a {0, 1} byte mask [H][W] (k = 0: the default 3 x 3; k = 1: a copy); tmp: H*W bytes
int qp_erode(const uint8_t* mask, int H, int W, int k, uint8_t* tmp, uint8_t* out, hipStream_t s);
// image u8 [3][H][W] RGB, mask u8 {0, 1} [H][W] -> up to n_points corners (x, y) f32 in out_xy [n_points][2]; out_info: 16 int32
// (device): [12] = corners found, [10] = k of the erosion that was kept (-1: none), [9] = pixels of the eroded mask, [5..8] its
// bounding box (ymin, ymax, xmin, xmax), [0..4] the mask's bounding box and pixel count
int qp_corners(const uint8_t* image, const uint8_t* mask, int H, int W, int n_points, float quality, float* out_xy, int* out_info,
               void* ws, size_t ws_bytes, hipStream_t s);

// ---- pips.hip ---------------------------------------------------------------------------------
struct PyramidLevels {
  const float* base[4];   // level l: [nframes][H_l][W_l][C] f32 NHWC
  int H[4], W[4];
};
// ffeat[n][c] = bilinear_sample2d(fmap[frame], x/stride..)   (samp.py:6-80)
// frame_idx: optional per-point frame index into fmap [frames][H][W][C]
int pips_sample_feat(const float* fmap, int H, int W, int C, const int* frame_idx, const float* xy, int n, float* out,
                     hipStream_t s);
// fused correlation + 7x7 window sampler (pips.py:364-407): writes x[n][s][xoff + lvl*49 + i*7+j]
// times != nullptr: the level-0 workgroups also do pips_build_input's job (PIPS layout: xoff == 128, 519 <= ldx <= 580)
int pips_corr_sample(const PyramidLevels& pyr, const int* frame_idx, int S, int n, int C, const float* ffeats,
                     const float* coords, float* x, int ldx, int xoff, hipStream_t s, const float* times = nullptr);
// mixer input assembly: x[n][s][0:128]=ffeats, x[...][324:519] = sincos embedding of (flow, t) (misc.py:30-55)
// times: device [S] = torch.linspace(0, S, S) (pips.py:527)
int pips_build_input(const float* ffeats, const float* coords, const float* times, int S, int n, float* x, int ldx,
                     hipStream_t s);
int vos_index_masks(const float* logits, int M, int T, long hw, const int* qt, const uint8_t* gt, uint8_t* out,
                    hipStream_t s);
int pil_resample_u8(const uint8_t* src, uint8_t* dst, long outer, int in_len, int out_len, int inner, const int* coef,
                    const int* bounds, int ksize, hipStream_t s);
int vos_index_masks_resized(const float* logits, int M, int T, int h, int w, const int* qt, const uint8_t* gt, int oh,
                            int ow, uint8_t* out, hipStream_t s);
int fill_rows_bias(void* out, int f16, const int* rows, int nrows, const float* bias, int N, hipStream_t s);
// ---- PIPS++ (pips2.hip; pips_plus_plus.py:263-342, 436-546) — rows are (point, frame): row = pt*S + s
int pips2_init(const float* trajs0, const float* fmap, int H, int W, const int* frame_idx, float stride, int S, int n,
               int have_init, float* coords, float* bak, float* f1, float* f2, float* f4, hipStream_t s);
int pips2_templates(const float* fmap, int H, int W, const int* frame_idx, const float* coords, int S, int n, float* f2,
                    float* f4, hipStream_t s);
int pips2_build_input(const float* coords, const float* omega, int S, int n, float* x, int ldx, hipStream_t s);
int instnorm1d_relu(const float* x, float* y, int n, int S, int C, hipStream_t s);
int add_chanpad(float* out, const float* identity, long rows, int cin, int cout, int relu, hipStream_t s);
int pips2_apply_delta(const float* delta, const float* bak, float stride, int S, int n, int last, float* coords,
                      float* trajs, hipStream_t s);
// coords[s][pt] = coords0[pt] = xys[pt]/stride ; ffeats[pt][s] = feat_init[pt]     (pips.py:458-476)
int pips_init_state(const float* xys, const float* feat_init, float stride, int S, int n, float* coords,
                    float* coords0, float* ffeats, hipStream_t s);
// token-mixing PreNormResidual block of the MLP-Mixer, grid (sequence, 64-channel chunk) (pips.py:116,120-121); out of
// place: xo != x
int pips_token_mix(const float* x, float* xo, const float* lnw, const float* lnb, const float* w1, const float* b1,
                   const float* w2, const float* b2, int nseq, int S, int D, hipStream_t s);
// device-side bookkeeping of the chained PIPS windows (pips/tracker.py:42-153; kernels and layouts: pips.hip)
int pips_chain_init(const float* q, int n, int T, int* cur, float* traj, float* vis, hipStream_t s);
int pips_round_begin(const int* cur, const unsigned char* flip, const float* traj, int T, int n, int S, int* fidx, float* xys,
                     float* xy_feat, int* f0, float stride, hipStream_t s);
int pips_round_end(int* cur, const float* tr, const float* vi, int T, int n, int S, float thr0, float* traj, float* vis,
                   int* n_active, hipStream_t s);
// ---- pips_mixer.hip: the mixer's channel MLP + everything between two channel MLPs, two launches per block (file header)
extern int g_pips_mixer_fused, g_pips_mixer_wgs;
// hidden slices (8, 16 or 32) a channel-MLP launch over nseq sequences uses to reach g_pips_mixer_wgs workgroups
int pips_mix_slices(int nseq);
// part[slice][nseq*8][512] = fc2 over the slice's hidden units of gelu(fc1(LN(x)) + b1); x [nseq*8][512]
int pips_mix_mlp(const float* x, const float* lnw, const float* lnb, const float* w1, const float* b1, const float* w2,
                 float* part, int nseq, int NS, hipStream_t s);
// x' = res + (sum of the NS slabs + bias) (NS = 0: x' = res); mode 0: out [nseq*8][512] = x' + token-mix(LN(x')) with the
// token-mixing weights (w1 [32][8], w2 [8][32]); mode 1: out [nseq][512] = mean over the 8 tokens of LN(x').  out != res
int pips_mix_reduce(const float* part, int NS, const float* bias, const float* res, int nseq, int mode, const float* lnw,
                    const float* lnb, const float* w1, const float* b1, const float* w2, const float* b2, float* out,
                    hipStream_t s);
// ---- pips_mixer_x3.hip: the same block with the channel MLP as 3-term split-fp16 products (file header)
extern int g_pips_mixer_x3;
size_t pips_mix_xop_halves(int nseq);            // size of the operand-image buffer between the two kernels
// x' = res + (slab sum + bias); xout = x' + token-mix(LN1(x')) (f32, the next residual); xop = operand images of 2^6 LN2(xout)
int pips_mix_pre(const float* part, int NS, const float* bias, const float* res, int nseq, const float* ln1w, const float* ln1b,
                 const float* tw1, const float* tb1, const float* tw2, const float* tb2, const float* ln2w, const float* ln2b,
                 float* xout, half_t* xop, hipStream_t s);
// part[slice][nseq*8][512] from the operand images and the packed weight stream of the block (pack.pips_mixer_x3_stream, NS = 16 | 32)
int pips_mix_mlp_x3(const half_t* xop, const half_t* wstream, const float* b1, float* part, int nseq, int NS, hipStream_t s);
// mean over the S tokens of LN(x): out[n][D]
int pips_ln_mean(const float* x, const float* lnw, const float* lnb, float* out, int nseq, int S, int D, hipStream_t s);
// feature / coordinate update (pips.py:536-544): delta [n][S][130]; ffeats [n][S][128]; coords [S][n][2]
// up_wT: ffeat_updater weight transposed to [in][out]
int pips_update(const float* delta, const float* gn_w, const float* gn_b, const float* up_wT, const float* up_b,
                float* ffeats, float* coords, const float* coords0, int S, int n, hipStream_t s);
// vis[s][n] = sigmoid(<ffeats[n][s], w> + b) ; traj[s][n][2] = coords*stride
int pips_finalize(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride,
                  int S, int n, float* traj, float* vis, hipStream_t s);

// ---- raft.hip (RAFT point tracker, sam_pt/point_tracker/raft/; layouts in the file header) ---------------------------------
struct RaftLevels {
  const float* base[4];   // level l: [pair-directions][h8 * w8][h[l] * w[l]] f32
  int h[4], w[4];
};
// uint8 (T,3,H,W) -> f32 NHWC4 (T,Hp,Wp,4) = 2 * (x / 255) - 1, replicate-padded by (Hp - H) / 2 before and the rest after
int raft_prep_frames(const uint8_t* frames, int T, int H, int W, int Hp, int Wp, float* dst, hipStream_t s);
int raft_add_relu(const float* a, const float* b, float* out, long n, hipStream_t s);
int raft_split_ctx(const float* c, long rows, float* net, float* inp, hipStream_t s);
// chunk of np pairs from pair p0: pair-direction j < np is (p0 + j -> p0 + j + 1), j >= np its reverse
int raft_init_state(const float* net, const float* inp, int p0, int np, int h8, int w8, float* hx, float* coords1, float* flow,
                    hipStream_t s);
// out [M][352]: channel l * 81 + i * 9 + j = level l sampled at (x / 2^l + i - 4, y / 2^l + j - 4), [324, 352) zero; coords [M][2]
int raft_lookup(const RaftLevels& lv, const float* coords, long M, float* out, hipStream_t s);
// relu(Conv2d(2, 128, 7, padding=3)) over flow [nimg][h][wd][2]; w [98][128] with k = (ky * 7 + kx) * 2 + ci
int raft_convf1(const float* flow, const float* w, const float* bias, float* out, int nimg, int h, int wd, hipStream_t s);
int raft_gru_a(const float* zr, const float* hx, float* z, float* rhx, long M, hipStream_t s);
int raft_gru_b(const float* q, const float* z, float* hx, float* hnet, long M, hipStream_t s);
int raft_flow_update(const float* delta, float* coords1, float* flow, float* hx, int h8, int w8, long M, hipStream_t s);
int raft_flow_low(const float* flow, float* out, int p0, int np, int npairs, int h8, int w8, hipStream_t s);
// convex upsampling + un-padding to (2, H, W) per pair-direction; bwd == nullptr: np planes, all written to fwd[p0 ..]
int raft_upsample(const float* flow, const float* mask, float mask_scale, int h8, int w8, int H, int W, int p0, int np, float* fwd,
                  float* bwd, hipStream_t s);
// flows [T-1][2][H][W], q [n][3] = (t, x, y) -> traj [T][n][2], vis bytes [T][n]   (tracker.py:46-88)
int raft_chain(const float* fwd, const float* bwd, int T, int H, int W, const float* q, int n, float* traj, unsigned char* vis,
               hipStream_t s);

// ---- tapir.hip (TAPIR point tracker, sam_pt/point_tracker/tapir/; layouts in the file header) ---------------------------------
// rows are (query, frame): row = q * T + t; the model's geometry is fixed: 256 x 256 frames, hires 64 x 64 x 128, lowres 32 x 32 x 256
struct TapirHeadW {
  const float *w1, *b1;   // cost_volume_regression_1: [16][9], [16]
  const float *w2, *b2;   // cost_volume_regression_2: [16][9] (input channel major), [1]
  const float *w3, *b3;   // cost_volume_occlusion_1: [16][9][32] (output channel fastest), [32]
  const float *w4, *b4;   // cost_volume_occlusion_2: [16][32], [16]
  const float *w5, *b5;   // occlusion_out: [2][16], [2] (TapNet: [1][16], [1])
};
// f32 (T,3,256,256) in [0, 1] -> NHWC4 (T,256,256,4) = 2 x - 1, 4th channel 0
int tapir_prep_frames(const float* chw, int T, float* dst, hipStream_t s);
// y = (x - mean) * rstd * scale[c] + offset[c] (+ ReLU); y_hi / y_lo as for instnorm_apply (y == nullptr: planes only)
int instnorm_affine_apply(const float* x, const float* mean_rstd, const float* scale, const float* offset, float* y, int nimg, long hw,
                          int C, int relu, hipStream_t s, half_t* y_hi = nullptr, half_t* y_lo = nullptr);
// y[row] = x[row] / sqrt(max(sum_c x[row][c]^2, 1e-12))
int tapir_l2norm_rows(const float* x, float* y, long rows, int C, hipStream_t s);
// qf [n][384] = hires (128) | lowres (256) read bilinearly (edge clamp) at the query (t, x, y) of frame round(t)
int tapir_query_feats(const float* hires, const float* lowres, int T, const float* q, int n, float* qf, hipStream_t s);
// cost-volume heads, one workgroup per (query, frame): qf rows of ldq floats whose 256 lowres channels start at qoff; pts [n T][2],
// occ / expd [n T]; iter_out (optional) [n T][4] = (x, y, occ, expd)
int tapir_heads(const float* lowres, int T, const float* qf, int ldq, int qoff, const float* q, int n, const TapirHeadW& w, float* pts,
                float* occ, float* expd, float* iter_out, hipStream_t s);
// mixer input rows x [n T][ldx >= 486]: 0, 0, occ, expd, features (384), 49 + 49 patch correlations, zeros up to ldx.  feat: [n][384]
// (feat_per_row == 0: the query features) or [n T][384] (the previous iteration's features); pos [n T][2] in 256 x 256 pixels
int tapir_patch_corr(const float* hires, const float* lowres, int T, int n, const float* pos, const float* occ, const float* expd,
                     const float* feat, int feat_per_row, float* x, int ldx, hipStream_t s);
// xo = x + sum of fours(dw2(gelu_tanh(dw1(LN(x))))) over time per query; x, xo [n][T][512], xo != x
int tapir_temporal_mix(const float* x, float* xo, const float* ln, const float* w1, const float* b1, const float* w2, const float* b2,
                       int n, int T, hipStream_t s);
// C [M][N] = act(A [M][K] W [N][K]^T + bias) (+ res): exact-f32 MFMA with one K order for every row whatever M is (K % 16 == 0, N % 4 == 0)
int tapir_gemm(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, long M, int N, int K, int act,
               const float* res, int ldr, hipStream_t s);
// pos += res[0:2], occ += res[2], expd += res[3], feats = (first ? qf[q] : feats) + res[4:388]; iter_out (optional) [n T][4]
int tapir_update(const float* res, const float* qf, int first, float* pos, float* occ, float* expd, float* feats, float* iter_out, int n,
                 int T, hipStream_t s);

// ---- tapnet.hip (TapNet point tracker, sam_pt/point_tracker/tapnet/; layouts in the file header) -------------------------------
// relu(a[c] x + b[c]) of x [T][hw][C] (BatchNorm folded on the host), written (1) temporally shifted by n channels — output channels
// [0, n) = channels [C - n, C) of frame t + 1, [C - n, C) = channels [0, n) of frame t - 1, zeros past the clip's ends — to ys (f32) and /
// or ys_hi / ys_lo (split-fp16 planes), and (2) unshifted to yu and / or yu_hi / yu_lo where given.  n % 4 == 0, 2 n <= C; n = 0: no shift.
int tapnet_bn_shift(const float* x, const float* a, const float* b, int T, long hw, int C, int n, float* ys, half_t* ys_hi, half_t* ys_lo,
                    float* yu, half_t* yu_hi, half_t* yu_lo, hipStream_t s);
// 3 x 3 max-pool, stride 2, TensorFlow "SAME" (padding never wins): x [n][H][W][C] -> y [n][ceil(H / 2)][ceil(W / 2)][C]
int tapnet_maxpool(const float* x, float* y, int n, int H, int W, int C, hipStream_t s);
// qf [n][256] = the grid [T][32][32][256] read trilinearly (every index clamped) at the query (t, x, y); t is not rounded
int tapnet_query_feats(const float* grid, int T, const float* q, int n, float* qf, hipStream_t s);
// cost-volume heads (cost_volume_heads.h: temperature 10, w5 [1][16], no ReLU after w3): qf [n][256]; pts [n T][2], occ [n T]
int tapnet_heads(const float* grid, int T, const float* qf, const float* q, int n, const TapirHeadW& w, float* pts, float* occ, hipStream_t s);

// ---- tinyvit.hip (TinyViT image encoder of MobileSAM / Light HQ-SAM; layouts in the file header) -----------------------------
// Sam.preprocess for the convolutional stem: uint8 (B,3,H,W) [chw] or (B,H,W,3) -> f32 (B,img,img,4) = (x - mean) / std inside the
// picture, zeros outside and in the 4th channel.  mean / stdv are HOST pointers (3 floats each)
int tinyvit_preprocess(const uint8_t* frames, int chw, int B, int H, int W, int img, const float* mean, const float* stdv, float* dst,
                       hipStream_t s);
// depthwise 3 x 3, pad 1, stride 1 | 2: y [n][OH][OW][C] = (gelu)(conv(x [n][H][W][C], w [3][3][C]) + bias [C]); C % 32 == 0
int tinyvit_dwconv3x3(const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int C, int stride, int gelu,
                      hipStream_t s);
// window attention with a learned per-offset bias over ws x ws windows (ws <= 14, head width 32): qkv [B][H][W][3 * 32 heads] per-head
// interleaved (q | k | v), table [heads][ws^2] read at |dy| ws + |dx|, pad_qkv [3 * 32 heads] = the qkv of a zero-padded position;
// out [B][H][W][32 heads], real positions only
int tinyvit_window_attention(const float* qkv, const float* table, const float* pad_qkv, float* out, int B, int H, int W, int heads, int ws,
                             hipStream_t s);
int tinyvit_gelu(const float* x, float* y, long n, hipStream_t s);      // y = erf-GELU(x), n % 4 == 0 (in place allowed)

// ---- superglue.hip (SuperGlue point tracker, sam_pt/point_tracker/superglue/; layouts in the file header) --------------------
// uint8 (T,3,H,W) -> f32 NHWC4 (T,H,W,4): channel 0 = uint8(0.2989 r + 0.587 g + 0.114 b) / 255, the rest zero
int sg_grey(const uint8_t* frames, int T, int H, int W, float* dst, hipStream_t s);
int maxpool2x2_nhwc(const float* src, int n, int h, int w, int C, float* dst, hipStream_t s);
// logits [nimg * h8 * w8][ld >= 65] -> dense score maps [nimg][8 h8][8 w8] (softmax over 65, dustbin dropped, depth-to-space)
int sg_scores(const float* logits, int ld, int nimg, int h8, int w8, float* dense, hipStream_t s);
// simple_nms + threshold (>) + remove_borders + row-major compaction: kpts [nimg][cap][2] (x, y), kscores [nimg][cap], count
// [nimg] = the true number of survivors (entries at or beyond cap are not written).  radius <= 16, Hs <= 4096
size_t sg_nms_workspace_bytes(int nimg, int Hs, int Ws);
int sg_nms_compact(const float* scores, int nimg, int Hs, int Ws, int radius, float thr, int border, int cap, float* kpts,
                   float* kscores, int* count, void* ws, size_t ws_bytes, hipStream_t s);
// dmap [nimg][h8 * w8][256] (raw) -> out [nimg][cap][256] for the first min(count[f], cap) keypoints of every image (count ==
// nullptr: cap of them); launch_n = the largest count (grid size)
int sg_sample_descriptors(const float* dmap, int nimg, int h8, int w8, const float* kpts, const int* count, int cap, int launch_n,
                          float* out, hipStream_t s);
int sg_kenc_input(const float* kpts, const float* scores, int n, int H, int W, float* out, hipStream_t s);
// out[i][h * 64 + d] = softmax_j(<q_i, k_j> / 8) v_j per head h, any N >= 1 queries and M >= 1 keys (row strides in floats)
int sg_attention(const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, int N, int M, int heads,
                 hipStream_t s);
// log_optimal_transport's u [N + 1] and v [M + 1] after `iters` iterations; bin: device scalar
int sg_sinkhorn(const float* S, int ld, int N, int M, const float* bin, int iters, float* u, float* v, hipStream_t s);
// matches0 / matching_scores0 [N] from S, u, v; scratch max0 [N], idx0 [N], idx1 [M]
int sg_match_from_scores(const float* S, int ld, int N, int M, const float* u, const float* v, float thr, float* max0, int* idx0,
                         int* idx1, int* matches0, float* mscores0, hipStream_t s);
int sg_no_match(int n, int* matches0, float* mscores0, hipStream_t s);
// per-mask ordered lists of the matched keypoint-1 indices inside (0) / outside (1) the mask: lists [n_masks][2][cap], counts [n_masks][2]
int sg_select_lists(const int* matches0, int n0, const float* kpts1, const float* masks, int n_masks, int H, int W, int cap,
                    int* lists, int* counts, hipStream_t s);
// lists [T-1][n_masks][2][list_cap], counts [T-1][n_masks][2], draw [T-1][n_masks][n_pos + n_neg] (list entry, < 0 = padding),
// kpts [T][kp_cap][2], query_xy [n_masks * P][2] -> traj [T][n_masks * P][2], vis [T][n_masks * P]
int sg_gather(const float* query_xy, const float* kpts, int kp_cap, const int* lists, int list_cap, const int* counts, const int* draw,
              int T, int n_masks, int n_pos, int n_neg, float* traj, float* vis, hipStream_t s);

// ---- cotracker.hip (CoTracker v1 windows: SURVEY.md App. A-6; layouts in the file header) -------------------------------
int cot_prepare(const float* qxy, const int* qt, const int* frame_map, float stride, int n, int T, float* xy0, int* fidx_pt,
                float* traj_out, float* vis_out, hipStream_t s);
int cot_window_init(int ind, int S_local, int prev, int na, int S, const int* qt, const float* xy0, const int* frame_map,
                    const float* coords_prev, const float* vis_prev, const float* feat_init, float* coords, float* visin,
                    float* mask, int* fidx, float* ffeats, hipStream_t s);
int cot_pos_embed(const float* coords, const float* pos_x, const float* pos_y, int H, int W, int E, int na, float* pos,
                  hipStream_t s);
int cot_build_input(const float* ffeats, const float* coords, const float* visin, const float* mask, const float* pos,
                    const float* times, int S, int na, float* x, hipStream_t s);
// attention over token groups taken from packed qkv rows [rows][3*heads*hd]: token t of group b = row b*bs + t*ts
int cot_attention(const float* qkv, float* out, int nbatch, int L, int bs, int ts, int heads, int hd, hipStream_t s);
int cot_window_store(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride, int S,
                     int na, int ind, int S_local, int n_total, float* coords_prev, float* vis_prev, float* traj_out,
                     float* vis_out, hipStream_t s);
// F.interpolate(bilinear, align_corners=False) of n single-channel planes (uint8 or f32) to f32
int resize_planes(const void* src, int src_u8, long n, int sh, int sw, float* dst, int dh, int dw, hipStream_t s);

// ---- sam_decoder.hip (every launcher takes the frame batch F; tensors are [F][...] contiguous) ---------------
// decoder tokens [F][Nt][256] (Nt = 5 + k + (box ? 2 : 1)): out tokens, then the sparse prompt tokens (App. A-4).
// pts [F][ld_pts][2] input-frame px, labels [F][ld_pts] i32, box [F][4] or null.
int sam_tokens(const float* out_tokens /*[n_out][256]*/, int n_out, const float* pts, const int* labels, int k, int ld_pts,
               const float* box, const float* gauss, const float* point_emb /*[4][256]*/, const float* not_a_point,
               float img_size, int F, const int* k_item /*[F] or null*/, int* ntok /*[F] out or null*/, float* tokens,
               hipStream_t s);
// small f32 attention, one workgroup per (query, head, frame): q [F][Nq][H*hd], k,v [F][Nk][H*hd]
// nk_item: optional per-frame key count (<= Nk) of a ragged batch
int attn_rowblock(const float* q, const float* k, const float* v, float* out, int F, int Nq, int Nk, int heads, int hd,
                  const int* nk_item, hipStream_t s);
// small f32 attention with few keys (Nk <= 64): one thread per (query, head)
// token -> image attention, 8 heads x 16 channels (q/k/v/out rows of 128 floats), any Nq / Nk: keys split over workgroups,
// partial softmax states merged by a second launch; ws: attn_t2i_workspace_floats(F, Nq, Nk) floats (0: none needed)
size_t attn_t2i_workspace_floats(int F, int Nq, int Nk);
int attn_t2i(const float* q, const float* k, const float* v, float* out, int F, int Nq, int Nk, float* ws, size_t ws_floats,
             hipStream_t s, int ldkv = 128 /* row stride of k and v in floats (slices of a fused projection) */,
             bool fixed_split = false /* key split from Nk alone: a query's result does not depend on F or Nq */);
// the key split attn_t2i makes: KS splits of kper keys (host only)
void attn_t2i_plan_query(int F, int Nq, int Nk, bool fixed_split, int* KS, int* kper);
int attn_fewkeys(const float* q, const float* k, const float* v, float* out, int F, int Nq, int Nk, int heads, int hd,
                 const int* nk_item, hipStream_t s, int ldq = 0 /* row stride of q in floats (0: heads*hd) */,
                 bool shared_q = false /* q is [Nq][ldq], the same queries for every item (8 heads x 16 channels only) */);
// low_res[f][p] = <hyper[f][0:C], up[f][p][0:C]>
int sam_mask_dot(const float* up, const float* hyper, int ld_hyper, const float* up2 /*or null*/, const float* hyper2,
                 int ld_hyper2, float* low_res, int F, int npix, int C, hipStream_t s);
// every mask of an item from one read of its upscaled map (C == 32): low_res [F][m_out][npix] = <hyper[f][j], up[f][p]>, hyper [F][mh][32],
// m_out = 3 (needs mh >= 3) or 1.  up2 / hyper2 (HQ-SAM, m_out = 1): the HQ term is added.  sel [F][mh] (with up2): the mask token with the
// largest sel[f][.] is the one used and iou_sel[f] receives that maximum (MaskDecoderHQ with multimask_output=True)
int sam_mask_dot_multi(const float* up, const float* hyper, int mh, int m_out, const float* up2, const float* hyper2,
                       int ld_hyper2, const float* sel, float* low_res, float* iou_sel, int F, int npix, int C, hipStream_t s);
// fused Sam.postprocess_masks: low (L x L) -> bilinear to (img x img) -> crop (in_h,in_w) -> bilinear to (oh,ow)
int sam_postprocess(const float* low, int L, int img, int in_h, int in_w, float* out, int oh, int ow, hipStream_t s);
// bbox state per frame: int[5] = {xmin, ymin, xmax, ymax, count} of logits > 0 (refinement box of sam_pt.py:809-820);
// bbox_partial: scratch of F * bbox_partial_ints(oh, ow) ints (deterministic two-stage reduction, no atomics)
size_t bbox_partial_ints(int oh, int ow);
int sam_postprocess_bbox(const float* low, int L, int img, int in_h, int in_w, float* out, int oh, int ow, int F,
                         int* bbox, int* bbox_partial, hipStream_t s);
// ---- amg.hip: scoring tail of the automatic mask generator on low-res masks [N][L][L] (no full-resolution logits are written)
// out8 int [N][8] = {#(v > thr + off), #(v > thr - off), #(v > thr), inclusive XYXY box of v > thr (zeros when empty), 0} of
// v = Sam.postprocess_masks(low) evaluated on the fly with k_sam_postprocess's arithmetic; ws: amg_score_workspace_bytes(N)
size_t amg_score_workspace_bytes(int N);
int amg_score(const float* low, int N, int L, int img, int in_h, int in_w, int oh, int ow, double thr, double off, int* out8,
              void* ws, size_t ws_bytes, hipStream_t s);
// out bytes [R][oh][ow] = (v(low[rows[r]]) > thr) as 0 / 1; rows: device int [R] with values in [0, N)
int amg_binarize(const float* low, int N, const int* rows, int R, int L, int img, int in_h, int in_w, int oh, int ow, double thr,
                 unsigned char* out, hipStream_t s);
// ---- amg_tail.hip: the generator's tail on the device, exactly the host functions' results
// small-region clean-up (holes, then islands; 8-connected; small = fewer than min_area pixels) of byte masks [n][h][w] ->
// masks_out bytes, changed bytes [n], area int [n], boxes int [n][4] (inclusive XYXY, zeros when empty).  The stack is processed
// in chunks of what ws holds (amg_regions_workspace_bytes(1, h, w) at least)
size_t amg_regions_workspace_bytes(int n, int h, int w);
int amg_regions(const unsigned char* masks_in, int n, int h, int w, int min_area, unsigned char* masks_out, unsigned char* changed,
                int* area, int* boxes, void* ws, size_t ws_bytes, hipStream_t s);
// greedy box NMS: boxes f32 [n][4] XYXY, scores f32 [n] -> keep (input indices in sweep order), count [1]
size_t amg_nms_workspace_bytes(int n);
int amg_nms(const float* boxes, const float* scores, int n, float thr, long long* keep, int* count, void* ws, size_t ws_bytes,
            hipStream_t s);
// ---- rle.hip: COCO run-length encoding of a stack [n][h][w] of bytes (non-zero = set) or of f32 values (set iff x > thr), exactly
// mask_to_rle's runs (column-major, the first run counts zeros) and maskApi's rleToString of them.  h * w < 2^31.
// count: offsets int64 [n + 1] (runs of the masks before m; [n] = the total the caller sizes `counts` by), area int32 [n]; it
//   leaves the transition words in ws (rle_workspace_bytes(n, h, w), 16-byte aligned) for emit, which takes the same n, h, w, ws.
// string_sizes: str_offsets[n] = characters of the whole stack; string_emit: the characters and str_offsets[0 .. n).
size_t rle_workspace_bytes(int n, int h, int w);
int rle_count(const void* x, int is_f32, float thr, int n, int h, int w, long long* offsets, int* area, void* ws, size_t ws_bytes,
              hipStream_t s);
int rle_emit(int n, int h, int w, const long long* offsets, unsigned* counts, const void* ws, size_t ws_bytes, hipStream_t s);
size_t rle_string_workspace_bytes(long total);
int rle_string_sizes(const unsigned* counts, const long long* offsets, int n, long total, long long* str_offsets, void* ws,
                     size_t ws_bytes, hipStream_t s);
int rle_string_emit(const unsigned* counts, const long long* offsets, int n, long total, long long* str_offsets, unsigned char* chars,
                    const void* ws, size_t ws_bytes, hipStream_t s);
// ---- vos_metrics.hip: the six integer counts of DAVIS J and F per item (inter, union, n_seg, n_ann, seg_match, ann_match) of two
// stacks of planes [.][h][w]; kind 0 = bytes (non-zero), 1 = f32 (x > thr), 2 = uint8 index map (x == values[i]); planes (or
// null: item i reads plane i) and values are int32 [n] on the device.  void_px: optional byte planes cleared from both images.
// 0 <= radius <= 64, h * w < 2^31; counts int32 [n][6]; ws of jf_workspace_bytes (16-byte aligned) holds the boundary bit-planes.
size_t jf_workspace_bytes(int n, int h, int w, int radius);
int jf_counts(const void* seg, int seg_kind, float seg_thr, const int* seg_values, const int* seg_planes, const void* ann, int ann_kind,
              float ann_thr, const int* ann_values, const int* ann_planes, const unsigned char* void_px, const int* void_planes, int n,
              int h, int w, int radius, int* counts, void* ws, size_t ws_bytes, hipStream_t s);
// ---- vos_pairs.hip: the counts of J and F of every (seg mask p, ann mask k) pair of every frame.  Sources as for jf_counts; seg mask
// (p, t) is item t * n_seg + p, ann mask (k, t) item t * n_ann + k; void_px: one optional byte plane per frame.  pair_out int32
// [n_frames][n_seg][n_ann][3] = inter, seg_match, ann_match; seg_stat [n_frames][n_seg][2] and ann_stat [n_frames][n_ann][2] = area,
// boundary count.  ws of jf_pairs_workspace_bytes (16-byte aligned) holds the mask, boundary and dilated-boundary bit-planes.
size_t jf_pairs_workspace_bytes(int n_seg, int n_ann, int n_frames, int h, int w, int radius);
int jf_pairs_counts(const void* seg, int seg_kind, float seg_thr, const int* seg_values, const int* seg_planes, int n_seg, const void* ann,
                    int ann_kind, float ann_thr, const int* ann_values, const int* ann_planes, int n_ann, const unsigned char* void_px,
                    const int* void_planes, int n_frames, int h, int w, int radius, int* pair_out, int* seg_stat, int* ann_stat, void* ws,
                    size_t ws_bytes, hipStream_t s);
// ---- vis_eval.hip: YouTube-VIS AP / AR.  Bit-planes: a stack [n][h][w] as uint64 [n][ceil(h / 64)][w], bit j of word (band b, column x)
// = pixel (64 b + j, x), bits of rows >= h are 0.  pack: the three kinds of jf_counts -> bit-planes + area int32 [n].  rle_decode_bits:
// the inverse of rle_count / rle_emit (status 0 = good; a bad mask's plane is zeros).  seq_iou_counts: int64 [D][G][2] = (inter, union)
// over the frames, plane -1 = no mask on that frame.  vis_match: the greedy matching of evaluateVid per (area range, IoU threshold).
int bits_pack(const void* x, int kind, float thr, const int* values, const int* planes, int n, int h, int w, unsigned long long* bits,
              int* area, hipStream_t s);
size_t rle_decode_workspace_bytes(long total);
int rle_decode_bits(const unsigned* counts, const long long* offsets, int n, long total, int h, int w, unsigned long long* bits, int* area,
                    int* status, void* ws, size_t ws_bytes, hipStream_t s);
int bits_unpack(const unsigned long long* bits, int n, int h, int w, unsigned char* out, hipStream_t s);
size_t seq_iou_workspace_bytes(int D, int G, int T, int h, int w);
int seq_iou_counts(const unsigned long long* dt_bits, const int* dt_area, const int* dt_planes, int D, int dt_n_planes,
                   const unsigned long long* gt_bits, const int* gt_area, const int* gt_planes, int G, int gt_n_planes, int T, int h, int w,
                   long long* counts, void* ws, size_t ws_bytes, hipStream_t s);
int vis_match(const long long* counts, int D, int G, int A, int n_thr, const double* thrs, const int* gt_order, const unsigned char* gt_ignore,
              const unsigned char* iscrowd, const unsigned char* dt_out, int* dt_match, int* gt_match, unsigned char* dt_ignore, hipStream_t s);
// ---- mask_points.hip: rank -> pixel on bit-planes.  bits_row_prefix: prefix int [n][h + 1], prefix[i][y] = set pixels of plane i in
// rows < y.  bits_select: queries int [nq][3] = (plane, invert, rank) -> yx f32 [nq][2], the rank-th set (invert: clear, inside the
// image) pixel in row-major order, (-1, -1) for a plane or rank out of range.
int bits_row_prefix(const unsigned long long* bits, int n, int h, int w, int* prefix, hipStream_t s);
int bits_select(const unsigned long long* bits, const int* prefix, int n, int h, int w, const int* queries, int nq, float* yx_out,
                hipStream_t s);
// ---- viz.hip: prediction overlays.  viz_band: bit-planes [n][nb][w] -> the contour band dil(m) & dil(~m) in the same layout (disk of
// radius 0 .. 64, ~m inside the image only).  viz_compose: frames uint8 [T][3][h][w] (or interleaved [T][h][w][3]) -> out [T][h][w][3],
// or [T][2 h][w][3] for panel 3; panel bit 0 = the input panel (frame + markers), bit 1 = the predictions panel (frame, per mask the
// table of its colour / bit / band, then the markers).  bits / band: mask m of frame t is plane m * T + t; lut [62][256]; markers int32
// [T][n_markers][8].
int viz_band(const unsigned long long* bits, int n, int h, int w, int radius, unsigned long long* band, hipStream_t s);
int viz_compose(const unsigned char* frames, int interleaved, int n_frames, int h, int w, const unsigned long long* bits,
                const unsigned long long* band, int n_masks, const unsigned char* lut, const int* markers, int n_markers, int panel,
                unsigned char* out, hipStream_t s);
// ---- patch_filter.hip: the patch-similarity filter of SamPt._track_points (sam_pt.py:597-690) in one launch, one workgroup per point.
// rgb uint8 [T][3][H][W], query f32 [N][3] = (t, x, y), traj f32 [T][N][2], vis_in f32 [T][N], companding = the 256-entry float64
// sRGB table of the host; vis_out f32 [T][N] (not vis_in), sim_out f32 [T][N] or null.  patch_size 1 .. PATCH_FILTER_MAX_PATCH_SIZE.
#define PATCH_FILTER_MAX_PATCH_SIZE 15
int patch_filter(const unsigned char* rgb, int T, int H, int W, const float* query, const float* traj, const float* vis_in, int N,
                 int patch_size, float threshold, const double* companding, int border_rule, float* vis_out, float* sim_out,
                 hipStream_t s);
// ---- prompt_assembly.hip: SamPt._prepare_points + apply_coords per (frame, object) item from tracks on the device.  traj f32
// [T][M][P][2], vis f32 [T][M][P] codes (visible iff == 1).  prompt_count: k_all / npos_all int [T * M].  prompt_fill: the F items
// named by items (int, item = t * M + m) -> pts f32 [F][ld][2], labels int [F][ld] (zeros past an item's k), k_item / npos_item int [F].
// mark_outside_frame: vis_out[i] = -2 where point i of traj [n][2] fails one of the four border comparisons, else vis_in[i] (may alias).
int prompt_count(const float* vis, int T, int M, int P, int pp, int negatives, int add_others, int* k_all, int* npos_all, hipStream_t s);
int prompt_fill(const float* traj, const float* vis, int T, int M, int P, int pp, int negatives, int add_others, double sx, double sy,
                const int* items, int F, int ld, float* pts, int* labels, int* k_item, int* npos_item, hipStream_t s);
int mark_outside_frame(const float* traj, const float* vis_in, long n, int H, int W, float* vis_out, hipStream_t s);
int bbox_from_logits_state(const float* logits, int h, int w, int* bbox_state, int* bbox_partial, hipStream_t s);
// mask-input embedding (PromptEncoder.mask_downscaling, App. A-4) fused with "src = image_embedding + dense":
//   mask (4g x 4g) -> conv2x2s2(1->c1) LN2d GELU -> conv2x2s2(c1->c2) LN2d GELU -> conv1x1(c2->256) ; src = feat + dense
struct MaskEmbedW {
  const float *w0, *b0, *ln0w, *ln0b, *w1, *b1, *ln1w, *ln1b, *w2, *b2;  // torch layouts [out][in][kh][kw]
};
int sam_mask_embed_src(const float* mask, int g, int F, const MaskEmbedW& w, const float* feat, float* tmp0,
                       float* tmp1, float* src, hipStream_t s);
// refinement gating (sam_pt.py:809-811): active[f] &= count(bbox_cur[f]) >= 2 ; box_f[f] = bbox_cur[f]
int sam_refine_gate(int* active, const int* bbox_cur, float* box_f, int F, bool first, hipStream_t s);
// where active[f]: cur <- cand for logits (n_logits), low-res (n_low), iou and the bbox state
int sam_commit(const int* active, const float* cand_logits, float* cur_logits, long n_logits, const float* cand_low,
               float* cur_low, long n_low, const float* cand_iou, float* cur_iou, const int* cand_bbox, int* cur_bbox,
               int F, hipStream_t s);
// out[f] = (iou[f] >= thr) ? logits[f] : -inf ; score_out[f] = iou[f]   (sam_pt.py:830-837)
int sam_finalize_mask(const float* logits, const float* iou, float thr, float* out, float* score_out, long n, int F,
                      hipStream_t s);

}  // namespace sampt
