// Host-side "engines": fixed launch sequences over the kernels in ops.h for the three stages of the SAM-PT hot
// path.  They own no device memory: weights are caller-owned device buffers looked up by their upstream
// checkpoint key, activations live in a caller-provided workspace carved by a bump allocator.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "ops.h"

namespace sampt {

struct WeightMap {
  std::unordered_map<std::string, const void*> m;
  mutable std::string missing;
  const void* get(const std::string& k) const {
    auto it = m.find(k);
    if (it == m.end()) {
      if (missing.size() < 900) missing += k + " ";
      return nullptr;
    }
    return it->second;
  }
  const float* f(const std::string& k) const { return (const float*)get(k); }
  const half_t* h(const std::string& k) const { return (const half_t*)get(k); }
  const int* i(const std::string& k) const { return (const int*)get(k); }
  bool has(const std::string& k) const { return m.count(k) != 0; }
};

// bump allocator over the caller's workspace; with base == nullptr it only measures.
struct Arena {
  char* base;
  size_t cap, off = 0, peak = 0;
  Arena(void* b, size_t c) : base((char*)b), cap(c) {}
  void* get(size_t bytes) {
    size_t a = (off + 255) & ~(size_t)255;
    off = a + bytes;
    if (off > peak) peak = off;
    return base ? (void*)(base + a) : (void*)(uintptr_t)(a + 256);  // fake non-null address when measuring
  }
  float* f32(size_t n) { return (float*)get(n * 4); }
  half_t* f16(size_t n) { return (half_t*)get(n * 2); }
  bool ok() const { return base == nullptr || peak <= cap; }
  bool dry() const { return base == nullptr; }
};

// -------------------------------------------------------------------------------------------------
// The two layer descriptors of every engine; engine_layers.h loads them and turns them into launches.
struct ConvW {
  const float* w = nullptr;  // [Cout][KH*KW*Cin] (ci fastest), f32
  const float* b = nullptr;
  const half_t* w_hl = nullptr;  // optional: the same weights split into fp16 planes [2][Cout][K] (conv_f16x3.hip)
  int cin = 0, cout = 0, kh = 1, kw = 1, stride = 1, ph = 0, pw = 0;
  int ph_after = -1, pw_after = -1;   // >= 0: padding after the last row / column where it differs from ph / pw (TensorFlow "SAME")
};
struct LinearW {
  const float *w = nullptr, *b = nullptr;   // [N][K], [N]
  int n = 0, k = 0;
};

struct PipsEngine {
  int S = 8, stride = 4;
  int frames_f32 = 0;   // fnet input: 0 = uint8 frames, 1 = float frames in [0, 255] (PIPS++ with image_size)
  ConvW stem, conv2, conv3;
  ConvW blk[4][2][3];  // [layer][block][conv1, conv2, downsample (where conv1 has a stride)]
  // mixer
  const float *in_w, *in_b, *head_w, *head_b, *oln_w, *oln_b;
  struct MixBlk {
    const float *ln1w, *ln1b, *tw1, *tb1, *tw2, *tb2, *ln2w, *ln2b, *cw1, *cb1, *cw2, *cb2;
    const half_t* x3s[2];      // optional: the channel MLP's weights as split-fp16 operand streams for 16 / 32 hidden slices
  } mix[12];
  const float *gn_w, *gn_b, *up_wT, *up_b, *vis_w, *vis_b, *times;
  std::string error;
  int window_launches = 0;   // kernel launches of the last update() call (one window of every chain = the body of a round)

  int init(const WeightMap& w);
  int init_fnet(const WeightMap& w);   // encoder only (shared with PIPS++: same BasicEncoder, other stride)
  // frames: uint8 (nf,3,H,W).  out[l]: level-l feature maps [nf][H_l][W_l][128] f32 (H_0 = H/stride).
  int fnet(const uint8_t* frames, int nf, int H, int W, float* const out[4], Arena& ws, hipStream_t s);
  // one PIPS window per point: frame_idx (device, [n][S] ints into the pyramid), xys (device [n][2], px at frame 0),
  // feat_init (device [n][128]).  traj_out [S][n][2] px, vis_out [S][n] = sigmoid(logit).
  int update(const PyramidLevels& pyr, const int* frame_idx, int n, const float* xys, const float* feat_init, int iters,
             float* traj_out, float* vis_out, Arena& ws, hipStream_t s);
  // All chained windows of n point chains over a T-frame pyramid (pips/tracker.py:42-153), bookkeeping on the device.
  // q (device [n][3]): query (t, x, y) of each chain in ITS OWN time axis; flip (device [n] bytes): chain d-axis frame d
  // reads pyramid frame T-1-d.  q_host / flip_host: the same values on the host (which pyramid chunks a round may touch).
  // chunk_*: events recorded (on another stream) when pyramid frames [chunk_lo, chunk_hi) became valid; every round waits
  // for the chunks it can reach.  Rounds are enqueued one ahead of the device: the host learns through `flag` (pinned
  // host int32[2]) + `flag_ev[2]` that no chain is left, so this call synchronises with the stream and spends at most one
  // idle round.  traj [T][n][2] px, vis [T][n] sigmoid (device); *rounds = window rounds run.
  int track(const PyramidLevels& pyr, int T, int n, const float* q, const unsigned char* flip, const float* q_host,
            const unsigned char* flip_host, float thr0, int iters, void* const* chunk_ev, const int* chunk_lo,
            const int* chunk_hi, int nchunks, int* flag, hipEvent_t flag_ev[2], float* traj, float* vis, Arena& ws,
            hipStream_t s, int* rounds);
};

// PIPS++ (pips_plus_plus.py): the PIPS encoder at stride 8 + a 1-D ResNet over time instead of the MLP-Mixer; one call
// refines a whole chunk of S <= max_sequence_length frames for n points.
struct Pips2Engine {
  PipsEngine enc;                      // fnet only
  int stride = 8;
  ConvW first, blk[8][2];              // Conv1d(k = 3) as 3 x 1 convolutions: [Cout][3*Cin] (tap-major, ci fastest), [Cout]
  const float *dense_w, *dense_b, *omega;
  std::string error;

  int init(const WeightMap& w, int stride);
  // frame_idx (device int [n][S]): pyramid frame of chunk frame s for point pt; trajs0 (device [S][n][2] px): initial
  // trajectory (zero velocity or the previous chunk's); feats[3] (device [n][S][128] each): templates, read as the
  // feat_init of the previous chunk when have_init != 0, always written back.  trajs_out [S][n][2] px.
  int update(const PyramidLevels& pyr, const int* frame_idx, int n, int S, const float* trajs0, int have_init,
             float* const feats[3], int iters, float* trajs_out, Arena& ws, hipStream_t s);
};

// CoTracker v1: the PIPS encoder at stride 4 + the UpdateFormer (6 time + 6 space attention blocks,
// hidden 384, 8 heads) refining sliding windows of 8 frames with step 4.
struct CotEngine {
  PipsEngine enc;  // fnet only
  int S = 8, stride = 4, hidden = 384, heads = 8, depth = 6;
  struct Blk {
    const float *qkv_w, *qkv_b, *proj_w, *proj_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
  } tb[6], sb[6];
  const float *in_w, *in_b, *head_w, *head_b, *gn_w, *gn_b, *up_wT, *up_b, *vis_w, *vis_b;
  const float *times;             // [S][456] 1-D sin/cos time embedding (host-built: float64 -> f32 like upstream)
  const float *ln_one, *ln_zero;  // affine-free LayerNorm as weight 1 / bias 0
  std::string error;

  int init(const WeightMap& w);
  // One temporal direction of CoTracker.forward over T >= S model frames.  frame_map (device int [T]): pyramid frame of
  // model frame t (identity, reversed for the time-flipped pass, clamped for clips shorter than S).  Points are SORTED by
  // query frame: qt_host / qt_dev int [n] (the same values on the host — window membership is host control flow — and on
  // the device), qxy (device [n][2], px of the model's frame size).  pos_x [W0][228] / pos_y [H0][228]: the two 1-D tables
  // of the 2-D sin/cos position grid.  traj_out [T][n][2] px (0 where never written), vis_out [T][n] = sigmoid(logit)
  // (0.5 where never written).
  int track(const PyramidLevels& pyr, int T, const int* frame_map, int n, const int* qt_host, const int* qt_dev,
            const float* qxy, const float* pos_x, const float* pos_y, int iters, float* traj_out, float* vis_out, Arena& ws,
            hipStream_t s);
};

// RAFT (sam_pt/point_tracker/raft/): both encoders once per frame, then every pair-direction of the clip through the
// 4-level all-pairs correlation and `iters` recurrent updates, a chunk of pairs at a time.  All convolutions run on the
// exact-f32 implicit GEMM; weights as packed by pack.pack_raft (cnet's BatchNorms folded into its convolutions).
struct RaftEngine {
  struct Enc {
    ConvW stem, blk[3][2][3], out;          // [layer][block][conv1, conv2, downsample]
  } fnet, cnet;
  ConvW convc1, convc2, convf2, conv, zr[2], q[2], fh1, fh2, mask0, mask2;
  const float *convf1_w = nullptr, *convf1_b = nullptr;   // [98][128], [128]
  std::string error;

  int init(const WeightMap& w);
  // frames uint8 (T,3,H,W) -> flows_fwd / flows_bwd [T-1][2][H][W] (pair t: t -> t+1 and t+1 -> t), flow_low (optional)
  // [2][T-1][2][H8][W8].  np = pairs per chunk (both directions of a pair travel together).
  int flows(const uint8_t* frames, int T, int H, int W, int iters, float* fwd, float* bwd, float* flow_low, int np, Arena& ws,
            hipStream_t s);
  // the largest chunk (in pairs, <= max_pairs) whose workspace fits ws_bytes; 0 if not even one pair fits
  int plan_pairs(int T, int H, int W, int max_pairs, size_t ws_bytes);
};
// corr levels of n pairs (RaftLevels layout over n "pair-directions"): level l [n][hw][h_l w_l] = fmap1 . pool_l(fmap2)^T / 16;
// fmap1 [n][hw][256] with image stride s1 floats, pooled[l] [n][h_l w_l][256] with image stride s2[l]
int raft_corr_levels(const float* fmap1, long s1, const float* const pooled[4], const long s2[4], int n, int h8, int w8,
                     float* const out[4], hipStream_t s);

// TAPIR (sam_pt/point_tracker/tapir/; engine_tapir.hip): the pre-activation ResNet once per 256 x 256 frame, the cost-volume heads per
// (query, frame), then `iters` refinements of all (query, frame) rows through the depthwise-conv mixer.  Rows are (query, frame):
// row = q * T + t.  Weights after sam_pt_amd.pack.pack_tapir.
struct TapirEngine {
  struct Blk {
    ConvW c0, c1, sc;                      // conv_0, conv_1, shortcut_conv (first block of a group only)
    const float *n0s, *n0o, *n1s, *n1o;    // InstanceNorm scale / offset
    bool proj;
  } blk[4][2];
  ConvW stem;
  TapirHeadW head;
  const float *in_w, *in_b, *out_w, *out_b, *ln_out, *zeros;
  struct Mix {
    const float *ln1, *dw1_w, *dw1_b, *dw2_w, *dw2_b, *ln2, *up_w, *up_b, *dn_w, *dn_b;
  } mix[12];
  std::string error;
  int launches = 0;                        // nominal kernel launches of the last track() call that ran (engine_tapir.hip; dry passes leave it)

  int init(const WeightMap& w);
  // frames f32 (T,3,256,256) in [0, 1]; q (device [n][3]) = (t, x, y) in 256 x 256 pixels.  tracks [n][T][2] px, occ / expd [n][T]
  // logits; iter_out (optional) [iters + 1][n][T][4] = (x, y, occlusion, expected_dist) after the heads and after every refinement.
  // qc = queries per chunk of the refinement.
  int track(const float* frames, int T, const float* q, int n, int iters, float* tracks, float* occ, float* expd, float* iter_out,
            int qc, Arena& ws, hipStream_t s);
  // feature maps of nf frames: hires [nf][64][64][128], lowres [nf][32][32][256], both divided by their channel norm
  int backbone(const float* frames, int nf, float* hires, float* lowres, Arena& ws, hipStream_t s);
  // the largest chunk (in queries, <= n) whose workspace fits ws_bytes; 0 if not even one query fits
  int plan_queries(int T, int n, size_t ws_bytes);
};

// TapNet (sam_pt/point_tracker/tapnet/; engine_tapnet.hip): TSM-ResNet-18 up to unit 2 over ALL frames of the clip per launch (BatchNorm
// in inference mode is a per-channel affine), then the query features and the cost-volume heads.  Weights after sam_pt_amd.pack.pack_tapnet.
struct TapnetEngine {
  struct Blk {
    ConvW c0, c2, sc;                      // conv_0, conv_2, shortcut_conv (block 0 of a unit only)
    const float *a0, *b0, *a1, *b1;        // the two folded BatchNorms
    bool proj;
    int shift;                             // channels shifted each way on the way to conv_0
  } blk[3][2];
  ConvW stem;
  TapirHeadW head;
  std::string error;
  int stem_chunk = 8;                      // frames per pass of the stem and the max-pool (the 128 x 128 x 64 map exists for these only)
  int launches = 0;                        // nominal kernel launches of the last track() that ran (engine_tapnet.hip; dry passes leave it)

  int init(const WeightMap& w);
  // frames f32 (T,3,256,256) in [0, 1]; q (device [n][3]) = (t, x, y) in 256 x 256 pixels.  tracks [n][T][2] px, occ [n][T] logits.
  int track(const float* frames, int T, const float* q, int n, float* tracks, float* occ, Arena& ws, hipStream_t s);
  // grid [T][32][32][256], channel-normalised.  stages (optional, each entry optional): the max-pooled stem [T][64][64][64] and the
  // outputs of units 0, 1, 2 ([T][64][64][64], [T][32][32][128], [T][32][32][256]), copied out for tests
  int backbone(const float* frames, int T, float* grid, float* const* stages, Arena& ws, hipStream_t s);
};

// -------------------------------------------------------------------------------------------------
// SuperPoint + SuperGlue (engine_superglue.hip).  Weights after sam_pt_amd.pack.pack_superglue.
struct SgDetectCfg {
  int nms_radius = 4, border = 4, cap = 0;
  float threshold = 0.005f;
};
struct SgEngine {
  ConvW sp[8], convPa, convPb, convDa, convDb;    // convPb: 65 outputs zero-padded to 68
  LinearW kenc[5];
  struct Layer { LinearW qkv, merge, mlp0, mlp1; } gnn[18];
  int cross[18];
  LinearW final_proj;
  const float* bin_score = nullptr;
  std::string error;

  int init(const WeightMap& w);
  // frames uint8 (T,3,H,W) -> kpts [T][cap][2], kscores [T][cap], desc [T][cap][256], counts_dev [T] and counts_host [T] (one
  // stream synchronisation); dense (optional) [T][8 (H/8)][8 (W/8)] score maps.  SAMPT_ERR_WORKSPACE... see c_abi for the codes
  int detect(const uint8_t* frames, int T, int H, int W, const SgDetectCfg& c, float* kpts, float* kscores, float* desc,
             int* counts_dev, int* counts_host, float* dense, Arena& ws, hipStream_t s);
  // one pair: keypoints / scores / descriptors of both images -> matches0 [n0], mscores0 [n0]; optional copies for tests:
  // gnn_out [n0 + n1][256] (the descriptors after the last layer), scores_out [n0][n1] (before Sinkhorn), uv_out [n0 + 1 + n1 + 1]
  int match(const float* kp0, const float* sc0, const float* d0, int n0, const float* kp1, const float* sc1, const float* d1, int n1,
            int H, int W, int iters, float thr, int* matches0, float* mscores0, float* gnn_out, float* scores_out, float* uv_out,
            Arena& ws, hipStream_t s);
};

// -------------------------------------------------------------------------------------------------
struct VitConfig {
  int D = 768, depth = 12, heads = 12, grid = 64, window = 14, patch = 16, out_chans = 256, mlp_ratio = 4;
  int img = 1024;
  int global_mask = 0;  // bit i set -> block i uses global attention (depth <= 32)
  int f16 = 1;          // 1: fp16 MFMA GEMMs + flash attention ; 0: exact fp32 everywhere
  float mean[3] = {123.675f, 116.28f, 103.53f}, stdv[3] = {58.395f, 57.12f, 57.375f};
};

struct VitEngine {
  VitConfig c;
  struct Blk {
    const float *ln1w, *ln1b, *ln2w, *ln2b, *qkv_b, *proj_b, *b1, *b2, *rel_h, *rel_w;
    const half_t* rel_ops = nullptr;   // optional: rel_h / rel_w as fp16 MFMA operand images (pack.rel_pos_operand_images)
    const void *qkv_w, *proj_w, *w1, *w2;  // f16 or f32 depending on c.f16
    const half_t* qkv_b16 = nullptr;       // 16-bit modes: the qkv bias as one row of the qkv matrix's format (fp16 / x3 row)
  };
  std::vector<Blk> blk;
  const void *patch_w, *neck0_w, *neck2_w;
  const half_t *patch_hl = nullptr, *neck0_hl = nullptr, *neck2_hl = nullptr;   // split-fp16 planes (fast mode)
  const float *patch_b, *pos, *neck1w, *neck1b, *neck3w, *neck3b;
  const int* win_rows;  // [Bmax * nwin * window^2] -> token row or -1
  const int* win_inv;   // [Bmax * grid^2] token row -> window-order row
  const int* win_pad;   // [Bmax * npad] window-order rows that are zero padding
  const int* win_inv_live[8] = {};   // the same two maps for the compact live grids of k+1 window rows x grid columns
  const int* win_pad_live[8] = {};
  int win_rows_batches = 0;
  std::string error;
  // Optional in-situ timing of the fp16 GEMM launches (bench.py's roofline): HIP events on the launching stream around
  // every gemm_f16 call of encode() while `profiling` is set; collected (and destroyed) by profile_end().
  struct GemmEv {
    hipEvent_t a, b;
    double flop;
  };
  mutable std::vector<GemmEv> prof;
  bool profiling = false;
  // persistent workgroups per XCD of the fp16 GEMMs (0 = one per CU).  A 512-thread, 128-KiB GEMM workgroup owns its CU, so
  // a caller that runs latency-bound kernels on another stream beside the encoder (the point tracker) asks for fewer.
  int gemm_wgs = 0;
  // per launch kind (0 qkv, 1 proj, 2 fc1, 3 fc2): overrides gemm_wgs when > 0 (tile counts of the four shapes quantise
  // differently on a given number of workgroups: sampt_vit_set_gemm_workgroups_kind)
  int gemm_wgs_kind[4] = {0, 0, 0, 0};
  // fp16 mode: the qkv GEMM writes, and the attention kernel reads, the head-major matrix [3][heads][rows][hd] instead of
  // token-major rows (GemmP::hm_hd, FlashPad::head_major; sampt_vit_set_attention_head_major: 0 = token-major).  Bitwise the same
  // results; the default by measurement (k_flash_f16).
  int attn_head_major = 1;
  // Calibration of the fp16 mode's static bias correction (sampt_vit_calibrate): while set, every block GEMM of encode() also
  // writes the column means of its A operand (over the real tokens) to calib[(block * 4 + kind) * calib_ld + k].
  float* calib = nullptr;
  int calib_ld = 0;
  mutable int cur_blk = 0;
  int profile_end(double* flop, double* ms, int* launches);

  int init(const WeightMap& w, const VitConfig& cfg, int win_rows_batches);
  // frames: uint8 (B,3,H,W) if chw else (B,H,W,3); features out: [B][grid*grid][out_chans] f32 (NHWC);
  // interm_out (optional): [B][grid*grid][D] f32 = token stream after the first global-attention block (HQ-SAM's
  // interm_embeddings[0])
  // dead_mode 0: full computation.  1: B == 1, computes `dead_cache` [(grid - live_rows) * grid][D] f32 (the residual
  // stream of the frame-independent padding tokens at the input of the first global block) and returns.  2: blocks before
  // the first global one run on the live rows only, the dead rows come from `dead_cache` (see encode()).
  int encode(const uint8_t* frames, int chw, int B, int H, int W, float* features, float* interm_out, Arena& ws,
             hipStream_t s, float* dead_cache = nullptr, int dead_mode = 0);
  int live_rows(int H, int W) const;   // token rows that depend on the frame before the first global block (grid = all)
};

// -------------------------------------------------------------------------------------------------
// TinyViT (MobileSAM / Light HQ-SAM image encoder; engine_tinyvit.hip).  Weights after sam_pt_amd.pack.pack_tinyvit: every BatchNorm
// folded into its convolution, dense layers with split-fp16 planes, depthwise weights [3][3][C].  One arithmetic: fp32 grade.
struct TinyVitConfig {
  int img = 1024, out_chans = 256, mlp_ratio = 4, expand = 4;
  int dims[4] = {64, 128, 160, 320}, depths[4] = {2, 2, 6, 2}, heads[4] = {2, 4, 5, 10}, windows[4] = {7, 7, 14, 7};
  float mean[3] = {123.675f, 116.28f, 103.53f}, stdv[3] = {58.395f, 57.12f, 57.375f};
};

struct TinyVitEngine {
  TinyVitConfig c;
  struct DwW {
    const float *w = nullptr, *b = nullptr;    // [3][3][C], [C]
  };
  struct MBConv {
    ConvW conv1, conv3;
    DwW conv2;
  };
  struct Merge {                               // PatchMerging: 1 x 1, depthwise 3 x 3 of stride `stride`, 1 x 1
    ConvW conv1, conv3;
    DwW conv2;
    int stride = 2;
  };
  struct Blk {
    const float *ln1w, *ln1b, *ln2w, *ln2b, *table, *pad_qkv;
    ConvW qkv, proj, fc1, fc2;                 // the Linears as 1 x 1 convolutions over the token map
    DwW local;
  };
  ConvW stem0, stem2;
  std::vector<MBConv> mb;
  Merge merge[3];
  std::vector<Blk> blk[4];                     // [1..3] used
  int res[4] = {0, 0, 0, 0};                   // side of the map layer i works on
  const half_t *neck0_hl = nullptr, *neck2_hl = nullptr;
  const float *neck0_w = nullptr, *neck2_w = nullptr, *neck1w, *neck1b, *neck3w, *neck3b;
  int max_batch = 0;
  std::string error;

  int init(const WeightMap& w, const TinyVitConfig& cfg, int max_batch);
  int grid() const { return res[3]; }
  // frames: uint8 (B,3,H,W) if chw else (B,H,W,3), H, W <= img; features out [B][grid^2][out_chans] f32; interm_out (optional)
  // [B][grid^2][dims[2]] = the token map that enters layers.2 (Light HQ-SAM's interm_embeddings[0]).  stages (optional, each entry
  // optional): the outputs of patch_embed and of layers 0..3 (after their downsample), copied out for tests; stage_ev (optional): 7
  // events recorded on s before patch_embed, after it, after each layer and after the neck.  No host synchronisation.
  int encode(const uint8_t* frames, int chw, int B, int H, int W, float* features, float* interm_out, float* const* stages,
             hipEvent_t* stage_ev, Arena& ws, hipStream_t s);
};

// -------------------------------------------------------------------------------------------------
struct DecConfig {
  int grid = 64, C = 256, heads = 8, depth = 2, mlp = 2048, img = 1024;
  int vit_dim = 0;  // > 0: HQ-SAM decoder (MaskDecoderHQ) fed by a ViT of that width
};

struct DecEngine {
  DecConfig c;
  int max_frames = 1;  // frame-batch capacity of the pixel-shuffle row maps
  struct Attn {
    const float *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob;
    int inner;
  };
  struct Layer {
    Attn self, t2i, i2t;
    const float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b, *n4w, *n4b, *m1w, *m1b, *m2w, *m2b;
  } layer[4];
  Attn fin;
  const float *nfw, *nfb;
  const float *out_tokens;                       // [5][256] = iou_token, mask_tokens
  const float *gauss, *point_emb, *not_a_point, *no_mask, *dense_pe;
  MaskEmbedW me;
  const float *up0_w, *up0_b, *upln_w, *upln_b, *up1_w, *up1_b;  // ConvT weights packed [(dy,dx)][cout][cin]
  const half_t *up0_hl = nullptr, *up1_hl = nullptr;             // their split-fp16 planes [2][4*cout][cin] (optional)
  // Fused image-side projections (pack.py): per layer W = [t2i.k_proj; t2i.v_proj; i2t.q_proj] (384 x C), bias likewise,
  // pe = dense_pe @ [Wk; 0; Wq]^T (P x 384) — (keys + pe) W^T = keys W^T + pe W^T, so the positional term is a constant
  // added in the epilogue and the image tokens are read ONCE per layer; final attention: [k_proj; v_proj] (256 x C).
  struct FusedProj {
    const float *w = nullptr, *b = nullptr, *pe = nullptr;
    const half_t* hl = nullptr;
    int n = 0;
  } kvq[4], fin_kv;
  const int *up0_map, *up1_map;                  // pixel-shuffle row maps [4][max_frames*g*g], [4][max_frames*4*g*g]
  const float *hyp_w[3], *hyp_b[3], *iou_w[3], *iou_b[3];         // hypernetwork MLP 0 and IoU head
  const float *hypx_w[3][3], *hypx_b[3][3];                       // hypernetwork MLPs 1..3 (multimask_output=True)
  // Batch-invariant decoding (sampt_dec_set_batch_invariant): an item's result does not depend on what shares its launch sequence.
  // Every plain f32 product takes GemmP::row_invariant, attn_t2i splits its keys by Nk alone, and the image / token side of
  // L::lin is told apart by the rows of one item.  Off: the routes by total row count, bit for bit as before.
  bool batch_invariant = false;
  bool multimask = false;  // next decode(): SAM's multimask_output=True — 3 masks / IoUs of mask tokens 1..3 (F == 1, SAM only)
  // HQ-SAM extras (c.vit_dim > 0): out_tokens has a 6th row (hf_token); ConvT weights packed like up0/up1
  struct HqW {
    const float *mlp_w[3], *mlp_b[3];                             // hf_mlp
    const float *cv0_w, *cv0_b, *cvln_w, *cvln_b, *cv1_w, *cv1_b;  // compress_vit_feat  (vit_dim -> C -> C/8)
    const float *ee0_w, *ee0_b, *eeln_w, *eeln_b, *ee1_w, *ee1_b;  // embedding_encoder  (C -> C/4 -> C/8)
    const float *mf0_w, *mf0_b, *mfln_w, *mfln_b, *mf1_w, *mf1_b;  // embedding_maskfeature: conv3x3 [Cout][9*Cin]
    const half_t *mf0_hl = nullptr, *mf1_hl = nullptr;             // their split-fp16 planes (optional)
    const half_t *cv0_hl = nullptr, *cv1_hl = nullptr, *ee0_hl = nullptr, *ee1_hl = nullptr;
  } hq;
  // optional (opt-in, pack.pack_decoder with SAMPT_DEC_F16X3=1): split-fp16 planes [2][N][K] of the attention projection
  // weights, keyed by the f32 weight pointer; projections over the image tokens (M = F*g*g rows) then run on the fp16
  // matrix pipe at fp32 grade (conv_f16x3.hip as a 1x1 convolution over an [1][M][1][K] image)
  std::unordered_map<const float*, const half_t*> w_hl;
  std::string error;

  bool is_hq() const { return c.vit_dim > 0; }
  int n_out() const { return is_hq() ? 6 : 5; }
  int init(const WeightMap& w, const DecConfig& cfg);
  // HQ-SAM per-frame features [F][16*g*g][C/8] = embedding_encoder(features) + compress_vit_feat(interm)
  // (features [F][g*g][C], interm [F][g*g][vit_dim]); computed once per frame, shared by all decode passes.
  int hq_features(int F, const float* features, const float* interm, float* out, Arena& ws, hipStream_t s);
  // One predict_torch pass (multimask_output=False, return_logits=True) for F frames with the same prompt shape.
  // features [F][g*g][256]; pts [F][ld_pts][2], labels [F][ld_pts] (first k used); box [F][4] or null;
  // mask_in [F][4g][4g] or null.  logits_out [F][oh][ow], iou_out [F], low_out [F][4g][4g];
  // bbox_out: optional int [F][5] state of logits > 0.  hq_feat: hq_features() output (HQ-SAM) or null (SAM).
  // k_item: optional device int [F]: item f only uses its first min(k, k_item[f]) points (ragged batch: its tokens are
  // packed in front, padding rows are masked out of every attention).
  int decode(int F, const float* features, const float* hq_feat, const float* pts, const int* labels, int k,
             const int* k_item, int ld_pts, const float* box, const float* mask_in, int in_h, int in_w, int oh, int ow, float* logits_out, float* iou_out, float* low_out,
             int* bbox_out, Arena& ws, hipStream_t s);
  // The whole per-(frame, object) chain of SamPt.predict_mask (sam_pt.py:760-837) for F frames, no host sync:
  // [positives-only pass when n_pos_first >= 0] -> all-points pass (+ mask) -> R box-refinement passes gated per frame
  // on device -> IoU-threshold rejection.  final_logits [F][oh][ow], score_out [F].
  // k_item / npos_item: optional per-item point counts (all points / leading positives) of a ragged batch.
  int track_decode(int F, const float* features, const float* hq_feat, const float* pts, const int* labels, int k,
                   const int* k_item, const int* npos_item, int ld_pts, int n_pos_first, int R, float iou_thr, int in_h, int in_w, int oh, int ow, float* final_logits, float* score_out,
                   Arena& ws, hipStream_t s);
  // n single-image point prompts (pts [n][k][2], labels [n][k], k >= 1) against ONE image: features [g*g][C], hq_feat
  // [16*g*g][C/8] or null.  low_out [n][m][4g][4g], iou_out [n][m]; m = 3 for SAM with multi, else 1 (HQ-SAM with multi: the
  // SAM mask of the best-IoU token + the HQ mask).  Image-side work that does not depend on the prompt runs once per call.
  int decode_points(int n, const float* features, const float* hq_feat, const float* pts, const int* labels, int k, bool multi,
                    float* low_out, float* iou_out, Arena& ws, hipStream_t s);
};

}  // namespace sampt
