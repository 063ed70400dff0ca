// SuperGlue point tracker engine: SuperPoint (superpoint.py:148-205) once per frame up to keypoints, scores and sampled
// descriptors, and SuperGlue (superglue.py:228-283) per pair of keypoint sets.  All products run on the exact-f32 GEMM /
// implicit-GEMM convolution (gemm.hip) with their bias + ReLU epilogues; superglue.hip holds everything in between.
//
// GNN data flow.  Both keypoint sets share every weight, so they travel as ONE row block [n0 + n1]: a layer is five launches
// of GEMMs over all rows plus two attention launches (set 0 and set 1 differ only in which rows are their keys).  The
// descriptors live in columns [0, 256) of a [rows][512] buffer whose columns [256, 512) receive the attention message, so the
// concatenation in front of the layer's MLP (superglue.py:123) is never made.
#include <algorithm>

#include "engine_layers.h"

namespace sampt {

int SgEngine::init(const WeightMap& w) {
  static const char* names[8] = {"conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"};
  static const int cin[8] = {4, 64, 64, 64, 64, 128, 128, 128}, cout[8] = {64, 64, 64, 64, 128, 128, 128, 128};   // conv1a: 1 -> 4
  int rc = SAMPT_OK;
  const std::string sp_ = "superpoint.", sg_ = "superglue.";
  for (int i = 0; i < 8; ++i) rc |= load_conv(w, sp_ + names[i], cin[i], cout[i], 3, 1, 1, sp[i]);
  rc |= load_conv(w, sp_ + "convPa", 128, 256, 3, 1, 1, convPa);
  rc |= load_conv(w, sp_ + "convPb", 256, 68, 1, 1, 0, convPb);
  rc |= load_conv(w, sp_ + "convDa", 128, 256, 3, 1, 1, convDa);
  rc |= load_conv(w, sp_ + "convDb", 256, 256, 1, 1, 0, convDb);
  static const int kd[6] = {4, 32, 64, 128, 256, 256};
  for (int i = 0; i < 5; ++i) rc |= load_linear(w, sg_ + "kenc." + std::to_string(i), kd[i + 1], kd[i], kenc[i]);
  for (int l = 0; l < 18; ++l) {
    const std::string p = sg_ + "gnn." + std::to_string(l);
    rc |= load_linear(w, p + ".qkv", 768, 256, gnn[l].qkv);
    rc |= load_linear(w, p + ".merge", 256, 256, gnn[l].merge);
    rc |= load_linear(w, p + ".mlp0", 512, 512, gnn[l].mlp0);
    rc |= load_linear(w, p + ".mlp1", 256, 512, gnn[l].mlp1);
    cross[l] = l & 1;                                     // ['self', 'cross'] * 9
  }
  rc |= load_linear(w, sg_ + "final_proj", 256, 256, final_proj);
  bin_score = w.f(sg_ + "bin_score");
  if (rc != SAMPT_OK || !bin_score || !w.missing.empty()) {
    error = "SgEngine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

int SgEngine::detect(const uint8_t* frames, int T, int H, int W, const SgDetectCfg& c, float* kpts, float* kscores, float* desc,
                     int* counts_dev, int* counts_host, float* dense, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  if (T < 1 || H < 8 || W < 8 || c.cap < 1) return SAMPT_ERR_ARG;
  const int h8 = H / 8, w8 = W / 8, Hs = h8 * 8, Ws = w8 * 8, cells = h8 * w8;
  float* dmap = ws.f32((size_t)T * cells * 256);
  if (!dense) dense = ws.f32((size_t)T * Hs * Ws);
  const size_t nms_bytes = sg_nms_workspace_bytes(T, Hs, Ws);
  void* nms_ws = ws.get(nms_bytes);
  float* x0 = ws.f32((size_t)H * W * 4);
  float* A = ws.f32((size_t)H * W * 64);
  float* B = ws.f32((size_t)H * W * 64);
  float* logits = ws.f32((size_t)cells * 68);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  for (int f = 0; f < T; ++f) {
    SAMPT_TRY(sg_grey(frames + (size_t)f * 3 * H * W, 1, H, W, x0, s));
    int h = H, w = W, oh, ow;
    const float* cur = x0;
    float* bufs[2] = {A, B};
    int nb = 0;
    for (int i = 0; i < 8; ++i) {
      float* y = bufs[nb];
      SAMPT_TRY(run_conv(sp[i], cur, 1, h, w, y, 0, ACT_RELU, nullptr, oh, ow, false, s));
      cur = y, nb ^= 1;
      if ((i & 1) && i < 7) {                             // pool after conv1b, conv2b, conv3b
        float* q = bufs[nb];
        SAMPT_TRY(maxpool2x2_nhwc(cur, 1, h, w, sp[i].cout, q, s));
        cur = q, nb ^= 1, h /= 2, w /= 2;
      }
    }
    float* head = bufs[nb];                               // the other buffer: cur stays alive for both heads
    SAMPT_TRY(run_conv(convPa, cur, 1, h8, w8, head, 0, ACT_RELU, nullptr, oh, ow, false, s));
    SAMPT_TRY(run_conv(convPb, head, 1, h8, w8, logits, 0, ACT_NONE, nullptr, oh, ow, false, s));
    SAMPT_TRY(sg_scores(logits, 68, 1, h8, w8, dense + (size_t)f * Hs * Ws, s));
    SAMPT_TRY(run_conv(convDa, cur, 1, h8, w8, head, 0, ACT_RELU, nullptr, oh, ow, false, s));
    SAMPT_TRY(run_conv(convDb, head, 1, h8, w8, dmap + (size_t)f * cells * 256, 0, ACT_NONE, nullptr, oh, ow, false, s));
  }
  SAMPT_TRY(sg_nms_compact(dense, T, Hs, Ws, c.nms_radius, c.threshold, c.border, c.cap, kpts, kscores, counts_dev, nms_ws, nms_bytes, s));
  if (hipMemcpyAsync(counts_host, counts_dev, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return SAMPT_ERR_HIP;
  int most = 0;
  for (int f = 0; f < T; ++f) most = std::max(most, counts_host[f]);
  if (most > c.cap) return SAMPT_ERR_CAPACITY;            // never truncated silently: nothing beyond cap was written, nothing is sampled
  return sg_sample_descriptors(dmap, T, h8, w8, kpts, counts_dev, c.cap, most, desc, s);
}

int SgEngine::match(const float* kp0, const float* sc0, const float* d0, int n0, const float* kp1, const float* sc1, const float* d1,
                    int n1, int H, int W, int iters, float thr, int* matches0, float* mscores0, float* gnn_out, float* scores_out,
                    float* uv_out, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  if (n0 < 0 || n1 < 0 || iters < 0) return SAMPT_ERR_ARG;
  if (n0 == 0 || n1 == 0) return dry ? SAMPT_OK : sg_no_match(n0, matches0, mscores0, s);
  const int N = n0 + n1, ldS = (n1 + 3) & ~3;
  float* kin = ws.f32((size_t)N * 4);
  float* t[2] = {ws.f32((size_t)N * 256), ws.f32((size_t)N * 256)};
  float* X[2] = {ws.f32((size_t)N * 512), ws.f32((size_t)N * 512)};
  float* qkv = ws.f32((size_t)N * 768);
  float* ao = ws.f32((size_t)N * 256);
  float* hid = ws.f32((size_t)N * 512);
  float* S = ws.f32((size_t)n0 * ldS);
  float* u = ws.f32((size_t)n0 + 1);
  float* v = ws.f32((size_t)n1 + 1);
  float* max0 = ws.f32((size_t)n0);
  int* idx0 = (int*)ws.get((size_t)n0 * 4);
  int* idx1 = (int*)ws.get((size_t)n1 * 4);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  // keypoint encoder (superglue.py:83-85, :247-248): 3 (+ 1 zero) -> 32 -> 64 -> 128 -> 256 -> 256, BatchNorms folded; + descriptors
  SAMPT_TRY(sg_kenc_input(kp0, sc0, n0, H, W, kin, s));
  SAMPT_TRY(sg_kenc_input(kp1, sc1, n1, H, W, kin + (size_t)n0 * 4, s));
  const float* cur = kin;
  for (int i = 0; i < 4; ++i) {
    SAMPT_TRY(run_linear(kenc[i], cur, kenc[i].k, t[i & 1], kenc[i].n, N, ACT_RELU, nullptr, 0, s));
    cur = t[i & 1];
  }
  SAMPT_TRY(run_linear(kenc[4], cur, 256, X[0], 512, n0, ACT_NONE, d0, 256, s));
  SAMPT_TRY(run_linear(kenc[4], cur + (size_t)n0 * 256, 256, X[0] + (size_t)n0 * 512, 512, n1, ACT_NONE, d1, 256, s));
  for (int l = 0; l < 18; ++l) {
    float *x = X[l & 1], *y = X[(l + 1) & 1];
    SAMPT_TRY(run_linear(gnn[l].qkv, x, 512, qkv, 768, N, ACT_NONE, nullptr, 0, s));
    const float* src0 = qkv + (cross[l] ? (size_t)n0 * 768 : 0);       // keys of set 0: its own rows, or set 1's
    const float* src1 = qkv + (cross[l] ? 0 : (size_t)n0 * 768);
    const int m0 = cross[l] ? n1 : n0, m1 = cross[l] ? n0 : n1;
    SAMPT_TRY(sg_attention(qkv, 768, src0 + 256, src0 + 512, 768, ao, 256, n0, m0, 4, s));
    SAMPT_TRY(sg_attention(qkv + (size_t)n0 * 768, 768, src1 + 256, src1 + 512, 768, ao + (size_t)n0 * 256, 256, n1, m1, 4, s));
    SAMPT_TRY(run_linear(gnn[l].merge, ao, 256, x + 256, 512, N, ACT_NONE, nullptr, 0, s));
    SAMPT_TRY(run_linear(gnn[l].mlp0, x, 512, hid, 512, N, ACT_RELU, nullptr, 0, s));
    SAMPT_TRY(run_linear(gnn[l].mlp1, hid, 512, y, 512, N, ACT_NONE, x, 512, s));
  }
  float* fin = X[0];                                       // 18 layers: back in the first buffer
  if (gnn_out && hipMemcpy2DAsync(gnn_out, 1024, fin, 2048, 1024, N, hipMemcpyDeviceToDevice, s) != hipSuccess) return SAMPT_ERR_HIP;
  float* md = t[0];
  SAMPT_TRY(run_linear(final_proj, fin, 512, md, 256, N, ACT_NONE, nullptr, 0, s));
  {
    GemmP p = gemm_linear(md, 256, md + (size_t)n0 * 256, nullptr, S, ldS, n0, n1, 256);    // scores = mdesc0 mdesc1^T / sqrt(256)
    p.alpha = 1.0f / 16.0f;
    SAMPT_TRY(gemm_f32(p, s));
  }
  if (scores_out && hipMemcpy2DAsync(scores_out, (size_t)n1 * 4, S, (size_t)ldS * 4, (size_t)n1 * 4, n0, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return SAMPT_ERR_HIP;
  SAMPT_TRY(sg_sinkhorn(S, ldS, n0, n1, bin_score, iters, u, v, s));
  if (uv_out && (hipMemcpyAsync(uv_out, u, (size_t)(n0 + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                 hipMemcpyAsync(uv_out + n0 + 1, v, (size_t)(n1 + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess))
    return SAMPT_ERR_HIP;
  return sg_match_from_scores(S, ldS, n0, n1, u, v, thr, max0, idx0, idx1, matches0, mscores0, s);
}

}  // namespace sampt
