// PIPS++ engine (row f4): whole-chunk iterative refinement (pips_plus_plus.py:436-546) on top of the PIPS kernels — the
// feature pyramid, the fused local correlation sampler (three templates per iteration) and the bilinear feature gather
// are shared; the DeltaBlock (1-D ResNet over time, :263-342) runs as implicit-GEMM convolutions over [n][S][1][C].
#include "engine_layers.h"

namespace sampt {

static const int kBlocks[8][2] = {{128, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 512}, {512, 512}, {512, 1024},
                                  {1024, 1024}};

int Pips2Engine::init(const WeightMap& w, int stride_) {
  stride = stride_;
  enc.stride = stride_;
  int rc = enc.init_fnet(w);
  if (rc != SAMPT_OK) {
    error = enc.error;
    return rc;
  }
  // Conv1dPad(k = 3, "same") over the S frames of every point, as a 3 x 1 convolution over an [n][S][1][C] image:
  // y[pt*S+s][co] = b + sum_{d,ci} x[pt*S+s+d-1][ci] W[co][d][ci]
  load_conv(w, "delta_block.first_block_conv.conv", 720, 128, 3, 1, 1, 1, 0, first);   // 718 input channels zero-padded to 720
  for (int i = 0; i < 8; ++i) {
    const std::string p = "delta_block.basicblock_list." + std::to_string(i);
    load_conv(w, p + ".conv1.conv", kBlocks[i][0], kBlocks[i][1], 3, 1, 1, 1, 0, blk[i][0]);
    load_conv(w, p + ".conv2.conv", kBlocks[i][1], kBlocks[i][1], 3, 1, 1, 1, 0, blk[i][1]);
  }
  dense_w = w.f("delta_block.dense.weight"), dense_b = w.f("delta_block.dense.bias");
  omega = w.f("__omega");
  if (!w.missing.empty()) {
    error = "Pips2Engine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

int Pips2Engine::update(const PyramidLevels& pyr, const int* frame_idx, int n, int S, const float* trajs0, int have_init,
                        float* const feats[3], int iters, float* trajs_out, Arena& ws, hipStream_t s) {
  if (n <= 0 || S <= 0 || iters <= 0) return SAMPT_ERR_ARG;
  const size_t R = (size_t)n * S;
  const int LDX = 720;
  float* coords = ws.f32((size_t)S * n * 2);
  float* bak = ws.f32((size_t)n * 2);
  float* x = ws.f32(R * LDX);
  float* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = ws.f32(R * 1024);
  float* delta = ws.f32(R * 2);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (ws.dry()) return SAMPT_OK;
  const int H = pyr.H[0], W = pyr.W[0];
  int oh, ow;
  SAMPT_TRY(pips2_init(trajs0, pyr.base[0], H, W, frame_idx, (float)stride, S, n, have_init, coords, bak, feats[0], feats[1],
                       feats[2], s));
  for (int it = 0; it < iters; ++it) {
    if (it >= 1) SAMPT_TRY(pips2_templates(pyr.base[0], H, W, frame_idx, coords, S, n, feats[1], feats[2], s));
    for (int t = 0; t < 3; ++t) SAMPT_TRY(pips_corr_sample(pyr, frame_idx, S, n, 128, feats[t], coords, x, LDX, 196 * t, s));
    SAMPT_TRY(pips2_build_input(coords, omega, S, n, x, LDX, s));
    // ---- DeltaBlock: h = relu(conv(x)); 8 residual blocks; relu; dense
    float *h = buf[0], *a = buf[1], *b = buf[2], *c = buf[3];
    SAMPT_TRY(run_conv(first, x, n, S, 1, h, 0, ACT_RELU, nullptr, oh, ow, false, s));
    for (int i = 0; i < 8; ++i) {
      const int cin = kBlocks[i][0], cout = kBlocks[i][1];
      const float* in1 = h;
      if (i > 0) {                                   // norm1 + relu1 (skipped in the first block, :80-86)
        SAMPT_TRY(instnorm1d_relu(h, a, n, S, cin, s));
        in1 = a;
      }
      SAMPT_TRY(run_conv(blk[i][0], in1, n, S, 1, b, 0, ACT_NONE, nullptr, oh, ow, false, s));
      SAMPT_TRY(instnorm1d_relu(b, b, n, S, cout, s));
      const bool fused_skip = cin == cout && i < 7;  // same width: the skip is the GEMM's residual operand
      SAMPT_TRY(run_conv(blk[i][1], b, n, S, 1, c, 0, ACT_NONE, fused_skip ? h : nullptr, oh, ow, false, s));
      if (!fused_skip) SAMPT_TRY(add_chanpad(c, h, (long)R, cin, cout, i == 7 ? 1 : 0, s));   // last block: + final_relu
      float* t = h;
      h = c, c = t;
    }
    SAMPT_TRY(run_linear(h, 1024, dense_w, dense_b, delta, 2, (int)R, 2, 1024, ACT_NONE, nullptr, 0, s));
    SAMPT_TRY(pips2_apply_delta(delta, bak, (float)stride, S, n, it == iters - 1, coords, trajs_out, s));
  }
  return SAMPT_OK;
}

}  // namespace sampt
