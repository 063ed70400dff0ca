// TinyViT image encoder of MobileSAM / Light HQ-SAM (ChaoningZhang/MobileSAM tiny_vit_sam.py) as a fixed launch sequence, B frames per
// call and one launch per operator for the whole batch.  Token maps are NHWC f32 [B][side^2][C] throughout, so a Linear over tokens and a
// 1 x 1 convolution over the map are the same launch and the neck's output is directly the decoder's image-token matrix.
//
//   patch_embed  preprocess -> conv 3x3 s2 (Cin 3 zero-padded to 4: exact-f32 implicit GEMM) + GELU -> conv 3x3 s2 (split-fp16)
//   layers.0     MBConv x depths[0]: 1x1 + GELU -> depthwise 3x3 + GELU -> 1x1 + shortcut (epilogue) -> GELU (one elementwise pass: the
//                GEMM epilogue's activation comes BEFORE its residual); then PatchMerging: 1x1 + GELU -> depthwise 3x3 stride s + GELU -> 1x1
//   layers.1..3  TinyViTBlock x depths[i]: LayerNorm -> qkv -> window attention (no padded map: tinyvit.hip) -> proj + residual (epilogue)
//                -> depthwise 3x3 (no residual, no activation) -> LayerNorm -> fc1 + GELU -> fc2 + residual (epilogue); PatchMerging for i < 3
//   neck         sam_neck (engine_layers.h), the ViT engine's
// Every BatchNorm is folded into its convolution by the packer.  Every dense layer but the stem runs on the split-fp16 path where the
// packer delivered planes (fp32 grade: three fp16 MFMAs per product, f32 accumulate), else on the exact-f32 implicit GEMM.
// A row of a GEMM, a LayerNorm row, a depthwise output and an attention window do not depend on what else shares the launch, so a frame's
// result is the same bits whatever batch it travels in.
#include <algorithm>

#include "engine_layers.h"

namespace sampt {

static int merge_stride(int out_dim) { return (out_dim == 320 || out_dim == 448 || out_dim == 576) ? 1 : 2; }   // upstream's rule, by value

static int load_dw(const WeightMap& w, const std::string& name, TinyVitEngine::DwW& d) {
  d.w = w.f(name + ".weight"), d.b = w.f(name + ".bias");
  return (d.w && d.b) ? SAMPT_OK : SAMPT_ERR_ARG;
}

int TinyVitEngine::init(const WeightMap& w, const TinyVitConfig& cfg, int mb_) {
  c = cfg, max_batch = mb_;
  const std::string e = "image_encoder.";
  for (int i = 0; i < 4; ++i) {
    if (c.dims[i] < 32 || c.dims[i] % 32 || c.depths[i] < 1 || c.heads[i] < 1) {
      error = "TinyVitEngine: embed_dims must be multiples of 32 and depths / num_heads positive";
      return SAMPT_ERR_ARG;
    }
    if (i > 0 && c.dims[i] != 32 * c.heads[i]) {
      error = "TinyVitEngine: embed_dims[i] / num_heads[i] must be 32 (the head width of every published TinyViT)";
      return SAMPT_ERR_UNSUPPORTED;
    }
    if (i > 0 && (c.windows[i] < 1 || c.windows[i] > 14)) {
      error = "TinyVitEngine: window_sizes must be 1 .. 14";
      return SAMPT_ERR_UNSUPPORTED;
    }
  }
  if (c.img < 32 || c.img % 32 || c.out_chans % 32 || c.mlp_ratio < 1 || c.expand < 1 || max_batch < 1) {
    error = "TinyVitEngine: img_size and out_chans must be multiples of 32";
    return SAMPT_ERR_ARG;
  }
  res[0] = c.img / 4;
  for (int i = 0; i < 3; ++i) {
    merge[i].stride = merge_stride(c.dims[i + 1]);
    if (merge[i].stride == 2 && res[i] % 2) {
      error = "TinyVitEngine: img_size does not divide down the stages";
      return SAMPT_ERR_ARG;
    }
    res[i + 1] = res[i] / merge[i].stride;
  }
  // the convolutions index their maps with int
  if ((double)max_batch * res[0] * res[0] * c.dims[0] * c.expand >= 2147483648.0 || (double)max_batch * c.img * c.img * 4 >= 2147483648.0) {
    error = "TinyVitEngine: max_batch x the stage-0 hidden map exceeds 2^31 elements";
    return SAMPT_ERR_ARG;
  }
  int rc = load_conv(w, e + "patch_embed.seq.0", 4, c.dims[0] / 2, 3, 2, 1, stem0);
  rc |= load_conv(w, e + "patch_embed.seq.2", c.dims[0] / 2, c.dims[0], 3, 2, 1, stem2);
  mb.resize(c.depths[0]);
  const int hid0 = c.dims[0] * c.expand;
  for (int b = 0; b < c.depths[0]; ++b) {
    const std::string p = e + "layers.0.blocks." + std::to_string(b);
    rc |= load_conv(w, p + ".conv1", c.dims[0], hid0, 1, 1, 0, mb[b].conv1);
    rc |= load_dw(w, p + ".conv2", mb[b].conv2);
    rc |= load_conv(w, p + ".conv3", hid0, c.dims[0], 1, 1, 0, mb[b].conv3);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string p = e + "layers." + std::to_string(i) + ".downsample";
    rc |= load_conv(w, p + ".conv1", c.dims[i], c.dims[i + 1], 1, 1, 0, merge[i].conv1);
    rc |= load_dw(w, p + ".conv2", merge[i].conv2);
    rc |= load_conv(w, p + ".conv3", c.dims[i + 1], c.dims[i + 1], 1, 1, 0, merge[i].conv3);
  }
  for (int i = 1; i < 4; ++i) {
    const int C = c.dims[i];
    blk[i].resize(c.depths[i]);
    for (int b = 0; b < c.depths[i]; ++b) {
      const std::string p = e + "layers." + std::to_string(i) + ".blocks." + std::to_string(b);
      Blk& k = blk[i][b];
      k.ln1w = w.f(p + ".attn.norm.weight"), k.ln1b = w.f(p + ".attn.norm.bias");
      k.ln2w = w.f(p + ".mlp.norm.weight"), k.ln2b = w.f(p + ".mlp.norm.bias");
      k.table = w.f(p + ".attn.attention_biases"), k.pad_qkv = w.f(p + ".attn.pad_qkv");
      rc |= load_conv(w, p + ".attn.qkv", C, 3 * C, 1, 1, 0, k.qkv);
      rc |= load_conv(w, p + ".attn.proj", C, C, 1, 1, 0, k.proj);
      rc |= load_dw(w, p + ".local_conv", k.local);
      rc |= load_conv(w, p + ".mlp.fc1", C, c.mlp_ratio * C, 1, 1, 0, k.fc1);
      rc |= load_conv(w, p + ".mlp.fc2", c.mlp_ratio * C, C, 1, 1, 0, k.fc2);
    }
  }
  neck0_hl = w.has(e + "neck.0.weight_hl") ? w.h(e + "neck.0.weight_hl") : nullptr;
  neck2_hl = w.has(e + "neck.2.weight_khwc_hl") ? w.h(e + "neck.2.weight_khwc_hl") : nullptr;
  neck0_w = neck0_hl ? nullptr : w.f(e + "neck.0.weight");
  neck2_w = neck2_hl ? nullptr : w.f(e + "neck.2.weight_khwc");
  neck1w = w.f(e + "neck.1.weight"), neck1b = w.f(e + "neck.1.bias");
  neck3w = w.f(e + "neck.3.weight"), neck3b = w.f(e + "neck.3.bias");
  if (rc != SAMPT_OK || !w.missing.empty()) {
    error = "TinyVitEngine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

namespace {
// a dense layer over the token map x [n][side^2][cin] -> y [n][side^2][cout] (+ act) (+ res)
int dense(const ConvW& cw, const float* x, int n, int side, float* y, int act, const float* res, bool dry, hipStream_t s) {
  int oh, ow;
  return run_conv(cw, x, n, side, side, y, 0, act, res, oh, ow, dry, s);
}
}  // namespace

int TinyVitEngine::encode(const uint8_t* frames, int chw, int B, int H, int W, float* features, float* interm_out, float* const* stages,
                          hipEvent_t* stage_ev, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  if (B < 1 || B > max_batch || H < 1 || W < 1 || H > c.img || W > c.img) {
    error = "TinyVitEngine::encode: 1 <= B <= max_batch frames of at most img_size x img_size";
    return SAMPT_ERR_ARG;
  }
  const int r0 = res[0], g = res[3];
  const size_t tok = (size_t)B * r0 * r0 * c.dims[0];            // the map patch_embed and layers.0 work on
  size_t tok_max = tok;                                          // the largest map any layer hands to the next
  for (int i = 1; i < 4; ++i) tok_max = std::max(tok_max, (size_t)B * res[i] * res[i] * c.dims[i]);
  float* cur = ws.f32(tok_max);
  float* nxt = ws.f32(tok_max);
  const size_t mark = ws.off;
  auto event = [&](int i) -> int {
    if (dry || !stage_ev) return SAMPT_OK;
    return hipEventRecord(stage_ev[i], s) == hipSuccess ? SAMPT_OK : SAMPT_ERR_HIP;
  };
  auto copy_out = [&](float* dst, const float* src, size_t elems) -> int {
    if (dry || !dst) return SAMPT_OK;
    const hipError_t e = hipMemcpyAsync(dst, src, elems * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      set_error("TinyVitEngine::encode: hipMemcpyAsync", e);
      return SAMPT_ERR_HIP;
    }
    return SAMPT_OK;
  };
  int oh, ow;
  SAMPT_TRY(event(0));
  // ---- patch_embed
  {
    float* x0 = ws.f32((size_t)B * c.img * c.img * 4);
    float* s1 = ws.f32((size_t)B * (c.img / 2) * (c.img / 2) * stem0.cout);
    if (!dry) SAMPT_TRY(tinyvit_preprocess(frames, chw, B, H, W, c.img, c.mean, c.stdv, x0, s));
    SAMPT_TRY(run_conv(stem0, x0, B, c.img, c.img, s1, 0, ACT_GELU, nullptr, oh, ow, dry, s));
    if (oh != c.img / 2 || ow != c.img / 2) return SAMPT_ERR_ARG;
    SAMPT_TRY(run_conv(stem2, s1, B, oh, ow, cur, 0, ACT_NONE, nullptr, oh, ow, dry, s));
    if (oh != r0 || ow != r0) return SAMPT_ERR_ARG;
  }
  SAMPT_TRY(copy_out(stages ? stages[0] : nullptr, cur, tok));
  SAMPT_TRY(event(1));
  // PatchMerging of layer i: cur [B][side^2][dims[i]] -> cur [B][(side / stride)^2][dims[i + 1]]
  auto downsample = [&](int i, int& side) -> int {
    const Merge& m = merge[i];
    const int C = c.dims[i + 1], os = side / m.stride;
    ws.off = mark;
    float* h1 = ws.f32((size_t)B * side * side * C);
    float* h2 = ws.f32((size_t)B * os * os * C);
    SAMPT_TRY(dense(m.conv1, cur, B, side, h1, ACT_GELU, nullptr, dry, s));
    if (!dry) SAMPT_TRY(tinyvit_dwconv3x3(h1, m.conv2.w, m.conv2.b, h2, B, side, side, C, m.stride, 1, s));
    SAMPT_TRY(dense(m.conv3, h2, B, os, nxt, ACT_NONE, nullptr, dry, s));
    std::swap(cur, nxt);
    side = os;
    return SAMPT_OK;
  };
  // ---- layers.0: MBConv blocks
  int side = r0;
  {
    const int C = c.dims[0], hid = C * c.expand;
    ws.off = mark;
    float* h1 = ws.f32((size_t)B * side * side * hid);
    float* h2 = ws.f32((size_t)B * side * side * hid);
    for (const MBConv& m : mb) {
      SAMPT_TRY(dense(m.conv1, cur, B, side, h1, ACT_GELU, nullptr, dry, s));
      if (!dry) SAMPT_TRY(tinyvit_dwconv3x3(h1, m.conv2.w, m.conv2.b, h2, B, side, side, hid, 1, 1, s));
      SAMPT_TRY(dense(m.conv3, h2, B, side, nxt, ACT_NONE, cur, dry, s));       // + shortcut
      if (!dry) SAMPT_TRY(tinyvit_gelu(nxt, nxt, (long)tok, s));
      std::swap(cur, nxt);
    }
    SAMPT_TRY(downsample(0, side));
  }
  SAMPT_TRY(copy_out(stages ? stages[1] : nullptr, cur, (size_t)B * side * side * c.dims[1]));
  SAMPT_TRY(event(2));
  // ---- layers.1..3: TinyViT blocks
  for (int i = 1; i < 4; ++i) {
    const int C = c.dims[i];
    const long M = (long)B * side * side;
    if (side != res[i]) return SAMPT_ERR_ARG;
    if (i == 2) SAMPT_TRY(copy_out(interm_out, cur, (size_t)M * C));
    ws.off = mark;
    float* xn = ws.f32((size_t)M * C);
    float* qkv = ws.f32((size_t)M * 3 * C);
    float* att = ws.f32((size_t)M * C);
    float* hid = ws.f32((size_t)M * c.mlp_ratio * C);
    for (const Blk& k : blk[i]) {
      if (!dry) SAMPT_TRY(layernorm_rows(cur, k.ln1w, k.ln1b, xn, M, C, 1e-5f, nullptr, 0, ACT_NONE, s));
      SAMPT_TRY(dense(k.qkv, xn, B, side, qkv, ACT_NONE, nullptr, dry, s));
      if (!dry) SAMPT_TRY(tinyvit_window_attention(qkv, k.table, k.pad_qkv, att, B, side, side, c.heads[i], c.windows[i], s));
      SAMPT_TRY(dense(k.proj, att, B, side, nxt, ACT_NONE, cur, dry, s));       // res + proj(attn)
      if (!dry) SAMPT_TRY(tinyvit_dwconv3x3(nxt, k.local.w, k.local.b, cur, B, side, side, C, 1, 0, s));   // (the block's input is dead)
      if (!dry) SAMPT_TRY(layernorm_rows(cur, k.ln2w, k.ln2b, xn, M, C, 1e-5f, nullptr, 0, ACT_NONE, s));
      SAMPT_TRY(dense(k.fc1, xn, B, side, hid, ACT_GELU, nullptr, dry, s));
      SAMPT_TRY(dense(k.fc2, hid, B, side, nxt, ACT_NONE, cur, dry, s));        // x + mlp(x)
      std::swap(cur, nxt);
    }
    if (i < 3) SAMPT_TRY(downsample(i, side));
    SAMPT_TRY(copy_out(stages ? stages[1 + i] : nullptr, cur, (size_t)B * side * side * c.dims[i < 3 ? i + 1 : 3]));
    SAMPT_TRY(event(2 + i));
  }
  if (side != g) return SAMPT_ERR_ARG;
  // ---- neck
  ws.off = mark;
  float* neck_a = ws.f32((size_t)B * g * g * c.out_chans);
  float* neck_b = ws.f32((size_t)B * g * g * c.out_chans);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  const NeckW nk{neck0_w, neck2_w, neck0_hl, neck2_hl, neck1w, neck1b, neck3w, neck3b};
  SAMPT_TRY(sam_neck(nk, cur, B, g, c.dims[3], c.out_chans, neck_a, neck_b, features, s));
  return event(6);
}

}  // namespace sampt
