// TAPIR engine (sam_pt/point_tracker/tapir/tapir_model.py): the pre-activation ResNet (models/resnet.py: v2 blocks, InstanceNorm with
// scale and offset, TensorFlow "SAME" padding, no max-pool) once per 256 x 256 frame, query features, the cost-volume heads for every
// (query, frame), then `iters` refinements (refine_pips + PIPSMLPMixer) over all (query, frame) rows of a chunk of queries.  One
// resolution: the adapter always delivers 256 x 256, so the result is the last refinement alone (tapir_model.py:1041-1047).
//
// Launches per clip, NOMINAL (TapirEngine::launches adds these constants where a stage ran; nothing counts at the launch sites, so an
// InstanceNorm is taken as its three kernels and every convolution / GEMM as one whatever its dispatcher does): T x 72 for the backbone (frame preparation, stem, 8 blocks of 2 norms x 3 launches + 2 convolutions, 4 shortcut
// projections, 2 channel normalisations) + 2 (query features, heads) + chunks x iters x 53 (patch correlation, input Linear, 12 x
// (temporal half, LayerNorm, 2 Linears), LayerNorm, output Linear, update).  With one chunk and 4 refinements that is 72 T + 214: the
// backbone bounds the count from 3 frames on.
#include <algorithm>

#include "engine_layers.h"

namespace sampt {

static const int kCh[4] = {64, 128, 256, 256}, kStride[4] = {1, 2, 2, 1};
constexpr int kLdx = 496;     // mixer input row: 486 columns zero-padded to a multiple of 16 (tapir_gemm's K step)

int TapirEngine::init(const WeightMap& w) {
  int rc = load_conv_same(w, "resnet.initial_conv", 4, 64, 7, 2, 256, stem);   // Cin zero-padded 3 -> 4
  int side = 128, cin = 64;
  for (int g = 0; g < 4; ++g) {
    for (int b = 0; b < 2; ++b) {
      Blk& B = blk[g][b];
      const std::string p = "resnet.g" + std::to_string(g) + ".b" + std::to_string(b);
      const int bc = b == 0 ? cin : kCh[g], st = b == 0 ? kStride[g] : 1;
      B.proj = b == 0;
      B.n0s = w.f(p + ".norm0.scale"), B.n0o = w.f(p + ".norm0.offset");
      B.n1s = w.f(p + ".norm1.scale"), B.n1o = w.f(p + ".norm1.offset");
      rc |= load_conv_same(w, p + ".conv0", bc, kCh[g], 3, st, side, B.c0);
      if (B.proj) rc |= load_conv_same(w, p + ".shortcut", bc, kCh[g], 1, st, side, B.sc);
      side = (side + st - 1) / st;
      rc |= load_conv_same(w, p + ".conv1", kCh[g], kCh[g], 3, 1, side, B.c1);
      if (!B.n0s || !B.n0o || !B.n1s || !B.n1o) rc |= SAMPT_ERR_ARG;
      // one normalised map feeds conv_0 and the shortcut: both read its planes or both read its f32 copy
      if (B.proj && (B.c0.w_hl == nullptr) != (B.sc.w_hl == nullptr)) B.c0.w_hl = B.sc.w_hl = nullptr;
    }
    cin = kCh[g];
  }
  head.w1 = w.f("heads.hid1.weight"), head.b1 = w.f("heads.hid1.bias");
  head.w2 = w.f("heads.hid2.weight"), head.b2 = w.f("heads.hid2.bias");
  head.w3 = w.f("heads.hid3.weight"), head.b3 = w.f("heads.hid3.bias");
  head.w4 = w.f("heads.hid4.weight"), head.b4 = w.f("heads.hid4.bias");
  head.w5 = w.f("heads.occ_out.weight"), head.b5 = w.f("heads.occ_out.bias");
  in_w = w.f("mixer.in.weight"), in_b = w.f("mixer.in.bias");
  out_w = w.f("mixer.out.weight"), out_b = w.f("mixer.out.bias");
  ln_out = w.f("mixer.ln_out.scale"), zeros = w.f("mixer.zeros");
  for (int i = 0; i < 12; ++i) {
    const std::string p = "mixer.blocks." + std::to_string(i);
    Mix& m = mix[i];
    m.ln1 = w.f(p + ".ln1.scale"), m.ln2 = w.f(p + ".ln2.scale");
    m.dw1_w = w.f(p + ".dw1.weight"), m.dw1_b = w.f(p + ".dw1.bias");
    m.dw2_w = w.f(p + ".dw2.weight"), m.dw2_b = w.f(p + ".dw2.bias");
    m.up_w = w.f(p + ".up.weight"), m.up_b = w.f(p + ".up.bias");
    m.dn_w = w.f(p + ".down.weight"), m.dn_b = w.f(p + ".down.bias");
  }
  if (rc != SAMPT_OK || !w.missing.empty()) {
    error = "TapirEngine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

// relu(InstanceNorm(x) * scale + offset) of one image: as f32 (y) or as the split-fp16 planes its consumers read
static int norm_relu(NormCtx& nc, const float* x, const float* scale, const float* offset, float* y, Planes pl, long hw, int C, bool dry,
                     hipStream_t s) {
  if (dry) return SAMPT_OK;
  SAMPT_TRY(instnorm_stats(x, 1, hw, C, 1e-5f, nc.partials, nc.mean_rstd, s));
  return instnorm_affine_apply(x, nc.mean_rstd, scale, offset, y, 1, hw, C, 1, s, pl.hi, pl.lo);
}

// BlockV2 (resnet.py:245-258) on cur [side][side][cin] -> out [oside][oside][c] (allocated here unless given)
static int block_v2(const TapirEngine::Blk& B, const float* cur, int& side, float*& out, NormCtx& nc, Arena& ws, int& launches, hipStream_t s) {
  const bool dry = ws.dry();
  const int cin = B.c0.cin, c = B.c0.cout, st = B.c0.stride, oside = (side + st - 1) / st;
  const size_t hw = (size_t)side * side, ohw = (size_t)oside * oside;
  int a, b;
  Planes p0 = planes_for(ws, hw * cin, B.c0);
  float* n0 = p0.hi ? nullptr : ws.f32(hw * cin);
  SAMPT_TRY(norm_relu(nc, cur, B.n0s, B.n0o, n0, p0, (long)hw, cin, dry, s));
  const float* in0 = n0 ? n0 : cur;                  // (with planes the f32 pointer is only a placeholder)
  const float* shortcut = cur;
  if (B.proj) {
    float* sc = ws.f32(ohw * c);
    SAMPT_TRY(run_conv(B.sc, in0, 1, side, side, sc, c, ACT_NONE, nullptr, a, b, dry, s, p0));
    shortcut = sc;
    if (!dry) ++launches;
  }
  float* y0 = ws.f32(ohw * c);
  SAMPT_TRY(run_conv(B.c0, in0, 1, side, side, y0, c, ACT_NONE, nullptr, a, b, dry, s, p0));
  if (a != oside || b != oside) return SAMPT_ERR_ARG;
  Planes p1 = planes_for(ws, ohw * c, B.c1);
  float* n1 = p1.hi ? nullptr : ws.f32(ohw * c);
  SAMPT_TRY(norm_relu(nc, y0, B.n1s, B.n1o, n1, p1, (long)ohw, c, dry, s));
  if (!out) out = ws.f32(ohw * c);
  SAMPT_TRY(run_conv(B.c1, n1 ? n1 : y0, 1, oside, oside, out, c, ACT_NONE, shortcut, a, b, dry, s, p1));
  if (!dry) launches += 2 * 3 + 2;
  side = oside;
  return SAMPT_OK;
}

int TapirEngine::backbone(const float* frames, int nf, float* hires, float* lowres, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  NormCtx nc = {nullptr, nullptr};
  size_t part = 0;
  part = std::max(part, instnorm_partial_doubles(1, 128L * 128, 64));      // the three shapes the norms of one frame take
  part = std::max(part, instnorm_partial_doubles(1, 64L * 64, 128));
  part = std::max(part, instnorm_partial_doubles(1, 32L * 32, 256));
  nc.partials = (double*)ws.get(part * sizeof(double));
  nc.mean_rstd = ws.f32(256 * 2);
  float* x0 = ws.f32((size_t)256 * 256 * 4);
  const size_t mark = ws.off;
  for (int f = 0; f < nf; ++f) {            // one frame per pass: InstanceNorm is per image, and the scratch stays that of one frame
    ws.off = mark;
    if (!dry) SAMPT_TRY(tapir_prep_frames(frames + (size_t)f * 3 * 256 * 256, 1, x0, s));
    float* cur = ws.f32((size_t)128 * 128 * 64);
    int side, b;
    SAMPT_TRY(run_conv(stem, x0, 1, 256, 256, cur, 64, ACT_NONE, nullptr, side, b, dry, s));
    if (side != 128 || b != 128) return SAMPT_ERR_ARG;
    if (!dry) launches += 2;
    for (int g = 0; g < 4; ++g)
      for (int bi = 0; bi < 2; ++bi) {
        float* out = nullptr;
        SAMPT_TRY(block_v2(blk[g][bi], cur, side, out, nc, ws, launches, s));
        cur = out;
        if (bi == 1 && (g == 1 || g == 3) && !dry) {
          if (g == 1) SAMPT_TRY(tapir_l2norm_rows(cur, hires + (size_t)f * 64 * 64 * 128, 64L * 64, 128, s));
          else SAMPT_TRY(tapir_l2norm_rows(cur, lowres + (size_t)f * 32 * 32 * 256, 32L * 32, 256, s));
          ++launches;
        }
      }
    if (side != 32) return SAMPT_ERR_ARG;
  }
  return ws.ok() ? SAMPT_OK : SAMPT_ERR_WORKSPACE;
}

int TapirEngine::track(const float* frames, int T, const float* q, int n, int iters, float* tracks, float* occ, float* expd, float* iter_out,
                       int qc, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  qc = std::max(1, std::min(qc, n));
  if (!dry) launches = 0;
  float* hires = ws.f32((size_t)T * 64 * 64 * 128);
  float* lowres = ws.f32((size_t)T * 32 * 32 * 256);
  float* qf = ws.f32((size_t)n * 384);
  const size_t mark = ws.off;
  SAMPT_TRY(backbone(frames, T, hires, lowres, ws, s));
  ws.off = mark;
  const size_t R = (size_t)qc * T;
  float* x = ws.f32(R * kLdx);
  float* h = ws.f32(R * 512);
  float* h2 = ws.f32(R * 512);
  float* lnb = ws.f32(R * 512);
  float* up = ws.f32(R * 2048);
  float* res = ws.f32(R * 388);
  float* feats = ws.f32(R * 384);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  SAMPT_TRY(tapir_query_feats(hires, lowres, T, q, n, qf, s));
  // pos / occ / expd of row (query, frame) live in the caller's outputs from the heads on
  SAMPT_TRY(tapir_heads(lowres, T, qf, 384, 128, q, n, head, tracks, occ, expd, iter_out, s));
  launches += 2;
  for (int q0 = 0; q0 < n; q0 += qc) {
    const int nq = std::min(qc, n - q0);
    const long M = (long)nq * T, r0 = (long)q0 * T;
    for (int it = 0; it < iters; ++it) {
      SAMPT_TRY(tapir_patch_corr(hires, lowres, T, nq, tracks + r0 * 2, occ + r0, expd + r0, it == 0 ? qf + (size_t)q0 * 384 : feats,
                                 it == 0 ? 0 : 1, x, kLdx, s));
      SAMPT_TRY(tapir_gemm(x, kLdx, in_w, in_b, h, 512, M, 512, kLdx, ACT_NONE, nullptr, 0, s));
      for (int i = 0; i < 12; ++i) {
        const Mix& m = mix[i];
        SAMPT_TRY(tapir_temporal_mix(h, h2, m.ln1, m.dw1_w, m.dw1_b, m.dw2_w, m.dw2_b, nq, T, s));
        SAMPT_TRY(layernorm_rows(h2, m.ln2, zeros, lnb, M, 512, 1e-5f, nullptr, 0, ACT_NONE, s));
        SAMPT_TRY(tapir_gemm(lnb, 512, m.up_w, m.up_b, up, 2048, M, 2048, 512, ACT_GELU_TANH, nullptr, 0, s));
        SAMPT_TRY(tapir_gemm(up, 2048, m.dn_w, m.dn_b, h, 512, M, 512, 2048, ACT_NONE, h2, 512, s));
      }
      SAMPT_TRY(layernorm_rows(h, ln_out, zeros, lnb, M, 512, 1e-5f, nullptr, 0, ACT_NONE, s));
      SAMPT_TRY(tapir_gemm(lnb, 512, out_w, out_b, res, 388, M, 388, 512, ACT_NONE, nullptr, 0, s));
      SAMPT_TRY(tapir_update(res, qf + (size_t)q0 * 384, it == 0, tracks + r0 * 2, occ + r0, expd + r0, feats,
                             iter_out ? iter_out + ((size_t)(it + 1) * n * T + r0) * 4 : nullptr, nq, T, s));
      launches += 2 + 12 * 4 + 3;
    }
  }
  return SAMPT_OK;
}

int TapirEngine::plan_queries(int T, int n, size_t ws_bytes) {
  for (int qc = n; qc >= 1; qc = qc > 1 ? (qc + 1) / 2 : 0) {
    Arena a(nullptr, 0);
    if (track(nullptr, T, nullptr, n, 1, nullptr, nullptr, nullptr, nullptr, qc, a, nullptr) == SAMPT_OK && a.peak + 256 <= ws_bytes) return qc;
  }
  return 0;
}

}  // namespace sampt
