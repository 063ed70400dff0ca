// TapNet engine (sam_pt/point_tracker/tapnet/tapnet_model.py): TSMResNetV2 (models/tsm_resnet.py) at depth 18 up to
// 'tsm_resnet_unit_2' with output stride 8 — stem 7 x 7 stride 2, max-pool 3 x 3 stride 2, three units of two non-bottleneck blocks
// (64 / 128 / 256 channels, strides 1 / 2 / 1, temporal shift of 1 / 8 of the channels in units 0 and 1) —, the channel normalisation,
// the trilinear query features and the cost-volume heads.  BatchNorm runs with its moving statistics, a per-channel affine folded on
// the host, so nothing is per image: every block takes all T frames in one launch per kernel.  Only the stem and the max-pool run in
// chunks of `stem_chunk` frames, so the 128 x 128 x 64 map never exists for the whole clip.
//
// A block (tsm_resnet.py:94-176, no conv_1 at depth 18): preact = relu(bn0(x)); shortcut = block 0 ? conv1x1_stride(preact) : x;
// y = conv3x3_stride(shift(preact)); out = conv3x3(relu(bn1(y))) + shortcut — two tapnet_bn_shift launches (the first writes the shifted
// map and, for block 0, the unshifted one), two or three convolutions, the residual in conv_2's epilogue.
//
// Launches per clip, NOMINAL (TapnetEngine::launches adds these constants where a stage ran; nothing counts at the launch sites, and a
// convolution is one whatever its dispatcher does): 3 x ceil(T / stem_chunk) (frame preparation, stem, max-pool) + 27 (6 blocks of 2 norm /
// shift passes + 2 convolutions, 3 shortcut projections) + 1 (channel normalisation) + 2 (query features, heads) = 3 ceil(T / stem_chunk) + 30.
#include <algorithm>

#include "engine_layers.h"

namespace sampt {

static const int kCh[3] = {64, 128, 256}, kStride[3] = {1, 2, 1}, kShiftDiv[3] = {8, 8, 0};   // shifted channels = C / 8 (fraction 0.125) or none
constexpr int kMaxFrames = 4096;      // T x 64 x 64 x 64 elements stay far below 2^31 (the convolutions index with int)

int TapnetEngine::init(const WeightMap& w) {
  int rc = load_conv_same(w, "tsm.stem", 4, 64, 7, 2, 256, stem);   // Cin zero-padded 3 -> 4
  int side = 64, cin = 64;
  for (int u = 0; u < 3; ++u) {
    for (int b = 0; b < 2; ++b) {
      Blk& B = blk[u][b];
      const std::string p = "tsm.u" + std::to_string(u) + ".b" + std::to_string(b);
      const int bc = b == 0 ? cin : kCh[u], st = b == 0 ? kStride[u] : 1;
      B.proj = b == 0, B.shift = kShiftDiv[u] ? bc / kShiftDiv[u] : 0;   // of the block's INPUT channels: 8 at 64, 16 at 128
      B.a0 = w.f(p + ".bn0.a"), B.b0 = w.f(p + ".bn0.b");
      B.a1 = w.f(p + ".bn1.a"), B.b1 = w.f(p + ".bn1.b");
      rc |= load_conv_same(w, p + ".conv0", bc, kCh[u], 3, st, side, B.c0);
      if (B.proj) rc |= load_conv_same(w, p + ".shortcut", bc, kCh[u], 1, st, side, B.sc);
      side = (side + st - 1) / st;
      rc |= load_conv_same(w, p + ".conv2", kCh[u], kCh[u], 3, 1, side, B.c2);
      if (!B.a0 || !B.b0 || !B.a1 || !B.b1) rc |= SAMPT_ERR_ARG;
    }
    cin = kCh[u];
  }
  head.w1 = w.f("heads.hid1.weight"), head.b1 = w.f("heads.hid1.bias");
  head.w2 = w.f("heads.hid2.weight"), head.b2 = w.f("heads.hid2.bias");
  head.w3 = w.f("heads.hid3.weight"), head.b3 = w.f("heads.hid3.bias");
  head.w4 = w.f("heads.hid4.weight"), head.b4 = w.f("heads.hid4.bias");
  head.w5 = w.f("heads.occ_out.weight"), head.b5 = w.f("heads.occ_out.bias");
  if (rc != SAMPT_OK || !w.missing.empty()) {
    error = "TapnetEngine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

// one TSMResNetBlock on cur [T][side][side][cin] -> out [T][oside][oside][c]; the scratch it takes from ws is the caller's to release
static int tsm_block(const TapnetEngine::Blk& B, const float* cur, int T, int& side, float* out, Arena& ws, int& launches, hipStream_t s) {
  const bool dry = ws.dry();
  const int cin = B.c0.cin, c = B.c0.cout, st = B.c0.stride, oside = (side + st - 1) / st;
  const size_t el = (size_t)T * side * side * cin, oel = (size_t)T * oside * oside * c;
  int a, b;
  Planes ps = planes_for(ws, el, B.c0), pu;
  float *fs = ps.hi ? nullptr : ws.f32(el), *fu = nullptr;
  if (B.proj) {
    pu = planes_for(ws, el, B.sc);
    if (!pu.hi) fu = ws.f32(el);
  }
  if (!dry) SAMPT_TRY(tapnet_bn_shift(cur, B.a0, B.b0, T, (long)side * side, cin, B.shift, fs, ps.hi, ps.lo, fu, pu.hi, pu.lo, s));
  const float* shortcut = cur;
  if (B.proj) {
    float* sc = ws.f32(oel);
    SAMPT_TRY(run_conv(B.sc, fu ? fu : cur, T, side, side, sc, c, ACT_NONE, nullptr, a, b, dry, s, pu));   // (with planes the f32 pointer is a placeholder)
    if (a != oside || b != oside) return SAMPT_ERR_ARG;
    shortcut = sc;
    if (!dry) ++launches;
  }
  float* y0 = ws.f32(oel);
  SAMPT_TRY(run_conv(B.c0, fs ? fs : cur, T, side, side, y0, c, ACT_NONE, nullptr, a, b, dry, s, ps));
  if (a != oside || b != oside) return SAMPT_ERR_ARG;
  Planes p1 = planes_for(ws, oel, B.c2);
  float* n1 = p1.hi ? nullptr : ws.f32(oel);
  if (!dry) SAMPT_TRY(tapnet_bn_shift(y0, B.a1, B.b1, T, (long)oside * oside, c, 0, n1, p1.hi, p1.lo, nullptr, nullptr, nullptr, s));
  SAMPT_TRY(run_conv(B.c2, n1 ? n1 : y0, T, oside, oside, out, c, ACT_NONE, shortcut, a, b, dry, s, p1));
  if (!dry) launches += 4;
  side = oside;
  return SAMPT_OK;
}

int TapnetEngine::backbone(const float* frames, int T, float* grid, float* const* stages, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  if (T < 1 || T > kMaxFrames) {
    error = "TapnetEngine: 1 <= T <= 4096 frames per clip";
    return SAMPT_ERR_ARG;
  }
  const size_t map = (size_t)T * 64 * 64 * 64;          // the largest trunk map: 64 x 64 x 64 = 32 x 32 x 256 per frame
  float* ping = ws.f32(map);
  float* pong = ws.f32(map);
  const size_t mark = ws.off;
  const int fc = std::max(1, std::min(stem_chunk, T));
  for (int f0 = 0; f0 < T; f0 += fc) {
    const int nf = std::min(fc, T - f0);
    ws.off = mark;
    float* x0 = ws.f32((size_t)nf * 256 * 256 * 4);
    float* st = ws.f32((size_t)nf * 128 * 128 * 64);
    int a, b;
    if (!dry) SAMPT_TRY(tapir_prep_frames(frames + (size_t)f0 * 3 * 256 * 256, nf, x0, s));
    SAMPT_TRY(run_conv(stem, x0, nf, 256, 256, st, 64, ACT_NONE, nullptr, a, b, dry, s));
    if (a != 128 || b != 128) return SAMPT_ERR_ARG;
    if (!dry) {
      SAMPT_TRY(tapnet_maxpool(st, ping + (size_t)f0 * 64 * 64 * 64, nf, 128, 128, 64, s));
      launches += 3;
    }
  }
  auto stage_out = [&](int i, const float* src, size_t elems) -> int {
    if (dry || !stages || !stages[i]) return SAMPT_OK;
    const hipError_t e = hipMemcpyAsync(stages[i], src, elems * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      set_error("TapnetEngine::backbone: hipMemcpyAsync", e);
      return SAMPT_ERR_HIP;
    }
    return SAMPT_OK;
  };
  SAMPT_TRY(stage_out(0, ping, map));
  float *cur = ping, *nxt = pong;
  int side = 64;
  for (int u = 0; u < 3; ++u) {
    for (int bi = 0; bi < 2; ++bi) {
      ws.off = mark;
      SAMPT_TRY(tsm_block(blk[u][bi], cur, T, side, nxt, ws, launches, s));
      std::swap(cur, nxt);
    }
    SAMPT_TRY(stage_out(1 + u, cur, (size_t)T * side * side * kCh[u]));
  }
  if (side != 32) return SAMPT_ERR_ARG;
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (!dry) {
    SAMPT_TRY(tapir_l2norm_rows(cur, grid, (long)T * 32 * 32, 256, s));
    ++launches;
  }
  return SAMPT_OK;
}

int TapnetEngine::track(const float* frames, int T, const float* q, int n, float* tracks, float* occ, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  if (!dry) launches = 0;
  float* grid = ws.f32((size_t)T * 32 * 32 * 256);
  float* qf = ws.f32((size_t)n * 256);
  SAMPT_TRY(backbone(frames, T, grid, nullptr, ws, s));
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  SAMPT_TRY(tapnet_query_feats(grid, T, q, n, qf, s));
  SAMPT_TRY(tapnet_heads(grid, T, qf, q, n, head, tracks, occ, s));
  launches += 2;
  return SAMPT_OK;
}

}  // namespace sampt
