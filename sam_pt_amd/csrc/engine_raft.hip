// RAFT engine: BasicEncoder x 2 (extractor.py:117-190) once per frame, the correlation pyramid (corr.py:15-30) as four
// products against the average-pooled second feature map, and the update block (update.py:84-143) as a device-resident
// loop over `iters` with no host round trip.  Mask head and convex upsampling run after the last iteration only.
#include <algorithm>

#include "engine_layers.h"

namespace sampt {

static const int kDims[3] = {64, 96, 128}, kStrides[3] = {1, 2, 2};

static int load_encoder(const WeightMap& w, const std::string& pre, RaftEngine::Enc& e) {
  int rc = load_conv(w, pre + ".conv1", 4, 64, 7, 2, 3, e.stem);      // Cin zero-padded 3 -> 4
  rc |= load_res_layers(w, pre, 3, kDims, kStrides, e.blk);
  return rc | load_conv(w, pre + ".conv2", 128, 256, 1, 1, 0, e.out);
}

int RaftEngine::init(const WeightMap& w) {
  int rc = load_encoder(w, "fnet", fnet) | load_encoder(w, "cnet", cnet);
  const std::string u = "update_block.";
  rc |= load_conv(w, u + "encoder.convc1", 352, 256, 1, 1, 1, 0, 0, convc1);     // 324 lookup channels zero-padded to 352
  rc |= load_conv(w, u + "encoder.convc2", 256, 192, 3, 3, 1, 1, 1, convc2);
  rc |= load_conv(w, u + "encoder.convf2", 128, 64, 3, 3, 1, 1, 1, convf2);
  rc |= load_conv(w, u + "encoder.conv", 256, 126, 3, 3, 1, 1, 1, conv);
  convf1_w = w.f(u + "encoder.convf1.weight"), convf1_b = w.f(u + "encoder.convf1.bias");
  rc |= load_conv(w, u + "gru.convzr1", 384, 256, 1, 5, 1, 0, 2, zr[0]);        // z and r share their input: one N = 256 convolution
  rc |= load_conv(w, u + "gru.convq1", 384, 128, 1, 5, 1, 0, 2, q[0]);
  rc |= load_conv(w, u + "gru.convzr2", 384, 256, 5, 1, 1, 2, 0, zr[1]);
  rc |= load_conv(w, u + "gru.convq2", 384, 128, 5, 1, 1, 2, 0, q[1]);
  rc |= load_conv(w, u + "flow_head.conv1", 128, 256, 3, 3, 1, 1, 1, fh1);
  rc |= load_conv(w, u + "flow_head.conv2", 256, 4, 3, 3, 1, 1, 1, fh2);        // N = 2 zero-padded to 4
  rc |= load_conv(w, u + "mask.0", 128, 256, 3, 3, 1, 1, 1, mask0);
  rc |= load_conv(w, u + "mask.2", 256, 576, 1, 1, 1, 0, 0, mask2);
  if (rc != SAMPT_OK || !convf1_w || !convf1_b || !w.missing.empty()) {
    error = "RaftEngine: missing weights: " + w.missing;
    return SAMPT_ERR_ARG;
  }
  return SAMPT_OK;
}

// BasicEncoder over nf prepared frames x0 [nf][Hp][Wp][4] -> out [nf][Hp/8 * Wp/8][256].  instance: InstanceNorm after every
// convolution of the trunk (fnet); otherwise the norms are already inside the weights (cnet) and only the ReLUs remain.
static int encode(const RaftEngine::Enc& e, bool instance, const float* x0, int nf, int Hp, int Wp, float* out, Arena& ws,
                  hipStream_t s) {
  const bool dry = ws.dry();
  const int H2 = Hp / 2, W2 = Wp / 2;
  NormCtx nc = {nullptr, nullptr};
  if (instance) {
    nc.partials = (double*)ws.get(instnorm_partial_doubles(nf, (long)H2 * W2, 256) * sizeof(double));
    nc.mean_rstd = ws.f32((size_t)nf * 256 * 2);
  }
  int h, w;
  float* cur = ws.f32((size_t)nf * H2 * W2 * 64);
  Planes cur_p;
  SAMPT_TRY(run_conv(e.stem, x0, nf, Hp, Wp, cur, 64, instance ? ACT_NONE : ACT_RELU, nullptr, h, w, dry, s));
  if (instance) SAMPT_TRY(run_inorm(nc, cur, nf, (long)h * w, 64, 1, nullptr, dry, s));
  for (int li = 0; li < 3; ++li)
    for (int bi = 0; bi < 2; ++bi) SAMPT_TRY(res_block(e.blk[li][bi], instance, nullptr, cur, cur_p, nf, h, w, nc, nc, ws, s));
  return run_conv(e.out, cur, nf, h, w, out, 256, ACT_NONE, nullptr, h, w, dry, s);
}

int raft_corr_levels(const float* fmap1, long s1, const float* const pooled[4], const long s2[4], int n, int h8, int w8,
                     float* const out[4], hipStream_t s) {
  const int hw = h8 * w8;
  int lh = h8, lw = w8;
  for (int l = 0; l < 4; ++l) {
    if (lh < 1 || lw < 1) return SAMPT_ERR_ARG;
    // one launch per pair: the dispatcher picks its kernel (and with it the order of the K sum) from the shape and the batch
    // count, so a batched launch would make a pair's bits depend on how many pairs share its chunk
    for (int i = 0; i < n; ++i) {
      GemmP p;
      p.A = fmap1 + i * s1, p.W = pooled[l] + i * s2[l], p.C = out[l] + (long)i * hw * lh * lw;
      p.M = hw, p.N = lh * lw, p.K = 256;
      p.lda = 256, p.ldw = 256, p.ldc = lh * lw;
      p.alpha = 1.0f / 16.0f;                     // 1 / sqrt(256)
      SAMPT_TRY(gemm_f32(p, s));
    }
    lh /= 2, lw /= 2;
  }
  return SAMPT_OK;
}

int RaftEngine::flows(const uint8_t* frames, int T, int H, int W, int iters, float* fwd, float* bwd, float* flow_low, int np,
                      Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  const int Hp = (H + 7) / 8 * 8, Wp = (W + 7) / 8 * 8, h8 = Hp / 8, w8 = Wp / 8, hw = h8 * w8, npairs = T - 1;
  if (npairs <= 0) return SAMPT_OK;
  np = std::max(1, std::min(np, npairs));
  int lh[4], lw[4];
  lh[0] = h8, lw[0] = w8;
  for (int l = 1; l < 4; ++l) lh[l] = lh[l - 1] / 2, lw[l] = lw[l - 1] / 2;
  // ---- per frame: fmap and its three pooled copies, tanh(net), relu(inp)
  float* pool[4];
  for (int l = 0; l < 4; ++l) pool[l] = ws.f32((size_t)T * lh[l] * lw[l] * 256);
  float* fmap = pool[0];
  float* net = ws.f32((size_t)T * hw * 128);
  float* inp = ws.f32((size_t)T * hw * 128);
  const size_t mark = ws.off;
  // one frame per encoder pass: InstanceNorm is per sample, a frame of the smallest legal size is already 4096 GEMM rows at the
  // stem, and the scratch of a pass then stays below that of one pair's update, so the workspace grows with the pairs in flight
  const int FC = 1;
  for (int f0 = 0; f0 < T; f0 += FC) {
    const int nf = std::min(FC, T - f0);
    ws.off = mark;
    float* x0 = ws.f32((size_t)nf * Hp * Wp * 4);
    float* ctx = ws.f32((size_t)nf * hw * 256);
    if (!dry) SAMPT_TRY(raft_prep_frames(frames + (size_t)f0 * 3 * H * W, nf, H, W, Hp, Wp, x0, s));
    const size_t m2 = ws.off;
    SAMPT_TRY(encode(fnet, true, x0, nf, Hp, Wp, fmap + (size_t)f0 * hw * 256, ws, s));
    ws.off = m2;
    SAMPT_TRY(encode(cnet, false, x0, nf, Hp, Wp, ctx, ws, s));
    if (!dry) SAMPT_TRY(raft_split_ctx(ctx, (long)nf * hw, net + (size_t)f0 * hw * 128, inp + (size_t)f0 * hw * 128, s));
  }
  if (!dry)
    for (int l = 1; l < 4; ++l) SAMPT_TRY(avgpool2x2_nhwc(pool[l - 1], T, lh[l - 1], lw[l - 1], 256, pool[l], s));
  // ---- per chunk of np pairs = P pair-directions = M rows
  ws.off = mark;
  const size_t Pm = 2 * (size_t)np, Mm = Pm * hw;
  float* corr[4];
  for (int l = 0; l < 4; ++l) corr[l] = ws.f32(Pm * hw * lh[l] * lw[l]);
  float* coords1 = ws.f32(Mm * 2);
  float* flow = ws.f32(Mm * 2);
  float* look = ws.f32(Mm * 352);
  float* cor1 = ws.f32(Mm * 256);
  float* corflo = ws.f32(Mm * 256);
  float* flo1 = ws.f32(Mm * 128);
  float* hx = ws.f32(Mm * 384);
  float* rhx = ws.f32(Mm * 384);
  float* zrb = ws.f32(Mm * 256);
  float* zb = ws.f32(Mm * 128);
  float* qb = ws.f32(Mm * 128);
  float* hnet = ws.f32(Mm * 128);
  float* wide = ws.f32(Mm * 256);      // hidden layer of the flow head, then of the mask head
  float* delta = ws.f32(Mm * 4);
  float* mask = ws.f32(Mm * 576);
  if (!ws.ok()) return SAMPT_ERR_WORKSPACE;
  if (dry) return SAMPT_OK;
  for (int p0 = 0; p0 < npairs; p0 += np) {
    const int n = std::min(np, npairs - p0), P = 2 * n;
    const long M = (long)P * hw;
    // forward directions read (frame p0 + j, pooled frame p0 + j + 1), backward ones swap the operands
    for (int dir = 0; dir < 2; ++dir) {
      const float* pl[4];
      long s2[4];
      float* out[4];
      for (int l = 0; l < 4; ++l) {
        s2[l] = (long)lh[l] * lw[l] * 256;
        pl[l] = pool[l] + (size_t)(p0 + (dir ? 0 : 1)) * s2[l];
        out[l] = corr[l] + (size_t)dir * n * hw * lh[l] * lw[l];
      }
      SAMPT_TRY(raft_corr_levels(fmap + (size_t)(p0 + (dir ? 1 : 0)) * hw * 256, (long)hw * 256, pl, s2, n, h8, w8, out, s));
    }
    SAMPT_TRY(raft_init_state(net, inp, p0, n, h8, w8, hx, coords1, flow, s));
    RaftLevels lv;
    for (int l = 0; l < 4; ++l) lv.base[l] = corr[l], lv.h[l] = lh[l], lv.w[l] = lw[l];
    int a, b;
    for (int it = 0; it < iters; ++it) {
      SAMPT_TRY(raft_lookup(lv, coords1, M, look, s));
      SAMPT_TRY(run_conv(convc1, look, P, h8, w8, cor1, 256, ACT_RELU, nullptr, a, b, false, s));
      SAMPT_TRY(run_conv(convc2, cor1, P, h8, w8, corflo, 256, ACT_RELU, nullptr, a, b, false, s));              // channels [0, 192)
      SAMPT_TRY(raft_convf1(flow, convf1_w, convf1_b, flo1, P, h8, w8, s));
      SAMPT_TRY(run_conv(convf2, flo1, P, h8, w8, corflo + 192, 256, ACT_RELU, nullptr, a, b, false, s));        // channels [192, 256)
      SAMPT_TRY(run_conv(conv, corflo, P, h8, w8, hx + 256, 384, ACT_RELU, nullptr, a, b, false, s));            // hx channels [256, 382)
      for (int pass = 0; pass < 2; ++pass) {                                                       // 1 x 5, then 5 x 1
        SAMPT_TRY(run_conv(zr[pass], hx, P, h8, w8, zrb, 256, ACT_NONE, nullptr, a, b, false, s));
        SAMPT_TRY(raft_gru_a(zrb, hx, zb, rhx, M, s));
        SAMPT_TRY(run_conv(q[pass], rhx, P, h8, w8, qb, 128, ACT_NONE, nullptr, a, b, false, s));
        SAMPT_TRY(raft_gru_b(qb, zb, hx, hnet, M, s));
      }
      SAMPT_TRY(run_conv(fh1, hnet, P, h8, w8, wide, 256, ACT_RELU, nullptr, a, b, false, s));
      SAMPT_TRY(run_conv(fh2, wide, P, h8, w8, delta, 4, ACT_NONE, nullptr, a, b, false, s));
      SAMPT_TRY(raft_flow_update(delta, coords1, flow, hx, h8, w8, M, s));
    }
    SAMPT_TRY(run_conv(mask0, hnet, P, h8, w8, wide, 256, ACT_RELU, nullptr, a, b, false, s));
    SAMPT_TRY(run_conv(mask2, wide, P, h8, w8, mask, 576, ACT_NONE, nullptr, a, b, false, s));
    SAMPT_TRY(raft_upsample(flow, mask, 0.25f, h8, w8, H, W, p0, n, fwd, bwd, s));
    if (flow_low) SAMPT_TRY(raft_flow_low(flow, flow_low, p0, n, npairs, h8, w8, s));
  }
  return SAMPT_OK;
}

int RaftEngine::plan_pairs(int T, int H, int W, int max_pairs, size_t ws_bytes) {
  for (int np = std::max(1, std::min(max_pairs, T - 1)); np >= 1; --np) {
    Arena a(nullptr, 0);
    if (flows(nullptr, T, H, W, 1, nullptr, nullptr, nullptr, np, a, nullptr) == SAMPT_OK && a.peak + 256 <= ws_bytes) return np;
  }
  return 0;
}

}  // namespace sampt
