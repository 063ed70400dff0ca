// Where a layer becomes a GemmP: weight loaders, descriptor builders and launchers shared by every engine and the C ABI,
// and the BasicEncoder residual block that PIPS' and RAFT's encoders have in common.  Host code only.
#pragma once
#include <algorithm>

#include "engine.h"

namespace sampt {

// ---- loaders -----------------------------------------------------------------------------------
// w_hl: only where the packer delivered `<name>.weight_hl` and the split-fp16 kernels can take the layer (Cin % 32 == 0)
inline int load_conv(const WeightMap& w, const std::string& name, int cin, int cout, int kh, int kw, int stride, int ph, int pw,
                     ConvW& c) {
  c.w = w.f(name + ".weight");
  c.b = w.f(name + ".bias");
  c.w_hl = (cin % 32 == 0 && w.has(name + ".weight_hl")) ? w.h(name + ".weight_hl") : nullptr;
  c.cin = cin, c.cout = cout, c.kh = kh, c.kw = kw, c.stride = stride, c.ph = ph, c.pw = pw;
  return (c.w && c.b) ? SAMPT_OK : SAMPT_ERR_ARG;
}
inline int load_conv(const WeightMap& w, const std::string& name, int cin, int cout, int k, int stride, int pad, ConvW& c) {
  return load_conv(w, name, cin, cout, k, k, stride, pad, pad, c);
}

// TensorFlow / Haiku padding "SAME" of a k x k convolution over a side x side map: total = max((ceil(side / stride) - 1) stride + k - side, 0),
// floor(total / 2) before and the rest after
inline void same_padding(int side, int k, int stride, int& before, int& after) {
  const int out = (side + stride - 1) / stride, total = std::max((out - 1) * stride + k - side, 0);
  before = total / 2, after = total - before;
}
// a bias-free (Haiku with_bias=False) k x k convolution with padding "SAME" over side x side maps
inline int load_conv_same(const WeightMap& w, const std::string& name, int cin, int cout, int k, int stride, int side, ConvW& c) {
  int b, a;
  same_padding(side, k, stride, b, a);
  c.w = w.f(name + ".weight");
  c.b = nullptr;
  c.w_hl = (cin % 32 == 0 && w.has(name + ".weight_hl")) ? w.h(name + ".weight_hl") : nullptr;
  c.cin = cin, c.cout = cout, c.kh = c.kw = k, c.stride = stride, c.ph = c.pw = b;
  if (a != b) c.ph_after = c.pw_after = a;
  return c.w ? SAMPT_OK : SAMPT_ERR_ARG;
}

inline int load_linear(const WeightMap& w, const std::string& name, int n, int k, LinearW& l) {
  l.w = w.f(name + ".weight");
  l.b = w.f(name + ".bias");
  l.n = n, l.k = k;
  return (l.w && l.b) ? SAMPT_OK : SAMPT_ERR_ARG;
}

// [layer][block][conv1, conv2, downsample] of a BasicEncoder trunk: <prefix>.layer<L>.<B>.conv1 / conv2 / downsample.0; the
// first block of a layer carries the layer's stride and, where that is not 1, the 1 x 1 downsample of the skip path
inline int load_res_layers(const WeightMap& w, const std::string& prefix, int n_layers, const int* dims, const int* strides,
                           ConvW (*blk)[2][3]) {
  int rc = SAMPT_OK, in_planes = dims[0];
  for (int li = 0; li < n_layers; ++li) {
    for (int bi = 0; bi < 2; ++bi) {
      const int cin = bi == 0 ? in_planes : dims[li], st = bi == 0 ? strides[li] : 1;
      const std::string p = prefix + ".layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      rc |= load_conv(w, p + ".conv1", cin, dims[li], 3, st, 1, blk[li][bi][0]);
      rc |= load_conv(w, p + ".conv2", dims[li], dims[li], 3, 1, 1, blk[li][bi][1]);
      if (st != 1) rc |= load_conv(w, p + ".downsample.0", cin, dims[li], 1, st, 0, blk[li][bi][2]);
    }
    in_planes = dims[li];
  }
  return rc;
}

// ---- descriptor builders -----------------------------------------------------------------------
const float kF16x3Alpha = 1.0f / (float)(1 << F16X3_WSHIFT);   // undoes the 2^F16X3_WSHIFT scale of split-fp16 weights

// C [M][N] (row stride ldc) = act(A [M][K] (row stride lda) . W [N][K]^T + bias) (+ res, row stride ldr; 0 = N)
inline GemmP gemm_linear(const void* A, int lda, const void* W, const float* bias, void* C, int ldc, int M, int N, int K,
                         int act = ACT_NONE, const float* res = nullptr, int ldr = 0, int res_mod = 0) {
  GemmP p;
  p.A = A, p.W = W, p.bias = bias, p.C = C, p.res = res, p.res_mod = res_mod;
  p.M = M, p.N = N, p.K = K, p.lda = lda, p.ldw = K, p.ldc = ldc, p.ldr = ldr ? ldr : N, p.act = act;
  return p;
}

// y [n][OH][OW][cout] (pixel stride ldc; 0 = cout) = conv(x [n][H][W][cin]) + bias, exact-f32 weights; OH / OW are in the result
inline GemmP gemm_conv(const ConvW& c, const void* x, int n, int H, int W, void* y, int ldc = 0) {
  GemmP p;
  // the kernels index the input from the padding BEFORE (cpad) and bound-check both sides, so padding after only sets OH / OW
  const int pha = c.ph_after >= 0 ? c.ph_after : c.ph, pwa = c.pw_after >= 0 ? c.pw_after : c.pw;
  p.OH = (H + c.ph + pha - c.kh) / c.stride + 1, p.OW = (W + c.pw + pwa - c.kw) / c.stride + 1;
  p.A = x, p.W = c.w, p.bias = c.b, p.C = y;
  p.M = n * p.OH * p.OW, p.N = c.cout, p.K = c.kh * c.kw * c.cin, p.ldw = p.K, p.ldc = ldc ? ldc : c.cout;
  p.conv = 1, p.cH = H, p.cW = W, p.cC = c.cin, p.KH = c.kh, p.KW = c.kw, p.cstride = c.stride, p.cpad = c.ph;
  if (c.pw != c.ph) p.cpadw = c.pw;     // the one rule: square padding keeps the halo / split-fp16 kernels eligible
  return p;
}

// the weights as split-fp16 planes hl [2][N][K] (conv_f16x3 and the kernels it hands over to): fp32-grade products on the fp16
// matrix pipe.  A plain GEMM becomes the 1 x 1 convolution over an [1][M][1][K] image those kernels expect.
inline void gemm_split_planes(GemmP& p, const half_t* hl) {
  p.W = hl, p.W_lo = hl + (size_t)p.N * p.K, p.alpha = kF16x3Alpha;
  if (!p.conv) p.conv = 1, p.cH = p.M, p.cW = 1, p.cC = p.K, p.KH = p.KW = 1, p.cstride = 1, p.cpad = 0, p.OH = p.M, p.OW = 1;
}

// ---- launchers ---------------------------------------------------------------------------------
inline int run_linear(const float* A, int lda, const float* W, const float* b, float* C, int ldc, int M, int N, int K, int act,
                      const float* res, int ldr, hipStream_t s, float* skws = nullptr, size_t skn = 0) {
  GemmP p = gemm_linear(A, lda, W, b, C, ldc, M, N, K, act, res, ldr);
  p.splitk_ws = skws, p.splitk_ws_floats = skn;
  return gemm_f32(p, s);
}
inline int run_linear(const LinearW& l, const float* A, int lda, float* C, int ldc, int M, int act, const float* res, int ldr,
                      hipStream_t s) {
  return run_linear(A, lda, l.w, l.b, C, ldc, M, l.n, l.k, act, res, ldr, s);
}

struct Planes {          // an activation map pre-split into fp16 planes (written by run_inorm), or {null, null}
  half_t *hi = nullptr, *lo = nullptr;
};

struct NormCtx {
  double* partials;
  float* mean_rstd;
  int chunks = 0;          // > 0: the convolution that produced the map already wrote its InstanceNorm partial sums (this many per image)
};

// a built convolution on the kernel its weights allow: split-fp16 planes -> conv_f16x3 (xp: activations already split by the
// producing InstanceNorm; nc non-null: an InstanceNorm follows — a convolution that can, the halo-tiled 3 x 3 kernel, sums its
// share of the statistics), else the exact-f32 implicit GEMM
inline int launch_conv(GemmP& p, const half_t* w_hl, hipStream_t s, Planes xp = Planes(), NormCtx* nc = nullptr) {
  if (!w_hl) return gemm_f32(p, s);
  gemm_split_planes(p, w_hl);
  if (xp.hi) p.A = xp.hi, p.A_lo = xp.lo;
  if (nc && g_conv_halo && (g_conv_in_stats & 1) && conv3x3_halo_eligible(p)) p.in_part = nc->partials, nc->chunks = conv3x3_halo_tiles(p);
  return conv_f16x3(p, s);
}

// y[.., 0:cout] (pixel stride ldc) = act(conv(x) + bias) (+ res, same layout as y); returns the output dims
inline int run_conv(const ConvW& c, const float* x, int n, int H, int W, float* y, int ldc, int act, const float* res, int& OH,
                    int& OW, bool dry, hipStream_t s, Planes xp = Planes(), NormCtx* nc = nullptr) {
  GemmP p = gemm_conv(c, x, n, H, W, y, ldc);
  OH = p.OH, OW = p.OW;
  if (dry) return SAMPT_OK;
  p.act = act, p.res = res, p.ldr = p.ldc;
  return launch_conv(p, c.w_hl, s, xp, nc);
}

// InstanceNorm (+ReLU) (+skip add + ReLU), in place on y.  planes_only: the normalised map is only ever read by a split-fp16
// convolution (through out.hi / out.lo), so its f32 copy is not written (y keeps the raw convolution output)
inline int run_inorm(NormCtx& nc, float* y, int n, long hw, int C, int relu1, const float* skip, bool dry, hipStream_t s,
                     Planes out = Planes(), bool planes_only = false) {
  if (dry) return SAMPT_OK;
  if (nc.chunks > 0) SAMPT_TRY(instnorm_finalize(nc.partials, n, nc.chunks, hw, C, 1e-5f, nc.mean_rstd, s));
  else SAMPT_TRY(instnorm_stats(y, n, hw, C, 1e-5f, nc.partials, nc.mean_rstd, s));
  nc.chunks = 0;
  return instnorm_apply(y, nc.mean_rstd, skip, planes_only && out.hi ? nullptr : y, n, hw, C, relu1, s, out.hi, out.lo);
}

// Every InstanceNorm output that feeds a split-fp16 convolution is also written as two fp16 planes (same bytes as the
// f32 map): the convolution then stages ready-made halves instead of splitting each element once per filter tap.
inline Planes planes_for(Arena& ws, size_t elems, const ConvW& consumer) {
  Planes pl;
  if (consumer.w_hl) pl.hi = ws.f16(elems), pl.lo = ws.f16(elems);
  return pl;
}

// SAM's neck (ImageEncoderViT.neck; the TinyViT encoder ends in the same one): conv1x1 (no bias) -> LayerNorm2d -> conv3x3, pad 1 (no
// bias) -> LayerNorm2d over the token map x [B g g][D] -> features [B g g][C].  Each convolution has exact f32 weights (w0 [C][D],
// w2 [C][3][3][C]) or, with those null, their split-fp16 planes (hl0, hl2): fp32 grade either way.  a, b: scratch [B g g][C] each.
struct NeckW {
  const void *w0 = nullptr, *w2 = nullptr;
  const half_t *hl0 = nullptr, *hl2 = nullptr;
  const float *n1w = nullptr, *n1b = nullptr, *n3w = nullptr, *n3b = nullptr;
};
inline int sam_neck(const NeckW& n, const float* x, int B, int g, int D, int C, float* a, float* b, float* features, hipStream_t s) {
  const long Mg = (long)B * g * g;
  GemmP p0 = gemm_linear(x, D, n.w0, nullptr, a, C, (int)Mg, C, D);
  if (n.hl0) {
    gemm_split_planes(p0, n.hl0);
    SAMPT_TRY(conv_f16x3(p0, s));
  } else {
    SAMPT_TRY(gemm_f32(p0, s));
  }
  // (split-fp16 neck: the first LayerNorm2d writes its output as the two fp16 planes the halo-tiled 3 x 3 convolution stages by
  //  LDS-DMA — same bytes as the f32 map in the same buffer, same hi / lo values the tiled kernel split on the fly, ~165 -> 110 us
  //  per 8 frames (profiles/r6_c40_*); conv_halo_x3.hip)
  const bool planes = n.hl2 && g_conv_halo && C % 256 == 0 && C <= 1536;
  SAMPT_TRY(layernorm_rows(a, n.n1w, n.n1b, b, Mg, C, 1e-6f, nullptr, planes ? 3 : 0, ACT_NONE, s));
  const ConvW neck2{(const float*)n.w2, nullptr, n.hl2, C, C, 3, 3, 1, 1, 1};
  Planes xp;
  if (planes) xp.hi = (half_t*)b, xp.lo = (half_t*)b + (size_t)Mg * C;
  int oh, ow;
  SAMPT_TRY(run_conv(neck2, b, B, g, g, a, 0, ACT_NONE, nullptr, oh, ow, false, s, xp));
  return layernorm_rows(a, n.n3w, n.n3b, features, Mg, C, 1e-6f, nullptr, 0, ACT_NONE, s);
}

// One BasicEncoder residual block (extractor.py ResidualBlock) on cur [n][h][w][cin] (+ its planes); cur / cur_p / h / w become
// the block's output.  next: the convolution that reads the output (null: none does), for its planes.
//   instance: InstanceNorm after each convolution, the skip folded into the last instnorm_apply;
//   otherwise (norms folded into the weights): ReLU in the convolutions' epilogues, raft_add_relu for the skip.
// nc2 takes conv2's statistics, which are summed before the downsample branch's InstanceNorm uses nc.partials; a caller
// without a second buffer passes nc twice and conv2 then leaves the statistics to the InstanceNorm.
inline int res_block(const ConvW (&b)[3], bool instance, const ConvW* next, float*& cur, Planes& cur_p, int n, int& h, int& w,
                     NormCtx& nc, NormCtx& nc2, Arena& ws, hipStream_t s) {
  const bool dry = ws.dry();
  const ConvW &c1 = b[0], &c2 = b[1];
  const int C = c1.cout, act = instance ? ACT_NONE : ACT_RELU;
  const int oh = (h + 2 - 3) / c1.stride + 1, ow = (w + 2 - 3) / c1.stride + 1;
  const size_t oel = (size_t)n * oh * ow * C;
  float *y1 = ws.f32(oel), *y2 = ws.f32(oel);
  Planes y1_p = planes_for(ws, oel, c2), y2_p = next ? planes_for(ws, oel, *next) : Planes();
  int t0, t1;
  SAMPT_TRY(run_conv(c1, cur, n, h, w, y1, C, act, nullptr, t0, t1, dry, s, cur_p, instance ? &nc : nullptr));
  if (instance) SAMPT_TRY(run_inorm(nc, y1, n, (long)oh * ow, C, 1, nullptr, dry, s, y1_p, true));   // y1 feeds conv2 only
  SAMPT_TRY(run_conv(c2, y1, n, oh, ow, y2, C, act, nullptr, t0, t1, dry, s, y1_p, instance && &nc2 != &nc ? &nc2 : nullptr));
  const float* skip = cur;
  if (c1.stride != 1) {
    float* dn = y1;  // y1 is dead after conv2 has consumed it (stream order)
    SAMPT_TRY(run_conv(b[2], cur, n, h, w, dn, C, ACT_NONE, nullptr, t0, t1, dry, s, cur_p));
    if (instance) SAMPT_TRY(run_inorm(nc, dn, n, (long)oh * ow, C, 0, nullptr, dry, s));
    skip = dn;
  }
  if (instance) SAMPT_TRY(run_inorm(nc2, y2, n, (long)oh * ow, C, 1, skip, dry, s, y2_p));   // relu(skip + relu(norm(y2)))
  else if (!dry) SAMPT_TRY(raft_add_relu(y2, skip, y2, (long)oel, s));
  cur = y2, cur_p = y2_p, h = oh, w = ow;
  return SAMPT_OK;
}

}  // namespace sampt
