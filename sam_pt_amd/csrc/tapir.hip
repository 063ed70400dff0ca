// TAPIR point tracker kernels (sam_pt/point_tracker/tapir/: tapir_model.py, utils/model_utils.py).  Fixed geometry of the
// reference's adapter: 256 x 256 frames, hires map 64 x 64 x 128, lowres map 32 x 32 x 256 (NHWC f32, channel-normalised).
// Rows are (query, frame): row = q * T + t.  Queries are (t, x, y) in 256 x 256 pixels.
//
//   k_cost_volume_heads   (cost_volume_heads.h, shared with tapnet.hip) tracks_from_cost_volume (tapir_model.py:349-417) + soft_argmax_heatmap / heatmaps_to_points
//                         (model_utils.py:101-206), one workgroup per (query, frame): the 1024 dot products, conv 1 -> 16 + ReLU
//                         (64 KiB, LDS only), conv 16 -> 1, first-maximum argmax, the softmax-weighted mean over the radius-5 disk,
//                         the stride-2 occlusion convolution with its mean and two Linears, the query-frame override.  The dot
//                         products are taken here and not from a GEMM-made cost volume: the sums then have ONE order whatever the
//                         number of queries in the call is (the GEMM dispatcher picks its kernel by shape), and the 1 MiB map a
//                         workgroup streams is shared through L2 by the n workgroups of a frame.
//   k_tapir_patch_corr    refine_pips' 7 x 7 bilinear patches (tapir_model.py:440-487; interp(mode='constant'): a corner outside
//                         the map is zero) of both maps dotted with the query / previous-iteration features, written straight
//                         into the mixer's input row together with the row's constant and state columns.
//   k_tapir_temporal_mix  the time half of PIPsConvBlock (tapir_model.py:39-89,109-119): LayerNorm (scale only) -> depthwise k = 3
//                         x 4 -> tanh-GELU -> depthwise k = 3 -> sum of fours -> + skip, zero padding at the clip ends.
//   k_tapir_gemm          exact-f32 MFMA product with one K order per row (see above) for the mixer's Linears.
#include "cost_volume_heads.h"
#include "ops.h"

namespace sampt {

constexpr int TP_HG = 64, TP_HC = 128, TP_FEAT = 384, TP_DIM = 512;     // TP_SIZE, TP_LG, TP_LC: cost_volume_heads.h

// ---------------------------------------------------------------------------------------------- frames
__global__ void k_tapir_prep(const float* __restrict__ src, float* __restrict__ dst, long npix_total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix_total) return;
  const long hw = (long)TP_SIZE * TP_SIZE, t = i / hw, p = i - t * hw;
  const float* b = src + t * 3 * hw + p;
  ((float4*)dst)[i] = make_float4(b[0] * 2.f - 1.f, b[hw] * 2.f - 1.f, b[2 * hw] * 2.f - 1.f, 0.f);
}

int tapir_prep_frames(const float* chw, int T, float* dst, hipStream_t s) {
  if (!chw || !dst || T < 1) return SAMPT_ERR_ARG;
  const long n = (long)T * TP_SIZE * TP_SIZE;
  hipLaunchKernelGGL(k_tapir_prep, dim3(cdiv(n, 256)), dim3(256), 0, s, chw, dst, n);
  SAMPT_CHECK_LAUNCH("tapir_prep_frames");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- InstanceNorm with scale and offset
template <bool HL>
__global__ void k_instnorm_affine_apply(const float4* __restrict__ x, const float* __restrict__ mr, const float* __restrict__ scale,
                                        const float* __restrict__ offset, float4* __restrict__ y, long n4, long hwc4, int c4n, int relu,
                                        h4* __restrict__ y_hi, h4* __restrict__ y_lo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const long img = i / hwc4;
  const int c = (int)(i % c4n) * 4;
  const float* m = mr + (img * c4n * 4 + c) * 2;
  const float4 v = x[i];
  float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = (o[j] - m[2 * j]) * m[2 * j + 1] * scale[c + j] + offset[c + j];
    if (relu) o[j] = fmaxf(o[j], 0.f);
  }
  if (y) y[i] = make_float4(o[0], o[1], o[2], o[3]);
  if (HL) {
    const h4 hi = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
    const h4 lo = {(half_t)(o[0] - (float)hi[0]), (half_t)(o[1] - (float)hi[1]), (half_t)(o[2] - (float)hi[2]),
                   (half_t)(o[3] - (float)hi[3])};
    y_hi[i] = hi, y_lo[i] = lo;
  }
}

int instnorm_affine_apply(const float* x, const float* mean_rstd, const float* scale, const float* offset, float* y, int nimg, long hw,
                          int C, int relu, hipStream_t s, half_t* y_hi, half_t* y_lo) {
  if (!x || !mean_rstd || !scale || !offset || nimg < 1 || hw < 1 || C < 4 || C % 4 || (!y && !(y_hi && y_lo))) return SAMPT_ERR_ARG;
  const long n4 = (long)nimg * hw * C / 4;
  if (y_hi && y_lo)
    hipLaunchKernelGGL(k_instnorm_affine_apply<true>, dim3(cdiv(n4, 256)), dim3(256), 0, s, (const float4*)x, mean_rstd, scale, offset,
                       (float4*)y, n4, hw * C / 4, C / 4, relu, (h4*)y_hi, (h4*)y_lo);
  else
    hipLaunchKernelGGL(k_instnorm_affine_apply<false>, dim3(cdiv(n4, 256)), dim3(256), 0, s, (const float4*)x, mean_rstd, scale, offset,
                       (float4*)y, n4, hw * C / 4, C / 4, relu, (h4*)nullptr, (h4*)nullptr);
  SAMPT_CHECK_LAUNCH("instnorm_affine_apply");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- channel normalisation
// one wave per row: y = x / sqrt(max(sum x^2, 1e-12))      (tapir_model.py:621-634)
__global__ __launch_bounds__(256) void k_tapir_l2norm(const float* __restrict__ x, float* __restrict__ y, long rows, int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * C;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) ss += xr[c] * xr[c];
  ss = wave_sum(ss);
  const float d = sqrtf(fmaxf(ss, 1e-12f));
  for (int c = lane; c < C; c += 64) y[row * C + c] = xr[c] / d;
}

int tapir_l2norm_rows(const float* x, float* y, long rows, int C, hipStream_t s) {
  if (!x || !y || rows < 1 || C < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_l2norm, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, y, rows, C);
  SAMPT_CHECK_LAUNCH("tapir_l2norm_rows");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- query features
// model_utils.interp(mode='nearest') at (t, y - 0.5, x - 0.5) of the grid: bilinear with the corner indices clamped to the map
__device__ __forceinline__ float tp_read_clamped(const float* __restrict__ map, int G, int C, float gy, float gx, int c) {
  const float y = gy - 0.5f, x = gx - 0.5f;
  const float fy = floorf(y), fx = floorf(x);
  const float wy1 = y - fy, wx1 = x - fx, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
  const int y0 = (int)fminf(fmaxf(fy, -2.f), (float)G + 1.f), x0 = (int)fminf(fmaxf(fx, -2.f), (float)G + 1.f);   // (no int overflow)
  const int ya = min(max(y0, 0), G - 1), yb = min(max(y0 + 1, 0), G - 1), xa = min(max(x0, 0), G - 1), xb = min(max(x0 + 1, 0), G - 1);
  float v = (wy0 * wx0) * map[((long)ya * G + xa) * C + c];
  v += (wy0 * wx1) * map[((long)ya * G + xb) * C + c];
  v += (wy1 * wx0) * map[((long)yb * G + xa) * C + c];
  v += (wy1 * wx1) * map[((long)yb * G + xb) * C + c];
  return v;
}

__global__ __launch_bounds__(128) void k_tapir_query_feats(const float* __restrict__ hires, const float* __restrict__ lowres, int T,
                                                           const float* __restrict__ q, float* __restrict__ qf) {
  const int i = blockIdx.x;
  int t = (int)rintf(q[i * 3]);
  t = min(max(t, 0), T - 1);
  const float x = q[i * 3 + 1], y = q[i * 3 + 2];
  const float* hm = hires + (long)t * TP_HG * TP_HG * TP_HC;
  const float* lm = lowres + (long)t * TP_LG * TP_LG * TP_LC;
  for (int c = threadIdx.x; c < TP_FEAT; c += blockDim.x) {
    qf[(long)i * TP_FEAT + c] = c < TP_HC ? tp_read_clamped(hm, TP_HG, TP_HC, y * ((float)TP_HG / TP_SIZE), x * ((float)TP_HG / TP_SIZE), c)
                                          : tp_read_clamped(lm, TP_LG, TP_LC, y * ((float)TP_LG / TP_SIZE), x * ((float)TP_LG / TP_SIZE), c - TP_HC);
  }
}

int tapir_query_feats(const float* hires, const float* lowres, int T, const float* q, int n, float* qf, hipStream_t s) {
  if (!hires || !lowres || !q || !qf || T < 1 || n < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_query_feats, dim3(n), dim3(128), 0, s, hires, lowres, T, q, qf);
  SAMPT_CHECK_LAUNCH("tapir_query_feats");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- cost-volume heads
// the kernel is cost_volume_heads.h's, shared with TapNet (tapnet.hip): softmax temperature 20, two outputs of the last Linear
// (occlusion, expected_dist), ReLU after the stride-2 occlusion convolution
int tapir_heads(const float* lowres, int T, const float* qf, int ldq, int qoff, const float* q, int n, const TapirHeadW& w, float* pts,
                float* occ, float* expd, float* iter_out, hipStream_t s) {
  if (!expd) return SAMPT_ERR_ARG;
  return cost_volume_heads<20, 2, true>("tapir_heads", lowres, T, qf, ldq, qoff, q, n, w, pts, occ, expd, iter_out, s);
}

// ---------------------------------------------------------------------------------------------- patch correlation
// one 7 x 7 patch of one map for one row: a wave per sample, CPL channels per lane
template <int G, int C>
__device__ __forceinline__ void tp_patch(const float* __restrict__ map, float px, float py, const float* __restrict__ vec,
                                         float* __restrict__ out, int wave, int lane) {
  constexpr int CPL = C / 64;
  const float gx = px * ((float)G / TP_SIZE), gy = py * ((float)G / TP_SIZE);
  float qv[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) qv[j] = vec[lane * CPL + j];
  for (int sidx = wave; sidx < 49; sidx += 4) {
    const float y = (gy + (float)(sidx / 7 - 3)) - 0.5f, x = (gx + (float)(sidx % 7 - 3)) - 0.5f;
    const float fy = floorf(y), fx = floorf(x);
    const float wy1 = y - fy, wx1 = x - fx, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    // |coordinates| far outside the map (a point the mixer threw away) must not overflow the int conversion
    const int y0 = (int)fminf(fmaxf(fy, -4.f), (float)G + 4.f), x0 = (int)fminf(fmaxf(fx, -4.f), (float)G + 4.f);
    float val[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) val[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
      const float wgt = ((k >> 1) ? wy1 : wy0) * ((k & 1) ? wx1 : wx0);
      if (yy >= 0 && yy < G && xx >= 0 && xx < G) {           // uniform over the wave
        const float* p = map + ((long)yy * G + xx) * C + lane * CPL;
#pragma unroll
        for (int j = 0; j < CPL; ++j) val[j] += wgt * p[j];
      }
    }
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) d += val[j] * qv[j];
    d = wave_sum(d);
    if (lane == 0) out[sidx] = d;
  }
}

__global__ __launch_bounds__(256) void k_tapir_patch_corr(const float* __restrict__ hires, const float* __restrict__ lowres, int T,
                                                          const float* __restrict__ pos, const float* __restrict__ occ,
                                                          const float* __restrict__ expd, const float* __restrict__ feat, int feat_per_row,
                                                          float* __restrict__ x, int ldx) {
  const long row = blockIdx.x;
  const int qi = (int)(row / T), t = (int)(row - (long)qi * T);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* f = feat + (feat_per_row ? row : (long)qi) * TP_FEAT;
  float* xr = x + row * ldx;
  const float px = pos[row * 2], py = pos[row * 2 + 1];
  tp_patch<TP_HG, TP_HC>(hires + (long)t * TP_HG * TP_HG * TP_HC, px, py, f, xr + 4 + TP_FEAT, wave, lane);
  tp_patch<TP_LG, TP_LC>(lowres + (long)t * TP_LG * TP_LG * TP_LC, px, py, f + TP_HC, xr + 4 + TP_FEAT + 49, wave, lane);
  // the position slot is zeroed (tapir_model.py:528), then the state, then the features
  if (tid < 4) xr[tid] = tid < 2 ? 0.f : (tid == 2 ? occ[row] : expd[row]);
  for (int c = tid; c < TP_FEAT; c += 256) xr[4 + c] = f[c];
  for (int c = 4 + TP_FEAT + 98 + tid; c < ldx; c += 256) xr[c] = 0.f;
}

int tapir_patch_corr(const float* hires, const float* lowres, int T, int n, const float* pos, const float* occ, const float* expd,
                     const float* feat, int feat_per_row, float* x, int ldx, hipStream_t s) {
  if (!hires || !lowres || !pos || !occ || !expd || !feat || !x || T < 1 || n < 1 || ldx < 4 + TP_FEAT + 98) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_patch_corr, dim3((unsigned)((long)n * T)), dim3(256), 0, s, hires, lowres, T, pos, occ, expd, feat, feat_per_row,
                     x, ldx);
  SAMPT_CHECK_LAUNCH("tapir_patch_corr");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- temporal half-block
constexpr int TM_TT = 8;                 // frames per workgroup; the two k = 3 convolutions need LayerNorm rows t0 - 2 .. t0 + TT + 1

__device__ __forceinline__ float4 tm_gelu4(float4 v) { return make_float4(gelu_tanh(v.x), gelu_tanh(v.y), gelu_tanh(v.z), gelu_tanh(v.w)); }

__global__ __launch_bounds__(512) void k_tapir_temporal_mix(const float* __restrict__ x, float* __restrict__ xo, const float* __restrict__ ln,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, int T) {
  __shared__ float lnr[TM_TT + 4][TP_DIM];
  const int qi = blockIdx.x, t0 = blockIdx.y * TM_TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xq = x + (long)qi * T * TP_DIM;
  // ---- LayerNorm (scale only, eps 1e-5, biased variance) of rows t0 - 2 .. t0 + TT + 1; rows outside the clip are the zero padding
  for (int rr = wave; rr < TM_TT + 4; rr += 8) {
    const int t = t0 - 2 + rr;
    if (t >= 0 && t < T) {
      float v[8], sum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = xq[(long)t * TP_DIM + lane + 64 * j], sum += v[j];
      const float mean = wave_sum(sum) * (1.f / TP_DIM);
      float var = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) var += (v[j] - mean) * (v[j] - mean);
      const float rstd = 1.f / sqrtf(wave_sum(var) * (1.f / TP_DIM) + 1e-5f);
#pragma unroll
      for (int j = 0; j < 8; ++j) lnr[rr][lane + 64 * j] = (v[j] - mean) * rstd * ln[lane + 64 * j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) lnr[rr][lane + 64 * j] = 0.f;
    }
  }
  __syncthreads();
  // ---- channel c = tid: outputs 4c .. 4c+3 of the first convolution, their GELU, the second convolution, the sum of the four
  const int c = tid;
  float4 w1k[3], w2k[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) w1k[k] = *(const float4*)(w1 + (long)k * 4 * TP_DIM + 4 * c), w2k[k] = *(const float4*)(w2 + (long)k * 4 * TP_DIM + 4 * c);
  const float4 b1v = *(const float4*)(b1 + 4 * c), b2v = *(const float4*)(b2 + 4 * c);
  auto hidden = [&](int t) -> float4 {          // gelu(dw1(LN)) at frame t; zero outside the clip (the second convolution's padding)
    if (t < 0 || t >= T) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int rr = t - t0 + 2;
    const float a0 = lnr[rr - 1][c], a1 = lnr[rr][c], a2 = lnr[rr + 1][c];
    float4 v;
    v.x = a0 * w1k[0].x + a1 * w1k[1].x + a2 * w1k[2].x + b1v.x;
    v.y = a0 * w1k[0].y + a1 * w1k[1].y + a2 * w1k[2].y + b1v.y;
    v.z = a0 * w1k[0].z + a1 * w1k[1].z + a2 * w1k[2].z + b1v.z;
    v.w = a0 * w1k[0].w + a1 * w1k[1].w + a2 * w1k[2].w + b1v.w;
    return tm_gelu4(v);
  };
  float4 gm = hidden(t0 - 1), g0 = hidden(t0);
  for (int t = t0; t < t0 + TM_TT && t < T; ++t) {
    const float4 gp = hidden(t + 1);
    const float zx = gm.x * w2k[0].x + g0.x * w2k[1].x + gp.x * w2k[2].x + b2v.x;
    const float zy = gm.y * w2k[0].y + g0.y * w2k[1].y + gp.y * w2k[2].y + b2v.y;
    const float zz = gm.z * w2k[0].z + g0.z * w2k[1].z + gp.z * w2k[2].z + b2v.z;
    const float zw = gm.w * w2k[0].w + g0.w * w2k[1].w + gp.w * w2k[2].w + b2v.w;
    const long o = ((long)qi * T + t) * TP_DIM + c;
    xo[o] = zx + zy + zz + zw + x[o];
    gm = g0, g0 = gp;
  }
}

int tapir_temporal_mix(const float* x, float* xo, const float* ln, const float* w1, const float* b1, const float* w2, const float* b2,
                       int n, int T, hipStream_t s) {
  if (!x || !xo || x == xo || !ln || !w1 || !b1 || !w2 || !b2 || n < 1 || T < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_temporal_mix, dim3(n, cdiv(T, TM_TT)), dim3(512), 0, s, x, xo, ln, w1, b1, w2, b2, T);
  SAMPT_CHECK_LAUNCH("tapir_temporal_mix");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- GEMM with a fixed K order
// A workgroup owns 64 rows x 128 columns, a wave 64 x 32 as 4 x 2 fragments of v_mfma_f32_16x16x4_f32.  Operands go straight from
// global memory (L2-resident: at most a few MB) into the MFMA registers in gemm_thin_f32's arrangement: a lane loads 16 bytes of
// its A row and of its W row per 16-deep chunk, MFMA j of a chunk multiplies k = chunk * 16 + 4 (lane / 16) + j of both, and with the
// operands swapped lane (lr, lq) ends up with row lr and columns 4 lq .. 4 lq + 3 of each fragment.  Every output is ONE accumulator
// summed over the chunks in increasing order, so a row's bits do not depend on how many rows the call has.
__global__ __launch_bounds__(256) void k_tapir_gemm(const float* __restrict__ A, int lda, const float* __restrict__ W, const float* __restrict__ bias,
                                                    float* __restrict__ C, int ldc, int M, int N, int K, int act, const float* __restrict__ res,
                                                    int ldr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 128 + wave * 32;
  if (n0 >= N) return;
  const float* ap[4];
  const float* wp[2];
#pragma unroll
  for (int f = 0; f < 4; ++f) ap[f] = A + (long)min(m0 + f * 16 + lr, M - 1) * lda + lq * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) wp[j] = W + (long)min(n0 + j * 16 + lr, N - 1) * K + lq * 4;
  f32x4 acc[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nchunk = K >> 4;
  for (int c = 0; c < nchunk; ++c) {
    float4 av[4], wv[2];
#pragma unroll
    for (int f = 0; f < 4; ++f) av[f] = *(const float4*)(ap[f] + c * 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) wv[j] = *(const float4*)(wp[j] + c * 16);
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j].x, av[f].x, acc[f][j], 0, 0, 0);
        acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j].y, av[f].y, acc[f][j], 0, 0, 0);
        acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j].z, av[f].z, acc[f][j], 0, 0, 0);
        acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j].w, av[f].w, acc[f][j], 0, 0, 0);
      }
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int row = m0 + f * 16 + lr;
    if (row >= M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + j * 16 + lq * 4;
      if (col >= N) continue;
      float o[4] = {acc[f][j][0], acc[f][j][1], acc[f][j][2], acc[f][j][3]};
      if (bias) {
        const float4 b = *(const float4*)(bias + col);
        o[0] += b.x, o[1] += b.y, o[2] += b.z, o[3] += b.w;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = apply_act(o[r], act);
      if (res) {
        const float4 rv = *(const float4*)(res + (long)row * ldr + col);
        o[0] += rv.x, o[1] += rv.y, o[2] += rv.z, o[3] += rv.w;
      }
      *(float4*)(C + (long)row * ldc + col) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

int tapir_gemm(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, long M, int N, int K, int act, const float* res,
               int ldr, hipStream_t s) {
  if (!A || !W || !C || M < 1 || M > 0x7fffffffL || N < 4 || K < 16 || (K % 16) || (N % 4) || (lda % 4) || (ldc % 4) || lda < K || ldc < N ||
      (res && ((ldr % 4) || ldr < N)))
    return SAMPT_ERR_ARG;
  if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)C | (uintptr_t)bias | (uintptr_t)res) & 15) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_gemm, dim3(cdiv(N, 128), cdiv(M, 64)), dim3(256), 0, s, A, lda, W, bias, C, ldc, (int)M, N, K, act, res, ldr);
  SAMPT_CHECK_LAUNCH("tapir_gemm");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- state update
// refine_pips' outputs (tapir_model.py:556-566): position, occlusion, expected_dist and features each gain their slice of the mixer's row
__global__ __launch_bounds__(128) void k_tapir_update(const float* __restrict__ res, const float* __restrict__ qf, int first, float* __restrict__ pos,
                                                      float* __restrict__ occ, float* __restrict__ expd, float* __restrict__ feats,
                                                      float* __restrict__ iter_out, int T) {
  const long row = blockIdx.x;
  const float* r = res + row * (4 + TP_FEAT);
  const float* base = first ? qf + (row / T) * TP_FEAT : feats + row * TP_FEAT;
  for (int c = threadIdx.x; c < TP_FEAT; c += 128) feats[row * TP_FEAT + c] = base[c] + r[4 + c];
  if (threadIdx.x == 0) {
    const float px = pos[row * 2] + r[0], py = pos[row * 2 + 1] + r[1], o = occ[row] + r[2], e = expd[row] + r[3];
    pos[row * 2] = px, pos[row * 2 + 1] = py, occ[row] = o, expd[row] = e;
    if (iter_out) *(float4*)(iter_out + row * 4) = make_float4(px, py, o, e);
  }
}

int tapir_update(const float* res, const float* qf, int first, float* pos, float* occ, float* expd, float* feats, float* iter_out, int n, int T,
                 hipStream_t s) {
  if (!res || !qf || !pos || !occ || !expd || !feats || n < 1 || T < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapir_update, dim3((unsigned)((long)n * T)), dim3(128), 0, s, res, qf, first, pos, occ, expd, feats, iter_out, T);
  SAMPT_CHECK_LAUNCH("tapir_update");
  return SAMPT_OK;
}

}  // namespace sampt
