// TapNet point tracker kernels (sam_pt/point_tracker/tapnet/: tapnet_model.py, models/tsm_resnet.py, models/tsm_utils.py).  Fixed
// geometry of the reference's adapter: 256 x 256 frames, a 32 x 32 x 256 feature grid per frame (NHWC f32, channel-normalised).
// Rows are (query, frame): row = q * T + t.  Queries are (t, x, y) in 256 x 256 pixels.
//
//   k_tapnet_bn_shift     relu(BatchNorm(x)) with the moving statistics folded into a per-channel a, b on the host, and
//                         temporal_shift_gpu (tsm_utils.py:116-148) in ONE pass over [T][hw][C]: a thread reads four channels of one
//                         pixel once and writes them where the shift sends them — channels [0, n) of frame t become channels
//                         [C - n, C) of frame t + 1, channels [C - n, C) become channels [0, n) of frame t - 1, the rest stays —
//                         and, where the block projects its shortcut, also unshifted.  The two slots of the shifted map that no frame
//                         feeds (the clip's ends) are zeroed by the threads whose own value has nowhere to go.  n = 0: no shift.
//   k_tapnet_maxpool      hk.MaxPool 3 x 3, stride 2, "SAME": taps outside the map are skipped, not read as zero.
//   k_tapnet_query_feats  interp (tapnet_model.py:33-60) over the (T, 32, 32) grid of every channel: trilinear, every corner index
//                         clamped to the grid, the frame index included; t is not rounded.
//   heads                 cost_volume_heads.h with temperature 10, one output of the last Linear, no ReLU after the stride-2 convolution.
// This file is compiled without fma contraction (Makefile): the affine is a product and a sum, each rounded, as the host's a * x + b.
#include <algorithm>

#include "cost_volume_heads.h"
#include "ops.h"

namespace sampt {

// ---------------------------------------------------------------------------------------------- BatchNorm + ReLU + temporal shift
__device__ __forceinline__ void tn_store4(float4* __restrict__ y, h4* __restrict__ y_hi, h4* __restrict__ y_lo, long i, const float* o) {
  if (y) y[i] = make_float4(o[0], o[1], o[2], o[3]);
  if (y_hi) {          // the split of k_instnorm_affine_apply (tapir.hip)
    const h4 hi = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
    const h4 lo = {(half_t)(o[0] - (float)hi[0]), (half_t)(o[1] - (float)hi[1]), (half_t)(o[2] - (float)hi[2]),
                   (half_t)(o[3] - (float)hi[3])};
    y_hi[i] = hi, y_lo[i] = lo;
  }
}

// i indexes float4s of x [T][hw][C]; fhw4 = hw * C / 4 (one frame), c4n = C / 4, n4 = n / 4
__global__ __launch_bounds__(256) void k_tapnet_bn_shift(const float4* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                                                         long total4, long fhw4, int T, int c4n, int n4, float4* __restrict__ ys,
                                                         h4* __restrict__ ys_hi, h4* __restrict__ ys_lo, float4* __restrict__ yu,
                                                         h4* __restrict__ yu_hi, h4* __restrict__ yu_lo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int t = (int)(i / fhw4);
  const int c4 = (int)(i % c4n);
  const float4 v = x[i];
  const float4 av = *(const float4*)(a + c4 * 4), bv = *(const float4*)(b + c4 * 4);
  const float o[4] = {fmaxf(__fadd_rn(__fmul_rn(v.x, av.x), bv.x), 0.f), fmaxf(__fadd_rn(__fmul_rn(v.y, av.y), bv.y), 0.f),
                      fmaxf(__fadd_rn(__fmul_rn(v.z, av.z), bv.z), 0.f), fmaxf(__fadd_rn(__fmul_rn(v.w, av.w), bv.w), 0.f)};
  if (yu || yu_hi) tn_store4(yu, yu_hi, yu_lo, i, o);
  const float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (c4 < n4) {                              // -> channels [C - n, C) of frame t + 1; the last frame's value has no reader and this
    const long up = c4n - n4;                 //    thread zeroes the slot of frame 0 that no frame feeds
    if (t + 1 < T) tn_store4(ys, ys_hi, ys_lo, i + fhw4 + up, o);
    if (t == T - 1) tn_store4(ys, ys_hi, ys_lo, i - (long)t * fhw4 + up, z);
  } else if (c4 >= c4n - n4) {                // -> channels [0, n) of frame t - 1; frame 0's thread zeroes the slot of frame T - 1
    const long dn = c4n - n4;
    if (t > 0) tn_store4(ys, ys_hi, ys_lo, i - fhw4 - dn, o);
    if (t == 0) tn_store4(ys, ys_hi, ys_lo, i + (long)(T - 1) * fhw4 - dn, z);
  } else {
    tn_store4(ys, ys_hi, ys_lo, i, o);
  }
}

int tapnet_bn_shift(const float* x, const float* a, const float* b, int T, long hw, int C, int n, float* ys, half_t* ys_hi, half_t* ys_lo,
                    float* yu, half_t* yu_hi, half_t* yu_lo, hipStream_t s) {
  if (!x || !a || !b || T < 1 || hw < 1 || C < 4 || (C % 4) || n < 0 || (n % 4) || 2 * n > C) return SAMPT_ERR_ARG;
  if ((!ys && !(ys_hi && ys_lo)) || (ys_hi == nullptr) != (ys_lo == nullptr) || (yu_hi == nullptr) != (yu_lo == nullptr)) return SAMPT_ERR_ARG;
  const long fhw4 = hw * C / 4, total4 = (long)T * fhw4;
  if (cdiv(total4, 256) > 0x7fffffffL) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapnet_bn_shift, dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, s, (const float4*)x, a, b, total4, fhw4, T, C / 4, n / 4,
                     (float4*)ys, (h4*)ys_hi, (h4*)ys_lo, (float4*)yu, (h4*)yu_hi, (h4*)yu_lo);
  SAMPT_CHECK_LAUNCH("tapnet_bn_shift");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- max-pool
// x [n][H][W][C] -> y [n][OH][OW][C], OH = ceil(H / 2); "SAME": total = max((OH - 1) 2 + 3 - H, 0) rows of padding, floor(total / 2) before
__global__ __launch_bounds__(256) void k_tapnet_maxpool(const float4* __restrict__ x, float4* __restrict__ y, long total4, int H, int W, int c4n,
                                                        int OH, int OW, int py, int px) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c4 = (int)(i % c4n);
  long r = i / c4n;
  const int ox = (int)(r % OW);
  r /= OW;
  const int oy = (int)(r % OH);
  const long img = r / OH;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = 2 * oy - py + k / 3, xx = 2 * ox - px + k % 3;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const float4 v = x[((img * H + yy) * W + xx) * c4n + c4];
      m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
    }
  }
  y[i] = m;
}

int tapnet_maxpool(const float* x, float* y, int n, int H, int W, int C, hipStream_t s) {
  if (!x || !y || n < 1 || H < 1 || W < 1 || C < 4 || (C % 4)) return SAMPT_ERR_ARG;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const int py = std::max((OH - 1) * 2 + 3 - H, 0) / 2, px = std::max((OW - 1) * 2 + 3 - W, 0) / 2;
  const long total4 = (long)n * OH * OW * (C / 4);
  if (cdiv(total4, 256) > 0x7fffffffL) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapnet_maxpool, dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, s, (const float4*)x, (float4*)y, total4, H, W, C / 4, OH, OW,
                     py, px);
  SAMPT_CHECK_LAUNCH("tapnet_maxpool");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- query features
// position in the grid = (t T / T, y 32 / 256, x 32 / 256) (transforms.convert_grid_coordinates: coords * output size / input size),
// read at (t, y - 0.5, x - 0.5) as map_coordinates(order=1, mode='nearest') does: the two indices of an axis are floor and floor + 1,
// both clamped to the grid
__global__ __launch_bounds__(64) void k_tapnet_query_feats(const float* __restrict__ grid, int T, const float* __restrict__ q, float* __restrict__ qf) {
  const int i = blockIdx.x;
  const float ft = (float)T;
  const float tc = (q[i * 3] * ft) / ft;
  const float yc = (q[i * 3 + 2] * (float)TP_LG) / (float)TP_SIZE - 0.5f, xc = (q[i * 3 + 1] * (float)TP_LG) / (float)TP_SIZE - 0.5f;
  const float f3[3] = {floorf(tc), floorf(yc), floorf(xc)};
  const float w1[3] = {tc - f3[0], yc - f3[1], xc - f3[2]};
  const int lim[3] = {T, TP_LG, TP_LG};
  int i0[3], i1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int b = (int)fminf(fmaxf(f3[d], -2.f), (float)lim[d] + 1.f);        // (no int overflow)
    i0[d] = min(max(b, 0), lim[d] - 1), i1[d] = min(max(b + 1, 0), lim[d] - 1);
  }
  const int c = threadIdx.x * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int tt = (k & 4) ? i1[0] : i0[0], yy = (k & 2) ? i1[1] : i0[1], xx = (k & 1) ? i1[2] : i0[2];
    const float wgt = ((k & 4) ? w1[0] : 1.f - w1[0]) * ((k & 2) ? w1[1] : 1.f - w1[1]) * ((k & 1) ? w1[2] : 1.f - w1[2]);
    const float4 v = *(const float4*)(grid + (((long)tt * TP_LG + yy) * TP_LG + xx) * TP_LC + c);
    acc.x += wgt * v.x, acc.y += wgt * v.y, acc.z += wgt * v.z, acc.w += wgt * v.w;
  }
  *(float4*)(qf + (long)i * TP_LC + c) = acc;
}

int tapnet_query_feats(const float* grid, int T, const float* q, int n, float* qf, hipStream_t s) {
  if (!grid || !q || !qf || T < 1 || n < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tapnet_query_feats, dim3(n), dim3(TP_LC / 4), 0, s, grid, T, q, qf);
  SAMPT_CHECK_LAUNCH("tapnet_query_feats");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- cost-volume heads
int tapnet_heads(const float* grid, int T, const float* qf, const float* q, int n, const TapirHeadW& w, float* pts, float* occ, hipStream_t s) {
  return cost_volume_heads<10, 1, false>("tapnet_heads", grid, T, qf, TP_LC, 0, q, n, w, pts, occ, nullptr, nullptr, s);
}

}  // namespace sampt
