// The cost-volume heads of TAPIR and TapNet as ONE kernel body (tracks_from_cost_volume + soft_argmax_heatmap / heatmaps_to_points of
// sam_pt/point_tracker/tapir/tapir_model.py:349-417 and sam_pt/point_tracker/tapnet/tapnet_model.py:63-167, 247-305), instantiated by
// tapir.hip and tapnet.hip.  The two models differ in three places, the template's parameters:
//   TEMP      softmax temperature (TAPIR 20, TapNet 10)
//   NOUT      outputs of the last Linear (TAPIR 2: occlusion, expected_dist; TapNet 1: occlusion)
//   OCC_RELU  whether the stride-2 occlusion convolution is followed by ReLU before its mean (TAPIR yes, TapNet no)
// One workgroup per (query, frame): the 1024 dot products, conv 1 -> 16 + ReLU (64 KiB, LDS only), conv 16 -> 1, first-maximum argmax,
// the softmax-weighted mean over the radius-5 disk, the occlusion branch, the query-frame override.  Geometry: 256 x 256 frames, a
// 32 x 32 x 256 channel-normalised grid per frame (NHWC f32).
#pragma once
#include "dyn_lds.h"
#include "ops.h"

namespace sampt {

constexpr int TP_SIZE = 256, TP_LG = 32, TP_LC = 256;

constexpr int HD_CELLS = TP_LG * TP_LG;                                   // 1024
constexpr int HD_LDS_FLOATS = 2 * HD_CELLS + 16 * HD_CELLS + 64;          // cost, logits, hidden [16][1024], scratch
constexpr size_t HD_LDS_BYTES = (size_t)HD_LDS_FLOATS * sizeof(float);    // 74 KiB

template <int TEMP, int NOUT, bool OCC_RELU>
__global__ __launch_bounds__(256) void k_cost_volume_heads(const float* __restrict__ lowres, int T, const float* __restrict__ qf, int ldq,
                                                           int qoff, const float* __restrict__ q, TapirHeadW w, float* __restrict__ pts,
                                                           float* __restrict__ occ, float* __restrict__ expd, float* __restrict__ iter_out) {
  extern __shared__ float hd_lds[];
  float* cost = hd_lds;
  float* logit = hd_lds + HD_CELLS;
  float* hid = hd_lds + 2 * HD_CELLS;           // [16][1024]; later the occlusion map [32][256]
  float* red = hid + 16 * HD_CELLS;             // 64 floats
  const int item = blockIdx.x, qi = item / T, t = item - qi * T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- 1. cost[cell] = <query feature, lowres[t][cell]>: a wave per cell, 4 cells in flight
  {
    const float4 qv = *(const float4*)(qf + (long)qi * ldq + qoff + lane * 4);
    const float* fm = lowres + (long)t * HD_CELLS * TP_LC + lane * 4;
    for (int c0 = wave * 4; c0 < HD_CELLS; c0 += 16) {
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 v = *(const float4*)(fm + (long)(c0 + j) * TP_LC);
        d[j] = qv.x * v.x + qv.y * v.y + qv.z * v.z + qv.w * v.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = wave_sum(d[j]);
      if (lane < 4) cost[c0 + lane] = lane == 0 ? d[0] : (lane == 1 ? d[1] : (lane == 2 ? d[2] : d[3]));
    }
  }
  __syncthreads();

  // ---- 2. hidden = relu(conv3x3(cost) + b1), 16 channels, zero padding
  for (int cell = tid; cell < HD_CELLS; cell += 256) {
    const int y = cell >> 5, x = cell & 31;
    float nb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
      nb[k] = (yy >= 0 && yy < TP_LG && xx >= 0 && xx < TP_LG) ? cost[yy * TP_LG + xx] : 0.f;
    }
    for (int ch = 0; ch < 16; ++ch) {
      float a = w.b1[ch];
#pragma unroll
      for (int k = 0; k < 9; ++k) a += w.w1[ch * 9 + k] * nb[k];
      hid[ch * HD_CELLS + cell] = fmaxf(a, 0.f);
    }
  }
  __syncthreads();

  // ---- 3. logits = conv3x3(hidden) + b2; the thread's first maximum over its cells (increasing cell order)
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  for (int cell = tid; cell < HD_CELLS; cell += 256) {
    const int y = cell >> 5, x = cell & 31;
    float a = w.b2[0];
    for (int ch = 0; ch < 16; ++ch) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        if (yy >= 0 && yy < TP_LG && xx >= 0 && xx < TP_LG) a += w.w2[ch * 9 + k] * hid[ch * HD_CELLS + yy * TP_LG + xx];
      }
    }
    logit[cell] = a;
    if (a > best) best = a, best_i = cell;
  }
  // ---- 4. argmax with the first-maximum rule: larger value wins, equal values -> smaller cell index.  The maximum is taken over the
  //         LOGITS; the reference (and tests/tapir_ref.py) takes it over the f32 softmax values.  exp is monotonic, so the two agree
  //         unless two distinct logits round to one softmax value (a gap below ~ 2^-24 / 20 relative to the spread), where the
  //         reference picks the earlier cell and this kernel the larger logit.  The soft average that follows starts from cells whose
  //         weights are then equal to f32, so the point moves by at most the distance between the two cells' disk means.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    if (ov > best || (ov == best && oi < best_i)) best = ov, best_i = oi;
  }
  if (lane == 0) red[wave] = best, red[4 + wave] = __int_as_float(best_i);
  __syncthreads();
  best = red[0], best_i = __float_as_int(red[4]);
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float ov = red[k];
    const int oi = __float_as_int(red[4 + k]);
    if (ov > best || (ov == best && oi < best_i)) best = ov, best_i = oi;
  }

  // ---- 5. softmax(TEMP logits)-weighted mean of the cell centres within 5 cells of the best one (wave 0; the softmax normaliser
  //         cancels between the two sums, and the 1e-12 floor of the reference cannot act: the best cell alone weighs >= 1 / 1024)
  float px = 0.f, py = 0.f;
  if (wave == 0) {
    const int by = best_i >> 5, bx = best_i & 31;
    const float m20 = __fmul_rn(best, (float)TEMP);
    float sw = 0.f, sx = 0.f, sy = 0.f;
    for (int k = lane; k < 81; k += 64) {
      const int dy = k / 9 - 4, dx = k % 9 - 4, yy = by + dy, xx = bx + dx;
      if (dy * dy + dx * dx < 25 && yy >= 0 && yy < TP_LG && xx >= 0 && xx < TP_LG) {
        const float e = expf(__fsub_rn(__fmul_rn(logit[yy * TP_LG + xx], (float)TEMP), m20));
        sw += e, sx += e * ((float)xx + 0.5f), sy += e * ((float)yy + 0.5f);
      }
    }
    sw = wave_sum(sw), sx = wave_sum(sx), sy = wave_sum(sy);
    px = sx / sw * ((float)TP_SIZE / TP_LG), py = sy / sw * ((float)TP_SIZE / TP_LG);
  }

  // ---- 6. occlusion: conv3x3 stride 2 (SAME: nothing before, one after) 16 -> 32 (+ ReLU where OCC_RELU), mean over 16 x 16,
  //         Linear 32 -> 16 + ReLU, Linear 16 -> NOUT.  One output cell per thread, 32 channels in registers.
  float acc[32];
#pragma unroll
  for (int oc = 0; oc < 32; ++oc) acc[oc] = w.b3[oc];
  {
    const int oy = tid >> 4, ox = tid & 15;
    for (int ch = 0; ch < 16; ++ch) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int yy = 2 * oy + k / 3, xx = 2 * ox + k % 3;
        const float v = (yy < TP_LG && xx < TP_LG) ? hid[ch * HD_CELLS + yy * TP_LG + xx] : 0.f;
        const float* wk = w.w3 + (ch * 9 + k) * 32;
#pragma unroll
        for (int oc = 0; oc < 32; ++oc) acc[oc] += wk[oc] * v;
      }
    }
  }
  __syncthreads();                                  // every read of hid is done: reuse it as [32][256]
#pragma unroll
  for (int oc = 0; oc < 32; ++oc) hid[oc * 256 + tid] = OCC_RELU ? fmaxf(acc[oc], 0.f) : acc[oc];
  __syncthreads();
  for (int oc = wave * 8; oc < wave * 8 + 8; ++oc) {
    float sacc = hid[oc * 256 + lane];
    sacc += hid[oc * 256 + 64 + lane];
    sacc += hid[oc * 256 + 128 + lane];
    sacc += hid[oc * 256 + 192 + lane];
    sacc = wave_sum(sacc);
    if (lane == 0) red[8 + oc] = sacc * (1.f / 256.f);
  }
  __syncthreads();
  if (tid == 0) {
    float h4v[16];
    for (int j = 0; j < 16; ++j) {
      float a = w.b4[j];
      for (int i = 0; i < 32; ++i) a += w.w4[j * 32 + i] * red[8 + i];
      h4v[j] = fmaxf(a, 0.f);
    }
    float o2[2] = {0.f, 0.f};
    for (int k = 0; k < NOUT; ++k) {
      float a = w.b5[k];
      for (int j = 0; j < 16; ++j) a += w.w5[k * 16 + j] * h4v[j];
      o2[k] = a;
    }
    // ---- 7. on the query's own frame the query point is returned verbatim (model_utils.py:186-204)
    if ((int)rintf(q[qi * 3]) == t) px = q[qi * 3 + 1], py = q[qi * 3 + 2];
    pts[(long)item * 2] = px, pts[(long)item * 2 + 1] = py;
    occ[item] = o2[0];
    if (NOUT == 2) expd[item] = o2[1];
    if (iter_out) *(float4*)(iter_out + (long)item * 4) = make_float4(px, py, o2[0], o2[1]);
  }
}

// one workgroup per (query, frame).  expd is written where NOUT == 2 only; iter_out (optional) [n T][4] = (x, y, o[0], o[1] or 0)
template <int TEMP, int NOUT, bool OCC_RELU>
int cost_volume_heads(const char* who, const float* lowres, int T, const float* qf, int ldq, int qoff, const float* q, int n, const TapirHeadW& w,
                      float* pts, float* occ, float* expd, float* iter_out, hipStream_t s) {
  if (!lowres || !qf || !q || !pts || !occ || T < 1 || n < 1 || ldq < TP_LC || qoff < 0 || qoff + TP_LC > ldq || (ldq % 4) || (qoff % 4))
    return SAMPT_ERR_ARG;
  if ((long)n * T > 0x7fffffffL) return SAMPT_ERR_ARG;
  if (!w.w1 || !w.b1 || !w.w2 || !w.b2 || !w.w3 || !w.b3 || !w.w4 || !w.b4 || !w.w5 || !w.b5) return SAMPT_ERR_ARG;
  // 74 KiB of dynamic LDS, above the default 64 KiB limit (gfx950: 160 KiB per CU)
  auto kern = k_cost_volume_heads<TEMP, NOUT, OCC_RELU>;
  static DeviceOnce once;
  SAMPT_TRY(allow_dynamic_lds(once, (const void*)kern, (int)HD_LDS_BYTES, who));
  hipLaunchKernelGGL(kern, dim3((unsigned)((long)n * T)), dim3(256), HD_LDS_BYTES, s, lowres, T, qf, ldq, qoff, q, w, pts, occ, expd, iter_out);
  SAMPT_CHECK_LAUNCH(who);
  return SAMPT_OK;
}

}  // namespace sampt
