// Patch-similarity filter of SamPt._track_points (reference sam_pt.py:597-690) in one launch: CIELAB taps, similarity, the two
// rejection scans and, on request, the border rule.  The arithmetic follows the host restatement (sam_pt_amd/sam_pt.py:
// rgb2lab + SamPt._patch_similarity_filter) operation by operation; this file is compiled with -ffp-contract=off and every fused
// multiply-add below is written out because the host's grid_sample has it there.
//
//   rgb   uint8 [T][3][H][W]      query f32 [N][3] = (t, x, y)      traj f32 [T][N][2]      vis_in f32 [T][N]
//   vis_out f32 [T][N]            sim_out f32 [T][N] or null
//
// One workgroup of 256 threads per point.  Nothing but the pixels under a tap's four bilinear corners is ever converted to Lab:
//   Lab of a pixel   the channels are swapped [2, 1, 0] first (sam_pt.py:645); sRGB companding is a 256-entry float64 table the host
//                    computes with its own arithmetic (bit-equal to rgb2lab's by construction); matrix, white point, cube root / linear
//                    branch in float64; the three results are rounded to f32, as the host rounds its Lab frame before sampling.
//   a tap            torch's grid_sample(align_corners=False, bilinear, zeros) on the CPU: g = ((x + d + 0.5) / w) * 2 - 1,
//                    i = fma(g + 1, w / 2, -0.5), weights from i - floor(i) and 1 - that, value = fma(se_v, se, fma(sw_v, sw,
//                    fma(ne_v, ne, nw_v * nw))); a corner outside the frame contributes 0.
//   similarity       exp(-sqrt(sum of squared differences over taps^2 * 3 values) / (2 ps^2)) in f32; the sum's order differs
//                    from the host's, the rest does not.
// Phase 1 writes the query patch to LDS.  Phase 2 gives every frame to a group of G lanes (G = the power of two that holds the taps,
// at most 64), which sums its squared differences with xor shuffles; the group's first lane writes the frame's first code to
// vis_out and folds a non-similar frame into the two LDS words "first hit after / before the query frame".  Phase 3 re-reads the
// codes, overwrites what lies beyond the hits and applies the border rule.
#include <limits.h>

#include "ops.h"

namespace sampt {

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_MAX_TAPS = 2 * (PATCH_FILTER_MAX_PATCH_SIZE / 2) + 1;

// Lab (f32) of pixel (px, py) of one frame; plane = H * W.  r / g / b are channels 2 / 1 / 0 of the frame.
__device__ __forceinline__ void pf_lab(const unsigned char* __restrict__ frame, long plane, long off, const double* tab, float* lab) {
  const double r = tab[frame[2 * plane + off]], g = tab[frame[plane + off]], b = tab[frame[off]];
  const double x = (r * 0.412453 + g * 0.357580 + b * 0.180423) / 0.95047;
  const double y = (r * 0.212671 + g * 0.715160 + b * 0.072169) / 1.0;
  const double z = (r * 0.019334 + g * 0.119193 + b * 0.950227) / 1.08883;
  const double fx = x > 0.008856 ? cbrt(x) : 7.787 * x + 16.0 / 116.0;
  const double fy = y > 0.008856 ? cbrt(y) : 7.787 * y + 16.0 / 116.0;
  const double fz = z > 0.008856 ? cbrt(z) : 7.787 * z + 16.0 / 116.0;
  lab[0] = (float)(116.0 * fy - 16.0);
  lab[1] = (float)(500.0 * (fx - fy));
  lab[2] = (float)(200.0 * (fy - fz));
}

// the bilinear Lab sample at (x, y) pixel coordinates of the tap (already x + d), grid_sample's arithmetic
__device__ __forceinline__ void pf_tap(const unsigned char* __restrict__ frame, int H, int W, float x, float y, const double* tab,
                                       float* out) {
  const float gx = __fdiv_rn(x + 0.5f, (float)W) * 2.f - 1.f;
  const float gy = __fdiv_rn(y + 0.5f, (float)H) * 2.f - 1.f;
  const float ix = fmaf(gx + 1.f, (float)W * 0.5f, -0.5f);
  const float iy = fmaf(gy + 1.f, (float)H * 0.5f, -0.5f);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float we = ix - x0, ww = 1.f - we, ws = iy - y0, wn = 1.f - ws;   // weights of the east / west columns, south / north rows
  const float wgt[4] = {wn * ww, wn * we, ws * ww, ws * we};              // nw, ne, sw, se
  out[0] = out[1] = out[2] = 0.f;
  const long plane = (long)H * W;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float cx = x0 + (float)(c & 1), cy = y0 + (float)(c >> 1);
    float lab[3] = {0.f, 0.f, 0.f};
    // (the comparisons are on floats: a coordinate too large for an int never reaches the conversion; NaN compares false)
    if (cx >= 0.f && cx < (float)W && cy >= 0.f && cy < (float)H) pf_lab(frame, plane, (long)(int)cy * W + (int)cx, tab, lab);
    if (c == 0) {
      out[0] = lab[0] * wgt[0], out[1] = lab[1] * wgt[0], out[2] = lab[2] * wgt[0];
    } else {
      out[0] = fmaf(lab[0], wgt[c], out[0]), out[1] = fmaf(lab[1], wgt[c], out[1]), out[2] = fmaf(lab[2], wgt[c], out[2]);
    }
  }
}

__device__ __forceinline__ bool pf_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

}  // namespace

__global__ __launch_bounds__(PF_THREADS) void k_patch_filter(const unsigned char* __restrict__ rgb, int T, int H, int W,
                                                             const float* __restrict__ query, const float* __restrict__ traj,
                                                             const float* __restrict__ vis_in, int N, int ps, int taps, int G,
                                                             float threshold, const double* __restrict__ companding, int border_rule,
                                                             float* __restrict__ vis_out, float* __restrict__ sim_out) {
  __shared__ double s_tab[256];
  __shared__ float s_qp[PF_MAX_TAPS * PF_MAX_TAPS * 3];
  __shared__ int s_hit[2];                                   // first hit after the query frame (min), first hit before it (max)
  const int n = blockIdx.x, tid = threadIdx.x;
  const int K = taps * taps, rad = ps / 2;
  const long frame_bytes = 3L * H * W;
  s_tab[tid] = companding[tid];                              // PF_THREADS == 256
  if (tid == 0) s_hit[0] = INT_MAX, s_hit[1] = -1;
  const float qtf = query[3L * n], qx = query[3L * n + 1], qy = query[3L * n + 2];
  // a query that cannot be sampled (non-finite, or a frame index outside the clip) makes every item of the point non-similar
  const bool q_ok = pf_finite(qtf) && pf_finite(qx) && pf_finite(qy) && qtf > -1.f && qtf < (float)T;
  const int t0 = q_ok ? (int)qtf : 0;                        // .long() / int(): truncation
  __syncthreads();
  if (q_ok)
    for (int k = tid; k < K; k += PF_THREADS)
      pf_tap(rgb + t0 * frame_bytes, H, W, qx + (float)(k / taps - rad), qy + (float)(k % taps - rad), s_tab, &s_qp[3 * k]);
  __syncthreads();

  // ---- phase 2: one frame per group of G lanes
  const int group = tid / G, lane = tid % G, n_groups = PF_THREADS / G;
  const float denom = (float)(2 * ps * ps);
  for (int tb = 0; tb < T; tb += n_groups) {                 // (uniform trip count: the shuffles below need every lane)
    const int t = tb + group;
    const bool live = t < T;
    const long item = live ? (long)t * N + n : 0;
    const float v = live ? vis_in[item] : 0.f;
    const bool need = live && (sim_out != nullptr || v == 1.f);
    const float x = need ? traj[2 * item] : 0.f, y = need ? traj[2 * item + 1] : 0.f;
    const bool ok = need && q_ok && pf_finite(x) && pf_finite(y);
    float acc = 0.f;
    if (ok)
      for (int k = lane; k < K; k += G) {
        float tp[3];
        pf_tap(rgb + t * frame_bytes, H, W, x + (float)(k / taps - rad), y + (float)(k % taps - rad), s_tab, tp);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = tp[c] - s_qp[3 * k + c];
          acc = fmaf(d, d, acc);
        }
      }
    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (need && lane == 0) {
      const float sim = ok ? expf(__fdiv_rn(-sqrtf(acc), denom)) : 0.f;
      if (sim_out) sim_out[item] = sim;
      const bool hit = v == 1.f && !(sim > threshold);       // (a NaN similarity is not similar)
      vis_out[item] = hit ? -3.f : v;
      if (hit && t > t0) atomicMin(&s_hit[0], t);
      if (hit && t < t0) atomicMax(&s_hit[1], t);
    } else if (live && lane == 0) {
      vis_out[item] = v;
    }
  }
  __syncthreads();                                           // (orders the vis_out stores above before the loads below, workgroup scope)

  // ---- phase 3: spread the rejection, then the border rule
  const int after = s_hit[0], before = s_hit[1];
  const float wf = (float)W, hf = (float)H;
  for (int t = tid; t < T; t += PF_THREADS) {
    const long item = (long)t * N + n;
    float c = vis_out[item];
    if (t > after || t < before) c = -4.f;
    if (border_rule) {
      const float x = traj[2 * item], y = traj[2 * item + 1];
      if (__fdiv_rn(x, wf) < 0.01f || __fdiv_rn(y, hf) < 0.01f || __fdiv_rn(x, wf) > 0.99f || __fdiv_rn(y, hf) > 0.99f) c = -2.f;
    }
    vis_out[item] = c;
  }
}

int patch_filter(const unsigned char* rgb, int T, int H, int W, const float* query, const float* traj, const float* vis_in, int N,
                 int patch_size, float threshold, const double* companding, int border_rule, float* vis_out, float* sim_out,
                 hipStream_t s) {
  if (T <= 0 || N <= 0 || H <= 0 || W <= 0 || patch_size < 1 || patch_size > PATCH_FILTER_MAX_PATCH_SIZE) return SAMPT_ERR_ARG;
  if (!rgb || !query || !traj || !vis_in || !companding || !vis_out) return SAMPT_ERR_ARG;
  const int taps = 2 * (patch_size / 2) + 1;
  int G = 1;
  while (G < taps * taps && G < 64) G <<= 1;
  hipLaunchKernelGGL(k_patch_filter, dim3(N), dim3(PF_THREADS), 0, s, rgb, T, H, W, query, traj, vis_in, N, patch_size, taps, G, threshold,
                     companding, border_rule ? 1 : 0, vis_out, sim_out);
  SAMPT_CHECK_LAUNCH("patch_filter");
  return SAMPT_OK;
}

}  // namespace sampt
