// Per-pixel arithmetic of Sam.postprocess_masks (low-res L x L -> img x img -> crop -> out_h x out_w, both bilinear with
// align_corners=False), shared by k_sam_postprocess (sam_decoder.hip) and the mask-scoring kernels (amg.hip): the latter
// evaluate the full-resolution logits on the fly and must see exactly the values the former writes.
#pragma once
#include "common.h"

namespace sampt {

__device__ __forceinline__ void src_index(int d, float scale, int in, int& i0, int& i1, float& l1) {
  float src = scale * ((float)d + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

__device__ __forceinline__ float up_sample(const float* __restrict__ low, int L, float s1, int Y, int X) {
  int y0, y1, x0, x1;
  float ly, lx;
  src_index(Y, s1, L, y0, y1, ly);
  src_index(X, s1, L, x0, x1, lx);
  float hy = 1.f - ly, hx = 1.f - lx;
  return hy * (hx * low[y0 * L + x0] + lx * low[y0 * L + x1]) + ly * (hx * low[y1 * L + x0] + lx * low[y1 * L + x1]);
}

// one output pixel (y, x) of Sam.postprocess_masks — the statements of k_sam_postprocess, in its operation order
__device__ __forceinline__ float postprocess_pixel(const float* __restrict__ low, int L, float s1, float sy, float sx, int in_h,
                                                   int in_w, int y, int x) {
  int Y0, Y1, X0, X1;
  float ly, lx;
  src_index(y, sy, in_h, Y0, Y1, ly);
  src_index(x, sx, in_w, X0, X1, lx);
  float v00 = up_sample(low, L, s1, Y0, X0);
  float v;
  if (ly == 0.f && lx == 0.f) {
    v = v00;
  } else {
    float v01 = up_sample(low, L, s1, Y0, X1), v10 = up_sample(low, L, s1, Y1, X0), v11 = up_sample(low, L, s1, Y1, X1);
    float hy = 1.f - ly, hx = 1.f - lx;
    v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
  }
  return v;
}

}  // namespace sampt
