// Scoring tail of the automatic mask generator (sam_pt_amd/automatic_mask_generator.py) on low-res masks.
//
// The generator needs, per candidate mask, three pixel counts of the full-resolution logits (v > thr + off, v > thr - off,
// v > thr) and the bounding box of v > thr — and the full-resolution mask itself only for the few candidates that pass its
// filters.  amg_score evaluates Sam.postprocess_masks on the fly (sam_postprocess.h: the arithmetic of k_sam_postprocess,
// operation for operation, so the counts are those of the logits that kernel would write) and reduces the seven integers
// without ever writing a logit; amg_binarize writes v > thr as bytes for a list of rows.  Both are bandwidth-shaped:
// capped grids, grid-stride loops, wave-64 shuffles, integer partials + a final reducer (order-independent: bitwise
// reproducible, no atomics).
#include "ops.h"
#include "sam_postprocess.h"

namespace sampt {

namespace {
constexpr int AMG_MAX_BLOCKS = 32;     // workgroups per mask of the scoring pass (x N masks: the chip is full from N = 8 on)
constexpr int AMG_PIX_PER_BLOCK = 2048;

struct AmgAcc {
  int hi, lo, area, xmin, ymin, xmax, ymax;
};

__device__ __forceinline__ AmgAcc amg_wave_reduce(AmgAcc a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.hi += __shfl_xor(a.hi, o, 64);
    a.lo += __shfl_xor(a.lo, o, 64);
    a.area += __shfl_xor(a.area, o, 64);
    a.xmin = min(a.xmin, __shfl_xor(a.xmin, o, 64));
    a.ymin = min(a.ymin, __shfl_xor(a.ymin, o, 64));
    a.xmax = max(a.xmax, __shfl_xor(a.xmax, o, 64));
    a.ymax = max(a.ymax, __shfl_xor(a.ymax, o, 64));
  }
  return a;
}

// the 4 waves of a 256-thread workgroup -> thread 0 holds the workgroup's record
__device__ __forceinline__ AmgAcc amg_block_reduce(AmgAcc a, int (*red)[7]) {
  a = amg_wave_reduce(a);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = a.hi, red[wave][1] = a.lo, red[wave][2] = a.area, red[wave][3] = a.xmin, red[wave][4] = a.ymin;
    red[wave][5] = a.xmax, red[wave][6] = a.ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.hi = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    a.lo = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    a.area = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    a.xmin = min(min(red[0][3], red[1][3]), min(red[2][3], red[3][3]));
    a.ymin = min(min(red[0][4], red[1][4]), min(red[2][4], red[3][4]));
    a.xmax = max(max(red[0][5], red[1][5]), max(red[2][5], red[3][5]));
    a.ymax = max(max(red[0][6], red[1][6]), max(red[2][6], red[3][6]));
  }
  return a;
}
}  // namespace

// partial [N][gridDim.x][8]
__global__ __launch_bounds__(256) void k_amg_score(const float* __restrict__ low, int L, int img, int in_h, int in_w, int oh,
                                                   int ow, float thr, float thr_hi, float thr_lo, int* __restrict__ partial) {
  __shared__ int red[4][7];
  const int n = blockIdx.y;
  low += (long)n * L * L;
  const float s1 = (float)L / (float)img;
  const float sy = (float)in_h / (float)oh, sx = (float)in_w / (float)ow;
  AmgAcc a{0, 0, 0, 0x7fffffff, 0x7fffffff, -1, -1};
  const int npix = oh * ow;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int y = i / ow, x = i - y * ow;
    const float v = postprocess_pixel(low, L, s1, sy, sx, in_h, in_w, y, x);
    a.hi += v > thr_hi ? 1 : 0;
    a.lo += v > thr_lo ? 1 : 0;
    if (v > thr) {
      a.area += 1;
      a.xmin = min(a.xmin, x), a.xmax = max(a.xmax, x), a.ymin = min(a.ymin, y), a.ymax = max(a.ymax, y);
    }
  }
  a = amg_block_reduce(a, red);
  if (threadIdx.x == 0) {
    int* o = partial + ((long)n * gridDim.x + blockIdx.x) * 8;
    o[0] = a.hi, o[1] = a.lo, o[2] = a.area, o[3] = a.xmin, o[4] = a.ymin, o[5] = a.xmax, o[6] = a.ymax, o[7] = 0;
  }
}

// out [N][8] = {hi, lo, area, x0, y0, x1, y1 (inclusive; zeros when the mask is empty), 0}: one wave per mask
__global__ __launch_bounds__(64) void k_amg_score_final(const int* __restrict__ partial, int nb, int* __restrict__ out) {
  const int n = blockIdx.x;
  AmgAcc a{0, 0, 0, 0x7fffffff, 0x7fffffff, -1, -1};
  for (int i = threadIdx.x; i < nb; i += 64) {
    const int* o = partial + ((long)n * nb + i) * 8;
    a.hi += o[0], a.lo += o[1], a.area += o[2];
    a.xmin = min(a.xmin, o[3]), a.ymin = min(a.ymin, o[4]), a.xmax = max(a.xmax, o[5]), a.ymax = max(a.ymax, o[6]);
  }
  a = amg_wave_reduce(a);
  if (threadIdx.x == 0) {
    int* o = out + (long)n * 8;
    const bool empty = a.area == 0;
    o[0] = a.hi, o[1] = a.lo, o[2] = a.area;
    o[3] = empty ? 0 : a.xmin, o[4] = empty ? 0 : a.ymin, o[5] = empty ? 0 : a.xmax, o[6] = empty ? 0 : a.ymax, o[7] = 0;
  }
}

static int amg_blocks(int oh, int ow) {
  const int nb = cdiv((long)oh * ow, AMG_PIX_PER_BLOCK);
  return nb < 1 ? 1 : (nb > AMG_MAX_BLOCKS ? AMG_MAX_BLOCKS : nb);
}

size_t amg_score_workspace_bytes(int N) { return (size_t)(N > 0 ? N : 0) * AMG_MAX_BLOCKS * 8 * sizeof(int); }

int amg_score(const float* low, int N, int L, int img, int in_h, int in_w, int oh, int ow, double thr, double off, int* out8,
              void* ws, size_t ws_bytes, hipStream_t s) {
  if (N == 0) return SAMPT_OK;
  if (!low || !out8 || !ws || N < 0 || N > 65535 || L <= 0 || in_h <= 0 || in_w <= 0 || in_h > img || in_w > img || oh <= 0 ||
      ow <= 0 || (long)oh * ow >= (1L << 31) - 256L * AMG_MAX_BLOCKS)
    return SAMPT_ERR_ARG;
  if (ws_bytes < amg_score_workspace_bytes(N)) return SAMPT_ERR_WORKSPACE;
  const int nb = amg_blocks(oh, ow);
  // the thresholds as the comparison `float tensor > python float` sees them: the sum in double, rounded to float once
  hipLaunchKernelGGL(k_amg_score, dim3(nb, N), dim3(256), 0, s, low, L, img, in_h, in_w, oh, ow, (float)thr, (float)(thr + off),
                     (float)(thr - off), (int*)ws);
  SAMPT_CHECK_LAUNCH("amg_score");
  hipLaunchKernelGGL(k_amg_score_final, dim3(N), dim3(64), 0, s, (const int*)ws, nb, out8);
  SAMPT_CHECK_LAUNCH("amg_score_final");
  return SAMPT_OK;
}

// out bytes [R][oh][ow] = postprocess(low[rows[r]]) > thr.  A thread owns 16 consecutive bytes of the flat output (which may
// straddle rows and masks): one 16-byte store when the group is whole and `out` is 16-byte aligned, byte stores otherwise.
__global__ __launch_bounds__(256) void k_amg_binarize(const float* __restrict__ low, int N, const int* __restrict__ rows, int R, int L,
                                                      int img, int in_h, int in_w, int oh, int ow, float thr,
                                                      unsigned char* __restrict__ out, int aligned) {
  const float s1 = (float)L / (float)img;
  const float sy = (float)in_h / (float)oh, sx = (float)in_w / (float)ow;
  const long npix = (long)oh * ow, total = (long)R * npix, ngroups = (total + 15) / 16;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long)gridDim.x * 256) {
    const long e0 = g * 16;
    int r = (int)(e0 / npix);
    const long rem = e0 - (long)r * npix;
    int y = (int)(rem / ow), x = (int)(rem - (long)y * ow);
    int src = rows[r];
    unsigned int w[4] = {0u, 0u, 0u, 0u};
    const int cnt = (int)(total - e0 < 16 ? total - e0 : 16);
    for (int b = 0; b < cnt; ++b) {
      unsigned int bit = 0u;
      if (src >= 0 && src < N)            // (a row index outside the batch reads nothing and gives an empty mask)
        bit = postprocess_pixel(low + (long)src * L * L, L, s1, sy, sx, in_h, in_w, y, x) > thr ? 1u : 0u;
      w[b >> 2] |= bit << (8 * (b & 3));
      if (++x == ow) {
        x = 0;
        if (++y == oh) {
          y = 0, ++r;
          if (r < R) src = rows[r];
        }
      }
    }
    if (cnt == 16 && aligned) {
      *(uint4*)(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int b = 0; b < cnt; ++b) out[e0 + b] = (unsigned char)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
    }
  }
}

int amg_binarize(const float* low, int N, const int* rows, int R, int L, int img, int in_h, int in_w, int oh, int ow, double thr,
                 unsigned char* out, hipStream_t s) {
  if (R == 0) return SAMPT_OK;
  if (!low || !rows || !out || N <= 0 || R < 0 || L <= 0 || in_h <= 0 || in_w <= 0 || in_h > img || in_w > img || oh <= 0 || ow <= 0)
    return SAMPT_ERR_ARG;
  const long ngroups = ((long)R * oh * ow + 15) / 16;
  long nb = (ngroups + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(k_amg_binarize, dim3((unsigned)nb), dim3(256), 0, s, low, N, rows, R, L, img, in_h, in_w, oh, ow, (float)thr,
                     out, ((uintptr_t)out & 15) == 0 ? 1 : 0);
  SAMPT_CHECK_LAUNCH("amg_binarize");
  return SAMPT_OK;
}

}  // namespace sampt
