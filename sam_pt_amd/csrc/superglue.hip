// SuperPoint + SuperGlue kernels of the SuperGlue point tracker (sam_pt/point_tracker/superglue/): everything between the
// convolutions / projections (gemm.hip) of the two networks.
//
// Layouts.  Feature maps are NHWC f32.  A frame's score map is dense [Hs][Ws] with Hs = 8 (H / 8), Ws = 8 (W / 8): the 8 x 8
// depth-to-space of superpoint.py:168-169 is the address the softmax kernel writes to.  Keypoints are (x, y) floats in
// torch.nonzero's row-major (y, x) order.  Descriptors and every GNN tensor are rows [keypoint][channel]; attention heads are
// BLOCKED (channel h * 64 + d) — pack.pack_superglue permutes the reference's interleaved heads (channel d * 4 + h).
//
// The file is compiled without fp contraction: the grey-scale conversion rounds every product and sum on its own, as the
// host does; the dot products below ask for their fmas by name.
#include <math.h>

#include "ops.h"

namespace sampt {

static __device__ __forceinline__ float neg_inf() { return -__builtin_huge_valf(); }

// ---------------------------------------------------------------------------------------------------------- grey
// torchvision's rgb_to_grayscale on uint8 (0.2989 r + 0.587 g + 0.114 b in f32, truncated back to uint8), then / 255
// (tracker.py:87, :107, :112).  dst NHWC4, channels 1..3 zero (the first convolution's K is padded to a float4).
__global__ void k_sg_grey(const uint8_t* __restrict__ src, float* __restrict__ dst, int T, long hw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * hw) return;
  const long t = i / hw, p = i - t * hw;
  const uint8_t* s = src + t * 3 * hw + p;
  const float l = (0.2989f * (float)s[0] + 0.587f * (float)s[hw]) + 0.114f * (float)s[2 * hw];
  const float g = (float)(uint8_t)l / 255.0f;
  *(float4*)(dst + i * 4) = make_float4(g, 0.f, 0.f, 0.f);
}

int sg_grey(const uint8_t* frames, int T, int H, int W, float* dst, hipStream_t s) {
  if (!frames || !dst || T < 1 || H < 1 || W < 1) return SAMPT_ERR_ARG;
  const long n = (long)T * H * W;
  hipLaunchKernelGGL(k_sg_grey, dim3(cdiv(n, 256)), dim3(256), 0, s, frames, dst, T, (long)H * W);
  SAMPT_CHECK_LAUNCH("k_sg_grey");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- 2 x 2 max-pool
__global__ void k_maxpool2x2(const float* __restrict__ src, float* __restrict__ dst, int n, int h, int w, int C) {
  const int oh = h / 2, ow = w / 2, c4 = C / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * oh * ow * c4) return;
  const int c = (int)(i % c4);
  long r = i / c4;
  const int x = (int)(r % ow);
  r /= ow;
  const int y = (int)(r % oh), img = (int)(r / oh);
  const float* p = src + (((long)img * h + 2 * y) * w + 2 * x) * C + c * 4;
  const float4 a = *(const float4*)p, b = *(const float4*)(p + C), d = *(const float4*)(p + (long)w * C),
               e = *(const float4*)(p + (long)w * C + C);
  float4 o;
  o.x = fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x));
  o.y = fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y));
  o.z = fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z));
  o.w = fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w));
  *(float4*)(dst + i * 4) = o;
}

int maxpool2x2_nhwc(const float* src, int n, int h, int w, int C, float* dst, hipStream_t s) {
  if (!src || !dst || n < 1 || h < 2 || w < 2 || C < 4 || C % 4) return SAMPT_ERR_ARG;
  const long total = (long)n * (h / 2) * (w / 2) * (C / 4);
  hipLaunchKernelGGL(k_maxpool2x2, dim3(cdiv(total, 256)), dim3(256), 0, s, src, dst, n, h, w, C);
  SAMPT_CHECK_LAUNCH("k_maxpool2x2");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- score map
// softmax over the 65 channels of a cell (one wave per cell), dustbin dropped, written depth-to-space (superpoint.py:166-169)
__global__ void k_sg_scores(const float* __restrict__ logits, int ld, long cells, int h8, int w8, float* __restrict__ dense) {
  const long cell = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  if (cell >= cells) return;
  const float* l = logits + cell * ld;
  const float a = l[lane], d = l[64];
  const float m = fmaxf(wave_max(a), d);
  const float e = expf(a - m), ed = expf(d - m);
  const float sum = wave_sum(e) + ed;
  const long per = (long)h8 * w8;
  const long f = cell / per, r = cell - f * per;
  const int cy = (int)(r / w8), cx = (int)(r - (long)cy * w8);
  dense[(f * h8 * 8 + cy * 8 + (lane >> 3)) * ((long)w8 * 8) + cx * 8 + (lane & 7)] = e / sum;
}

int sg_scores(const float* logits, int ld, int nimg, int h8, int w8, float* dense, hipStream_t s) {
  if (!logits || !dense || ld < 65 || nimg < 1 || h8 < 1 || w8 < 1) return SAMPT_ERR_ARG;
  const long cells = (long)nimg * h8 * w8;
  hipLaunchKernelGGL(k_sg_scores, dim3(cdiv(cells, 4)), dim3(256), 0, s, logits, ld, cells, h8, w8, dense);
  SAMPT_CHECK_LAUNCH("k_sg_scores");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- simple_nms
// One pass = one max_pool2d(kernel 2 r + 1, stride 1, padding r) over a 32 x 32 tile with its halo in LDS, rows then columns
// (the maximum is separable and exact), followed by the comparison that uses it (superpoint.py:51-66):
//   MODE 0: mask = (s == pool(s))
//   MODE 1: supp = pool(mask) > 0 ; ss = supp ? 0 : s
//   MODE 2: mask |= (ss == pool(ss)) & ~supp
// max_pool2d pads with -inf.  Equality on f32, so the result is defined to the bit by the score map.
template <int MODE>
__global__ void k_sg_nms_pass(const float* __restrict__ s, float* __restrict__ ss, uint8_t* __restrict__ supp,
                              uint8_t* __restrict__ mask, int H, int W, int r) {
  extern __shared__ float lds[];
  const int TW = 32 + 2 * r;
  float* a = lds;                 // [TW][TW]
  float* b = lds + TW * TW;       // [TW][32]: row maxima
  const long img = (long)blockIdx.z * H * W;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  for (int i = threadIdx.x; i < TW * TW; i += blockDim.x) {
    const int ty = i / TW, tx = i - ty * TW, y = y0 + ty - r, x = x0 + tx - r;
    float v = neg_inf();
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const long p = img + (long)y * W + x;
      v = MODE == 0 ? s[p] : (MODE == 1 ? (mask[p] ? 1.f : 0.f) : ss[p]);
    }
    a[i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TW * 32; i += blockDim.x) {
    const int ty = i / 32, tx = i - ty * 32;
    float m = neg_inf();
    for (int d = 0; d <= 2 * r; ++d) m = fmaxf(m, a[ty * TW + tx + d]);
    b[i] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * 32; i += blockDim.x) {
    const int ty = i / 32, tx = i - ty * 32, y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    float m = neg_inf();
    for (int d = 0; d <= 2 * r; ++d) m = fmaxf(m, b[(ty + d) * 32 + tx]);
    const long p = img + (long)y * W + x;
    const float c = a[(ty + r) * TW + tx + r];
    if (MODE == 0) {
      mask[p] = (c == m) ? 1 : 0;
    } else if (MODE == 1) {
      const bool sp = m > 0.f;
      supp[p] = sp ? 1 : 0;
      ss[p] = sp ? 0.f : s[p];
    } else {
      if (c == m && !supp[p]) mask[p] = 1;
    }
  }
}

// Threshold, remove_borders and the ordered compaction of one frame per workgroup (superpoint.py:173-190).  Row counts, an
// exclusive scan over the rows, then every row writes its survivors in x order: torch.nonzero's order.  count[f] is the TRUE
// number of survivors; nothing is written at or beyond `cap` (the caller turns count > cap into an error).
#define SG_MAX_ROWS 4096
__global__ void k_sg_compact(const float* __restrict__ s, const uint8_t* __restrict__ mask, int H, int W, float thr, int border,
                             int cap, float* __restrict__ kpts, float* __restrict__ kscores, int* __restrict__ count) {
  __shared__ int rowoff[SG_MAX_ROWS];
  const int f = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float* sf = s + (long)f * H * W;
  const uint8_t* mf = mask + (long)f * H * W;
  const int ylo = border > 0 ? border : 0, yhi = H - border, xlo = border > 0 ? border : 0, xhi = W - border;
  for (int y = wv; y < H; y += nw) {
    int c = 0;
    if (y >= ylo && y < yhi)
      for (int x = xlo + lane; x < xhi; x += 64) c += (mf[(long)y * W + x] && sf[(long)y * W + x] > thr) ? 1 : 0;
    c = (int)wave_sum((float)c);          // a row has fewer than 2^24 pixels: exact
    if (lane == 0) rowoff[y] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int y = 0; y < H; ++y) {
      const int c = rowoff[y];
      rowoff[y] = acc;
      acc += c;
    }
    count[f] = acc;
  }
  __syncthreads();
  float* kp = kpts + (long)f * cap * 2;
  float* ks = kscores + (long)f * cap;
  for (int y = wv + ylo; y < yhi; y += nw) {
    int base = rowoff[y];
    for (int xb = xlo; xb < xhi; xb += 64) {
      const int x = xb + lane;
      const bool keep = x < xhi && mf[(long)y * W + x] && sf[(long)y * W + x] > thr;
      const unsigned long long bal = __ballot(keep);
      const int o = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (keep && o < cap) {
        kp[2 * (long)o] = (float)x;
        kp[2 * (long)o + 1] = (float)y;
        ks[o] = sf[(long)y * W + x];
      }
      base += __popcll(bal);
    }
  }
}

size_t sg_nms_workspace_bytes(int nimg, int Hs, int Ws) {
  const size_t px = (size_t)nimg * Hs * Ws;
  return px * 4 + 2 * ((px + 255) & ~(size_t)255) + 256;
}

int sg_nms_compact(const float* scores, int nimg, int Hs, int Ws, int radius, float thr, int border, int cap, float* kpts,
                   float* kscores, int* count, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!scores || !kpts || !kscores || !count || !ws || nimg < 1 || Hs < 1 || Ws < 1 || radius < 0 || cap < 1) return SAMPT_ERR_ARG;
  if (radius > 16 || Hs > SG_MAX_ROWS || nimg > 65535) return SAMPT_ERR_UNSUPPORTED;
  if (ws_bytes < sg_nms_workspace_bytes(nimg, Hs, Ws)) return SAMPT_ERR_WORKSPACE;
  const size_t px = (size_t)nimg * Hs * Ws, pxa = (px + 255) & ~(size_t)255;
  float* ss = (float*)ws;
  uint8_t* supp = (uint8_t*)ws + px * 4;
  uint8_t* mask = supp + pxa;
  const int TW = 32 + 2 * radius;
  const size_t lds = (size_t)(TW * TW + TW * 32) * 4;
  dim3 grid(cdiv(Ws, 32), cdiv(Hs, 32), nimg), block(256);
  hipLaunchKernelGGL(k_sg_nms_pass<0>, grid, block, lds, s, scores, ss, supp, mask, Hs, Ws, radius);
  for (int round = 0; round < 2; ++round) {
    hipLaunchKernelGGL(k_sg_nms_pass<1>, grid, block, lds, s, scores, ss, supp, mask, Hs, Ws, radius);
    hipLaunchKernelGGL(k_sg_nms_pass<2>, grid, block, lds, s, scores, ss, supp, mask, Hs, Ws, radius);
  }
  SAMPT_CHECK_LAUNCH("k_sg_nms_pass");
  hipLaunchKernelGGL(k_sg_compact, dim3(nimg), dim3(256), 0, s, scores, mask, Hs, Ws, thr, border, cap, kpts, kscores, count);
  SAMPT_CHECK_LAUNCH("k_sg_compact");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- descriptors
static __device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per keypoint, one thread per channel: the channel L2-normalisation of the four neighbouring cells of the
// dense map (superpoint.py:195), sample_descriptors' coordinate transform and bilinear grid_sample (align_corners=True, zero
// padding; :84-93) and the second normalisation (:94-95).  dmap [nimg][h8 * w8][256] raw convDb output.
__global__ void k_sg_sample_desc(const float* __restrict__ dmap, int h8, int w8, const float* __restrict__ kpts,
                                 const int* __restrict__ count, int cap, float* __restrict__ out) {
  __shared__ float red[4];
  const int f = blockIdx.y, k = blockIdx.x, c = threadIdx.x;
  const int n = count ? min(count[f], cap) : cap;
  if (k >= n) return;
  const float* kp = kpts + ((long)f * cap + k) * 2;
  const float sx = (float)(w8 * 8) - 4.0f - 0.5f, sy = (float)(h8 * 8) - 4.0f - 0.5f;
  const float gx = ((kp[0] - 4.0f + 0.5f) / sx) * 2.0f - 1.0f, gy = ((kp[1] - 4.0f + 0.5f) / sy) * 2.0f - 1.0f;
  const float ix = ((gx + 1.0f) / 2.0f) * (float)(w8 - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(h8 - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
  const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};      // nw, ne, sw, se
  const float* base = dmap + (long)f * h8 * w8 * 256;
  float acc = 0.f;
  for (int q = 0; q < 4; ++q) {
    const int x = x0 + (q & 1), y = y0 + (q >> 1);
    const bool in = x >= 0 && x < w8 && y >= 0 && y < h8;      // uniform over the workgroup
    const float v = in ? base[((long)y * w8 + x) * 256 + c] : 0.f;
    const float nrm = sqrtf(block_sum256(v * v, red));
    acc += (v / fmaxf(nrm, 1e-12f)) * wgt[q];
  }
  const float nrm = sqrtf(block_sum256(acc * acc, red));
  out[((long)f * cap + k) * 256 + c] = acc / fmaxf(nrm, 1e-12f);
}

int sg_sample_descriptors(const float* dmap, int nimg, int h8, int w8, const float* kpts, const int* count, int cap, int launch_n,
                          float* out, hipStream_t s) {
  if (!dmap || !kpts || !out || nimg < 1 || nimg > 65535 || h8 < 1 || w8 < 1 || cap < 1 || launch_n < 0 || launch_n > cap) return SAMPT_ERR_ARG;
  if (launch_n == 0) return SAMPT_OK;
  hipLaunchKernelGGL(k_sg_sample_desc, dim3(launch_n, nimg), dim3(256), 0, s, dmap, h8, w8, kpts, count, cap, out);
  SAMPT_CHECK_LAUNCH("k_sg_sample_desc");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- keypoint encoder input
// normalize_keypoints (superglue.py:65-72) and the score: rows [n][4] = ((x - W / 2) / s, (y - H / 2) / s, score, 0), s = 0.7 max(W, H)
__global__ void k_sg_kenc_input(const float* __restrict__ kpts, const float* __restrict__ scores, int n, float cx, float cy,
                                float scale, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  *(float4*)(out + 4 * (long)i) = make_float4((kpts[2 * i] - cx) / scale, (kpts[2 * i + 1] - cy) / scale, scores[i], 0.f);
}

int sg_kenc_input(const float* kpts, const float* scores, int n, int H, int W, float* out, hipStream_t s) {
  if (!kpts || !scores || !out || n < 1) return SAMPT_ERR_ARG;
  const float scale = (float)(W > H ? W : H) * 0.7f;
  hipLaunchKernelGGL(k_sg_kenc_input, dim3(cdiv(n, 256)), dim3(256), 0, s, kpts, scores, n, (float)W / 2.0f, (float)H / 2.0f, scale, out);
  SAMPT_CHECK_LAUNCH("k_sg_kenc_input");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- ragged attention
// softmax(q k^T / 8) v for N queries and M keys of any size, 4 (or any number of) heads of 64 channels, exact f32, flash style:
// the N x M scores never leave the workgroup.  A workgroup = 16 queries of one head, 4 per wave; K / V go through LDS in
// tiles of 64 keys.  Scores: lane = key, 4 queries per K read (the queries' 4 values of a channel are one broadcast float4).
// Output: lane = channel, 4 queries per V read (the 4 probabilities of a key are one broadcast float4).
#define SGA_Q 16
__global__ void __launch_bounds__(256)
k_sg_attention(const float* __restrict__ q, int ldq, const float* __restrict__ k, const float* __restrict__ v, int ldkv,
               float* __restrict__ out, int ldo, int N, int M, float scale) {
  __shared__ float Ks[64][65];
  __shared__ float Vs[64][64];
  __shared__ float4 Qs[4][64];       // [wave][channel] -> its 4 queries
  __shared__ float4 Ps[4][64];       // [wave][key] -> its 4 queries
  const int h = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q0 = blockIdx.x * SGA_Q + wv * 4;
  {
    float t[4];
    for (int i = 0; i < 4; ++i) t[i] = q0 + i < N ? q[(long)(q0 + i) * ldq + h * 64 + lane] * scale : 0.f;
    Qs[wv][lane] = make_float4(t[0], t[1], t[2], t[3]);
  }
  float m[4], l[4], o[4];
  for (int i = 0; i < 4; ++i) m[i] = neg_inf(), l[i] = 0.f, o[i] = 0.f;
  for (int k0 = 0; k0 < M; k0 += 64) {
    __syncthreads();                  // the previous tile is consumed (and Qs is visible)
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
      const int r = i >> 6, c = i & 63;
      const bool in = k0 + r < M;
      Ks[r][c] = in ? k[(long)(k0 + r) * ldkv + h * 64 + c] : 0.f;
      Vs[r][c] = in ? v[(long)(k0 + r) * ldkv + h * 64 + c] : 0.f;
    }
    __syncthreads();
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int d = 0; d < 64; ++d) {
      const float kv = Ks[lane][d];
      const float4 qq = Qs[wv][d];
      s[0] = fmaf(qq.x, kv, s[0]), s[1] = fmaf(qq.y, kv, s[1]), s[2] = fmaf(qq.z, kv, s[2]), s[3] = fmaf(qq.w, kv, s[3]);
    }
    const bool valid = k0 + lane < M;
    float p[4], corr[4];
    for (int i = 0; i < 4; ++i) {
      const float sv = valid ? s[i] : neg_inf();
      const float mn = fmaxf(m[i], wave_max(sv));     // finite: the tile holds at least one key
      p[i] = valid ? expf(sv - mn) : 0.f;
      corr[i] = expf(m[i] - mn);                      // exp(-inf) = 0 on the first tile
      l[i] = l[i] * corr[i] + wave_sum(p[i]);
      m[i] = mn;
    }
    Ps[wv][lane] = make_float4(p[0], p[1], p[2], p[3]);
    __syncthreads();                  // uniform: every wave walks the same key tiles
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const float vv = Vs[j][lane];
      const float4 pp = Ps[wv][j];
      a[0] = fmaf(pp.x, vv, a[0]), a[1] = fmaf(pp.y, vv, a[1]), a[2] = fmaf(pp.z, vv, a[2]), a[3] = fmaf(pp.w, vv, a[3]);
    }
    for (int i = 0; i < 4; ++i) o[i] = o[i] * corr[i] + a[i];
  }
  for (int i = 0; i < 4; ++i)
    if (q0 + i < N) out[(long)(q0 + i) * ldo + h * 64 + lane] = o[i] / l[i];
}

int sg_attention(const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, int N, int M, int heads,
                 hipStream_t s) {
  if (!q || !k || !v || !out || N < 1 || M < 1 || heads < 1 || heads > 65535 || ldq < heads * 64 || ldkv < heads * 64 || ldo < heads * 64)
    return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_sg_attention, dim3(cdiv(N, SGA_Q), heads), dim3(256), 0, s, q, ldq, k, v, ldkv, out, ldo, N, M, 0.125f);
  SAMPT_CHECK_LAUNCH("k_sg_attention");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- log-domain Sinkhorn
// log_optimal_transport (superglue.py:145-174) on S [N][M] (row stride ld) without the (N + 1) x (M + 1) couplings matrix:
// entry (i, j) of it is S[i][j] inside and alpha = *bin on the dustbin row i = N and column j = M.
//   rows:  u[i] = log_mu[i] - logsumexp_j (Z[i][j] + v[j]),  i <= N;  log_mu = norm (i < N), log(M) + norm (i = N)
//   cols:  v[j] = log_nu[j] - logsumexp_i (Z[i][j] + u[i]),  j <= M;  log_nu = norm (j < M), log(N) + norm (j = M)
__global__ void k_sg_sinkhorn_rows(const float* __restrict__ S, int ld, int N, int M, const float* __restrict__ bin,
                                   const float* __restrict__ v, float* __restrict__ u, float norm, float log_last) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i > N) return;
  const float alpha = *bin;
  const float* row = S + (long)i * ld;
  float mx = neg_inf();
  for (int j = lane; j <= M; j += 64) mx = fmaxf(mx, ((i < N && j < M) ? row[j] : alpha) + v[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j <= M; j += 64) sum += expf((((i < N && j < M) ? row[j] : alpha) + v[j]) - mx);
  sum = wave_sum(sum);
  if (lane == 0) u[i] = (i < N ? norm : log_last) - (logf(sum) + mx);
}

#define SGC_WAVES 16
__global__ void __launch_bounds__(1024)
k_sg_sinkhorn_cols(const float* __restrict__ S, int ld, int N, int M, const float* __restrict__ bin, const float* __restrict__ u,
                   float* __restrict__ v, float norm, float log_last) {
  __shared__ float red_m[SGC_WAVES][64], red_s[SGC_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
  const float alpha = *bin;
  const bool in = j <= M;
  float mx = neg_inf(), sum = 0.f;
  if (in)
    for (int i = wv; i <= N; i += SGC_WAVES) {
      const float x = ((i < N && j < M) ? S[(long)i * ld + j] : alpha) + u[i];
      const float mn = fmaxf(mx, x);
      sum = sum * expf(mx - mn) + expf(x - mn);
      mx = mn;
    }
  red_m[wv][lane] = mx, red_s[wv][lane] = sum;
  __syncthreads();
  if (wv == 0 && in) {
    float gm = neg_inf();
    for (int w = 0; w < SGC_WAVES; ++w) gm = fmaxf(gm, red_m[w][lane]);
    float gs = 0.f;
    for (int w = 0; w < SGC_WAVES; ++w)
      if (red_s[w][lane] > 0.f) gs += red_s[w][lane] * expf(red_m[w][lane] - gm);     // a wave without rows holds (-inf, 0)
    v[j] = (j < M ? norm : log_last) - (logf(gs) + gm);
  }
}

int sg_sinkhorn(const float* S, int ld, int N, int M, const float* bin, int iters, float* u, float* v, hipStream_t s) {
  if (!S || !bin || !u || !v || N < 1 || M < 1 || ld < M || iters < 0) return SAMPT_ERR_ARG;
  const float norm = -logf((float)N + (float)M), log_m = logf((float)M) + norm, log_n = logf((float)N) + norm;
  if (hipMemsetAsync(u, 0, (size_t)(N + 1) * 4, s) != hipSuccess || hipMemsetAsync(v, 0, (size_t)(M + 1) * 4, s) != hipSuccess)
    return SAMPT_ERR_HIP;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_sg_sinkhorn_rows, dim3(cdiv(N + 1, 4)), dim3(256), 0, s, S, ld, N, M, bin, v, u, norm, log_m);
    hipLaunchKernelGGL(k_sg_sinkhorn_cols, dim3(cdiv(M + 1, 64)), dim3(64 * SGC_WAVES), 0, s, S, ld, N, M, bin, u, v, norm, log_n);
  }
  SAMPT_CHECK_LAUNCH("k_sg_sinkhorn");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- matches
// Z[i][j] = S[i][j] + u[i] + v[j] - norm is never written: its row and column maxima over the inner N x M block, the mutual
// check, exp and the threshold (superglue.py:266-276).  Ties go to the smallest index.
static __device__ __forceinline__ void argmax_merge(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
}

__global__ void k_sg_rowmax(const float* __restrict__ S, int ld, int N, int M, const float* __restrict__ u,
                            const float* __restrict__ v, float norm, float* __restrict__ max0, int* __restrict__ idx0) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const float ui = u[i];
  float bv = neg_inf();
  int bi = 0x7fffffff;
  for (int j = lane; j < M; j += 64) {
    const float z = ((S[(long)i * ld + j] + ui) + v[j]) - norm;
    if (z > bv || bi == 0x7fffffff) bv = z, bi = j;
  }
  for (int o = 32; o > 0; o >>= 1) argmax_merge(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) max0[i] = bv, idx0[i] = bi;
}

__global__ void __launch_bounds__(1024)
k_sg_colmax(const float* __restrict__ S, int ld, int N, int M, const float* __restrict__ u, const float* __restrict__ v, float norm,
            int* __restrict__ idx1) {
  __shared__ float red_v[SGC_WAVES][64];
  __shared__ int red_i[SGC_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
  float bv = neg_inf();
  int bi = 0x7fffffff;
  if (j < M) {
    const float vj = v[j];
    for (int i = wv; i < N; i += SGC_WAVES) {
      const float z = ((S[(long)i * ld + j] + u[i]) + vj) - norm;
      if (z > bv || bi == 0x7fffffff) bv = z, bi = i;
    }
  }
  red_v[wv][lane] = bv, red_i[wv][lane] = bi;
  __syncthreads();
  if (wv == 0 && j < M) {
    for (int w = 1; w < SGC_WAVES; ++w) argmax_merge(bv, bi, red_v[w][lane], red_i[w][lane]);
    idx1[j] = bi;
  }
}

__global__ void k_sg_mutual(const float* __restrict__ max0, const int* __restrict__ idx0, const int* __restrict__ idx1, int N,
                            float thr, int* __restrict__ matches0, float* __restrict__ mscores0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int j = idx0[i];
  const bool mutual = idx1[j] == i;
  const float ms = mutual ? expf(max0[i]) : 0.f;
  matches0[i] = (mutual && ms > thr) ? j : -1;
  mscores0[i] = ms;
}

int sg_match_from_scores(const float* S, int ld, int N, int M, const float* u, const float* v, float thr, float* max0, int* idx0,
                         int* idx1, int* matches0, float* mscores0, hipStream_t s) {
  if (!S || !u || !v || !max0 || !idx0 || !idx1 || !matches0 || !mscores0 || N < 1 || M < 1 || ld < M) return SAMPT_ERR_ARG;
  const float norm = -logf((float)N + (float)M);
  hipLaunchKernelGGL(k_sg_rowmax, dim3(cdiv(N, 4)), dim3(256), 0, s, S, ld, N, M, u, v, norm, max0, idx0);
  hipLaunchKernelGGL(k_sg_colmax, dim3(cdiv(M, 64)), dim3(64 * SGC_WAVES), 0, s, S, ld, N, M, u, v, norm, idx1);
  hipLaunchKernelGGL(k_sg_mutual, dim3(cdiv(N, 256)), dim3(256), 0, s, max0, idx0, idx1, N, thr, matches0, mscores0);
  SAMPT_CHECK_LAUNCH("k_sg_match");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------------------- selection
// The tracker's per-mask split of the matched pairs (tracker.py:131-152), one wave per mask, in keypoint-0 order.  NOTE the
// reference's quirk, kept on purpose: the positives are the matched frame-i points whose OWN coordinates fall inside the
// frame-0 mask (``mkpts1_positive`` tests mkpts1 against the query mask), the negatives the complement by the same test.
// lists [n_masks][2][cap] = keypoint-1 indices (0: positives, 1: negatives), counts [n_masks][2].
__global__ void k_sg_select_lists(const int* __restrict__ matches0, int n0, const float* __restrict__ kpts1,
                                  const float* __restrict__ masks, int H, int W, int cap, int* __restrict__ lists,
                                  int* __restrict__ counts) {
  const int mi = blockIdx.x, lane = threadIdx.x;
  const float* mk = masks + (long)mi * H * W;
  int* lp = lists + (long)mi * 2 * cap;
  int* ln = lp + cap;
  int np = 0, nn = 0;
  for (int b = 0; b < n0; b += 64) {
    const int i = b + lane;
    const int j = i < n0 ? matches0[i] : -1;
    bool pos = false, neg = false;
    if (j >= 0) {
      int x = (int)kpts1[2 * (long)j], y = (int)kpts1[2 * (long)j + 1];
      x = min(max(x, 0), W - 1), y = min(max(y, 0), H - 1);            // keypoints are inside the frame; never read outside
      pos = mk[(long)y * W + x] > 0.5f;
      neg = !pos;
    }
    const unsigned long long bp = __ballot(pos), bn = __ballot(neg), below = (1ull << lane) - 1ull;
    if (pos) {
      const int o = np + __popcll(bp & below);
      if (o < cap) lp[o] = j;
    }
    if (neg) {
      const int o = nn + __popcll(bn & below);
      if (o < cap) ln[o] = j;
    }
    np += __popcll(bp), nn += __popcll(bn);
  }
  if (lane == 0) counts[2 * mi] = np, counts[2 * mi + 1] = nn;
}

int sg_select_lists(const int* matches0, int n0, const float* kpts1, const float* masks, int n_masks, int H, int W, int cap,
                    int* lists, int* counts, hipStream_t s) {
  if (!matches0 || !kpts1 || !masks || !lists || !counts || n0 < 0 || n_masks < 1 || H < 1 || W < 1 || cap < 1 || n0 > cap) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_sg_select_lists, dim3(n_masks), dim3(64), 0, s, matches0, n0, kpts1, masks, H, W, cap, lists, counts);
  SAMPT_CHECK_LAUNCH("k_sg_select_lists");
  return SAMPT_OK;
}

// traj [T][n_masks * P][2], vis [T][n_masks * P], P = n_pos + n_neg.  Frame 0 carries the query points with visibility 0 (the
// reference never sets it); slot p of (frame t >= 1, mask m) takes entry draw[t - 1][m][p] of the mask's positive (p < n_pos) or
// negative list, draw < 0 = padding: (-1, -1), visibility 0 (tracker.py:164-186).
__global__ void k_sg_gather(const float* __restrict__ query_xy, const float* __restrict__ kpts, int kp_cap, const int* __restrict__ lists,
                            int list_cap, const int* __restrict__ counts, const int* __restrict__ draw, int T, int n_masks, int n_pos,
                            int n_neg, float* __restrict__ traj, float* __restrict__ vis) {
  const int P = n_pos + n_neg;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * n_masks * P) return;
  const int p = (int)(i % P), m = (int)((i / P) % n_masks), t = (int)(i / ((long)P * n_masks));
  float x = -1.f, y = -1.f, vv = 0.f;
  if (t == 0) {
    x = query_xy[2 * ((long)m * P + p)], y = query_xy[2 * ((long)m * P + p) + 1];
  } else {
    const int d = draw[((long)(t - 1) * n_masks + m) * P + p], which = p < n_pos ? 0 : 1;
    const long lm = (long)(t - 1) * n_masks + m;
    if (d >= 0 && d < counts[2 * lm + which] && d < list_cap) {
      const int j = lists[(lm * 2 + which) * list_cap + d];
      if (j >= 0 && j < kp_cap) {
        x = kpts[((long)t * kp_cap + j) * 2], y = kpts[((long)t * kp_cap + j) * 2 + 1];
        vv = 1.f;
      }
    }
  }
  traj[2 * i] = x, traj[2 * i + 1] = y, vis[i] = vv;
}

int sg_gather(const float* query_xy, const float* kpts, int kp_cap, const int* lists, int list_cap, const int* counts, const int* draw,
              int T, int n_masks, int n_pos, int n_neg, float* traj, float* vis, hipStream_t s) {
  if (!query_xy || !traj || !vis || T < 1 || n_masks < 1 || n_pos < 0 || n_neg < 0 || n_pos + n_neg < 1) return SAMPT_ERR_ARG;
  if (T > 1 && (!kpts || !lists || !counts || !draw || kp_cap < 1 || list_cap < 1)) return SAMPT_ERR_ARG;
  const long total = (long)T * n_masks * (n_pos + n_neg);
  hipLaunchKernelGGL(k_sg_gather, dim3(cdiv(total, 256)), dim3(256), 0, s, query_xy, kpts, kp_cap, lists, list_cap, counts, draw, T,
                     n_masks, n_pos, n_neg, traj, vis);
  SAMPT_CHECK_LAUNCH("k_sg_gather");
  return SAMPT_OK;
}

// the zero-keypoint branch (superglue.py:233-240): all -1 / 0, two fills and no kernel
int sg_no_match(int n, int* matches0, float* mscores0, hipStream_t s) {
  if (n <= 0) return SAMPT_OK;
  if (!matches0 || !mscores0) return SAMPT_ERR_ARG;
  if (hipMemsetAsync(matches0, 0xff, (size_t)n * 4, s) != hipSuccess || hipMemsetAsync(mscores0, 0, (size_t)n * 4, s) != hipSuccess)
    return SAMPT_ERR_HIP;
  return SAMPT_OK;
}

}  // namespace sampt
