// TinyViT image-encoder kernels (MobileSAM / Light HQ-SAM; ChaoningZhang/MobileSAM tiny_vit_sam.py).  Activations are NHWC f32
// throughout: a token map (B, L = H W, C) and a feature map (B, H, W, C) are the same bytes.
//
//   k_tv_preprocess   Sam.preprocess into the stem's input: uint8 frames (B,3,H,W) or (B,H,W,3) -> (B, img, img, 4) f32 =
//                     (x - mean[c]) / std[c] inside the picture, zeros below / right of it (a zero in normalised space is a zero)
//                     and in the 4th channel (one float4 is one pixel, as rgb_u8chw_to_nhwc4 writes it).
//   k_tv_dwconv3x3    depthwise 3 x 3 convolution, stride 1 or 2, pad 1, + bias (the folded BatchNorm) (+ erf-GELU).  A thread owns
//                     four channels of one output column and DW_ROWS consecutive output rows: it walks the input rows its strip
//                     needs once, three float4 per row, and adds each row into every output row that taps it — an input row is
//                     read (DW_ROWS S + 2) / (DW_ROWS S) times by the strip, its two horizontal neighbours are the adjacent
//                     lanes' own loads (same cache lines).  Weights [3][3][C]: the nine float4 of a thread stay in registers.
//                     Sum order per output: bias, then taps (ky, kx) ascending — the same whatever else shares the launch.
//   k_tv_window_attn  TinyViT's window attention over the UN-padded qkv map (B, H, W, 3C), per-head interleaved (head h = channels
//                     [96 h, 96 h + 96) = q | k | v, head width 32).  One workgroup per (frame, window, head): K and V of the
//                     window's ws^2 positions go to LDS — a position below / right of the map is zero padding AFTER the norm, so
//                     its q / k / v is the packer's pad_qkv row (W_qkv beta + b_qkv) and it takes part in every softmax —, then
//                     one thread per real query runs an online softmax over the keys in window order, four keys per rescale,
//                     every product an f32 FMA.  Bias: table[h][|dy| ws + |dx|].  Padded queries are not computed; nothing padded
//                     is ever written.  H == W == ws is the same kernel with no padding.
//   k_tv_gelu         y = gelu(x): MBConv's activation AFTER the shortcut add (the GEMM epilogue adds the residual after its
//                     activation, so this one runs as its own pass).
#include "ops.h"

namespace sampt {

// ---------------------------------------------------------------------------------------------- preprocess
struct TvNorm {
  float mean[3], stdv[3];
};

__global__ __launch_bounds__(256) void k_tv_preprocess(const uint8_t* __restrict__ src, int chw, int H, int W, int img, long total,
                                                       TvNorm nm, float4* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % img);
  const long r = i / img;
  const int y = (int)(r % img);
  const long b = r / img;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (y < H && x < W) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long at = chw ? ((b * 3 + c) * H + y) * W + x : ((b * H + y) * W + x) * 3 + c;
      v[c] = ((float)src[at] - nm.mean[c]) / nm.stdv[c];
    }
    o = make_float4(v[0], v[1], v[2], 0.f);
  }
  dst[i] = o;
}

int tinyvit_preprocess(const uint8_t* frames, int chw, int B, int H, int W, int img, const float* mean, const float* stdv, float* dst,
                       hipStream_t s) {
  if (!frames || !dst || !mean || !stdv || B < 1 || H < 1 || W < 1 || H > img || W > img) return SAMPT_ERR_ARG;
  const long total = (long)B * img * img;
  if (cdiv(total, 256) > 0x7fffffffL) return SAMPT_ERR_ARG;
  TvNorm nm;
  for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.stdv[c] = stdv[c];
  hipLaunchKernelGGL(k_tv_preprocess, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, frames, chw, H, W, img, total, nm, (float4*)dst);
  SAMPT_CHECK_LAUNCH("tinyvit_preprocess");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- depthwise 3 x 3
constexpr int DW_ROWS = 4;    // output rows per thread

__device__ __forceinline__ void tv_fma4(float4& a, const float4 v, const float4 w) {
  a.x = fmaf(v.x, w.x, a.x), a.y = fmaf(v.y, w.y, a.y), a.z = fmaf(v.z, w.z, a.z), a.w = fmaf(v.w, w.w, a.w);
}

// grid (ceil(OW c4n / 256), ceil(OH / DW_ROWS), n); x, y as float4 arrays of [n][H][W][c4n] / [n][OH][OW][c4n]
template <int S>
__global__ __launch_bounds__(256) void k_tv_dwconv3x3(const float4* __restrict__ x, const float4* __restrict__ w, const float4* __restrict__ bias,
                                                      float4* __restrict__ y, int H, int W, int c4n, int OH, int OW, int gelu) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= OW * c4n) return;
  const int c4 = i % c4n, ox = i / c4n;
  const int oy0 = blockIdx.y * DW_ROWS;
  const long img = blockIdx.z;
  float4 wt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wt[k] = w[k * c4n + c4];
  const float4 bv = bias[c4];
  float4 acc[DW_ROWS];
#pragma unroll
  for (int o = 0; o < DW_ROWS; ++o) acc[o] = bv;
  const float4* xi = x + img * H * W * c4n;
  const int ix0 = ox * S - 1;
  constexpr int IN_ROWS = (DW_ROWS - 1) * S + 3;
#pragma unroll
  for (int r = 0; r < IN_ROWS; ++r) {
    const int iy = oy0 * S - 1 + r;
    if (iy < 0 || iy >= H) continue;             // (uniform over the workgroup)
    float4 v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ix = ix0 + k;
      v[k] = (ix >= 0 && ix < W) ? xi[((long)iy * W + ix) * c4n + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int o = 0; o < DW_ROWS; ++o) {
      const int ky = r - o * S;                  // (compile-time after unrolling)
      if (ky < 0 || ky > 2) continue;
#pragma unroll
      for (int k = 0; k < 3; ++k) tv_fma4(acc[o], v[k], wt[ky * 3 + k]);
    }
  }
  // a strip adds its input rows in ascending order, so every output sums its taps as (ky, kx) ascending
  float4* yo = y + img * OH * OW * c4n;
#pragma unroll
  for (int o = 0; o < DW_ROWS; ++o) {
    const int oy = oy0 + o;
    if (oy >= OH) break;
    float4 a = acc[o];
    if (gelu) a = make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w));
    yo[((long)oy * OW + ox) * c4n + c4] = a;
  }
}

int tinyvit_dwconv3x3(const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int C, int stride, int gelu,
                      hipStream_t s) {
  if (!x || !w || !bias || !y || n < 1 || n > 65535 || H < 1 || W < 1 || C < 32 || (C % 32) || (stride != 1 && stride != 2)) return SAMPT_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15)) return SAMPT_ERR_ARG;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1, c4n = C / 4;
  if ((long)OW * c4n > 0x7fffffffL || cdiv(OH, DW_ROWS) > 65535) return SAMPT_ERR_ARG;
  const dim3 grid((unsigned)cdiv((long)OW * c4n, 256), (unsigned)cdiv(OH, DW_ROWS), (unsigned)n);
  if (stride == 1)
    hipLaunchKernelGGL(k_tv_dwconv3x3<1>, grid, dim3(256), 0, s, (const float4*)x, (const float4*)w, (const float4*)bias, (float4*)y, H, W, c4n, OH,
                       OW, gelu);
  else
    hipLaunchKernelGGL(k_tv_dwconv3x3<2>, grid, dim3(256), 0, s, (const float4*)x, (const float4*)w, (const float4*)bias, (float4*)y, H, W, c4n, OH,
                       OW, gelu);
  SAMPT_CHECK_LAUNCH("tinyvit_dwconv3x3");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- window attention
constexpr int TV_HD = 32;          // head width of every published TinyViT
constexpr int TV_MAX_WS = 14;

// dynamic LDS: K [np][32] | V [np][32] | bias table [ws^2] with np = ws^2 rounded up to a multiple of 4 (tail rows zero)
// grid: frames * nwy * nwx * heads workgroups of NT threads (NT >= ws^2)
template <int NT>
__global__ __launch_bounds__(NT) void k_tv_window_attn(const float* __restrict__ qkv, const float* __restrict__ table, const float* __restrict__ pad_qkv,
                                                       float* __restrict__ out, int H, int W, int C, int heads, int ws, int nwy, int nwx,
                                                       float scale) {
  extern __shared__ float4 tv_smem[];
  const int n = ws * ws, np = (n + 3) & ~3;
  float4* Ks = tv_smem;                       // [np][8]
  float4* Vs = tv_smem + np * 8;              // [np][8]
  float* tab = (float*)(tv_smem + np * 16);   // [n]
  int g = blockIdx.x;
  const int h = g % heads;
  g /= heads;
  const int wx = g % nwx;
  g /= nwx;
  const int wy = g % nwy;
  const long b = g / nwy;
  const int tid = threadIdx.x;
  const long C3 = 3L * C;
  const float* base = qkv + b * H * W * C3 + h * 3 * TV_HD;
  const float* padrow = pad_qkv + h * 3 * TV_HD;
  // ---- stage K | V: 16 float4 per key (the k and v of a head are 64 contiguous floats of a qkv row)
  for (int e = tid; e < np * 16; e += NT) {
    const int j = e >> 4, part = e & 15;                      // part < 8: k, else v
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n) {
      const int y = wy * ws + j / ws, x = wx * ws + j % ws;
      const float* row = (y < H && x < W) ? base + ((long)y * W + x) * C3 : padrow;
      v = *(const float4*)(row + TV_HD + part * 4);
    }
    if (part < 8) Ks[j * 8 + part] = v;
    else Vs[j * 8 + part - 8] = v;
  }
  for (int e = tid; e < n; e += NT) tab[e] = table[(long)h * n + e];
  __syncthreads();
  const int qy = tid / ws, qx = tid % ws;
  const int y = wy * ws + qy, x = wx * ws + qx;
  if (tid >= n || y >= H || x >= W) return;                   // padded queries are not computed (no barrier follows)
  float q[TV_HD];
  {
    const float4* qr = (const float4*)(base + ((long)y * W + x) * C3);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const float4 v = qr[d];
      q[d * 4] = v.x * scale, q[d * 4 + 1] = v.y * scale, q[d * 4 + 2] = v.z * scale, q[d * 4 + 3] = v.w * scale;
    }
  }
  float m = -INFINITY, l = 0.f, acc[TV_HD];
#pragma unroll
  for (int d = 0; d < TV_HD; ++d) acc[d] = 0.f;
  int ky = 0, kx = 0;                                          // window coordinates of key j (uniform)
  for (int j0 = 0; j0 < np; j0 += 4) {
    float sc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const float4 kv = Ks[j * 8 + d];
        s0 = fmaf(q[d * 4], kv.x, s0), s1 = fmaf(q[d * 4 + 1], kv.y, s1);
        s0 = fmaf(q[d * 4 + 2], kv.z, s0), s1 = fmaf(q[d * 4 + 3], kv.w, s1);
      }
      const int dy = qy > ky ? qy - ky : ky - qy, dx = qx > kx ? qx - kx : kx - qx;
      sc[u] = j < n ? (s0 + s1) + tab[min(dy * ws + dx, n - 1)] : -INFINITY;      // (the clamp only acts on the tail keys)
      if (++kx == ws) kx = 0, ++ky;
    }
    const float mn = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), m);   // finite: key j0 < n always is
    const float alpha = expf(m - mn);                       // first group: exp(-inf) = 0
    m = mn;
    l *= alpha;
#pragma unroll
    for (int d = 0; d < TV_HD; ++d) acc[d] *= alpha;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float p = expf(sc[u] - mn);                     // tail keys: exp(-inf) = 0 against zero V rows
      l += p;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const float4 vv = Vs[(j0 + u) * 8 + d];
        acc[d * 4] = fmaf(p, vv.x, acc[d * 4]), acc[d * 4 + 1] = fmaf(p, vv.y, acc[d * 4 + 1]);
        acc[d * 4 + 2] = fmaf(p, vv.z, acc[d * 4 + 2]), acc[d * 4 + 3] = fmaf(p, vv.w, acc[d * 4 + 3]);
      }
    }
  }
  const float inv = 1.0f / l;
  float4* o = (float4*)(out + (b * H * W + (long)y * W + x) * C + h * TV_HD);
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] = make_float4(acc[d * 4] * inv, acc[d * 4 + 1] * inv, acc[d * 4 + 2] * inv, acc[d * 4 + 3] * inv);
}

int tinyvit_window_attention(const float* qkv, const float* table, const float* pad_qkv, float* out, int B, int H, int W, int heads, int ws,
                             hipStream_t s) {
  if (!qkv || !table || !pad_qkv || !out || B < 1 || H < 1 || W < 1 || heads < 1 || ws < 1 || ws > TV_MAX_WS) return SAMPT_ERR_ARG;
  if ((((uintptr_t)qkv | (uintptr_t)pad_qkv | (uintptr_t)out) & 15)) return SAMPT_ERR_ARG;
  const int C = heads * TV_HD, nwy = cdiv(H, ws), nwx = cdiv(W, ws), n = ws * ws, np = (n + 3) & ~3;
  const long wgs = (long)B * nwy * nwx * heads;
  if (wgs > 0x7fffffffL || (long)B * H * W * 3 * C > 0x7fffffffffL) return SAMPT_ERR_ARG;
  const size_t lds = (size_t)np * 2 * TV_HD * sizeof(float) + (size_t)n * sizeof(float);     // <= 50960 bytes at ws = 14
  const float scale = 0.17677669529663687f;                   // 32^-0.5
  if (n <= 64)
    hipLaunchKernelGGL(k_tv_window_attn<64>, dim3((unsigned)wgs), dim3(64), lds, s, qkv, table, pad_qkv, out, H, W, C, heads, ws, nwy, nwx, scale);
  else
    hipLaunchKernelGGL(k_tv_window_attn<256>, dim3((unsigned)wgs), dim3(256), lds, s, qkv, table, pad_qkv, out, H, W, C, heads, ws, nwy, nwx, scale);
  SAMPT_CHECK_LAUNCH("tinyvit_window_attention");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------- GELU
__global__ __launch_bounds__(256) void k_tv_gelu(const float4* __restrict__ x, float4* __restrict__ y, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 v = x[i];
  y[i] = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
}

int tinyvit_gelu(const float* x, float* y, long n, hipStream_t s) {
  if (!x || !y || n < 4 || (n % 4) || cdiv(n / 4, 256) > 0x7fffffffL || (((uintptr_t)x | (uintptr_t)y) & 15)) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_tv_gelu, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, s, (const float4*)x, (float4*)y, n / 4);
  SAMPT_CHECK_LAUNCH("tinyvit_gelu");
  return SAMPT_OK;
}

}  // namespace sampt
