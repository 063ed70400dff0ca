// RAFT point tracker (sam_pt/point_tracker/raft/): the kernels around the convolutions — frame preparation, the 4-level
// correlation lookup, the motion encoder's 7 x 7 flow convolution, the GRU's elementwise halves, the convex upsampling
// and the flow chaining of tracker.py:46-88.  All f32.  This file is compiled without fp contraction (Makefile) so that
// the chain's bilinear_sample2d rounds every operation separately, as the host arithmetic does; kernels that want a
// fused multiply-add ask for it with fmaf.
//
// Layouts: activations are NHWC over the coarse grid, one "image" per pair-direction: row m = pd * h8 * w8 + y * w8 + x.
// Correlation level l: [pair-directions][h8 * w8][h_l * w_l] — a pixel's plane is contiguous.
#include "ops.h"

namespace sampt {

// ---------------------------------------------------------------------------------------------
// uint8 (T,3,H,W) -> f32 NHWC4 (T,Hp,Wp,4) = 2 * (x / 255) - 1 of the replicate-padded frame (InputPadder "sintel":
// pad // 2 before, the rest after), 4th channel 0
// ---------------------------------------------------------------------------------------------
__global__ void k_raft_prep(const uint8_t* __restrict__ src, float4* __restrict__ dst, int H, int W, int Hp, int Wp, int pt,
                            int pl, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int x = (int)(i % Wp);
  long r = i / Wp;
  int y = (int)(r % Hp);
  long t = r / Hp;
  int sy = min(max(y - pt, 0), H - 1), sx = min(max(x - pl, 0), W - 1);
  const uint8_t* p = src + (t * 3 * H + sy) * (long)W + sx;
  const long plane = (long)H * W;
  float4 o;
  o.x = 2.0f * ((float)p[0] / 255.0f) - 1.0f;
  o.y = 2.0f * ((float)p[plane] / 255.0f) - 1.0f;
  o.z = 2.0f * ((float)p[2 * plane] / 255.0f) - 1.0f;
  o.w = 0.f;
  dst[i] = o;
}

int raft_prep_frames(const uint8_t* frames, int T, int H, int W, int Hp, int Wp, float* dst, hipStream_t s) {
  if (!frames || !dst || T <= 0 || Hp < H || Wp < W || Hp - H >= 8 || Wp - W >= 8) return SAMPT_ERR_ARG;
  long total = (long)T * Hp * Wp;
  hipLaunchKernelGGL(k_raft_prep, dim3(cdiv(total, 256)), dim3(256), 0, s, frames, (float4*)dst, H, W, Hp, Wp, (Hp - H) / 2,
                     (Wp - W) / 2, total);
  SAMPT_CHECK_LAUNCH("raft_prep");
  return SAMPT_OK;
}

// out = max(a + b, 0)   (residual blocks of the context encoder, whose folded BatchNorm leaves no norm kernel to carry it)
__global__ void k_raft_add_relu(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ out, long n4) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 u = a[i], v = b[i], o;
  o.x = fmaxf(u.x + v.x, 0.f), o.y = fmaxf(u.y + v.y, 0.f), o.z = fmaxf(u.z + v.z, 0.f), o.w = fmaxf(u.w + v.w, 0.f);
  out[i] = o;
}

int raft_add_relu(const float* a, const float* b, float* out, long n, hipStream_t s) {
  if (n % 4) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_raft_add_relu, dim3(cdiv(n / 4, 256)), dim3(256), 0, s, (const float4*)a, (const float4*)b, (float4*)out,
                     n / 4);
  SAMPT_CHECK_LAUNCH("raft_add_relu");
  return SAMPT_OK;
}

// context encoder output [rows][256] -> net = tanh(first 128), inp = relu(last 128)   (raft.py:113-116)
__global__ void k_raft_split_ctx(const float* __restrict__ c, float* __restrict__ net, float* __restrict__ inp, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  long row = i >> 8;
  int ch = (int)(i & 255);
  float v = c[i];
  if (ch < 128) net[row * 128 + ch] = tanhf(v);
  else inp[row * 128 + ch - 128] = fmaxf(v, 0.f);
}

int raft_split_ctx(const float* c, long rows, float* net, float* inp, hipStream_t s) {
  long total = rows * 256;
  hipLaunchKernelGGL(k_raft_split_ctx, dim3(cdiv(total, 256)), dim3(256), 0, s, c, net, inp, total);
  SAMPT_CHECK_LAUNCH("raft_split_ctx");
  return SAMPT_OK;
}

// state of a chunk of np pairs starting at pair p0: pair-direction j < np is (p0 + j -> p0 + j + 1), j >= np the reverse.
// hx [M][384] = [net(frame1) | inp(frame1) | 0], coords1 = the pixel grid
__global__ void k_raft_init_state(const float* __restrict__ net, const float* __restrict__ inp, int p0, int np, int hw, int w8,
                                  float* __restrict__ hx, float* __restrict__ coords1, float* __restrict__ flow, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  long m = i / 384;
  int ch = (int)(i - m * 384);
  int pd = (int)(m / hw), pix = (int)(m - (long)pd * hw);
  int f1 = pd < np ? p0 + pd : p0 + (pd - np) + 1;
  long srow = (long)f1 * hw + pix;
  float v = 0.f;
  if (ch < 128) v = net[srow * 128 + ch];
  else if (ch < 256) v = inp[srow * 128 + ch - 128];
  hx[i] = v;
  if (ch < 2) {
    coords1[m * 2 + ch] = ch == 0 ? (float)(pix % w8) : (float)(pix / w8);
    flow[m * 2 + ch] = 0.f;
  }
}

int raft_init_state(const float* net, const float* inp, int p0, int np, int h8, int w8, float* hx, float* coords1, float* flow,
                    hipStream_t s) {
  long total = (long)2 * np * h8 * w8 * 384;
  hipLaunchKernelGGL(k_raft_init_state, dim3(cdiv(total, 256)), dim3(256), 0, s, net, inp, p0, np, h8 * w8, w8, hx, coords1, flow,
                     total);
  SAMPT_CHECK_LAUNCH("raft_init_state");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------
// Correlation lookup (corr.py:32-53): one workgroup per pixel, one wave per level.  The 81 taps of a level sit at integer
// offsets from one point, so they share their four corners' 10 x 10 patch of the pixel's plane: the wave reads it once
// (rows of 10 consecutive floats) into LDS and forms the taps from there.  grid_sample(align_corners=True, zeros): a corner
// outside the level adds nothing.  Channel l * 81 + i * 9 + j samples at (x + i - 4, y + j - 4) — the reference adds
// meshgrid(dy, dx) to (x, y).  Rows of 352 floats, [324, 352) zero.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_raft_lookup(RaftLevels lv, const float* __restrict__ coords, float* __restrict__ out) {
  __shared__ float patch[4][10][11];
  const long m = blockIdx.x;
  const int l = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int H = lv.h[l], W = lv.w[l];
  const float* __restrict__ plane = lv.base[l] + m * (long)(H * W);
  const float sc = 1.0f / (float)(1 << l);
  // far-away or non-finite coordinates sample nothing; the clamp keeps the int conversion defined
  const float cx = fminf(fmaxf(coords[m * 2] * sc, -1.0e6f), 1.0e6f);
  const float cy = fminf(fmaxf(coords[m * 2 + 1] * sc, -1.0e6f), 1.0e6f);
  const int bx = (int)floorf(cx) - 4, by = (int)floorf(cy) - 4;
  for (int e = lane; e < 100; e += 64) {
    int py = e / 10, px = e - py * 10;
    int gy = by + py, gx = bx + px;
    patch[l][py][px] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? plane[(long)gy * W + gx] : 0.f;
  }
  __syncthreads();
  auto fetch = [&](int yy, int xx) -> float {
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) return 0.f;
    int py = yy - by, px = xx - bx;
    if (py >= 0 && py < 10 && px >= 0 && px < 10) return patch[l][py][px];
    return plane[(long)yy * W + xx];    // only when the f32 sum x + (i - 4) rounds across an integer
  };
  float* __restrict__ orow = out + m * 352 + l * 81;
  for (int e = lane; e < 81; e += 64) {
    int i = e / 9, j = e - i * 9;
    float x = cx + (float)(i - 4), y = cy + (float)(j - 4);
    float x0 = floorf(x), y0 = floorf(y);
    int ix = (int)x0, iy = (int)y0;
    float wx1 = x - x0, wx0 = (x0 + 1.0f) - x, wy1 = y - y0, wy0 = (y0 + 1.0f) - y;
    float v = fetch(iy, ix) * (wx0 * wy0);
    v += fetch(iy, ix + 1) * (wx1 * wy0);
    v += fetch(iy + 1, ix) * (wx0 * wy1);
    v += fetch(iy + 1, ix + 1) * (wx1 * wy1);
    orow[e] = v;
  }
  if (threadIdx.x < 28) out[m * 352 + 324 + threadIdx.x] = 0.f;
}

int raft_lookup(const RaftLevels& lv, const float* coords, long M, float* out, hipStream_t s) {
  if (!coords || !out || M <= 0 || M > 0x7fffffffL) return SAMPT_ERR_ARG;
  for (int l = 0; l < 4; ++l)
    if (!lv.base[l] || lv.h[l] < 1 || lv.w[l] < 1) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_raft_lookup, dim3((unsigned)M), dim3(256), 0, s, lv, coords, out);
  SAMPT_CHECK_LAUNCH("raft_lookup");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------
// convf1: Conv2d(2, 128, 7, padding=3) + ReLU over the flow [img][h][w][2].  K is 98: a direct kernel, a workgroup per 8
// pixels of a row, a thread per output channel; weights [98][128] (k = (ky * 7 + kx) * 2 + ci) are read coalesced.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_raft_convf1(const float* __restrict__ flow, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ out, int h, int wd) {
  __shared__ float tile[7][14][2];
  const int xt = blockIdx.x * 8, y = blockIdx.y, img = blockIdx.z;
  const float* __restrict__ f = flow + (long)img * h * wd * 2;
  for (int e = threadIdx.x; e < 7 * 14 * 2; e += 128) {
    int c = e & 1, px = (e >> 1) % 14, py = (e >> 1) / 14;
    int gy = y + py - 3, gx = xt + px - 3;
    tile[py][px][c] = (gy >= 0 && gy < h && gx >= 0 && gx < wd) ? f[((long)gy * wd + gx) * 2 + c] : 0.f;
  }
  __syncthreads();
  const int co = threadIdx.x;
  float acc[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) acc[p] = 0.f;
  for (int ky = 0; ky < 7; ++ky)
    for (int kx = 0; kx < 7; ++kx)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float wv = w[((ky * 7 + kx) * 2 + c) * 128 + co];
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[p] = fmaf(tile[ky][p + kx][c], wv, acc[p]);
      }
  const float b = bias[co];
#pragma unroll
  for (int p = 0; p < 8; ++p)
    if (xt + p < wd) out[(((long)img * h + y) * wd + xt + p) * 128 + co] = fmaxf(acc[p] + b, 0.f);
}

int raft_convf1(const float* flow, const float* w, const float* bias, float* out, int nimg, int h, int wd, hipStream_t s) {
  if (!flow || !w || !bias || !out || nimg <= 0 || nimg > 65535 || h <= 0 || h > 65535 || wd <= 0) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_raft_convf1, dim3(cdiv(wd, 8), h, nimg), dim3(128), 0, s, flow, w, bias, out, h, wd);
  SAMPT_CHECK_LAUNCH("raft_convf1");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------
// SepConvGRU halves (update.py:48-63).  zr [M][256] = the fused z | r convolution before its sigmoid; hx [M][384] = [h | x].
//   a: z = sigmoid(zr[:128]) ; rhx = [sigmoid(zr[128:]) * h | x]         (input of the q convolution)
//   b: h = (1 - z) * h + z * tanh(q), written to hx[:128] and to the dense hnet [M][128] (input of the heads)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void k_raft_gru_a(const float* __restrict__ zr, const float* __restrict__ hx, float* __restrict__ z,
                             float* __restrict__ rhx, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  long m = i / 384;
  int ch = (int)(i - m * 384);
  float v = hx[i];
  if (ch < 128) {
    z[m * 128 + ch] = sigmoidf_(zr[m * 256 + ch]);
    v = sigmoidf_(zr[m * 256 + 128 + ch]) * v;
  }
  rhx[i] = v;
}

__global__ void k_raft_gru_b(const float* __restrict__ q, const float* __restrict__ z, float* __restrict__ hx,
                             float* __restrict__ hnet, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  long m = i >> 7;
  int ch = (int)(i & 127);
  float zz = z[i], h = hx[m * 384 + ch];
  float hn = (1.0f - zz) * h + zz * tanhf(q[i]);
  hx[m * 384 + ch] = hn;
  hnet[i] = hn;
}

int raft_gru_a(const float* zr, const float* hx, float* z, float* rhx, long M, hipStream_t s) {
  long total = M * 384;
  hipLaunchKernelGGL(k_raft_gru_a, dim3(cdiv(total, 256)), dim3(256), 0, s, zr, hx, z, rhx, total);
  SAMPT_CHECK_LAUNCH("raft_gru_a");
  return SAMPT_OK;
}

int raft_gru_b(const float* q, const float* z, float* hx, float* hnet, long M, hipStream_t s) {
  long total = M * 128;
  hipLaunchKernelGGL(k_raft_gru_b, dim3(cdiv(total, 256)), dim3(256), 0, s, q, z, hx, hnet, total);
  SAMPT_CHECK_LAUNCH("raft_gru_b");
  return SAMPT_OK;
}

// coords1 += delta ; flow = coords1 - coords0 (raft.py:128-133), written to the dense flow [M][2] and to channels 382, 383
// of hx (the motion features end in the flow).  delta rows have 4 floats (the N = 2 convolution padded to 4).
__global__ void k_raft_flow_update(const float* __restrict__ delta, float* __restrict__ coords1, float* __restrict__ flow,
                                   float* __restrict__ hx, int hw, int w8, long M) {
  long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int pix = (int)(m % hw);
  float x0 = (float)(pix % w8), y0 = (float)(pix / w8);
  float cx = coords1[m * 2] + delta[m * 4], cy = coords1[m * 2 + 1] + delta[m * 4 + 1];
  coords1[m * 2] = cx, coords1[m * 2 + 1] = cy;
  float fx = cx - x0, fy = cy - y0;
  flow[m * 2] = fx, flow[m * 2 + 1] = fy;
  hx[m * 384 + 382] = fx, hx[m * 384 + 383] = fy;
}

int raft_flow_update(const float* delta, float* coords1, float* flow, float* hx, int h8, int w8, long M, hipStream_t s) {
  hipLaunchKernelGGL(k_raft_flow_update, dim3(cdiv(M, 256)), dim3(256), 0, s, delta, coords1, flow, hx, h8 * w8, w8, M);
  SAMPT_CHECK_LAUNCH("raft_flow_update");
  return SAMPT_OK;
}

// flow [M][2] (NHWC) -> flow_low [dir][pair][2][h8][w8] (NCHW, what the reference returns as coords1 - coords0)
__global__ void k_raft_flow_low(const float* __restrict__ flow, float* __restrict__ out, int p0, int np, int npairs, int hw,
                                long M) {
  long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int pd = (int)(m / hw), pix = (int)(m - (long)pd * hw);
  int dir = pd >= np, pair = p0 + (dir ? pd - np : pd);
  float* o = out + ((long)dir * npairs + pair) * 2 * hw;
  o[pix] = flow[m * 2], o[hw + pix] = flow[m * 2 + 1];
}

int raft_flow_low(const float* flow, float* out, int p0, int np, int npairs, int h8, int w8, hipStream_t s) {
  long M = (long)2 * np * h8 * w8;
  hipLaunchKernelGGL(k_raft_flow_low, dim3(cdiv(M, 256)), dim3(256), 0, s, flow, out, p0, np, npairs, h8 * w8, M);
  SAMPT_CHECK_LAUNCH("raft_flow_low");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------
// Convex upsampling + un-padding (raft.py:75-86, util.py:24-27): a thread per full-resolution pixel of the un-padded frame.
// mask [M][576] with channel k * 64 + i * 8 + j (k = the 3 x 3 tap, (i, j) = the sub-pixel), scaled by mask_scale before the
// softmax over k; the taps are the zero-padded 3 x 3 neighbourhood of 8 * flow.  Pair-direction j of the chunk goes to
// fwd[p0 + j] (j < np) or bwd[p0 + j - np], each (2, H, W).
// ---------------------------------------------------------------------------------------------
__global__ void k_raft_upsample(const float* __restrict__ flow, const float* __restrict__ mask, float mask_scale, int h8, int w8,
                                int H, int W, int pt, int pl, int p0, int np, float* __restrict__ fwd, float* __restrict__ bwd,
                                long total) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int x = (int)(idx % W);
  long r = idx / W;
  int y = (int)(r % H);
  int pd = (int)(r / H);
  int yp = y + pt, xp = x + pl;
  int hh = yp >> 3, i = yp & 7, ww = xp >> 3, j = xp & 7;
  const float* __restrict__ mrow = mask + (((long)pd * h8 + hh) * w8 + ww) * 576 + i * 8 + j;
  float lg[9], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    lg[k] = mask_scale * mrow[k * 64];
    mx = fmaxf(mx, lg[k]);
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    lg[k] = expf(lg[k] - mx);
    sum += lg[k];
  }
  float ox = 0.f, oy = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    int ny = hh + k / 3 - 1, nx = ww + k % 3 - 1;
    float fx = 0.f, fy = 0.f;
    if (ny >= 0 && ny < h8 && nx >= 0 && nx < w8) {
      const float* fp = flow + (((long)pd * h8 + ny) * w8 + nx) * 2;
      fx = 8.0f * fp[0], fy = 8.0f * fp[1];
    }
    float pk = lg[k] / sum;
    ox += pk * fx, oy += pk * fy;
  }
  float* dst = (pd < np ? fwd + (long)(p0 + pd) * 2 * H * W : bwd + (long)(p0 + pd - np) * 2 * H * W);
  dst[(long)y * W + x] = ox;
  dst[(long)H * W + (long)y * W + x] = oy;
}

int raft_upsample(const float* flow, const float* mask, float mask_scale, int h8, int w8, int H, int W, int p0, int np, float* fwd,
                  float* bwd, hipStream_t s) {
  const int Hp = h8 * 8, Wp = w8 * 8;
  if (!flow || !mask || !fwd || np <= 0 || H > Hp || W > Wp || Hp - H >= 8 || Wp - W >= 8 || H <= 0 || W <= 0)
    return SAMPT_ERR_ARG;
  const int npd = bwd ? 2 * np : np;       // bwd == nullptr: np forward planes only (the test entry point)
  long total = (long)npd * H * W;
  hipLaunchKernelGGL(k_raft_upsample, dim3(cdiv(total, 256)), dim3(256), 0, s, flow, mask, mask_scale, h8, w8, H, W, (Hp - H) / 2,
                     (Wp - W) / 2, p0, bwd ? np : npd, fwd, bwd, total);
  SAMPT_CHECK_LAUNCH("raft_upsample");
  return SAMPT_OK;
}

// ---------------------------------------------------------------------------------------------
// Flow chaining (tracker.py:46-88): a thread per point, sequential over the frames.  bilinear_sample2d (samp.py:6-80):
// indices clamped to the frame, weights from the un-clamped floor, every operation rounded separately.
// flows [T-1][2][H][W]; q [n][3] = (t, x, y); traj [T][n][2]; vis [T][n] bytes.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void chain_sample(const float* __restrict__ fl, int H, int W, float x, float y, float& dx, float& dy) {
  // (coordinates beyond +-2^30 px would overflow the reference's int conversion; they are clamped for the index only)
  float x0f = floorf(fminf(fmaxf(x, -1.0e9f), 1.0e9f)), y0f = floorf(fminf(fmaxf(y, -1.0e9f), 1.0e9f));
  int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  float x1f = (float)x1, y1f = (float)y1;
  x0f = (float)x0, y0f = (float)y0;
  int x0c = min(max(x0, 0), W - 1), x1c = min(max(x1, 0), W - 1), y0c = min(max(y0, 0), H - 1), y1c = min(max(y1, 0), H - 1);
  float w00 = (x1f - x) * (y1f - y), w01 = (x - x0f) * (y1f - y), w10 = (x1f - x) * (y - y0f), w11 = (x - x0f) * (y - y0f);
  const long plane = (long)H * W;
  const long i00 = (long)y0c * W + x0c, i01 = (long)y0c * W + x1c, i10 = (long)y1c * W + x0c, i11 = (long)y1c * W + x1c;
  dx = ((w00 * fl[i00] + w01 * fl[i01]) + w10 * fl[i10]) + w11 * fl[i11];
  dy = ((w00 * fl[plane + i00] + w01 * fl[plane + i01]) + w10 * fl[plane + i10]) + w11 * fl[plane + i11];
}

__global__ void k_raft_chain(const float* __restrict__ fwd, const float* __restrict__ bwd, int T, int H, int W,
                             const float* __restrict__ q, int n, float* __restrict__ traj, unsigned char* __restrict__ vis) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float qt = q[p * 3], qx = q[p * 3 + 1], qy = q[p * 3 + 2];
  const long fsz = (long)2 * H * W;
  float cx = 0.f, cy = 0.f;
  for (int t = 0; t < T; ++t) {
    if (t > 0) {
      float dx, dy;
      chain_sample(fwd + (t - 1) * fsz, H, W, cx, cy, dx, dy);
      cx = cx + dx, cy = cy + dy;
    }
    if (qt == (float)t) cx = qx, cy = qy;
    traj[((long)t * n + p) * 2] = cx, traj[((long)t * n + p) * 2 + 1] = cy;
  }
  for (int t = T - 2; t >= 0; --t) {
    if (!((float)t < qt)) continue;
    float sx = traj[((long)(t + 1) * n + p) * 2], sy = traj[((long)(t + 1) * n + p) * 2 + 1];
    float dx, dy;
    chain_sample(bwd + t * fsz, H, W, sx, sy, dx, dy);
    traj[((long)t * n + p) * 2] = sx + dx, traj[((long)t * n + p) * 2 + 1] = sy + dy;
  }
  for (int t = 0; t < T; ++t) {
    float x = traj[((long)t * n + p) * 2], y = traj[((long)t * n + p) * 2 + 1];
    vis[(long)t * n + p] = (x >= 0.f && y >= 0.f && x < (float)W && y < (float)H) ? 1 : 0;
  }
}

int raft_chain(const float* fwd, const float* bwd, int T, int H, int W, const float* q, int n, float* traj, unsigned char* vis,
               hipStream_t s) {
  if (!q || !traj || !vis || T < 1 || n <= 0 || H <= 0 || W <= 0 || (T > 1 && (!fwd || !bwd))) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_raft_chain, dim3(cdiv(n, 64)), dim3(64), 0, s, fwd, bwd, T, H, W, q, n, traj, vis);
  SAMPT_CHECK_LAUNCH("raft_chain");
  return SAMPT_OK;
}

}  // namespace sampt
