// YouTube-VIS AP / AR on the device: bit-planes of mask stacks, the spatio-temporal intersection / union of every (detection, ground
// truth) pair of a video, and the greedy matching of the reference's evaluateVid.  Integer work throughout, and one IEEE float64
// division per IoU (this file is built without fp contraction, see the Makefile): every result is bitwise repeatable and equals the
// host restatement of sam_pt_amd/vis_metrics.py exactly.
//
// Bit-plane format (public, include/sampt_hip.h; the column words of csrc/bitplane.h, stored): a stack
// [n][h][w] becomes uint64 [n][ceil(h / 64)][w]; bit j of word (band b, column x) is pixel (64 b + j, x); bits of rows >= h are 0.
//
//   k_bits_pack     one wave per tile of 64 rows x 256 columns: the tile reader of csrc/bitplane.h (4 pixels per load from any pixel
//                   address; images narrower than 4 take the element-load form), its words stored as they are.  Every pixel is read
//                   once; the area is an integer atomic.
//   k_rle_scan      one workgroup per mask: inclusive prefix sums (uint64) of the mask's runs into the workspace, the sum of the odd
//                   runs (the area) and the status (the runs must sum to h * w).
//   k_rle_bits      one thread per output word: a binary search for the run that holds position x * h + 64 b, then a walk over the
//                   runs up to the end of the word (the column's end for the last band).  A mask with a non-zero status is written
//                   as zeros and none of its runs is read.
//   k_bits_unpack   bit-planes -> bytes [n][h][w] (0 / 1), one thread per pixel.
//   k_seq_iou       a small GEMM over bit words: a workgroup holds the words of 32 detections and of 32 ground truths for 64 word
//                   positions of one frame in LDS ([word][item], padded by one item) and every thread adds popc(d & g) of a 2 x 2
//                   block of pairs, so a word is fetched once per tile and never once per pair.  The word positions of all frames
//                   are dealt round-robin to the workgroups of a tile; each writes its partial sums (uint64) to the workspace.
//   k_seq_iou_sum   one thread per pair: adds the partials in a fixed order, union = sum of the present frames' areas - inter.
//   k_vis_match     one wave per area range, one lane per IoU threshold; the per-threshold "matched" flags live in LDS.
#include "ops.h"
#include "bitplane.h"

namespace sampt {

namespace {
constexpr int SI_B = 32;                     // detections / ground truths per tile
constexpr int SI_KW = 64;                    // word positions per step
constexpr int SI_TARGET_BLOCKS = 1024;       // workgroups of one call (about 4 per CU)
constexpr int VM_MAX_G = 960;                // 66 bytes of LDS per ground truth
constexpr int VM_MAX_THR = 64;
}  // namespace

// tiles = n * nb * ncb in (item, band, column block) order; out: words [n][nb][w]; area int32 [n] (zeroed)
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void k_bits_pack(BpSrc src, int h, int w, int nb, int ncb, long tiles, int wvec, u64* __restrict__ out,
                                                   int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const BpTile k = bp_tile(t, nb, ncb, lane);
    int val;
    const void* p = bp_plane<KIND>(src, k.item, npix, val);
    u64 word[4];
    bp_words<KIND, VEC>(p, src.thr, val, k.y0, k.x0, h, w, word);
    bp_store4(out + (k.item * nb + k.rb) * (long)w + k.x0, word, k.x0, w, wvec);
    int a = __popcll(word[0]) + __popcll(word[1]) + __popcll(word[2]) + __popcll(word[3]);
    a = bp_wave_sum(a);
    if (lane == 0 && a) atomicAdd(area + k.item, a);
  }
}

// cum[offsets[m] + i] = counts[offsets[m]] + .. + counts[offsets[m] + i]; status 0: the runs sum to hw; 1: they do not; 2: the
// mask's offsets are not inside [0, total] in order (nothing of it is read)
__global__ __launch_bounds__(256) void k_rle_scan(const u32* __restrict__ counts, const long long* __restrict__ offsets, int n, long total,
                                                  u64 hw, u64* __restrict__ cum, int* __restrict__ area, int* __restrict__ status) {
  __shared__ u64 wsum[4], wodd[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int m = blockIdx.x; m < n; m += gridDim.x) {            // block-uniform
    const long o0 = offsets[m], o1 = offsets[m + 1];
    if (o0 < 0 || o1 < o0 || o1 > total) {
      if (tid == 0) status[m] = 2, area[m] = 0;
      continue;
    }
    const long nr = o1 - o0;
    u64 carry = 0, odd = 0;
    for (long b = 0; b < nr; b += 256) {
      const long i = b + tid;
      const u64 c = i < nr ? (u64)counts[o0 + i] : 0ull;
      if (i & 1) odd += c;
      u64 v = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
      }
      if (lane == 63) wsum[wv] = v;
      __syncthreads();
      u64 pre = carry;
      for (int k = 0; k < wv; ++k) pre += wsum[k];
      carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
      if (i < nr) cum[o0 + i] = pre + v;
      __syncthreads();                                         // (wsum is rewritten by the next round)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) odd += __shfl_down(odd, o, 64);
    if (lane == 0) wodd[wv] = odd;
    __syncthreads();
    if (tid == 0) {
      const bool ok = carry == hw;
      status[m] = ok ? 0 : 1;
      area[m] = ok ? (int)(wodd[0] + wodd[1] + wodd[2] + wodd[3]) : 0;
    }
    __syncthreads();
  }
}

// nwords = n * nb * w in (mask, band, column) order
__global__ __launch_bounds__(256) void k_rle_bits(const u64* __restrict__ cum, const long long* __restrict__ offsets,
                                                  const int* __restrict__ status, int h, int w, int nb, long nwords, u64* __restrict__ out) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < nwords; idx += (long)gridDim.x * 256) {
    const int x = (int)(idx % w);
    const long q = idx / w;
    const int b = (int)(q % nb);
    const long m = q / nb;
    u64 word = 0;
    if (status[m] == 0) {                                      // the runs are inside the array and sum to h * w: end <= cum[nr - 1]
      const long o0 = offsets[m], nr = offsets[m + 1] - o0;
      const u64* c = cum + o0;
      const u64 p0 = (u64)x * h + 64ull * b;
      const int len = h - 64 * b < 64 ? h - 64 * b : 64;       // the word of a column's last band ends at the column's end
      const u64 end = p0 + len;
      long lo = 0, hi = nr - 1;                                // the first run that ends beyond p0 (zero-length runs never do)
      while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (c[mid] > p0) hi = mid; else lo = mid + 1;
      }
      u64 pos = p0;
      for (long i = lo; pos < end && i < nr; ++i) {
        const u64 ce = c[i], re = ce < end ? ce : end;
        if ((i & 1) && re > pos) {
          const int a = (int)(pos - p0), e = (int)(re - p0);   // bits a .. e - 1, 0 <= a < e <= 64
          word |= (e == 64 ? ~0ull : (1ull << e) - 1ull) & ~((1ull << a) - 1ull);
        }
        pos = re > pos ? re : pos;
      }
    }
    out[idx] = word;
  }
}

__global__ __launch_bounds__(256) void k_bits_unpack(const u64* __restrict__ bits, int h, int w, int nb, long npix_all,
                                                     unsigned char* __restrict__ out) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < npix_all; idx += (long)gridDim.x * 256) {
    const int x = (int)(idx % w);
    const long q = idx / w;
    const int y = (int)(q % h);
    const long m = q / h;
    out[idx] = (unsigned char)((bits[(m * nb + (y >> 6)) * (long)w + x] >> (y & 63)) & 1ull);
  }
}

// grid (kb, G tiles, D tiles); chunk c of nchunks = T * cpp is frame c / cpp, word positions (c % cpp) * 64 .. + 63 of wp per plane
__global__ __launch_bounds__(256) void k_seq_iou(const u64* __restrict__ dbits, const int* __restrict__ dplanes, int D, int dnp,
                                                 const u64* __restrict__ gbits, const int* __restrict__ gplanes, int G, int gnp, int T,
                                                 long wp, int cpp, long nchunks, int Dp, int Gp, u64* __restrict__ partial) {
  __shared__ u64 sd[SI_KW][SI_B + 1], sg[SI_KW][SI_B + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int d0 = blockIdx.z * SI_B, g0 = blockIdx.y * SI_B;
  const int k = tid & 63, r4 = tid >> 6;
  u64 acc[2][2] = {{0, 0}, {0, 0}};
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {     // block-uniform
    const int t = (int)(c / cpp);
    const long kk = (long)(c % cpp) * SI_KW + k;
#pragma unroll
    for (int i = 0; i < SI_B / 4; ++i) {
      const int r = r4 + 4 * i;
      const int dp = d0 + r < D ? dplanes[(long)(d0 + r) * T + t] : -1;
      const int gp = g0 + r < G ? gplanes[(long)(g0 + r) * T + t] : -1;
      sd[k][r] = (dp >= 0 && dp < dnp && kk < wp) ? dbits[(long)dp * wp + kk] : 0ull;
      sg[k][r] = (gp >= 0 && gp < gnp && kk < wp) ? gbits[(long)gp * wp + kk] : 0ull;
    }
    __syncthreads();
    u32 a00 = 0, a01 = 0, a10 = 0, a11 = 0;                    // at most 64 * 64 per step
#pragma unroll 8
    for (int q = 0; q < SI_KW; ++q) {
      const u64 da = sd[q][ty], db = sd[q][ty + 16], ga = sg[q][tx], gb = sg[q][tx + 16];
      a00 += __popcll(da & ga), a01 += __popcll(da & gb), a10 += __popcll(db & ga), a11 += __popcll(db & gb);
    }
    acc[0][0] += a00, acc[0][1] += a01, acc[1][0] += a10, acc[1][1] += a11;
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      partial[((long)blockIdx.x * Dp + d0 + ty + 16 * i) * Gp + g0 + tx + 16 * j] = acc[i][j];
}

__global__ __launch_bounds__(256) void k_seq_iou_sum(const u64* __restrict__ partial, int kb, int Dp, int Gp, const int* __restrict__ dplanes,
                                                     const int* __restrict__ darea, int D, int dnp, const int* __restrict__ gplanes,
                                                     const int* __restrict__ garea, int G, int gnp, int T, long long* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)D * G) return;
  const int d = (int)(idx / G), g = (int)(idx % G);
  u64 inter = 0;
  for (int b = 0; b < kb; ++b) inter += partial[((long)b * Dp + d) * Gp + g];
  long long areas = 0;                                         // an absent frame contributes nothing of its own
  for (int t = 0; t < T; ++t) {
    const int dp = dplanes[(long)d * T + t], gp = gplanes[(long)g * T + t];
    if (dp >= 0 && dp < dnp) areas += darea[dp];
    if (gp >= 0 && gp < gnp) areas += garea[gp];
  }
  out[idx * 2] = (long long)inter;
  out[idx * 2 + 1] = areas - (long long)inter;
}

// one wave per area range a, lane = IoU threshold.  LDS: matched flags [G][64], then the ignore and the crowd flags in the range's order.
__global__ __launch_bounds__(64) void k_vis_match(const long long* __restrict__ counts, int D, int G, int nthr, const double* __restrict__ thrs,
                                                  const int* __restrict__ order, const unsigned char* __restrict__ ign,
                                                  const unsigned char* __restrict__ crowd, const unsigned char* __restrict__ dout,
                                                  int* __restrict__ dtm, int* __restrict__ gtm, unsigned char* __restrict__ dtig) {
  extern __shared__ unsigned char vm_lds[];
  unsigned char* flag = vm_lds;
  unsigned char* ig = vm_lds + (long)G * 64;
  unsigned char* cr = ig + G;
  const int a = blockIdx.x, lane = threadIdx.x;
  const int* ord = order + (long)a * G;
  for (int g = lane; g < G; g += 64) {
    int gg = ord[g];
    gg = gg < 0 ? 0 : gg >= G ? G - 1 : gg;                    // (the caller validates the order; a bad one still reads in bounds)
    ig[g] = ign[(long)a * G + g] != 0, cr[g] = crowd[gg] != 0;
  }
  for (int i = lane; i < G * 64; i += 64) flag[i] = 0;
  if (lane < nthr)
    for (int g = 0; g < G; ++g) gtm[((long)a * nthr + lane) * G + g] = 0;
  __syncthreads();
  if (lane >= nthr) return;
  const double thr = thrs[lane];
  for (int d = 0; d < D; ++d) {
    double best = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
    int m = -1;
    for (int gi = 0; gi < G; ++gi) {
      if (flag[gi * 64 + lane] && !cr[gi]) continue;           // already matched, and not a crowd
      if (m > -1 && !ig[m] && ig[gi]) break;                   // matched to a regular ground truth, and the ignored ones begin
      int gg = ord[gi];
      gg = gg < 0 ? 0 : gg >= G ? G - 1 : gg;
      const long long in = counts[((long)d * G + gg) * 2], un = counts[((long)d * G + gg) * 2 + 1];
      const double v = un > 0 ? (double)in / (double)un : 0.0;
      if (v < best) continue;                                  // among equal IoUs the last ground truth wins
      best = v, m = gi;
    }
    const long o = ((long)a * nthr + lane) * D + d;
    if (m < 0) {
      dtm[o] = 0, dtig[o] = dout[(long)a * D + d] != 0;        // unmatched: ignored iff outside the area range
    } else {
      int gg = ord[m];
      gg = gg < 0 ? 0 : gg >= G ? G - 1 : gg;
      dtm[o] = gg + 1, dtig[o] = ig[m];
      gtm[((long)a * nthr + lane) * G + m] = d + 1;
      flag[m * 64 + lane] = 1;
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------
int bits_pack(const void* x, int kind, float thr, const int* values, const int* planes, int n, int h, int w, unsigned long long* bits,
              int* area, hipStream_t s) {
  if (!bp_shape_ok(n, h, w) || !bp_kind_ok(kind)) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  BpSrc X;
  if (!bp_source(X, x, kind, thr, values, planes)) return SAMPT_ERR_ARG;
  if (!bits || !area || ((uintptr_t)bits & 15) || ((uintptr_t)area & 3)) return SAMPT_ERR_ARG;
  const hipError_t me = hipMemsetAsync(area, 0, (size_t)n * sizeof(int), s);
  if (me != hipSuccess) {
    set_error("bits_pack memset", me);
    return SAMPT_ERR_HIP;
  }
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long tiles = (long)n * nb * ncb;
  typedef void (*pack_fn)(BpSrc, int, int, int, int, long, int, u64*, int*);
  static const pack_fn table[3][2] = {{k_bits_pack<0, false>, k_bits_pack<0, true>},
                                      {k_bits_pack<1, false>, k_bits_pack<1, true>},
                                      {k_bits_pack<2, false>, k_bits_pack<2, true>}};
  hipLaunchKernelGGL(table[kind][w >= 4 ? 1 : 0], dim3(bp_blocks(tiles, 4)), dim3(256), 0, s, X, h, w, nb, ncb, tiles, w % 4 == 0 ? 1 : 0,
                     (u64*)bits, area);
  SAMPT_CHECK_LAUNCH("bits_pack");
  return SAMPT_OK;
}

size_t rle_decode_workspace_bytes(long total) { return total < 0 ? 0 : (size_t)total * 8 + 16; }

int rle_decode_bits(const unsigned* counts, const long long* offsets, int n, long total, int h, int w, unsigned long long* bits, int* area,
                    int* status, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!bp_shape_ok(n, h, w) || total < 0) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!offsets || !bits || !area || !status || !ws || (total > 0 && !counts)) return SAMPT_ERR_ARG;
  if (((uintptr_t)bits & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)offsets & 7) || ((uintptr_t)area & 3) || ((uintptr_t)status & 3) ||
      ((uintptr_t)counts & 3))
    return SAMPT_ERR_ARG;
  if (ws_bytes < rle_decode_workspace_bytes(total)) return SAMPT_ERR_WORKSPACE;
  const int nb = cdiv(h, 64);
  hipLaunchKernelGGL(k_rle_scan, dim3(n < 65535 ? n : 65535), dim3(256), 0, s, counts, offsets, n, total, (u64)h * (u64)w, (u64*)ws, area, status);
  SAMPT_CHECK_LAUNCH("rle_decode_bits scan");
  const long nwords = (long)n * nb * w;
  hipLaunchKernelGGL(k_rle_bits, dim3(bp_blocks(nwords, 256)), dim3(256), 0, s, (const u64*)ws, offsets, (const int*)status, h, w, nb, nwords,
                     (u64*)bits);
  SAMPT_CHECK_LAUNCH("rle_decode_bits words");
  return SAMPT_OK;
}

int bits_unpack(const unsigned long long* bits, int n, int h, int w, unsigned char* out, hipStream_t s) {
  if (!bp_shape_ok(n, h, w)) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!bits || !out || ((uintptr_t)bits & 7)) return SAMPT_ERR_ARG;
  const long npix = (long)n * h * w;
  hipLaunchKernelGGL(k_bits_unpack, dim3(bp_blocks(npix, 256)), dim3(256), 0, s, (const u64*)bits, h, w, cdiv(h, 64), npix, out);
  SAMPT_CHECK_LAUNCH("bits_unpack");
  return SAMPT_OK;
}

static bool si_shape_ok(int D, int G, int T, int h, int w) {
  return D > 0 && G > 0 && T > 0 && D <= 65535 * SI_B && G <= 65535 * SI_B && bp_shape_ok(1, h, w);
}

// the workgroups that share a tile's word positions: a function of the shapes alone (the sums do not depend on it)
static int si_kblocks(int D, int G, int T, int h, int w) {
  const long nchunks = (long)T * cdiv((long)cdiv(h, 64) * w, (long)SI_KW);
  const long tiles = (long)cdiv(D, SI_B) * cdiv(G, SI_B);
  long kb = SI_TARGET_BLOCKS / tiles;
  kb = kb < 1 ? 1 : kb;
  return (int)(kb < nchunks ? kb : nchunks);
}

size_t seq_iou_workspace_bytes(int D, int G, int T, int h, int w) {
  if (!si_shape_ok(D, G, T, h, w)) return 0;
  return (size_t)si_kblocks(D, G, T, h, w) * cdiv(D, SI_B) * SI_B * cdiv(G, SI_B) * SI_B * 8;
}

int seq_iou_counts(const unsigned long long* dt_bits, const int* dt_area, const int* dt_planes, int D, int dt_n_planes,
                   const unsigned long long* gt_bits, const int* gt_area, const int* gt_planes, int G, int gt_n_planes, int T, int h, int w,
                   long long* counts, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!si_shape_ok(D, G, T, h, w) || dt_n_planes < 0 || gt_n_planes < 0) return SAMPT_ERR_ARG;
  if (!dt_bits || !dt_area || !dt_planes || !gt_bits || !gt_area || !gt_planes || !counts || !ws) return SAMPT_ERR_ARG;
  if (((uintptr_t)dt_bits & 7) || ((uintptr_t)gt_bits & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)ws & 7)) return SAMPT_ERR_ARG;
  if (ws_bytes < seq_iou_workspace_bytes(D, G, T, h, w)) return SAMPT_ERR_WORKSPACE;
  const long wp = (long)cdiv(h, 64) * w;
  const int cpp = (int)cdiv(wp, (long)SI_KW);
  const long nchunks = (long)T * cpp;
  const int kb = si_kblocks(D, G, T, h, w), dt = cdiv(D, SI_B), gt = cdiv(G, SI_B);
  hipLaunchKernelGGL(k_seq_iou, dim3(kb, gt, dt), dim3(256), 0, s, (const u64*)dt_bits, dt_planes, D, dt_n_planes, (const u64*)gt_bits, gt_planes,
                     G, gt_n_planes, T, wp, cpp, nchunks, dt * SI_B, gt * SI_B, (u64*)ws);
  SAMPT_CHECK_LAUNCH("seq_iou_counts");
  hipLaunchKernelGGL(k_seq_iou_sum, dim3(bp_blocks((long)D * G, 256)), dim3(256), 0, s, (const u64*)ws, kb, dt * SI_B, gt * SI_B, dt_planes,
                     dt_area, D, dt_n_planes, gt_planes, gt_area, G, gt_n_planes, T, counts);
  SAMPT_CHECK_LAUNCH("seq_iou_counts sum");
  return SAMPT_OK;
}

int vis_match(const long long* counts, int D, int G, int A, int n_thr, const double* thrs, const int* gt_order, const unsigned char* gt_ignore,
              const unsigned char* iscrowd, const unsigned char* dt_out, int* dt_match, int* gt_match, unsigned char* dt_ignore, hipStream_t s) {
  if (D <= 0 || G <= 0 || G > VM_MAX_G || A <= 0 || A > 65535 || n_thr <= 0 || n_thr > VM_MAX_THR) return SAMPT_ERR_ARG;
  if (!counts || !thrs || !gt_order || !gt_ignore || !iscrowd || !dt_out || !dt_match || !gt_match || !dt_ignore) return SAMPT_ERR_ARG;
  if (((uintptr_t)counts & 7) || ((uintptr_t)thrs & 7) || ((uintptr_t)gt_order & 3) || ((uintptr_t)dt_match & 3) || ((uintptr_t)gt_match & 3))
    return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_vis_match, dim3(A), dim3(64), (size_t)G * 66, s, counts, D, G, n_thr, thrs, gt_order, gt_ignore, iscrowd, dt_out, dt_match,
                     gt_match, dt_ignore);
  SAMPT_CHECK_LAUNCH("vis_match");
  return SAMPT_OK;
}

}  // namespace sampt
