// "The r-th set pixel of this mask, in nonzero() order" on bit-planes: what query-point selection from masks (SamPt.extract_query_points
// in query_masks mode, and every re-initialisation segment; sam_pt_amd/query_points.py) needs so that the host draws ranks from a
// mask's AREA alone and the pixels never leave the device.  Planes are in the format of bits_pack (vis_eval.hip): uint64
// [n][ceil(h / 64)][w], bit j of word (band b, column x) = pixel (64 b + j, x), the bits of rows >= h are 0.  The specification is the
// host restatement sam_pt_amd/mask_points.py (row_prefix / select_ranks); the results equal it word for word.  Integer work only, no
// atomics, stream-ordered.
//
//   k_mp_row_counts   one wave per (plane, band): a lane holds column x0 + lane of the band; a ballot per row bit over the 64 columns,
//                     its popcount goes to the lane that owns the row -> prefix[plane][1 + y] = set pixels of row y.
//   k_mp_row_scan     one wave per plane: the counts become the exclusive prefix over rows, 64 rows per step (shuffle scan + carry);
//                     prefix[plane][0] = 0, prefix[plane][h] = the plane's area.  The complement's prefix is y * w - prefix[y]: not stored.
//   k_mp_select       one wave per query (plane, invert, rank): binary search of the row in the prefix, then the row's columns 64 at
//                     a time - ballot of (bit ^ invert) guarded by x < w, popcount to skip whole groups, and inside the group the lane
//                     whose lower lanes hold exactly the remaining rank.  (y, x) as floats; (-1, -1) for a plane or rank out of range.
//
// The loader invariants of bitplane.h hold here too: indices are clamped (plane to [0, n), column to w - 1, row by the search's
// bounds), masks are applied after the loads, never as branches around them.
#include "ops.h"
#include "bitplane.h"

namespace sampt {

namespace {
constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
}  // namespace

// tiles = n * nb in (plane, band) order; prefix int [n][h + 1]
__global__ __launch_bounds__(MP_THREADS) void k_mp_row_counts(const u64* __restrict__ bits, int h, int w, int nb, long tiles,
                                                              int* __restrict__ prefix) {
  const int lane = threadIdx.x & 63;
  for (long t = (long)blockIdx.x * MP_WAVES + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * MP_WAVES) {   // wave-uniform
    const long plane = t / nb;
    const int rb = (int)(t % nb);
    const u64* row = bits + t * (long)w;                       // words of (plane, band)
    int cnt = 0;                                               // set pixels of row 64 rb + lane
    for (int x0 = 0; x0 < w; x0 += 64) {
      const int x = x0 + lane;
      const u64 loaded = row[x < w ? x : w - 1];
      const u64 word = x < w ? loaded : 0ull;
#pragma unroll 8
      for (int j = 0; j < 64; ++j) {
        const int c = __popcll(__ballot((word >> j) & 1ull));
        cnt += lane == j ? c : 0;
      }
    }
    const int y = rb * 64 + lane;
    if (y < h) prefix[plane * (long)(h + 1) + 1 + y] = cnt;
  }
}

// in place: prefix[plane][1 + y] = count of row y  ->  prefix[plane][y] = set pixels in rows < y, y = 0 .. h
__global__ __launch_bounds__(MP_THREADS) void k_mp_row_scan(int n, int h, int* __restrict__ prefix) {
  const int lane = threadIdx.x & 63;
  for (long plane = (long)blockIdx.x * MP_WAVES + (threadIdx.x >> 6); plane < n; plane += (long)gridDim.x * MP_WAVES) {   // wave-uniform
    int* p = prefix + plane * (long)(h + 1);
    if (lane == 0) p[0] = 0;
    int carry = 0;
    for (int y0 = 0; y0 < h; y0 += 64) {
      const int y = y0 + lane;
      const int loaded = p[1 + (y < h ? y : h - 1)];
      int v = y < h ? loaded : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o, 64);
        v += lane >= o ? up : 0;
      }
      if (y < h) p[1 + y] = carry + v;                         // (every lane wrote back only what it had read itself)
      carry += __shfl(v, 63, 64);
    }
  }
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_select(const u64* __restrict__ bits, const int* __restrict__ prefix, int n, int h, int w,
                                                          int nb, const int* __restrict__ queries, int nq, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (long q = (long)blockIdx.x * MP_WAVES + (threadIdx.x >> 6); q < nq; q += (long)gridDim.x * MP_WAVES) {   // wave-uniform
    const int plane_q = queries[3 * q], inv = queries[3 * q + 1] != 0 ? 1 : 0, rank = queries[3 * q + 2];
    const bool plane_ok = plane_q >= 0 && plane_q < n;
    const long plane = plane_ok ? plane_q : 0;
    const int* pf = prefix + plane * (long)(h + 1);
    const int area = pf[h];
    const int total = inv ? h * w - area : area;               // (h * w < 2^31)
    const bool ok = plane_ok && rank >= 0 && rank < total;
    // the last row y of [0, h) with cnt(y) <= rank, cnt(y) = pixels that count in rows < y (non-decreasing, cnt(0) = 0)
    int lo = 0, hi = h - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;                  // 1 .. h - 1
      const int c = inv ? mid * w - pf[mid] : pf[mid];
      if (ok && c <= rank) lo = mid; else hi = mid - 1;
    }
    const int y = lo;
    int k = rank - (inv ? y * w - pf[y] : pf[y]);              // the k-th counting pixel of row y
    const u64* row = bits + (plane * nb + (y >> 6)) * (long)w;
    bool found = false;
    for (int x0 = 0; ok && x0 < w && !found; x0 += 64) {       // wave-uniform
      const int x = x0 + lane;
      const u64 word = row[x < w ? x : w - 1];
      const bool on = ok && x < w && ((int)((word >> (y & 63)) & 1ull) ^ inv) != 0;
      const u64 b = __ballot(on);
      const int c = __popcll(b);
      if (k >= 0 && k < c) {
        if (on && __popcll(b & ((1ull << lane) - 1ull)) == k) out[2 * q] = (float)y, out[2 * q + 1] = (float)x;
        found = true;
      }
      k -= c;
    }
    // out of range, or a prefix that does not belong to these planes
    if (!found && lane == 0) out[2 * q] = -1.f, out[2 * q + 1] = -1.f;
  }
}

int bits_row_prefix(const unsigned long long* bits, int n, int h, int w, int* prefix, hipStream_t s) {
  if (!bp_shape_ok(n, h, w)) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!bits || !prefix || ((uintptr_t)bits & 7) || ((uintptr_t)prefix & 3)) return SAMPT_ERR_ARG;
  const int nb = cdiv(h, 64);
  const long tiles = (long)n * nb;
  hipLaunchKernelGGL(k_mp_row_counts, dim3(bp_blocks(tiles, MP_WAVES)), dim3(MP_THREADS), 0, s, (const u64*)bits, h, w, nb, tiles, prefix);
  SAMPT_CHECK_LAUNCH("bits_row_prefix counts");
  hipLaunchKernelGGL(k_mp_row_scan, dim3(bp_blocks(n, MP_WAVES)), dim3(MP_THREADS), 0, s, n, h, prefix);
  SAMPT_CHECK_LAUNCH("bits_row_prefix scan");
  return SAMPT_OK;
}

int bits_select(const unsigned long long* bits, const int* prefix, int n, int h, int w, const int* queries, int nq, float* yx_out,
                hipStream_t s) {
  if (!bp_shape_ok(n, h, w) || nq < 0) return SAMPT_ERR_ARG;
  if (n == 0 || nq == 0) return SAMPT_OK;
  if (!bits || !prefix || !queries || !yx_out) return SAMPT_ERR_ARG;
  if (((uintptr_t)bits & 7) || ((uintptr_t)prefix & 3) || ((uintptr_t)queries & 3) || ((uintptr_t)yx_out & 3)) return SAMPT_ERR_ARG;
  hipLaunchKernelGGL(k_mp_select, dim3(bp_blocks(nq, MP_WAVES)), dim3(MP_THREADS), 0, s, (const u64*)bits, prefix, n, h, w, cdiv(h, 64), queries,
                     nq, yx_out);
  SAMPT_CHECK_LAUNCH("bits_select");
  return SAMPT_OK;
}

}  // namespace sampt
