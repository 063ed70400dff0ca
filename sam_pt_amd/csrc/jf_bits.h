// Device helpers of the DAVIS J / F kernels (vos_metrics.hip, vos_pairs.hip) on top of the bit-plane tile reader (bitplane.h): a
// tile's column words with the column east of it and the row below it, seg2bmap on those words, the table of the disk's spans and
// the disk dilation of a tile of boundary words.  Everything is internal to the translation unit that includes it.
#pragma once
#include "bitplane.h"

namespace sampt {

namespace {
constexpr int JF_MAX_R = 64;                 // one band of halo above and below

// disk rows per level: the dx whose column span is V_k are lo[k] .. hi[k] (none if lo > hi)
struct JfDisk {
  unsigned char lo[JF_MAX_R + 1], hi[JF_MAX_R + 1];
};

// what one lane knows of one image around its 4 columns of a tile
struct JfBits {
  u64 word[4];                               // rows y0 .. y0 + 63 of columns x0 .. x0 + 3 (0 outside the image)
  u64 east;                                  // the same rows of the column after the tile (wave-uniform)
  u32 below;                                 // bit c: pixel (y0 + 64, x0 + c); bit 4: (y0 + 64, column after the tile)
};

// bp_words plus the east column and the row below, loaded by bitplane.h's rules: unconditional on a clamped index, masked afterwards
template <int KIND, bool VEC>
__device__ __forceinline__ void jf_bits_k(const void* p, float thr, int val, const BpTile& k, int h, int w, int lane, JfBits& b) {
  const int y0 = k.y0, x0 = k.x0, xe = k.xe;
  const int ye = y0 + lane < h ? y0 + lane : h - 1, yb = y0 + 64 < h ? y0 + 64 : h - 1;
  const int xec = xe < w ? xe : w - 1;
  const u32 e_on = bp_on<KIND>(p, (long)ye * w + xec, thr, val);
  u32 below = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int xc = x0 + c < w ? x0 + c : w - 1;
    below |= bp_on<KIND>(p, (long)yb * w + xc, thr, val) << c;
  }
  below |= bp_on<KIND>(p, (long)yb * w + xec, thr, val) << 4;
  bp_words<KIND, VEC>(p, thr, val, y0, x0, h, w, b.word);
  const int rows = h - y0 < 64 ? h - y0 : 64;
  const u64 vmask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
  u32 bmask = xe < w ? 1u << 4 : 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) bmask |= (x0 + c < w ? 1u : 0u) << c;
  b.east = xe < w ? (u64)__ballot(e_on != 0) & vmask : 0ull;
  b.below = y0 + 64 < h ? below & bmask : 0u;
}

template <int KIND, bool VEC>
__device__ __forceinline__ void jf_bits(const BpSrc& s, long item, long npix, const BpTile& k, int h, int w, int lane, JfBits& b) {
  int val;
  const void* p = bp_plane<KIND>(s, item, npix, val);
  jf_bits_k<KIND, VEC>(p, s.thr, val, k, h, w, lane, b);
}

__device__ __forceinline__ void jf_clear(JfBits& b, const JfBits& v) {
#pragma unroll
  for (int c = 0; c < 4; ++c) b.word[c] &= ~v.word[c];
  b.east &= ~v.east;
  b.below &= ~v.below;
}

// seg2bmap of the lane's 4 columns: b = (m ^ e) | (m ^ s) | (m ^ se); last row: m ^ e; last column: m ^ s; the corner: 0
__device__ __forceinline__ void jf_boundary(const JfBits& b, int y0, int x0, int h, int w, int lane, u64* out) {
  u64 nw = __shfl_down(b.word[0], 1, 64);                      // the next lane's first column
  u32 nb = __shfl_down(b.below, 1, 64) & 1u;
  if (lane == 63) nw = b.east, nb = (b.below >> 4) & 1u;
  const int last = h - 1 - y0;                                 // the image's last row is bit `last` of this band (if 0 .. 63)
  const u64 lbit = (last >= 0 && last < 64) ? 1ull << last : 0ull;
  const int rows = h - y0 < 64 ? h - y0 : 64;
  const u64 vmask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const u64 m = b.word[c];
    const u64 e = c < 3 ? b.word[c < 3 ? c + 1 : 3] : nw;
    const u32 eb = c < 3 ? (b.below >> (c + 1)) & 1u : nb;
    const u64 s = (m >> 1) | ((u64)((b.below >> c) & 1u) << 63);
    const u64 se = (e >> 1) | ((u64)eb << 63);
    u64 v = (m ^ e) | (m ^ s) | (m ^ se);
    v = (v & ~lbit) | ((m ^ e) & lbit);
    if (x0 + c == w - 1) v = (m ^ s) & ~lbit;
    out[c] = x0 + c < w ? v & vmask : 0ull;
  }
}

// The disk dilation of a tile of 64 rows x 256 columns of a plane of words src [nb][w], one thread per column.  jf_halo: the
// thread's two columns tid and tid + 256 of the 256 + 2 r halo columns, in the tile's band (mid) and the bands above and below.
__device__ __forceinline__ void jf_halo(const u64* __restrict__ src, const BpTile& k, int nb, int w, int r, int tid, u64* mid, u64* up,
                                        u64* dn) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {                                // halo column tid + 256 i of 256 + 2 r = image column xx
    const int hc = tid + i * 256, xx = k.cb * 256 - r + hc;
    const bool ok = hc < 256 + 2 * r && xx >= 0 && xx < w;
    mid[i] = ok ? src[(long)k.rb * w + xx] : 0ull;
    up[i] = ok && k.rb > 0 ? src[(long)(k.rb - 1) * w + xx] : 0ull;
    dn[i] = ok && k.rb + 1 < nb ? src[(long)(k.rb + 1) * w + xx] : 0ull;
  }
}

// jf_dilate: the vertical dilations V_k (k = 0 .. r) of the halo columns grow in registers; the disk is the union over dx of
// V_isqrt(r^2 - dx^2)(x + dx): a level that some dx uses is staged in lv (two buffers in turn, one barrier per level) and every
// thread ORs the columns x +- dx of it.  Returns the dilation of the thread's column (bits of rows >= h not cleared).
// The caller has passed a workgroup barrier since lv's previous readers: the first level is written without one.  Inside, a
// level's buffer is rewritten only two levels later, past the barrier its readers have passed.
__device__ __forceinline__ u64 jf_dilate(const u64* mid, const u64* up, const u64* dn, int r, const JfDisk& disk,
                                         u64 (*lv)[256 + 2 * JF_MAX_R], int tid) {
  u64 V[2] = {mid[0], mid[1]};
  u64 D = 0;
  int p = 0;
  for (int k = 0; k <= r; ++k) {
    if (k > 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)                              // rows y - k and y + k (k = 64: the neighbouring bands themselves)
        V[i] |= k < 64 ? (mid[i] << k) | (up[i] >> (64 - k)) | (mid[i] >> k) | (dn[i] << (64 - k)) : up[i] | dn[i];
    }
    const int lo = disk.lo[k], hi = disk.hi[k];
    if (lo > hi) continue;                                     // no dx has this half-height
    lv[p][tid] = V[0];
    if (tid + 256 < 256 + 2 * r) lv[p][tid + 256] = V[1];
    __syncthreads();                                           // (the buffer written two levels on is free: its readers passed here)
    for (int dx = lo; dx <= hi; ++dx) D |= lv[p][tid + r - dx] | lv[p][tid + r + dx];
    p ^= 1;
  }
  return D;
}

// ---- host side
inline int jf_isqrt(int v) {
  int s = 0;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}

// the spans of the disk of radius r (0 .. JF_MAX_R) per level
inline JfDisk jf_disk(int r) {
  JfDisk disk;
  for (int k = 0; k <= JF_MAX_R; ++k) disk.lo[k] = 1, disk.hi[k] = 0;
  for (int k = 0; k <= r; ++k) {                               // isqrt(r^2 - dx^2) == k  <=>  lo <= dx <= hi
    disk.lo[k] = (unsigned char)(k == r ? 0 : jf_isqrt(r * r - (k + 1) * (k + 1)) + 1);
    disk.hi[k] = (unsigned char)jf_isqrt(r * r - k * k);
  }
  return disk;
}
}  // namespace

}  // namespace sampt
