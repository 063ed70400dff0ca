// Device helpers of the DAVIS J / F kernels (vos_metrics.hip, vos_pairs.hip): the description of a source of binary images, the
// loader of a tile of 64 rows x 256 columns into 64-bit column words (4 pixels per load from any pixel address), seg2bmap on those
// words, and the table of the disk's spans.  Everything is internal to the translation unit that includes it.
#pragma once
#include "ops.h"

namespace sampt {

namespace {
typedef unsigned long long u64;
typedef unsigned int u32;

// 4 pixels in one load from any pixel address: rows of a width that is no multiple of 4 start at any byte (f32: any 4-byte) offset
typedef float jf_f32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int jf_u8x4 __attribute__((aligned(1)));

constexpr int JF_MAX_BLOCKS = 1 << 20;       // grid cap (stride loops beyond)
constexpr int JF_MAX_R = 64;                 // one band of halo above and below
constexpr int JF_KIND_BYTES = 0, JF_KIND_F32 = 1, JF_KIND_INDEX = 2;

struct JfSrc {
  const void* base;                          // stack of planes [.][h][w]
  const int* planes;                         // plane of item i (null: plane i)
  const int* values;                         // JF_KIND_INDEX: the value of item i
  float thr;
  int kind;
};

// disk rows per level: the dx whose column span is V_k are lo[k] .. hi[k] (none if lo > hi)
struct JfDisk {
  unsigned char lo[JF_MAX_R + 1], hi[JF_MAX_R + 1];
};

template <int KIND>
__device__ __forceinline__ u32 jf_on(const void* p, long idx, float thr, int val) {
  if (KIND == JF_KIND_F32) return ((const float*)p)[idx] > thr ? 1u : 0u;
  if (KIND == JF_KIND_INDEX) return (int)((const unsigned char*)p)[idx] == val ? 1u : 0u;
  return ((const unsigned char*)p)[idx] != 0 ? 1u : 0u;
}

// pixels (y, x .. x + 3) of a row starting at element `row` -> acc[c] |= on << j
template <int KIND, bool VEC>
__device__ __forceinline__ void jf_row4(const void* p, long row, int x, int w, float thr, int val, int j, u32* acc) {
  if (VEC) {
    if (KIND == JF_KIND_F32) {
      const jf_f32x4 v = *(const jf_f32x4*)((const float*)p + row + x);
      acc[0] |= (v.x > thr ? 1u : 0u) << j, acc[1] |= (v.y > thr ? 1u : 0u) << j;
      acc[2] |= (v.z > thr ? 1u : 0u) << j, acc[3] |= (v.w > thr ? 1u : 0u) << j;
    } else {
      const u32 v = *(const jf_u8x4*)((const unsigned char*)p + row + x);
      if (KIND == JF_KIND_INDEX) {
        acc[0] |= ((int)(v & 0xffu) == val ? 1u : 0u) << j, acc[1] |= ((int)((v >> 8) & 0xffu) == val ? 1u : 0u) << j;
        acc[2] |= ((int)((v >> 16) & 0xffu) == val ? 1u : 0u) << j, acc[3] |= ((int)(v >> 24) == val ? 1u : 0u) << j;
      } else {
        acc[0] |= ((v & 0xffu) ? 1u : 0u) << j, acc[1] |= ((v & 0xff00u) ? 1u : 0u) << j;
        acc[2] |= ((v & 0xff0000u) ? 1u : 0u) << j, acc[3] |= ((v & 0xff000000u) ? 1u : 0u) << j;
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int xc = x + c < w ? x + c : w - 1;                // (clamped: the load is always inside the row; unused beyond w)
      acc[c] |= jf_on<KIND>(p, row + xc, thr, val) << j;
    }
  }
}

// what one lane knows of one image around its 4 columns of a tile
struct JfBits {
  u64 word[4];                               // rows y0 .. y0 + 63 of columns x0 .. x0 + 3 (0 outside the image)
  u64 east;                                  // the same rows of the column after the tile (wave-uniform)
  u32 below;                                 // bit c: pixel (y0 + 64, x0 + c); bit 4: (y0 + 64, column after the tile)
};

// every load is unconditional on a clamped index and masked afterwards (rows past h re-read row h - 1, lanes past w the row's end)
template <int KIND, bool VEC>
__device__ __forceinline__ void jf_bits_k(const void* p, float thr, int val, int y0, int x0, int xe, int h, int w, int lane,
                                          JfBits& b) {
  // VEC (w >= 4): a lane whose 4 pixels would pass the row's end loads the row's last 4 and moves its columns down afterwards
  const int xl = VEC ? (x0 + 4 <= w ? x0 : w - 4) : (x0 < w ? x0 : w - 1);
  const int ye = y0 + lane < h ? y0 + lane : h - 1, yb = y0 + 64 < h ? y0 + 64 : h - 1;
  const int xec = xe < w ? xe : w - 1;
  const u32 e_on = jf_on<KIND>(p, (long)ye * w + xec, thr, val);
  u32 below = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int xc = x0 + c < w ? x0 + c : w - 1;
    below |= jf_on<KIND>(p, (long)yb * w + xc, thr, val) << c;
  }
  below |= jf_on<KIND>(p, (long)yb * w + xec, thr, val) << 4;
  u64 word[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int g = 0; g < 4; ++g) {                                // a real loop, as in k_rle_words: 16 rows' loads in flight, then their bits
    u32 piece[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int y = y0 + g * 16 + j < h ? y0 + g * 16 + j : h - 1;
      jf_row4<KIND, VEC>(p, (long)y * w, xl, w, thr, val, j, piece);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) word[c] |= (u64)piece[c] << (g * 16);
  }
  if (VEC) {
    const int d = x0 < w ? x0 - xl : 0;                        // 0 .. 3: column x0 + c was loaded as column c + d (beyond w: masked below)
    const u64 w0 = word[0], w1 = word[1], w2 = word[2], w3 = word[3];
    word[0] = d == 0 ? w0 : d == 1 ? w1 : d == 2 ? w2 : w3;
    word[1] = d == 0 ? w1 : d == 1 ? w2 : w3;
    word[2] = d == 0 ? w2 : w3;
  }
  const int rows = h - y0 < 64 ? h - y0 : 64;
  const u64 vmask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
  u32 bmask = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool in = x0 + c < w;
    b.word[c] = in ? word[c] & vmask : 0ull;
    bmask |= (in ? 1u : 0u) << c;
  }
  bmask |= (xe < w ? 1u : 0u) << 4;
  b.east = xe < w ? (u64)__ballot(e_on != 0) & vmask : 0ull;
  b.below = y0 + 64 < h ? below & bmask : 0u;
}

template <int KIND, bool VEC>
__device__ __forceinline__ void jf_bits(const JfSrc& s, long item, long npix, int y0, int x0, int xe, int h, int w, int lane,
                                        JfBits& b) {
  const long plane = s.planes ? (long)s.planes[item] : item;
  const int val = KIND == JF_KIND_INDEX ? s.values[item] : 0;
  const void* p = KIND == JF_KIND_F32 ? (const void*)((const float*)s.base + plane * npix)
                                      : (const void*)((const unsigned char*)s.base + plane * npix);
  jf_bits_k<KIND, VEC>(p, s.thr, val, y0, x0, xe, h, w, lane, b);
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

__device__ __forceinline__ int jf_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                                    // (lane 0 holds the sum)
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

inline bool jf_src(JfSrc& s, const void* base, int kind, float thr, const int* values, const int* planes, int w) {
  if (kind != JF_KIND_BYTES && kind != JF_KIND_F32 && kind != JF_KIND_INDEX) return false;
  if (!base || (kind == JF_KIND_INDEX && !values) || (kind == JF_KIND_F32 && ((uintptr_t)base & 3))) return false;
  s.base = base, s.planes = planes, s.values = kind == JF_KIND_INDEX ? values : nullptr, s.thr = thr, s.kind = kind;
  return true;
}
}  // namespace

}  // namespace sampt
