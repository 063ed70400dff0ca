// The bit-plane tile reader shared by the RLE (rle.hip), J&F (vos_metrics.hip, vos_pairs.hip, through jf_bits.h) and VIS
// (vis_eval.hip) kernels: one wave takes a tile of 64 rows x 256 columns of a plane [h][w] of bytes (set iff non-zero), f32 values
// (set iff x > thr; NaN and x == thr are clear) or uint8 indices (set iff x == value), every lane loads 4 adjacent pixels per row and
// shifts them into four 64-bit column words held in registers (bit j = row y0 + j; 0 outside the image).  With it: the decode of a
// tile number, the guarded store of a lane's four values, the wave sum, and on the host the description of a source of planes, the
// shape test and the grid size.  Everything is internal to the translation unit that includes it.
//
// Loader invariants (breaking any of them reads outside a plane):
//   - VEC (4 pixels in one load) only when w >= 4;
//   - the 4-pixel load starts at min(x0, w - 4) for lanes inside the row and at w - 4 for lanes beyond it (the lane at a row's end
//     loads the row's last 4 pixels and moves its columns down afterwards);
//   - row indices are clamped to h - 1 (rows past h re-read row h - 1);
//   - element loads are clamped to w - 1;
//   - masks are applied after the loads, never as branches around them.
#pragma once
#include "ops.h"

namespace sampt {

namespace {
typedef unsigned long long u64;
typedef unsigned int u32;

// 4 pixels in one load from any pixel address: rows of a width that is no multiple of 4 start at any byte (f32: any 4-byte) offset
typedef float bp_f32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int bp_u8x4 __attribute__((aligned(1)));

constexpr int BP_MAX_BLOCKS = 1 << 20;       // grid cap (stride loops beyond)
constexpr int BP_KIND_BYTES = 0, BP_KIND_F32 = 1, BP_KIND_INDEX = 2;

struct BpSrc {
  const void* base;                          // stack of planes [.][h][w]
  const int* planes;                         // plane of item i (null: plane i)
  const int* values;                         // BP_KIND_INDEX: the value of item i
  float thr;
  int kind;
};

template <int KIND>
__device__ __forceinline__ u32 bp_on(const void* p, long idx, float thr, int val) {
  if (KIND == BP_KIND_F32) return ((const float*)p)[idx] > thr ? 1u : 0u;
  if (KIND == BP_KIND_INDEX) return (int)((const unsigned char*)p)[idx] == val ? 1u : 0u;
  return ((const unsigned char*)p)[idx] != 0 ? 1u : 0u;
}

// pixels (y, x .. x + 3) of a row starting at element `row` -> acc[c] |= on << j
template <int KIND, bool VEC>
__device__ __forceinline__ void bp_row4(const void* p, long row, int x, int w, float thr, int val, int j, u32* acc) {
  if (VEC) {
    if (KIND == BP_KIND_F32) {
      const bp_f32x4 v = *(const bp_f32x4*)((const float*)p + row + x);
      acc[0] |= (v.x > thr ? 1u : 0u) << j, acc[1] |= (v.y > thr ? 1u : 0u) << j;
      acc[2] |= (v.z > thr ? 1u : 0u) << j, acc[3] |= (v.w > thr ? 1u : 0u) << j;
    } else {
      const u32 v = *(const bp_u8x4*)((const unsigned char*)p + row + x);
      if (KIND == BP_KIND_INDEX) {
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
      acc[c] |= bp_on<KIND>(p, row + xc, thr, val) << j;
    }
  }
}

// rows y0 .. y0 + 63 of columns x0 .. x0 + 3 of one plane as column words (0 outside the image).  TAIL = false promises w % 4 == 0:
// no lane's 4 pixels straddle the row's end, so no columns move down (k_rle_words keeps its registers for aligned widths that way)
template <int KIND, bool VEC, bool TAIL = VEC>
__device__ __forceinline__ void bp_words(const void* p, float thr, int val, int y0, int x0, int h, int w, u64* out) {
  const int xl = VEC ? (x0 + 4 <= w ? x0 : w - 4) : (x0 < w ? x0 : w - 1);
  u64 word[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int g = 0; g < 4; ++g) {                                // a real loop: 16 rows' loads in flight per wave, then their bits
    u32 piece[4] = {0, 0, 0, 0};                               // (fully unrolled, all 64 loads are hoisted: 256 VGPRs, one wave per SIMD)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int y = y0 + g * 16 + j < h ? y0 + g * 16 + j : h - 1;
      bp_row4<KIND, VEC>(p, (long)y * w, xl, w, thr, val, j, piece);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) word[c] |= (u64)piece[c] << (g * 16);
  }
  if (TAIL) {
    const int d = x0 < w ? x0 - xl : 0;                        // 0 .. 3: column x0 + c was loaded as column c + d (beyond w: masked below)
    const u64 w0 = word[0], w1 = word[1], w2 = word[2], w3 = word[3];
    word[0] = d == 0 ? w0 : d == 1 ? w1 : d == 2 ? w2 : w3;
    word[1] = d == 0 ? w1 : d == 1 ? w2 : w3;
    word[2] = d == 0 ? w2 : w3;
  }
  const int rows = h - y0 < 64 ? h - y0 : 64;
  const u64 vmask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = x0 + c < w ? word[c] & vmask : 0ull;
}

// plane `plane` of a stack of planes of npix pixels
template <int KIND>
__device__ __forceinline__ const void* bp_plane(const void* base, long plane, long npix) {
  return KIND == BP_KIND_F32 ? (const void*)((const float*)base + plane * npix) : (const void*)((const unsigned char*)base + plane * npix);
}

// the plane of item `item` of a source, and the value that marks the item in an index map
template <int KIND>
__device__ __forceinline__ const void* bp_plane(const BpSrc& s, long item, long npix, int& val) {
  val = KIND == BP_KIND_INDEX ? s.values[item] : 0;
  return bp_plane<KIND>(s.base, s.planes ? (long)s.planes[item] : item, npix);
}

// tile t of n * nb * ncb in (item, band, column block) order: rows y0 .. y0 + 63; a wave's lane holds columns x0 .. x0 + 3 (a
// workgroup with one thread per column: column cb * 256 + thread); xe is the column after the tile
struct BpTile {
  long item;
  int rb, cb, y0, x0, xe;
};

__device__ __forceinline__ BpTile bp_tile(long t, int nb, int ncb, int lane) {
  BpTile k;
  k.cb = (int)(t % ncb);
  const long q = t / ncb;
  k.rb = (int)(q % nb);
  k.item = q / nb;
  k.y0 = k.rb * 64, k.x0 = k.cb * 256 + lane * 4, k.xe = k.cb * 256 + 256;
  return k;
}

// a lane's four values to dst[0 .. 3] = columns x0 .. x0 + 3 of a row of w.  wvec (one wide store of 16 or 32 bytes) needs
// w % 4 == 0 and the array's base 16-byte aligned, which every host function checks of its workspace or output: x0 and every
// row's start are then multiples of 4 elements, so dst is 16-byte aligned (the type below claims no more than that)
template <typename T>
__device__ __forceinline__ void bp_store4(T* dst, const T* v, int x0, int w, int wvec) {
  typedef T T4 __attribute__((ext_vector_type(4), aligned(16)));
  if (wvec) {                                                  // w % 4 == 0: 16-byte aligned, x0 < w means all four columns
    if (x0 < w) *(T4*)dst = T4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (x0 + c < w) dst[c] = v[c];
  }
}

__device__ __forceinline__ int bp_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                                    // (lane 0 holds the sum)
}

// ---- host side
inline BpSrc bp_no_source() { return BpSrc{nullptr, nullptr, nullptr, 0.f, BP_KIND_BYTES}; }

inline bool bp_kind_ok(int kind) { return kind == BP_KIND_BYTES || kind == BP_KIND_F32 || kind == BP_KIND_INDEX; }

// false: not a source (unknown kind, no base, an index map without values, f32 values that are not 4-byte aligned)
inline bool bp_source(BpSrc& s, const void* base, int kind, float thr, const int* values, const int* planes) {
  if (!bp_kind_ok(kind)) return false;
  if (!base || (kind == BP_KIND_INDEX && !values) || (kind == BP_KIND_F32 && ((uintptr_t)base & 3))) return false;
  s.base = base, s.planes = planes, s.values = kind == BP_KIND_INDEX ? values : nullptr, s.thr = thr, s.kind = kind;
  return true;
}

inline bool bp_shape_ok(int n, int h, int w) { return n >= 0 && h > 0 && w > 0 && (long)h * w < (1L << 31); }

inline int bp_blocks(long work, long per_block) {
  const long b = (work + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b < BP_MAX_BLOCKS ? b : BP_MAX_BLOCKS);
}
}  // namespace

}  // namespace sampt
