// DAVIS region similarity J and boundary measure F on the device: six integer counts per (seg, ann) pair of binary images,
//   inter = |seg & ann|, union = |seg | ann|, n_seg = |B(seg)|, n_ann = |B(ann)|,
//   seg_match = |B(seg) & dil(B(ann))|, ann_match = |B(ann) & dil(B(seg))|,
// B = the boundary map seg2bmap (sam_pt_amd/vos_metrics.py), dil = binary dilation with the disk dy^2 + dx^2 <= r^2, everything
// outside the image 0.  An image is a plane [h][w] of bytes (set iff non-zero), of f32 values (set iff x > thr; NaN and x == thr
// are clear) or of a uint8 index map (set iff x == value[item]); an optional plane index per item lets several items share one
// plane.  An optional byte plane `void` clears its non-zero pixels in both images first.
//
//   k_jf_words  (pass A) one wave per tile of 64 rows x 256 columns, the tile shape of k_rle_words (csrc/rle.hip): per row every
//               lane loads 4 adjacent pixels of void, seg and ann with one 4-byte or 16-byte load (from any pixel address: the
//               rows of a width that is no multiple of 4, 854 for one, are not aligned; the lane at a row's end loads the row's
//               last 4 pixels and moves its columns down; images narrower than 4 take the element-load form) and shifts them into
//               64-bit column words held in registers (bit j = row y0 + j).
//               The south neighbour of a word is word >> 1 with the pixel of the band below carried into bit 63; the east
//               neighbour is the next column's word: the next register, the next lane's first one (a shuffle) or, for the
//               tile's last column, a word that the wave builds with one pixel per lane and a ballot.  Writes the two boundary
//               bit-planes (workspace [item][seg | ann][band][x], 8 B per 64 pixels of a column) and adds the popcounts of
//               inter, union, n_seg, n_ann.  Every pixel of the tile is read once.
//   k_jf_match  (pass B) one workgroup per (item, side, tile), one thread per column.  The threads hold the other image's boundary
//               words of the tile's columns and of r columns to each side, with the words of the band above and below, and build
//               the vertical dilations V_k (k = 0 .. r) of their columns incrementally in registers.  The disk is the union over
//               dx of V_isqrt(r^2 - dx^2)(x + dx): a level k that some dx uses is staged in LDS (two buffers in turn, one barrier
//               per level) and every thread ORs the columns x +- dx of that level.  popcount(own word & dilation) is added to
//               seg_match / ann_match; the dilated map is never written.  Tiles whose own boundary is empty are skipped.
// All sums are integer atomics on int32 (h * w < 2^31): bitwise repeatable whatever the order.
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
}  // namespace

// tiles = n * nb * ncb in (item, band, column block) order; bw: boundary words [n][2][nb][w]; counts int32 [n][6] (zeroed)
// SK / AK: the kinds of seg and ann (void is bytes); VEC: 4 pixels per load (w >= 4)
template <int SK, int AK, bool VEC>
__global__ __launch_bounds__(256) void k_jf_words(JfSrc seg, JfSrc ann, JfSrc vd, int h, int w, int nb, int ncb, long tiles, int wvec,
                                                  u64* __restrict__ bw, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const int cb = (int)(t % ncb);
    const long q = t / ncb;
    const int rb = (int)(q % nb);
    const long item = q / nb;
    const int y0 = rb * 64, x0 = cb * 256 + lane * 4, xe = cb * 256 + 256;
    JfBits S, A;
    jf_bits<SK, VEC>(seg, item, npix, y0, x0, xe, h, w, lane, S);
    jf_bits<AK, VEC>(ann, item, npix, y0, x0, xe, h, w, lane, A);
    if (vd.base) {
      JfBits V;
      jf_bits<JF_KIND_BYTES, VEC>(vd, item, npix, y0, x0, xe, h, w, lane, V);
      jf_clear(S, V);
      jf_clear(A, V);
    }
    u64 bs[4], ba[4];
    jf_boundary(S, y0, x0, h, w, lane, bs);
    jf_boundary(A, y0, x0, h, w, lane, ba);
    int inter = 0, uni = 0, ns = 0, na = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      inter += __popcll(S.word[c] & A.word[c]), uni += __popcll(S.word[c] | A.word[c]);
      ns += __popcll(bs[c]), na += __popcll(ba[c]);
    }
    u64* ps = bw + ((item * 2) * nb + rb) * (long)w + x0;
    u64* pa = bw + ((item * 2 + 1) * nb + rb) * (long)w + x0;
    if (wvec) {                                                // w % 4 == 0: 32-byte aligned, x0 < w means all four columns
      if (x0 < w) {
        *(ulonglong2*)ps = make_ulonglong2(bs[0], bs[1]), *(ulonglong2*)(ps + 2) = make_ulonglong2(bs[2], bs[3]);
        *(ulonglong2*)pa = make_ulonglong2(ba[0], ba[1]), *(ulonglong2*)(pa + 2) = make_ulonglong2(ba[2], ba[3]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (x0 + c < w) ps[c] = bs[c], pa[c] = ba[c];
    }
    inter = jf_wave_sum(inter), uni = jf_wave_sum(uni), ns = jf_wave_sum(ns), na = jf_wave_sum(na);
    if (lane == 0) {
      int* o = counts + item * 6;
      if (inter) atomicAdd(o + 0, inter);
      if (uni) atomicAdd(o + 1, uni);
      if (ns) atomicAdd(o + 2, ns);
      if (na) atomicAdd(o + 3, na);
    }
  }
}

// tiles = n * 2 * nb * ncb in (item, side, band, column block) order; side 0: B(seg) & dil(B(ann)), side 1: the other way round
__global__ __launch_bounds__(256) void k_jf_match(const u64* __restrict__ bw, int w, int nb, int ncb, int r, JfDisk disk, long tiles,
                                                  int* __restrict__ counts) {
  __shared__ u64 lv[2][256 + 2 * JF_MAX_R];
  __shared__ int red[4];
  const int tid = threadIdx.x;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {       // block-uniform
    const int cb = (int)(t % ncb);
    long q = t / ncb;
    const int rb = (int)(q % nb);
    q /= nb;
    const int side = (int)(q & 1);
    const long item = q >> 1;
    const u64* own = bw + ((item * 2 + side) * nb) * (long)w;
    const u64* oth = bw + ((item * 2 + (side ^ 1)) * nb) * (long)w;
    const int x = cb * 256 + tid;
    const u64 mine = x < w ? own[(long)rb * w + x] : 0ull;
    if (!__syncthreads_or(mine != 0ull)) continue;             // (also: the previous tile's readers of lv and red are done)
    u64 up[2], mid[2], dn[2], V[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {                              // halo column tid + 256 i of 256 + 2 r = image column xx
      const int hc = tid + i * 256, xx = cb * 256 - r + hc;
      const bool ok = hc < 256 + 2 * r && xx >= 0 && xx < w;
      mid[i] = ok ? oth[(long)rb * w + xx] : 0ull;
      up[i] = ok && rb > 0 ? oth[(long)(rb - 1) * w + xx] : 0ull;
      dn[i] = ok && rb + 1 < nb ? oth[(long)(rb + 1) * w + xx] : 0ull;
      V[i] = mid[i];
    }
    u64 D = 0;
    int p = 0;
    for (int k = 0; k <= r; ++k) {
      if (k > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)                            // rows y - k and y + k (k = 64: the neighbouring bands themselves)
          V[i] |= k < 64 ? (mid[i] << k) | (up[i] >> (64 - k)) | (mid[i] >> k) | (dn[i] << (64 - k)) : up[i] | dn[i];
      }
      const int lo = disk.lo[k], hi = disk.hi[k];
      if (lo > hi) continue;                                   // no dx has this half-height
      lv[p][tid] = V[0];
      if (tid + 256 < 256 + 2 * r) lv[p][tid + 256] = V[1];
      __syncthreads();                                         // (the buffer written two levels on is free: its readers passed here)
      for (int dx = lo; dx <= hi; ++dx) D |= lv[p][tid + r - dx] | lv[p][tid + r + dx];
      p ^= 1;
    }
    const int m = jf_wave_sum(__popcll(mine & D));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      const int tot = red[0] + red[1] + red[2] + red[3];
      if (tot) atomicAdd(counts + item * 6 + 4 + side, tot);
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------
static bool jf_shape_ok(int n, int h, int w, int r) {
  return n > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31) && r >= 0 && r <= JF_MAX_R;
}

size_t jf_workspace_bytes(int n, int h, int w, int radius) {
  if (!jf_shape_ok(n, h, w, radius)) return 0;
  return (size_t)n * 2 * cdiv(h, 64) * (size_t)w * 8;
}

static int jf_isqrt(int v) {
  int s = 0;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}

static bool jf_src(JfSrc& s, const void* base, int kind, float thr, const int* values, const int* planes, int w) {
  if (kind != JF_KIND_BYTES && kind != JF_KIND_F32 && kind != JF_KIND_INDEX) return false;
  if (!base || (kind == JF_KIND_INDEX && !values) || (kind == JF_KIND_F32 && ((uintptr_t)base & 3))) return false;
  s.base = base, s.planes = planes, s.values = kind == JF_KIND_INDEX ? values : nullptr, s.thr = thr, s.kind = kind;
  return true;
}

int jf_counts(const void* seg, int seg_kind, float seg_thr, const int* seg_values, const int* seg_planes, const void* ann, int ann_kind,
              float ann_thr, const int* ann_values, const int* ann_planes, const unsigned char* void_px, const int* void_planes, int n,
              int h, int w, int radius, int* counts, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!jf_shape_ok(n, h, w, radius)) return SAMPT_ERR_ARG;
  JfSrc S, A, V;
  if (!jf_src(S, seg, seg_kind, seg_thr, seg_values, seg_planes, w)) return SAMPT_ERR_ARG;
  if (!jf_src(A, ann, ann_kind, ann_thr, ann_values, ann_planes, w)) return SAMPT_ERR_ARG;
  if (void_px) {
    jf_src(V, void_px, JF_KIND_BYTES, 0.f, nullptr, void_planes, w);
  } else {
    V.base = nullptr, V.planes = nullptr, V.values = nullptr, V.thr = 0.f, V.kind = JF_KIND_BYTES;
  }
  if (!counts || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)counts & 3)) return SAMPT_ERR_ARG;
  if (ws_bytes < jf_workspace_bytes(n, h, w, radius)) return SAMPT_ERR_WORKSPACE;
  JfDisk disk;
  const int r = radius;
  for (int k = 0; k <= JF_MAX_R; ++k) disk.lo[k] = 1, disk.hi[k] = 0;
  for (int k = 0; k <= r; ++k) {                               // isqrt(r^2 - dx^2) == k  <=>  lo <= dx <= hi
    disk.lo[k] = (unsigned char)(k == r ? 0 : jf_isqrt(r * r - (k + 1) * (k + 1)) + 1);
    disk.hi[k] = (unsigned char)jf_isqrt(r * r - k * k);
  }
  const hipError_t me = hipMemsetAsync(counts, 0, (size_t)n * 6 * sizeof(int), s);
  if (me != hipSuccess) {
    set_error("jf_counts memset", me);
    return SAMPT_ERR_HIP;
  }
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long tiles = (long)n * nb * ncb;
  const int blocks = (int)((tiles + 3) / 4 < JF_MAX_BLOCKS ? (tiles + 3) / 4 : JF_MAX_BLOCKS);
  typedef void (*words_fn)(JfSrc, JfSrc, JfSrc, int, int, int, int, long, int, u64*, int*);
#define JF_W(sk, ak) {k_jf_words<sk, ak, false>, k_jf_words<sk, ak, true>}
  static const words_fn table[3][3][2] = {{JF_W(0, 0), JF_W(0, 1), JF_W(0, 2)}, {JF_W(1, 0), JF_W(1, 1), JF_W(1, 2)},
                                          {JF_W(2, 0), JF_W(2, 1), JF_W(2, 2)}};
#undef JF_W
  hipLaunchKernelGGL(table[seg_kind][ann_kind][w >= 4 ? 1 : 0], dim3(blocks), dim3(256), 0, s, S, A, V, h, w, nb, ncb, tiles,
                     w % 4 == 0 ? 1 : 0, (u64*)ws, counts);
  SAMPT_CHECK_LAUNCH("jf_counts words");
  const long mtiles = tiles * 2;
  hipLaunchKernelGGL(k_jf_match, dim3((int)(mtiles < JF_MAX_BLOCKS ? mtiles : JF_MAX_BLOCKS)), dim3(256), 0, s, (const u64*)ws, w, nb, ncb,
                     r, disk, mtiles, counts);
  SAMPT_CHECK_LAUNCH("jf_counts match");
  return SAMPT_OK;
}

}  // namespace sampt
