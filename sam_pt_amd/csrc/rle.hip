// COCO run-length encoding of a stack of masks on the device: the runs of mask_to_rle (sam_pt_amd/automatic_mask_generator.py)
// and maskApi's rleToString of them, from bytes (non-zero = set) or from f32 values with a threshold (set iff x > thr; NaN and
// x == thr are clear).  Runs go over the column-major flattening p = x * h + y, the first run counts zeros.
//
// Only the pass over the pixels is hot:
//   k_rle_words   one wave per tile of 64 rows x 256 columns, read by the tile reader of csrc/bitplane.h: per row every lane loads 4
//                 adjacent pixels (one 4-byte or one 16-byte load: the wave reads a contiguous 256 B / 1 KiB segment) into four
//                 64-bit column words held in registers (bit j = row y0 + j); no LDS.  transitions = word ^ ((word << 1) | carry), carry =
//                 the pixel before the word in column-major order: (y0 - 1, x), or (h - 1, x - 1) for the first word of a
//                 column, or 0 for the first pixel of a mask (so a mask that starts set opens with a 0 run and nothing leaks
//                 from the mask before it).  Written per word: the transition word, popcount(transitions) | popcount(word) << 16.
//                 Any width and base take the 4-pixel loads; only images narrower than 4 take the element-load form.
// The rest moves a thousandth of that:
//   k_rle_scan    one workgroup per mask walks its words in run order (x, then row block): exclusive sum of the transition
//                 counts, exclusive max of the last transition's position, the mask's area and number of runs
//   k_rle_offsets exclusive scan of the run numbers over the stack -> int64 offsets [n + 1] (the host reads the last one)
//   k_rle_emit    one thread per word: counts[k] = pos[k] - pos[k - 1]; the last word of a mask adds the closing h * w - pos[last]
//   k_str_*       length of every count's chunk string, a scan over the whole stack, the characters
// Everything is integer, every sum has a fixed order and there is no atomic: bitwise repeatable.
//
// Workspace (storage order [mask][row block][x], so the hot kernel's stores are contiguous per wave): 8 B transition word +
// 4 B count (then: run offset inside the mask) + 4 B previous position per 64 pixels of a column, + 16 B per mask.
#include "ops.h"
#include "bitplane.h"

namespace sampt {

namespace {
constexpr int STR_PER_THREAD = 8, STR_PER_BLOCK = 256 * STR_PER_THREAD;

struct OpAdd {
  template <typename V>
  __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};
struct OpMax {
  template <typename V>
  __device__ __forceinline__ V operator()(V a, V b) const { return a > b ? a : b; }
};

// exclusive scan of one value per thread over a 256-thread workgroup (op associative and commutative, `zero` its identity);
// total = the reduction of all 256.  Wave scans by shuffles, the four wave totals through sm (4 values of LDS).
template <typename V, typename Op>
__device__ __forceinline__ V block_scan_excl(V v, Op op, V zero, V* sm, V& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  V inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(inc, o, 64);
    if (lane >= o) inc = op(u, inc);
  }
  V exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = zero;
  __syncthreads();                                             // (a previous call's readers are done)
  if (lane == 63) sm[wave] = inc;
  __syncthreads();
  V pre = zero;
  total = zero;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const V t = sm[k];
    if (k < wave) pre = op(pre, t);
    total = op(total, t);
  }
  return op(pre, exc);
}
}  // namespace

// tiles = n * nb * ncb in (mask, row block, column block) order; KIND: bytes or f32; VEC: 4 pixels per load (w >= 4); WVEC: w % 4 == 0
// (a template argument here, not the run-time flag of the other pixel kernels: with the column move-down and both store forms
// compiled in, the bytes / VEC kernel spills SGPRs into a 73rd VGPR and loses its 7th wave per SIMD on the aligned widths)
template <int KIND, bool VEC, bool WVEC>
__global__ __launch_bounds__(256) void k_rle_words(const void* __restrict__ x_in, float thr, int h, int w, int nb, int ncb, long tiles,
                                                   u64* __restrict__ tw, u32* __restrict__ cp) {
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const BpTile k = bp_tile(t, nb, ncb, lane);
    const int y0 = k.y0, x0 = k.x0;
    const void* base = bp_plane<KIND>(x_in, k.item, npix);
    // carries first (their latency hides under the rows): unconditional loads of a clamped index, masked afterwards
    u32 carry[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int xc = x0 + c;
      const bool has = xc < w && (y0 > 0 || xc > 0);           // (the first pixel of a mask has no predecessor)
      const long ci = !has ? 0 : (y0 > 0 ? (long)(y0 - 1) * w + xc : (long)(h - 1) * w + xc - 1);
      carry[c] = bp_on<KIND>(base, ci, thr, 0) & (has ? 1u : 0u);
    }
    u64 word[4];
    bp_words<KIND, VEC, VEC && !WVEC>(base, thr, 0, y0, x0, h, w, word);
    const int rows = h - y0 < 64 ? h - y0 : 64;
    const u64 vmask = rows == 64 ? ~0ull : (1ull << rows) - 1ull;   // (the words are masked already; the bit shifted in is not)
    u64 tr[4];
    u32 cnt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tr[c] = (word[c] ^ ((word[c] << 1) | carry[c])) & vmask;
      cnt[c] = (u32)__popcll(tr[c]) | ((u32)__popcll(word[c]) << 16);
    }
    const long s = (k.item * nb + k.rb) * (long)w + x0;
    bp_store4(tw + s, tr, x0, w, WVEC);
    bp_store4(cp + s, cnt, x0, w, WVEC);
  }
}

// One workgroup per mask.  Word q = x * nb + rb of the run order lives at storage index rb * w + x.  cp: count | area << 16 in,
// the number of the mask's transitions before the word out; pp: position of the last transition before the word (0 if none,
// which is also the position "before the first run").  runs[m] = transitions + 1.
__global__ __launch_bounds__(256) void k_rle_scan(const u64* __restrict__ tw, u32* __restrict__ cp, u32* __restrict__ pp, int n, int h,
                                                  int w, int nb, u32* __restrict__ runs, int* __restrict__ area) {
  __shared__ u32 sm[4];
  const long W = (long)w * nb;
  for (int m = blockIdx.x; m < n; m += gridDim.x) {
    const u64* twm = tw + (long)m * W;
    u32* cpm = cp + (long)m * W;
    u32* ppm = pp + (long)m * W;
    u32 run_sum = 0, run_max = 0, a = 0;
    for (long q0 = 0; q0 < W; q0 += 1024) {
      u32 c[4], last[4];
      long s[4];
      u32 tsum = 0, tmax = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long q = q0 + threadIdx.x * 4 + i;
        c[i] = 0, last[i] = 0, s[i] = -1;
        if (q < W) {
          const int x = (int)(q / nb), rb = (int)(q - (long)x * nb);
          s[i] = (long)rb * w + x;
          const u64 t = twm[s[i]];
          const u32 v = cpm[s[i]];
          c[i] = v & 0xffffu, a += v >> 16;
          if (t) last[i] = (u32)((long)x * h + rb * 64 + 63 - __clzll((long long)t));
        }
        tsum += c[i], tmax = last[i] > tmax ? last[i] : tmax;
      }
      u32 tot_sum, tot_max;
      u32 e_sum = run_sum + block_scan_excl(tsum, OpAdd(), 0u, sm, tot_sum);
      u32 e_max = block_scan_excl(tmax, OpMax(), 0u, sm, tot_max);
      e_max = e_max > run_max ? e_max : run_max;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (s[i] >= 0) cpm[s[i]] = e_sum, ppm[s[i]] = e_max;
        e_sum += c[i], e_max = last[i] > e_max ? last[i] : e_max;
      }
      run_sum += tot_sum, run_max = tot_max > run_max ? tot_max : run_max;
    }
    u32 tot_a;
    block_scan_excl(a, OpAdd(), 0u, sm, tot_a);
    if (threadIdx.x == 0) runs[m] = run_sum + 1u, area[m] = (int)tot_a;
    __syncthreads();
  }
}

// one workgroup: offsets[m] = sum of runs[< m], offsets[n] = the total
__global__ __launch_bounds__(256) void k_rle_offsets(const u32* __restrict__ runs, int n, long long* __restrict__ offsets) {
  __shared__ long long sm[4];
  long long run = 0;
  for (int m0 = 0; m0 < n; m0 += 256) {
    const int m = m0 + threadIdx.x;
    const long long v = m < n ? (long long)runs[m] : 0;
    long long tot;
    const long long e = run + block_scan_excl(v, OpAdd(), 0ll, sm, tot);
    if (m < n) offsets[m] = e;
    run += tot;
  }
  if (threadIdx.x == 0) offsets[n] = run;
}

// one thread per word (storage order); grid.y strides over the masks
__global__ __launch_bounds__(256) void k_rle_emit(const u64* __restrict__ tw, const u32* __restrict__ cp, const u32* __restrict__ pp, int n,
                                                  int h, int w, int nb, const long long* __restrict__ offsets, u32* __restrict__ counts) {
  const long W = (long)w * nb;
  const u32 hw = (u32)((long)h * w);
  for (int m = blockIdx.y; m < n; m += gridDim.y) {
    const long off = offsets[m];
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < W; s += (long)gridDim.x * 256) {
      const int rb = (int)(s / w), x = (int)(s - (long)rb * w);
      u64 t = tw[(long)m * W + s];
      u32 prev = pp[(long)m * W + s];
      long k = off + cp[(long)m * W + s];
      const u32 p0 = (u32)((long)x * h + rb * 64);
      while (t) {
        const u32 p = p0 + (u32)(__ffsll((long long)t) - 1);
        counts[k++] = p - prev;
        prev = p, t &= t - 1;
      }
      if (s == W - 1) counts[k] = hw - prev;                   // (x = w - 1, last row block): the last word of the run order
    }
  }
}

namespace {
// maskApi rleToString of one value: 5 bits at a time, low bits first, bit 5 = "more"; returns the number of characters
__device__ __forceinline__ int rle_chunks(long long x, unsigned char* out) {
  int nch = 0;
  bool more;
  do {
    int c = (int)(x & 0x1f);
    x >>= 5;                                                   // arithmetic: -1 stays -1
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (out) out[nch] = (unsigned char)(c + 48);
    ++nch;
  } while (more);
  return nch;
}
__device__ __forceinline__ int rle_mask_of(const long long* __restrict__ offsets, int n, long k) {   // offsets[m] <= k < offsets[m + 1]
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// the value that is written for count k of mask m: c[i] - c[i - 2] for i > 2
__device__ __forceinline__ long long rle_delta(const u32* __restrict__ counts, long k, long first) {
  const long long c = counts[k];
  return k - first > 2 ? c - (long long)counts[k - 2] : c;
}
}  // namespace

// PASS 0: bsum[block] = characters of the block's 2048 counts.  PASS 1: the characters, and str_offsets[m] at a mask's first count
template <int PASS>
__global__ __launch_bounds__(256) void k_str(const u32* __restrict__ counts, const long long* __restrict__ offsets, int n, long total,
                                             long long* __restrict__ bsum, long long* __restrict__ str_offsets,
                                             unsigned char* __restrict__ chars) {
  __shared__ long long sm[4];
  for (long b = blockIdx.x; b * STR_PER_BLOCK < total; b += gridDim.x) {
    const long k0 = b * STR_PER_BLOCK + (long)threadIdx.x * STR_PER_THREAD;
    int m = 0;
    long long len = 0;
    if (k0 < total) {
      m = rle_mask_of(offsets, n, k0);
      int mm = m;
      for (int i = 0; i < STR_PER_THREAD && k0 + i < total; ++i) {
        while (k0 + i >= offsets[mm + 1]) ++mm;
        len += rle_chunks(rle_delta(counts, k0 + i, offsets[mm]), nullptr);
      }
    }
    long long tot;
    long long e = block_scan_excl(len, OpAdd(), 0ll, sm, tot);
    if (PASS == 0) {
      if (threadIdx.x == 0) bsum[b] = tot;
    } else if (k0 < total) {
      e += bsum[b];
      for (int i = 0; i < STR_PER_THREAD && k0 + i < total; ++i) {
        while (k0 + i >= offsets[m + 1]) ++m;
        if (k0 + i == offsets[m]) str_offsets[m] = e;
        e += rle_chunks(rle_delta(counts, k0 + i, offsets[m]), chars + e);
      }
    }
  }
}

// one workgroup: bsum -> its exclusive scan in place, str_offsets[n] = the total
__global__ __launch_bounds__(256) void k_str_blocks(long long* __restrict__ bsum, long nblk, int n, long long* __restrict__ str_offsets) {
  __shared__ long long sm[4];
  long long run = 0;
  for (long b0 = 0; b0 < nblk; b0 += 256) {
    const long b = b0 + threadIdx.x;
    const long long v = b < nblk ? bsum[b] : 0;
    long long tot;
    const long long e = run + block_scan_excl(v, OpAdd(), 0ll, sm, tot);
    if (b < nblk) bsum[b] = e;
    run += tot;
  }
  if (threadIdx.x == 0) str_offsets[n] = run;
}

// --------------------------------------------------------------------------------------------------------------------
static size_t rle_bytes_per_mask(int h, int w) { return (size_t)w * cdiv(h, 64) * 16 + 16; }

size_t rle_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || !bp_shape_ok(n, h, w)) return 0;
  return (size_t)n * rle_bytes_per_mask(h, w);
}

namespace {
struct RleWs {
  u64* tw;
  u32 *cp, *pp, *runs;
};
RleWs rle_carve(void* ws, int n, int h, int w) {
  const size_t words = (size_t)n * w * cdiv(h, 64);
  RleWs r;
  r.tw = (u64*)ws;
  r.cp = (u32*)((char*)ws + words * 8);
  r.pp = r.cp + words;
  r.runs = r.pp + words;
  return r;
}
}  // namespace

int rle_count(const void* x, int is_f32, float thr, int n, int h, int w, long long* offsets, int* area, void* ws, size_t ws_bytes,
              hipStream_t s) {
  if (!bp_shape_ok(n, h, w)) return SAMPT_ERR_ARG;
  if (!offsets) return SAMPT_ERR_ARG;
  if (n > 0 && (!x || !area || !ws || ((uintptr_t)ws & 15) || (is_f32 && ((uintptr_t)x & 3)))) return SAMPT_ERR_ARG;
  if (n > 0 && ws_bytes < rle_workspace_bytes(n, h, w)) return SAMPT_ERR_WORKSPACE;
  if (n > 0) {
    const RleWs k = rle_carve(ws, n, h, w);
    const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
    const long tiles = (long)n * nb * ncb;
    typedef void (*words_fn)(const void*, float, int, int, int, int, long, u64*, u32*);
#define RLE_W(kind) {k_rle_words<kind, false, false>, k_rle_words<kind, true, false>, k_rle_words<kind, true, true>}
    static const words_fn table[2][3] = {RLE_W(BP_KIND_BYTES), RLE_W(BP_KIND_F32)};   // w < 4; w % 4 != 0; w % 4 == 0
#undef RLE_W
    hipLaunchKernelGGL(table[is_f32 ? 1 : 0][w < 4 ? 0 : w % 4 ? 1 : 2], dim3(bp_blocks(tiles, 4)), dim3(256), 0, s, x, thr, h, w, nb, ncb,
                       tiles, k.tw, k.cp);
    SAMPT_CHECK_LAUNCH("rle_count words");
    hipLaunchKernelGGL(k_rle_scan, dim3(n < 65535 ? n : 65535), dim3(256), 0, s, (const u64*)k.tw, k.cp, k.pp, n, h, w, nb, k.runs, area);
    SAMPT_CHECK_LAUNCH("rle_count scan");
  }
  hipLaunchKernelGGL(k_rle_offsets, dim3(1), dim3(256), 0, s, n > 0 ? (const u32*)rle_carve(ws, n, h, w).runs : nullptr, n, offsets);
  SAMPT_CHECK_LAUNCH("rle_count offsets");
  return SAMPT_OK;
}

int rle_emit(int n, int h, int w, const long long* offsets, unsigned* counts, const void* ws, size_t ws_bytes, hipStream_t s) {
  if (!bp_shape_ok(n, h, w)) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!offsets || !counts || !ws || ((uintptr_t)ws & 15)) return SAMPT_ERR_ARG;
  if (ws_bytes < rle_workspace_bytes(n, h, w)) return SAMPT_ERR_WORKSPACE;
  const RleWs k = rle_carve(const_cast<void*>(ws), n, h, w);
  const int nb = cdiv(h, 64);
  const long W = (long)w * nb;
  const int bx = (int)((W + 255) / 256 < 65535 ? (W + 255) / 256 : 65535);
  hipLaunchKernelGGL(k_rle_emit, dim3(bx, n < 65535 ? n : 65535), dim3(256), 0, s, (const u64*)k.tw, (const u32*)k.cp, (const u32*)k.pp, n,
                     h, w, nb, offsets, counts);
  SAMPT_CHECK_LAUNCH("rle_emit");
  return SAMPT_OK;
}

size_t rle_string_workspace_bytes(long total) {
  if (total <= 0) return 0;
  return (size_t)((total + STR_PER_BLOCK - 1) / STR_PER_BLOCK) * 8;
}

int rle_string_sizes(const unsigned* counts, const long long* offsets, int n, long total, long long* str_offsets, void* ws,
                     size_t ws_bytes, hipStream_t s) {
  if (n <= 0 || total < n || !counts || !offsets || !str_offsets || !ws || ((uintptr_t)ws & 7)) return SAMPT_ERR_ARG;
  if (ws_bytes < rle_string_workspace_bytes(total)) return SAMPT_ERR_WORKSPACE;
  const long nblk = (total + STR_PER_BLOCK - 1) / STR_PER_BLOCK;
  hipLaunchKernelGGL(k_str<0>, dim3(bp_blocks(nblk, 1)), dim3(256), 0, s, counts, offsets, n, total, (long long*)ws, str_offsets,
                     (unsigned char*)nullptr);
  SAMPT_CHECK_LAUNCH("rle_string_sizes lengths");
  hipLaunchKernelGGL(k_str_blocks, dim3(1), dim3(256), 0, s, (long long*)ws, nblk, n, str_offsets);
  SAMPT_CHECK_LAUNCH("rle_string_sizes scan");
  return SAMPT_OK;
}

int rle_string_emit(const unsigned* counts, const long long* offsets, int n, long total, long long* str_offsets, unsigned char* chars,
                    const void* ws, size_t ws_bytes, hipStream_t s) {
  if (n <= 0 || total < n || !counts || !offsets || !str_offsets || !chars || !ws || ((uintptr_t)ws & 7)) return SAMPT_ERR_ARG;
  if (ws_bytes < rle_string_workspace_bytes(total)) return SAMPT_ERR_WORKSPACE;
  const long nblk = (total + STR_PER_BLOCK - 1) / STR_PER_BLOCK;
  hipLaunchKernelGGL(k_str<1>, dim3(bp_blocks(nblk, 1)), dim3(256), 0, s, counts, offsets, n, total, (long long*)const_cast<void*>(ws),
                     str_offsets, chars);
  SAMPT_CHECK_LAUNCH("rle_string_emit");
  return SAMPT_OK;
}

}  // namespace sampt
