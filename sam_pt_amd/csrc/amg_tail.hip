// Tail of the automatic mask generator (sam_pt_amd/automatic_mask_generator.py) on the device: the small-region clean-up of a
// stack of boolean masks and greedy box NMS.  Both are integer / threshold logic and equal the host functions
// (remove_small_regions holes-then-islands, nms) exactly.
//
// Clean-up = two passes of 8-connected component labelling by union-find with label = SMALLEST linear pixel index of the
// component, so labels, sizes and the "largest, first in raster order" tie-break do not depend on scheduling:
//   k_rg_label    one workgroup per 64 x 16 tile: min-root links in LDS, tile-local roots written as global pixel indices;
//                 zeroes the per-pixel size counters (and, in the first pass, the per-mask record)
//   k_rg_merge    unions across tile seams.  Other workgroups change labels during this launch and XCD L2s are private: every
//                 label access here is an agent-scope atomic (relaxed load, atomicMin with its return value checked)
//   k_rg_flatten  label -> root, size[root] += 1 with one integer atomic per (wave, root)
//   k_rg_roots    (islands) per mask: is any component small, is any not, and max (size, then smallest root)
//   k_rg_apply    the per-pixel decision; the islands pass also reduces area and box (integer partials + k_rg_final)
// Workspace per mask in flight: 4 B label + 4 B size per pixel, + 1 KiB of partials.  Kernel nodes only, no memset.
//
// NMS: stable descending rank of the scores (O(n^2) compares, n <= a few thousand), an n x ceil(n / 64) bit matrix of
// IoU > thr built with one wave-64 ballot per word, and one workgroup that sweeps it 64 rows at a time: the 64 x 64 diagonal
// block is resolved serially from LDS, the kept rows are then OR-ed into the removed set in parallel.
//
// The IoU must round like torch's separately rounded f32 operations: no a * b + c -> fma contraction in this file.
#pragma clang fp contract(off)
#include "ops.h"

namespace sampt {

namespace {
typedef unsigned long long u64;

constexpr int RG_TW = 64, RG_TH = 16, RG_TPIX = RG_TW * RG_TH;   // tile of the LDS labelling (256 threads x 4 pixels)
constexpr int RG_MAX_BLOCKS = 32;                                 // workgroups per mask of the apply pass's reduction
constexpr int RG_PIX_BLOCKS = 1024;                               // cap of the per-pixel grids (x masks), grid-stride beyond
constexpr size_t RG_FIXED_BYTES = RG_MAX_BLOCKS * 8 * sizeof(int) + 16;

struct RgStat {
  u64 best;      // islands: max over roots of (size << 32 | ~root): the largest component, the first in raster order among equals
  int small_h;   // holes pass filled something
  int flags_i;   // islands: bit 0 = a component is small, bit 1 = a component is not
};

#define RG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- union-find in LDS (label[x] <= x always; atomicMin only lowers a label, so find terminates) ----
__device__ __forceinline__ int lds_ld(int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(int* L, int a) {
  int p;
  while ((p = lds_ld(L, a)) != a) a = p;
  return a;
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a), b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = atomicMin(&L[a], b);       // a was a root when found; if someone re-linked it meanwhile, go on from there
    if (old == a) return;
    a = old;
  }
}
// ---- the same on global labels during the seam-merge launch: agent-scope atomics only ----
__device__ __forceinline__ int g_ld(int* L, int i) { return __hip_atomic_load(L + i, RG_RLX_AGENT); }
__device__ __forceinline__ int g_find(int* L, int a) {
  int p;
  while ((p = g_ld(L, a)) != a) a = p;
  return a;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
  for (;;) {
    a = g_find(L, a), b = g_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

struct RgAcc {
  int area, xmin, ymin, xmax, ymax;
};
__device__ __forceinline__ RgAcc rg_wave_reduce(RgAcc a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.area += __shfl_xor(a.area, o, 64);
    a.xmin = min(a.xmin, __shfl_xor(a.xmin, o, 64));
    a.ymin = min(a.ymin, __shfl_xor(a.ymin, o, 64));
    a.xmax = max(a.xmax, __shfl_xor(a.xmax, o, 64));
    a.ymax = max(a.ymax, __shfl_xor(a.ymax, o, 64));
  }
  return a;
}
}  // namespace

// work pixel = background (HOLES) or foreground of m; lab = -1 elsewhere
template <int HOLES>
__global__ __launch_bounds__(256) void k_rg_label(const unsigned char* __restrict__ m, int h, int w, int ntx, long npix,
                                                  int* __restrict__ lab, int* __restrict__ size, RgStat* __restrict__ stat) {
  __shared__ int L[RG_TPIX];
  const int n = blockIdx.y, tile = blockIdx.x;
  const int x0 = (tile % ntx) * RG_TW, y0 = (tile / ntx) * RG_TH;
  m += (long)n * npix, lab += (long)n * npix, size += (long)n * npix;
  if (HOLES && tile == 0 && threadIdx.x == 0) stat[n] = RgStat{0ull, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = k * 256 + threadIdx.x, y = y0 + (i >> 6), x = x0 + (i & 63);
    const bool work = y < h && x < w && ((m[(long)y * w + x] != 0) != (HOLES != 0));
    L[i] = work ? i : -1;
  }
  __syncthreads();
  // links to the four neighbours that precede a pixel in raster order.  With N present, NW and NE are reached through it
  // (N links to its own W = NW, NE links to its own W = N).
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = k * 256 + threadIdx.x, ly = i >> 6, lx = i & 63;
    if (lds_ld(L, i) < 0) continue;
    if (lx > 0 && lds_ld(L, i - 1) >= 0) lds_union(L, i, i - 1);
    if (ly > 0) {
      if (lds_ld(L, i - RG_TW) >= 0) {
        lds_union(L, i, i - RG_TW);
      } else {
        if (lx > 0 && lds_ld(L, i - RG_TW - 1) >= 0) lds_union(L, i, i - RG_TW - 1);
        if (lx < RG_TW - 1 && lds_ld(L, i - RG_TW + 1) >= 0) lds_union(L, i, i - RG_TW + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = k * 256 + threadIdx.x, y = y0 + (i >> 6), x = x0 + (i & 63);
    if (y >= h || x >= w) continue;
    const long g = (long)y * w + x;
    int r = -1;
    if (L[i] >= 0) {
      r = lds_find(L, i);                                    // (raster order inside a tile = order of the global indices)
      r = (y0 + (r >> 6)) * w + x0 + (r & 63);
    }
    lab[g] = r, size[g] = 0;
  }
}

// one thread per pixel of the first column of a tile (x > 0) and of the first row of a tile (y > 0): its three neighbours
// across the seam.  Every pair of 8-adjacent pixels in different tiles is one of these.
__global__ __launch_bounds__(256) void k_rg_merge(int* lab, int h, int w, int ntx, int nty, long npix) {
  lab += (long)blockIdx.y * npix;
  const long nv = (long)(ntx - 1) * h, nh = (long)(nty - 1) * w;
  for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < nv + nh; s += (long)gridDim.x * 256) {
    const bool vert = s < nv;
    int x, y;
    if (vert) {
      x = (int)(s / h + 1) * RG_TW, y = (int)(s % h);
    } else {
      const long t = s - nv;
      y = (int)(t / w + 1) * RG_TH, x = (int)(t % w);
    }
    const int p = y * w + x;
    if (g_ld(lab, p) < 0) continue;
    for (int d = -1; d <= 1; ++d) {
      const int qx = vert ? x - 1 : x + d, qy = vert ? y + d : y - 1;
      if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
      const int q = qy * w + qx;
      if (g_ld(lab, q) >= 0) g_union(lab, p, q);
    }
  }
}

// labels are final here (previous launch): plain loads.  A label is compressed in place; a concurrent reader sees the old
// parent or the root, both ancestors.  size[root] += pixels: one atomic per distinct root of a wave (integer: any order).
__global__ __launch_bounds__(256) void k_rg_flatten(int* lab, int* size, long npix) {
  lab += (long)blockIdx.y * npix, size += (long)blockIdx.y * npix;
  const int lane = threadIdx.x & 63;
  for (long i0 = (long)blockIdx.x * 256; i0 < npix; i0 += (long)gridDim.x * 256) {
    const long i = i0 + threadIdx.x;
    int root = -1;
    if (i < npix) {
      const int p0 = lab[i];
      if (p0 >= 0) {
        int a = p0, p;
        while ((p = lab[a]) != a) a = p;
        root = a;
        if (root != p0) lab[i] = root;
      }
    }
    u64 todo = __ballot(root >= 0);
    while (todo) {                                             // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int r = __shfl(root, leader, 64);
      const u64 same = __ballot(root == r);
      if (lane == leader) atomicAdd(&size[r], (int)__popcll(same));
      todo &= ~same;
    }
  }
}

__global__ __launch_bounds__(256) void k_rg_roots(const int* __restrict__ lab, const int* __restrict__ size, long npix, int min_area,
                                                  RgStat* __restrict__ stat) {
  __shared__ u64 s_best[4];
  __shared__ int s_flags[4];
  const int n = blockIdx.y;
  lab += (long)n * npix, size += (long)n * npix;
  u64 best = 0;
  int flags = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    if (lab[i] != (int)i) continue;
    const int sz = size[i];
    flags |= sz < min_area ? 1 : 2;
    const u64 key = ((u64)(unsigned)sz << 32) | (u64)(0xffffffffu - (unsigned)i);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64), lo = __shfl_xor((unsigned)best, o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    best = other > best ? other : best;
    flags |= __shfl_xor(flags, o, 64);
  }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best, s_flags[threadIdx.x >> 6] = flags;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) best = s_best[k] > best ? s_best[k] : best, flags |= s_flags[k];
    if (flags) {                                               // (a workgroup without roots has nothing to add)
      atomicMax(&stat[n].best, best);
      atomicOr(&stat[n].flags_i, flags);
    }
  }
}

// HOLES: out = foreground | background component smaller than min_area.  Islands: out = component not smaller than min_area,
// or — when every component is small — the one of stat.best; partial [n][gridDim.x][8] = area and box of out.
template <int HOLES>
__global__ __launch_bounds__(256) void k_rg_apply(const int* __restrict__ lab, const int* __restrict__ size, int w, long npix,
                                                  int min_area, RgStat* __restrict__ stat, unsigned char* __restrict__ out,
                                                  int* __restrict__ partial) {
  __shared__ int red[4][5];
  const int n = blockIdx.y;
  lab += (long)n * npix, size += (long)n * npix, out += (long)n * npix;
  int keep_root = -1;
  if (!HOLES) {
    const RgStat st = stat[n];
    if (!(st.flags_i & 2) && (st.flags_i & 1)) keep_root = (int)(0xffffffffu - (unsigned)(st.best & 0xffffffffull));
  }
  RgAcc a{0, 0x7fffffff, 0x7fffffff, -1, -1};
  int filled = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const int r = lab[i];
    bool on;
    if (HOLES) {
      on = true;
      if (r >= 0) {
        on = size[r] < min_area;
        filled |= on ? 1 : 0;
      }
    } else {
      on = r >= 0 && (size[r] >= min_area || r == keep_root);
      if (on) {
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        a.area += 1;
        a.xmin = min(a.xmin, x), a.xmax = max(a.xmax, x), a.ymin = min(a.ymin, y), a.ymax = max(a.ymax, y);
      }
    }
    out[i] = on ? 1 : 0;
  }
  if (HOLES) {
    if (__syncthreads_or(filled) && threadIdx.x == 0) atomicOr(&stat[n].small_h, 1);
  } else {
    a = rg_wave_reduce(a);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
      red[wave][0] = a.area, red[wave][1] = a.xmin, red[wave][2] = a.ymin, red[wave][3] = a.xmax, red[wave][4] = a.ymax;
    __syncthreads();
    if (threadIdx.x == 0) {
      int* o = partial + ((long)n * gridDim.x + blockIdx.x) * 8;
      o[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
      o[1] = min(min(red[0][1], red[1][1]), min(red[2][1], red[3][1]));
      o[2] = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
      o[3] = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
      o[4] = max(max(red[0][4], red[1][4]), max(red[2][4], red[3][4]));
    }
  }
}

// one wave per mask: area, inclusive XYXY box (zeros when empty), changed = a small hole was filled | a small island existed
__global__ __launch_bounds__(64) void k_rg_final(const int* __restrict__ partial, int nb, const RgStat* __restrict__ stat,
                                                 unsigned char* __restrict__ changed, int* __restrict__ area, int* __restrict__ boxes) {
  const int n = blockIdx.x;
  RgAcc a{0, 0x7fffffff, 0x7fffffff, -1, -1};
  for (int i = threadIdx.x; i < nb; i += 64) {
    const int* o = partial + ((long)n * nb + i) * 8;
    a.area += o[0];
    a.xmin = min(a.xmin, o[1]), a.ymin = min(a.ymin, o[2]), a.xmax = max(a.xmax, o[3]), a.ymax = max(a.ymax, o[4]);
  }
  a = rg_wave_reduce(a);
  if (threadIdx.x == 0) {
    const bool empty = a.area == 0;
    area[n] = a.area;
    boxes[4 * n + 0] = empty ? 0 : a.xmin, boxes[4 * n + 1] = empty ? 0 : a.ymin;
    boxes[4 * n + 2] = empty ? 0 : a.xmax, boxes[4 * n + 3] = empty ? 0 : a.ymax;
    changed[n] = (stat[n].small_h | (stat[n].flags_i & 1)) ? 1 : 0;
  }
}

static size_t rg_bytes_per_mask(long npix) { return (((size_t)npix * 8 + 15) & ~(size_t)15) + RG_FIXED_BYTES; }

size_t amg_regions_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0 || (long)h * w >= (1L << 31)) return 0;
  return (size_t)n * rg_bytes_per_mask((long)h * w);
}

int amg_regions(const unsigned char* masks_in, int n, int h, int w, int min_area, unsigned char* masks_out, unsigned char* changed,
                int* area, int* boxes, void* ws, size_t ws_bytes, hipStream_t s) {
  if (n < 0 || h <= 0 || w <= 0 || (long)h * w >= (1L << 31)) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!masks_in || !masks_out || !changed || !area || !boxes || !ws || ((uintptr_t)ws & 15)) return SAMPT_ERR_ARG;
  const long npix = (long)h * w;
  const size_t per = rg_bytes_per_mask(npix);
  long cap = (long)(ws_bytes / per);
  if (cap < 1) return SAMPT_ERR_WORKSPACE;
  if (cap > 32768) cap = 32768;                                // (grid y)
  const int ntx = cdiv(w, RG_TW), nty = cdiv(h, RG_TH);
  const long seam = (long)(ntx - 1) * h + (long)(nty - 1) * w;
  const int pix_blocks = (int)(cdiv(npix, 256) < RG_PIX_BLOCKS ? cdiv(npix, 256) : RG_PIX_BLOCKS);
  const int seam_blocks = (int)(cdiv(seam, 256) < RG_PIX_BLOCKS ? cdiv(seam, 256) : RG_PIX_BLOCKS);
  int nb = cdiv(npix, 2048);
  nb = nb < 1 ? 1 : (nb > RG_MAX_BLOCKS ? RG_MAX_BLOCKS : nb);
  for (int c0 = 0; c0 < n; c0 += (int)cap) {                   // the stack in chunks of what the workspace holds
    const int c = n - c0 < cap ? n - c0 : (int)cap;
    int* lab = (int*)ws;
    int* size = lab + (size_t)c * npix;
    char* tail = (char*)ws + (((size_t)c * npix * 8 + 15) & ~(size_t)15);
    int* partial = (int*)tail;
    RgStat* stat = (RgStat*)(tail + (size_t)c * RG_MAX_BLOCKS * 8 * sizeof(int));
    const unsigned char* in = masks_in + (size_t)c0 * npix;
    unsigned char* out = masks_out + (size_t)c0 * npix;
    for (int pass = 0; pass < 2; ++pass) {
      const bool holes = pass == 0;
      if (holes)
        hipLaunchKernelGGL(k_rg_label<1>, dim3(ntx * nty, c), dim3(256), 0, s, in, h, w, ntx, npix, lab, size, stat);
      else
        hipLaunchKernelGGL(k_rg_label<0>, dim3(ntx * nty, c), dim3(256), 0, s, out, h, w, ntx, npix, lab, size, stat);
      SAMPT_CHECK_LAUNCH("amg_regions label");
      if (seam > 0) {
        hipLaunchKernelGGL(k_rg_merge, dim3(seam_blocks, c), dim3(256), 0, s, lab, h, w, ntx, nty, npix);
        SAMPT_CHECK_LAUNCH("amg_regions merge");
      }
      hipLaunchKernelGGL(k_rg_flatten, dim3(pix_blocks, c), dim3(256), 0, s, lab, size, npix);
      SAMPT_CHECK_LAUNCH("amg_regions flatten");
      if (holes) {
        hipLaunchKernelGGL(k_rg_apply<1>, dim3(pix_blocks, c), dim3(256), 0, s, lab, size, w, npix, min_area, stat, out, partial);
      } else {
        hipLaunchKernelGGL(k_rg_roots, dim3(pix_blocks, c), dim3(256), 0, s, lab, size, npix, min_area, stat);
        SAMPT_CHECK_LAUNCH("amg_regions roots");
        hipLaunchKernelGGL(k_rg_apply<0>, dim3(nb, c), dim3(256), 0, s, lab, size, w, npix, min_area, stat, out, partial);
      }
      SAMPT_CHECK_LAUNCH("amg_regions apply");
    }
    hipLaunchKernelGGL(k_rg_final, dim3(c), dim3(64), 0, s, partial, nb, stat, changed + c0, area + c0, boxes + 4 * (size_t)c0);
    SAMPT_CHECK_LAUNCH("amg_regions final");
  }
  return SAMPT_OK;
}

// --------------------------------------------------------------------------------------------------------------------
// greedy box NMS
// --------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int NMS_MAX_N = 65535;

// a sorts before b in a stable descending sort (nan first, as torch orders it)
__device__ __forceinline__ bool nms_before(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}
}  // namespace

// order[rank(i)] = i, sorted[rank(i)] = boxes[i]
__global__ __launch_bounds__(256) void k_nms_rank(const float4* __restrict__ boxes, const float* __restrict__ scores, int n,
                                                  int* __restrict__ order, float4* __restrict__ sorted) {
  __shared__ float sc[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float si = i < n ? scores[i] : 0.f;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    if (j0 + threadIdx.x < n) sc[threadIdx.x] = scores[j0 + threadIdx.x];
    __syncthreads();
    const int cnt = n - j0 < 256 ? n - j0 : 256;
    for (int j = 0; j < cnt; ++j) rank += nms_before(sc[j], j0 + j, si, i) ? 1 : 0;
  }
  if (i < n) order[rank] = i, sorted[rank] = boxes[i];
}

// bits[i][cb] bit l = (j = 64 cb + l > i) && IoU(sorted i, sorted j) > thr; words left of the diagonal are never read
__global__ __launch_bounds__(256) void k_nms_bits(const float4* __restrict__ sorted, int n, int nw, float thr, u64* __restrict__ bits) {
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, cb = blockIdx.x;
  if (i >= n || cb < (i >> 6)) return;                         // wave-uniform
  const int j = cb * 64 + lane;
  bool over = false;
  if (j < n && j > i) {
    const float4 a = sorted[i], b = sorted[j];
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x), ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    iw = iw < 0.f ? 0.f : iw, ih = ih < 0.f ? 0.f : ih;
    const float inter = iw * ih;
    over = inter / ((area_a + area_b) - inter) > thr;          // 0 / 0 = nan: never suppresses
  }
  const u64 word = __ballot(over);
  if (lane == 0) bits[(size_t)i * nw + cb] = word;
}

__global__ __launch_bounds__(256) void k_nms_sweep(const u64* __restrict__ bits, const int* __restrict__ order, int n, int nw,
                                                   long long* __restrict__ keep, int* __restrict__ count_out) {
  __shared__ u64 removed[(NMS_MAX_N + 64) / 64];
  __shared__ u64 diag[64];
  __shared__ u64 s_kept;
  const int tid = threadIdx.x;
  for (int k = tid; k < nw; k += 256) removed[k] = 0;
  u64 next_diag = tid < 64 && tid < n ? bits[(size_t)tid * nw] : 0;
  int count = 0;
  __syncthreads();
  for (int c = 0; c < nw; ++c) {
    const int r0 = c * 64, rows = n - r0 < 64 ? n - r0 : 64;
    if (tid < 64) {
      diag[tid] = next_diag;
      const int rn = r0 + 64 + tid;                            // the next diagonal block, off the serial chain
      next_diag = rn < n ? bits[(size_t)rn * nw + c + 1] : 0;
    }
    __syncthreads();
    if (tid == 0) {
      u64 rem = removed[c], kept = 0;
      for (int r = 0; r < rows; ++r) {
        const u64 d = diag[r];
        const bool k = !((rem >> r) & 1ull);
        kept |= k ? 1ull << r : 0ull;
        rem |= k ? d : 0ull;
      }
      s_kept = kept;
    }
    __syncthreads();
    const u64 kept = s_kept;
    for (int k = c + 1 + tid; k < nw; k += 256) {
      u64 acc = removed[k];
      for (u64 t = kept; t; t &= t - 1) acc |= bits[(size_t)(r0 + __ffsll((long long)t) - 1) * nw + k];
      removed[k] = acc;
    }
    if (tid < 64 && ((kept >> tid) & 1ull)) keep[count + (int)__popcll(kept & ((1ull << tid) - 1ull))] = order[r0 + tid];
    count += (int)__popcll(kept);
    __syncthreads();
  }
  if (tid == 0) *count_out = count;
}

static __global__ void k_nms_zero(int* count_out) { *count_out = 0; }

size_t amg_nms_workspace_bytes(int n) {
  if (n <= 0 || n > NMS_MAX_N) return 0;
  const size_t nw = (size_t)(n + 63) / 64;
  return (((size_t)n * 4 + 15) & ~(size_t)15) + (size_t)n * 16 + (size_t)n * nw * 8;
}

int amg_nms(const float* boxes, const float* scores, int n, float thr, long long* keep, int* count, void* ws, size_t ws_bytes,
            hipStream_t s) {
  if (n < 0 || n > NMS_MAX_N || !count) return SAMPT_ERR_ARG;
  if (n == 0) {
    hipLaunchKernelGGL(k_nms_zero, dim3(1), dim3(1), 0, s, count);
    SAMPT_CHECK_LAUNCH("amg_nms zero");
    return SAMPT_OK;
  }
  if (!boxes || !scores || !keep || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)boxes & 15)) return SAMPT_ERR_ARG;
  if (ws_bytes < amg_nms_workspace_bytes(n)) return SAMPT_ERR_WORKSPACE;
  const int nw = (n + 63) / 64;
  int* order = (int*)ws;
  float4* sorted = (float4*)((char*)ws + (((size_t)n * 4 + 15) & ~(size_t)15));
  u64* bits = (u64*)(sorted + n);
  hipLaunchKernelGGL(k_nms_rank, dim3(cdiv(n, 256)), dim3(256), 0, s, (const float4*)boxes, scores, n, order, sorted);
  SAMPT_CHECK_LAUNCH("amg_nms rank");
  hipLaunchKernelGGL(k_nms_bits, dim3(nw, cdiv(n, 4)), dim3(256), 0, s, (const float4*)sorted, n, nw, thr, bits);
  SAMPT_CHECK_LAUNCH("amg_nms bits");
  hipLaunchKernelGGL(k_nms_sweep, dim3(1), dim3(256), 0, s, (const u64*)bits, (const int*)order, n, nw, keep, count);
  SAMPT_CHECK_LAUNCH("amg_nms sweep");
  return SAMPT_OK;
}

}  // namespace sampt
