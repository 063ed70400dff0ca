// Interactive point correction on the device: exact DBSCAN labels of a pixel set, the choice of its largest cluster, and the frame
// state the click rule reads (reference: sam_pt/modeling/sam_pt_interactive.py:330-395 and :678-729, extract_largest_cluster_points).
//
// The reference clusters up to 18 000 error pixels per click with sklearn.cluster.DBSCAN(eps, min_samples = 10) on the host.  Its
// sequential expansion has an order-free restatement (sam_pt_amd/interactive.py:dbscan_labels, pinned on scikit-learn's labels):
//   * a point is core iff its neighbour count, itself included, is >= min_samples;
//   * clusters are the connected components of the core points under the neighbour relation;
//   * a cluster's id is the rank of its smallest core index among all clusters' smallest core indices;
//   * a non-core point with a core neighbour takes the SMALLEST cluster id among its core neighbours; everything else is -1.
// Pixel coordinates are integers, so squared distances are exact in int32 and "neighbour" is d^2 <= r2 with r2 = floor(eps^2)
// computed once on the host in float64 (equal to scikit-learn's dist <= eps unless eps^2 is within rounding of an integer: the
// wrapper refuses such an eps).  The labels are therefore unique: no order of the atomics below can change them.
//
// Kernels (n = 18 000: 3.2e8 integer distance tests per pass, three passes):
//   k_db_prepare   float (row, col) -> int2, parent[i] = i, counters cleared
//   k_db_pairs<0>  neighbour counts: 256 points per workgroup against tiles of 256 points staged in LDS (every lane reads the same
//                  LDS word: a broadcast); the j tiles are split over blockIdx.y and the partial counts meet in an integer atomicAdd
//   k_db_pairs<1>  union of every core pair (i > j) in a lock-free union-find whose hooks always point to the SMALLER index
//                  (atomicCAS on a root), so a component's root is its smallest core index whatever the schedule was.  There is no
//                  convergence loop: one pass over the pairs is complete.  Pointer chases and CAS retries are capped at n + 8 steps
//                  (a forest over n nodes cannot need more); a cap that is hit sets the status word instead of spinning
//   k_db_flatten   parent[i] = root(i)
//   k_db_rank      one workgroup: exclusive prefix sum over the root flags = cluster id of each root
//   k_db_pairs<2>  border pass: non-core points take the minimum cluster id over their core neighbours (atomicMin)
//   k_db_labels    labels out
//   k_db_largest   one workgroup: Counter(labels).most_common(1) without -1 (largest size, ties to the cluster that appears first),
//                  its members in ascending order, info
//   k_int_points / k_int_pixels   the frame state of the click rule
#include "ops.h"

namespace sampt {

namespace {
constexpr int DB_T = 256;              // threads per workgroup of the pair passes = points per i block = points per j tile
constexpr int DB_ONE = 1024;           // threads of the single-workgroup kernels
constexpr int DB_MAXN = 1 << 20;
constexpr int DB_MAXCOORD = 32767;     // 2 * 32767^2 < 2^31: squared distances stay exact in int32
constexpr int DB_BIG = 0x7fffffff;

// workspace layout (int32 words): [0] status (bit 0: a hop cap was hit, bit 1: a coordinate is no integer pixel), [1] number of
// clusters, [2..3] pad, then pts int2 [n], cnt [n], parent [n], rank [n],
// bmin [n]
struct DbWs {
  int* status;
  int2* pts;
  int *cnt, *parent, *rank, *bmin;
};
__host__ __device__ inline size_t db_words(int n) { return 4 + (size_t)n * 6; }
inline DbWs db_carve(void* ws, int n) {
  int* w = (int*)ws;
  DbWs d;
  d.status = w;
  d.pts = (int2*)(w + 4);
  d.cnt = w + 4 + (size_t)n * 2;
  d.parent = d.cnt + n;
  d.rank = d.parent + n;
  d.bmin = d.rank + n;
  return d;
}

__device__ __forceinline__ int db_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; at most `cap` hops (a forest over n nodes has no longer path), else the status word is set and the walk ends
__device__ int db_find(const int* parent, int x, int cap, int* status) {
  int p = db_load(parent + x);
  for (int hops = 0; p != x; ++hops) {
    if (hops > cap) {
      atomicOr(status, 1);
      break;
    }
    x = p;
    p = db_load(parent + x);
  }
  return x;
}

// joins the sets of a and b; the larger root is hooked under the smaller.  Returns the root both now share
__device__ int db_union(int* parent, int a, int b, int cap, int* status) {
  a = db_find(parent, a, cap, status);
  b = db_find(parent, b, cap, status);
  for (int tries = 0; a != b; ++tries) {
    if (tries > cap) {
      atomicOr(status, 1);
      break;
    }
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = db_find(parent, old, cap, status);   // hi was hooked by someone else meanwhile: continue from where it points
    b = db_find(parent, lo, cap, status);
  }
  return a;
}
}  // namespace

__global__ __launch_bounds__(DB_T) void k_db_prepare(const float* __restrict__ xy, int n, int2* __restrict__ pts, int* __restrict__ cnt,
                                                     int* __restrict__ parent, int* __restrict__ bmin, int* __restrict__ status) {
  const int i = blockIdx.x * DB_T + threadIdx.x;
  if (i >= n) return;
  const float r = xy[2 * (size_t)i], c = xy[2 * (size_t)i + 1];
  const bool ok = r >= 0.f && r <= (float)DB_MAXCOORD && c >= 0.f && c <= (float)DB_MAXCOORD && r == truncf(r) && c == truncf(c);
  if (!ok) atomicOr(status, 2);            // not an integer pixel coordinate in 0 .. 32767
  pts[i] = ok ? make_int2((int)r, (int)c) : make_int2(0, 0);
  cnt[i] = 0;
  parent[i] = i;
  bmin[i] = DB_BIG;
}

// MODE 0: cnt[i] += neighbours of i in this workgroup's j tiles.  MODE 1: union of the core pairs (i > j).  MODE 2: bmin[i] = min
// cluster id over the core neighbours of a non-core i.
template <int MODE>
__global__ __launch_bounds__(DB_T) void k_db_pairs(const int2* __restrict__ pts, int n, int r2, int min_samples, int* __restrict__ cnt,
                                                   int* __restrict__ parent, const int* __restrict__ rank, int* __restrict__ bmin,
                                                   int* __restrict__ status) {
  __shared__ int2 tp[DB_T];
  __shared__ int tv[DB_T];               // MODE 1: core flag of j; MODE 2: cluster id of a core j, -1 otherwise
  const int tid = threadIdx.x, i = blockIdx.x * DB_T + tid;
  const bool live = i < n;
  const int2 me = live ? pts[i] : make_int2(0, 0);
  bool active = live;
  if (MODE == 1) active = live && cnt[i] >= min_samples;
  if (MODE == 2) active = live && cnt[i] < min_samples;
  const int cap = n + 8;
  int acc = MODE == 2 ? DB_BIG : 0;
  int ri = i;                            // MODE 1: a root i has been seen under (possibly stale; still in i's set)
  const int ntiles = (n + DB_T - 1) / DB_T;
  // MODE 1 only joins j < i: tiles beyond this workgroup's own hold no such j
  const int tile_end = MODE == 1 ? min(ntiles, (int)blockIdx.x + 1) : ntiles;
  for (int t = blockIdx.y; t < tile_end; t += gridDim.y) {
    const int j0 = t * DB_T, jn = min(DB_T, n - j0);
    __syncthreads();
    if (tid < jn) {
      tp[tid] = pts[j0 + tid];
      if (MODE == 1) tv[tid] = cnt[j0 + tid] >= min_samples;
      if (MODE == 2) tv[tid] = cnt[j0 + tid] >= min_samples ? rank[parent[j0 + tid]] : -1;
    }
    __syncthreads();
    if (!active) continue;
    for (int jj = 0; jj < jn; ++jj) {
      const int2 q = tp[jj];
      const int dr = me.x - q.x, dc = me.y - q.y;
      const bool near = dr * dr + dc * dc <= r2;
      if (MODE == 0) acc += near;
      if (MODE == 1) {
        const int j = j0 + jj;
        if (near && tv[jj] && j < i && db_load(parent + j) != ri) {
          ri = db_union(parent, i, j, cap, status);
          atomicMin(parent + j, ri);       // path compression: ri is an ancestor of both, and so is anything smaller found there
          atomicMin(parent + i, ri);
        }
      }
      if (MODE == 2) {
        if (near && tv[jj] >= 0) acc = min(acc, tv[jj]);
      }
    }
  }
  if (MODE == 0 && live) atomicAdd(cnt + i, acc);
  if (MODE == 2 && active && acc != DB_BIG) atomicMin(bmin + i, acc);
}

__global__ __launch_bounds__(DB_T) void k_db_flatten(int n, int* __restrict__ parent, int* __restrict__ status) {
  const int i = blockIdx.x * DB_T + threadIdx.x;
  if (i >= n) return;
  const int r = db_find(parent, i, n + 8, status);   // roots do not move any more: every walk ends at the component's smallest core index
  if (r != i) parent[i] = r;
}

// rank[i] = number of cluster roots below i (meaningful at the roots); status[1] = number of clusters
__global__ __launch_bounds__(DB_ONE) void k_db_rank(int n, int min_samples, const int* __restrict__ cnt, const int* __restrict__ parent,
                                                    int* __restrict__ rank, int* __restrict__ status) {
  __shared__ int wave_tot[DB_ONE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n + DB_ONE - 1) / DB_ONE;
  const int j0 = min(n, tid * per), j1 = min(n, j0 + per);
  int c = 0;
  for (int j = j0; j < j1; ++j) c += cnt[j] >= min_samples && parent[j] == j;
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  int pos = base + inc - c;
  for (int j = j0; j < j1; ++j) {
    rank[j] = pos;
    pos += cnt[j] >= min_samples && parent[j] == j;
  }
  if (tid == DB_ONE - 1) status[1] = base + inc;
}

__global__ __launch_bounds__(DB_T) void k_db_labels(int n, int min_samples, const int* __restrict__ cnt, const int* __restrict__ parent,
                                                    const int* __restrict__ rank, const int* __restrict__ bmin, int* __restrict__ labels) {
  const int i = blockIdx.x * DB_T + threadIdx.x;
  if (i >= n) return;
  labels[i] = cnt[i] >= min_samples ? rank[parent[i]] : (bmin[i] == DB_BIG ? -1 : bmin[i]);
}

// one workgroup.  hist / first: n int32 each (workspace)
__global__ __launch_bounds__(DB_ONE) void k_db_largest(const int* __restrict__ labels, int n, int min_points, int* __restrict__ members,
                                                       int* __restrict__ info, int* __restrict__ hist, int* __restrict__ first) {
  __shared__ int s_ncl, s_best;
  __shared__ int red_s[DB_ONE / 64], red_f[DB_ONE / 64], red_c[DB_ONE / 64], wave_tot[DB_ONE / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_ncl = 0;
  for (int c = tid; c < n; c += DB_ONE) hist[c] = 0, first[c] = DB_BIG;
  __syncthreads();
  int mx = -1;
  for (int i = tid; i < n; i += DB_ONE) {
    const int c = labels[i];
    if (c >= 0 && c < n) {
      atomicAdd(hist + c, 1);
      atomicMin(first + c, i);
      mx = max(mx, c);
    }
  }
  atomicMax(&s_ncl, mx + 1);
  __syncthreads();
  const int ncl = s_ncl;
  // largest size; among equals the cluster whose first member comes first
  int bs = -1, bf = DB_BIG, bc = -1;
  for (int c = tid; c < ncl; c += DB_ONE) {
    const int s = hist[c], f = first[c];
    if (s > bs || (s == bs && f < bf)) bs = s, bf = f, bc = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int os = __shfl_xor(bs, o, 64), of = __shfl_xor(bf, o, 64), oc = __shfl_xor(bc, o, 64);
    if (os > bs || (os == bs && of < bf)) bs = os, bf = of, bc = oc;
  }
  if (lane == 0) red_s[wave] = bs, red_f[wave] = bf, red_c[wave] = bc;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DB_ONE / 64; ++w)
      if (red_s[w] > bs || (red_s[w] == bs && red_f[w] < bf)) bs = red_s[w], bf = red_f[w], bc = red_c[w];
    const bool use = bc >= 0 && bs >= min_points;
    info[0] = use ? bc : -1;
    info[1] = bc >= 0 ? bs : 0;
    info[2] = ncl;
    info[3] = bc;                          // the largest cluster itself, also when it is below min_points (-1: no cluster)
    s_best = use ? bc : -1;
  }
  __syncthreads();
  const int best = s_best;
  if (best < 0) return;
  // ordered compaction of the members
  const int per = (n + DB_ONE - 1) / DB_ONE;
  const int j0 = min(n, tid * per), j1 = min(n, j0 + per);
  int c = 0;
  for (int j = j0; j < j1; ++j) c += labels[j] == best;
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int pos = inc - c;
  for (int w = 0; w < wave; ++w) pos += wave_tot[w];
  for (int j = j0; j < j1; ++j)
    if (labels[j] == best) members[pos++] = j;
}

// ---- frame state of the click rule (sam_pt_interactive.py:330-361)
// category bits per point: 1 visible, 2 positive, 4 correct, 8 tp, 16 tn, 32 fp, 64 fn (an invisible point is 0)
// info: [0] |TP| [1] |FN| [2] |FP| [3] first incorrect visible negative point or -1 [4] first incorrect visible positive point or -1
//       [5] 1 = a visible point's rounded coordinate is off the frame
__global__ __launch_bounds__(DB_T) void k_int_points(const float* __restrict__ logits, const unsigned char* __restrict__ gt, int h, int w,
                                                     const float* __restrict__ xy, const float* __restrict__ vis,
                                                     const int* __restrict__ label, int np, int* __restrict__ info,
                                                     unsigned char* __restrict__ cat) {
  __shared__ int s_neg, s_pos, s_off;
  if (threadIdx.x == 0) s_neg = DB_BIG, s_pos = DB_BIG, s_off = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < np; p += DB_T) {
    int bits = 0;
    if (vis[p] == 1.0f) {
      const bool positive = label[p] == 1;
      // torch.round: half to even (rintf in the default rounding mode), then .int()
      const float fx = rintf(xy[2 * p]), fy = rintf(xy[2 * p + 1]);
      const bool inx = fx >= -(float)w && fx < (float)w, iny = fy >= -(float)h && fy < (float)h;   // (a NaN fails both)
      if (!(inx && iny)) {
        atomicOr(&s_off, 1);
        bits = 1 | (positive ? 2 : 0);
      } else {
        int x = (int)fx, y = (int)fy;
        if (x < 0) x += w;                 // Python's indexing of -1 .. -size
        if (y < 0) y += h;
        const bool m = logits[(size_t)y * w + x] > 0.f, g = gt[(size_t)y * w + x] != 0;
        const bool tp = m && g, tn = !m && !g, fp = m && !g, fn = !m && g;
        const bool correct = positive ? (tp || fn) : (tn || fp);
        bits = 1 | (positive ? 2 : 0) | (correct ? 4 : 0) | (tp ? 8 : 0) | (tn ? 16 : 0) | (fp ? 32 : 0) | (fn ? 64 : 0);
        if (!correct) atomicMin(positive ? &s_pos : &s_neg, p);
      }
    }
    cat[p] = (unsigned char)bits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    info[0] = info[1] = info[2] = 0;       // k_int_pixels (next on the stream) adds into these
    info[3] = s_neg == DB_BIG ? -1 : s_neg;
    info[4] = s_pos == DB_BIG ? -1 : s_pos;
    info[5] = s_off;
    info[6] = info[7] = 0;
  }
}

__global__ __launch_bounds__(DB_T) void k_int_pixels(const float* __restrict__ logits, const unsigned char* __restrict__ gt, long hw,
                                                     int* __restrict__ info, unsigned char* __restrict__ fn_out,
                                                     unsigned char* __restrict__ fp_out) {
  __shared__ int s_c[3];
  if (threadIdx.x < 3) s_c[threadIdx.x] = 0;
  __syncthreads();
  int tp = 0, fn = 0, fp = 0;
  for (long i = (long)blockIdx.x * DB_T + threadIdx.x; i < hw; i += (long)gridDim.x * DB_T) {
    const bool m = logits[i] > 0.f, g = gt[i] != 0;
    tp += m && g;
    fn += !m && g;
    fp += m && !g;
    fn_out[i] = !m && g;
    fp_out[i] = m && !g;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tp += __shfl_xor(tp, o, 64);
    fn += __shfl_xor(fn, o, 64);
    fp += __shfl_xor(fp, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_c[0], tp);
    atomicAdd(&s_c[1], fn);
    atomicAdd(&s_c[2], fp);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_c[threadIdx.x]) atomicAdd(info + threadIdx.x, s_c[threadIdx.x]);
}

size_t dbscan_workspace_bytes(int n) { return n <= 0 || n > DB_MAXN ? 0 : db_words(n) * sizeof(int); }

int dbscan_labels(const float* xy, int n, int r2, int min_samples, int* labels, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!xy || !labels || !ws || ((uintptr_t)ws & 15) || n <= 0 || n > DB_MAXN || r2 < 0 || min_samples < 1) return SAMPT_ERR_ARG;
  if (ws_bytes < dbscan_workspace_bytes(n)) return SAMPT_ERR_WORKSPACE;
  const DbWs d = db_carve(ws, n);
  const int nb = cdiv(n, DB_T);
  // the j tiles of the full passes are split over blockIdx.y until the grid has about 1024 workgroups (256 CUs, a few each)
  const int split = max(1, min(nb, 1024 / nb));
  if (hipMemsetAsync(d.status, 0, 4 * sizeof(int), s) != hipSuccess) {
    set_error("dbscan_labels", hipGetLastError());
    return SAMPT_ERR_HIP;
  }
  hipLaunchKernelGGL(k_db_prepare, dim3(nb), dim3(DB_T), 0, s, xy, n, d.pts, d.cnt, d.parent, d.bmin, d.status);
  hipLaunchKernelGGL(k_db_pairs<0>, dim3(nb, split), dim3(DB_T), 0, s, d.pts, n, r2, min_samples, d.cnt, d.parent, d.rank, d.bmin, d.status);
  hipLaunchKernelGGL(k_db_pairs<1>, dim3(nb, split), dim3(DB_T), 0, s, d.pts, n, r2, min_samples, d.cnt, d.parent, d.rank, d.bmin, d.status);
  hipLaunchKernelGGL(k_db_flatten, dim3(nb), dim3(DB_T), 0, s, n, d.parent, d.status);
  hipLaunchKernelGGL(k_db_rank, dim3(1), dim3(DB_ONE), 0, s, n, min_samples, d.cnt, d.parent, d.rank, d.status);
  hipLaunchKernelGGL(k_db_pairs<2>, dim3(nb, split), dim3(DB_T), 0, s, d.pts, n, r2, min_samples, d.cnt, d.parent, d.rank, d.bmin, d.status);
  hipLaunchKernelGGL(k_db_labels, dim3(nb), dim3(DB_T), 0, s, n, min_samples, d.cnt, d.parent, d.rank, d.bmin, labels);
  SAMPT_CHECK_LAUNCH("dbscan_labels");
  return SAMPT_OK;
}

int dbscan_largest(const int* labels, int n, int min_points, int* members, int* info, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!labels || !members || !info || !ws || ((uintptr_t)ws & 15) || n <= 0 || n > DB_MAXN) return SAMPT_ERR_ARG;
  if (ws_bytes < dbscan_workspace_bytes(n)) return SAMPT_ERR_WORKSPACE;
  int* w = (int*)ws + 4;                   // (the status words of dbscan_labels stay readable after this call)
  hipLaunchKernelGGL(k_db_largest, dim3(1), dim3(DB_ONE), 0, s, labels, n, min_points, members, info, w, w + n);
  SAMPT_CHECK_LAUNCH("dbscan_largest");
  return SAMPT_OK;
}

int int_frame_state(const float* logits, const unsigned char* gt, int h, int w, const float* xy, const float* vis, const int* label,
                    int n_points, int* info, unsigned char* cat, unsigned char* fn_out, unsigned char* fp_out, hipStream_t s) {
  if (!logits || !gt || !info || !fn_out || !fp_out || h <= 0 || w <= 0 || n_points < 0) return SAMPT_ERR_ARG;
  if (n_points > 0 && (!xy || !vis || !label || !cat)) return SAMPT_ERR_ARG;
  const long hw = (long)h * w;
  hipLaunchKernelGGL(k_int_points, dim3(1), dim3(DB_T), 0, s, logits, gt, h, w, xy, vis, label, n_points, info, cat);
  hipLaunchKernelGGL(k_int_pixels, dim3(min(1024, cdiv(hw, DB_T))), dim3(DB_T), 0, s, logits, gt, hw, info, fn_out, fp_out);
  SAMPT_CHECK_LAUNCH("int_frame_state");
  return SAMPT_OK;
}

}  // namespace sampt
