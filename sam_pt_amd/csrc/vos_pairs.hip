// DAVIS J and F of every (proposal, object) pair of every frame: the unsupervised protocol scores P proposals against K objects, and
// the expensive part of F, the disk dilation of a boundary map, depends on one mask only.  Fed to jf_counts (vos_metrics.hip) as
// P * K items per frame, every mask is read K (or P) times and dilated as often; here every mask is read and dilated once.
// Mask (p, t) of the seg side is item t * P + p of its source, mask (k, t) of the ann side item t * K + k; the frame's void plane
// (optional bytes) is cleared from both.  Sources, boundary map, disk and radius range are those of vos_metrics.hip (bitplane.h,
// jf_bits.h).
//
//   k_jfp_words   one wave per (mask, tile of 64 rows x 256 columns), the tile reader of bitplane.h: every pixel is read once into 64-bit
//                 column words; writes the mask bit-plane and the boundary bit-plane (workspace [mask][band][x]) and adds the mask's
//                 area and boundary count to its stat pair.  Run once for the seg side and once for the ann side.
//   k_jfp_dilate  one workgroup per (mask, band, 256 columns), one thread per column: the disk dilation of the boundary words (jf_halo /
//                 jf_dilate of jf_bits.h).  The dilated map is written as a third bit-plane, because every partner of the mask reuses
//                 it.  A tile with nothing in reach writes zeros and leaves early.
//   k_jfp_pairs   a popcount GEMM over the bit words: a workgroup takes a tile of 4 x 4 pairs of one frame and a slice of the
//                 planes' words; a thread loads word j of the 3 planes of 4 proposals and of 4 objects (24 words) and adds the
//                 48 popcounts inter = m_p & m_k, seg_match = b_p & dil(b_k), ann_match = b_k & dil(b_p).  A word is fetched once
//                 per tile of pairs.  Wave sums, then LDS, then one integer atomic per (pair, count) and slice.
// All sums are integer atomics on int32 (h * w < 2^31): bitwise repeatable whatever the order.
#include "ops.h"
#include "jf_bits.h"

namespace sampt {

namespace {
constexpr int JP_TP = 4, JP_TK = 4;          // the pair tile of k_jfp_pairs
constexpr int JP_SLICE = 2048;               // words of a plane per workgroup of k_jfp_pairs (8 per thread)
}  // namespace

// tiles = n * nb * ncb in (item, band, column block) order, item = frame * per_frame + mask of the frame; the item's planes are
// number plane0 + item of mb / bb ([.][nb][w]); stat int32 [n][2] (zeroed) = area, boundary count
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void k_jfp_words(BpSrc src, BpSrc vd, int per_frame, int h, int w, int nb, int ncb, long tiles, int wvec,
                                                   long plane0, u64* __restrict__ mb, u64* __restrict__ bb, int* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const BpTile k = bp_tile(t, nb, ncb, lane);
    JfBits M;
    jf_bits<KIND, VEC>(src, k.item, npix, k, h, w, lane, M);
    if (vd.base) {
      JfBits V;
      jf_bits<BP_KIND_BYTES, VEC>(vd, k.item / per_frame, npix, k, h, w, lane, V);
      jf_clear(M, V);
    }
    u64 b[4];
    jf_boundary(M, k.y0, k.x0, h, w, lane, b);
    int area = 0, nbd = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) area += __popcll(M.word[c]), nbd += __popcll(b[c]);
    const long o = ((plane0 + k.item) * nb + k.rb) * (long)w + k.x0;
    bp_store4(mb + o, M.word, k.x0, w, wvec);
    bp_store4(bb + o, b, k.x0, w, wvec);
    area = bp_wave_sum(area), nbd = bp_wave_sum(nbd);
    if (lane == 0) {
      if (area) atomicAdd(stat + k.item * 2, area);
      if (nbd) atomicAdd(stat + k.item * 2 + 1, nbd);
    }
  }
}

// tiles = n_planes * nb * ncb in (plane, band, column block) order; bb -> db, both [n_planes][nb][w]
__global__ __launch_bounds__(256) void k_jfp_dilate(const u64* __restrict__ bb, u64* __restrict__ db, int h, int w, int nb, int ncb, int r,
                                                    JfDisk disk, long tiles) {
  __shared__ u64 lv[2][256 + 2 * JF_MAX_R];
  const int tid = threadIdx.x;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {       // block-uniform
    const BpTile k = bp_tile(t, nb, ncb, 0);                   // k.item = the plane
    const int x = k.cb * 256 + tid;
    u64 up[2], mid[2], dn[2];
    jf_halo(bb + k.item * nb * (long)w, k, nb, w, r, tid, mid, up, dn);
    u64* dst = db + (k.item * nb + k.rb) * (long)w;
    const u64 any = mid[0] | mid[1] | up[0] | up[1] | dn[0] | dn[1];
    // the barrier that jf_dilate asks for: past it, the previous tile's readers of lv are done
    if (!__syncthreads_or(any != 0ull)) {
      if (x < w) dst[x] = 0ull;
      continue;
    }
    const u64 D = jf_dilate(mid, up, dn, r, disk, lv, tid);
    const int rows = h - k.y0 < 64 ? h - k.y0 : 64;            // the bits of rows >= h stay 0, as in every bit-plane
    if (x < w) dst[x] = rows == 64 ? D : D & ((1ull << rows) - 1ull);
  }
}

// tiles = nf * ptiles * ktiles * nsl in (frame, proposal tile, object tile, slice) order; planes of W words each: proposal (t, p) is
// plane t * P + p, object (t, k) plane nf * P + t * K + k of mb / bb / db; out int32 [nf][P][K][3] (zeroed)
__global__ __launch_bounds__(256) void k_jfp_pairs(const u64* __restrict__ mb, const u64* __restrict__ bb, const u64* __restrict__ db, int P,
                                                   int K, int nf, long W, int ptiles, int ktiles, int nsl, long tiles, int* __restrict__ out) {
  __shared__ int red[JP_TP * JP_TK * 3];
  const int tid = threadIdx.x;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {       // block-uniform
    const int sl = (int)(t % nsl);
    long q = t / nsl;
    const int kt = (int)(q % ktiles);
    q /= ktiles;
    const int pt = (int)(q % ptiles);
    const long f = q / ptiles;
    if (tid < JP_TP * JP_TK * 3) red[tid] = 0;
    __syncthreads();                                           // (the previous tile's readers of red passed its last barrier)
    long sp[JP_TP], ko[JP_TK];                                 // first word of each plane (clamped: a pair past the edge adds nothing)
    bool sv[JP_TP], kv[JP_TK];
#pragma unroll
    for (int a = 0; a < JP_TP; ++a) {
      const int p = pt * JP_TP + a;
      sv[a] = p < P;
      sp[a] = (f * P + (sv[a] ? p : P - 1)) * W;
    }
#pragma unroll
    for (int c = 0; c < JP_TK; ++c) {
      const int k = kt * JP_TK + c;
      kv[c] = k < K;
      ko[c] = ((long)nf * P + f * K + (kv[c] ? k : K - 1)) * W;
    }
    int acc[JP_TP][JP_TK][3];
#pragma unroll
    for (int a = 0; a < JP_TP; ++a)
#pragma unroll
      for (int c = 0; c < JP_TK; ++c) acc[a][c][0] = acc[a][c][1] = acc[a][c][2] = 0;
    const long j1 = (long)(sl + 1) * JP_SLICE < W ? (long)(sl + 1) * JP_SLICE : W;
    for (long j = (long)sl * JP_SLICE + tid; j < j1; j += 256) {
      u64 sm[JP_TP], sb[JP_TP], sd[JP_TP], km[JP_TK], kb[JP_TK], kd[JP_TK];
#pragma unroll
      for (int a = 0; a < JP_TP; ++a) {
        const u64 m = mb[sp[a] + j], b = bb[sp[a] + j], d = db[sp[a] + j];
        sm[a] = sv[a] ? m : 0ull, sb[a] = sv[a] ? b : 0ull, sd[a] = sv[a] ? d : 0ull;
      }
#pragma unroll
      for (int c = 0; c < JP_TK; ++c) {
        const u64 m = mb[ko[c] + j], b = bb[ko[c] + j], d = db[ko[c] + j];
        km[c] = kv[c] ? m : 0ull, kb[c] = kv[c] ? b : 0ull, kd[c] = kv[c] ? d : 0ull;
      }
#pragma unroll
      for (int a = 0; a < JP_TP; ++a)
#pragma unroll
        for (int c = 0; c < JP_TK; ++c) {
          acc[a][c][0] += __popcll(sm[a] & km[c]);
          acc[a][c][1] += __popcll(sb[a] & kd[c]);
          acc[a][c][2] += __popcll(kb[c] & sd[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < JP_TP; ++a)
#pragma unroll
      for (int c = 0; c < JP_TK; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int v = bp_wave_sum(acc[a][c][i]);
          if ((tid & 63) == 0 && v) atomicAdd(&red[(a * JP_TK + c) * 3 + i], v);
        }
    __syncthreads();
    if (tid < JP_TP * JP_TK * 3) {
      const int a = tid / (JP_TK * 3), c = (tid / 3) % JP_TK, i = tid % 3;
      const int p = pt * JP_TP + a, k = kt * JP_TK + c, v = red[tid];
      if (p < P && k < K && v) atomicAdd(out + ((f * P + p) * K + k) * 3 + i, v);
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------
static bool jfp_shape_ok(int P, int K, int T, int h, int w, int r) {
  return P > 0 && K > 0 && T > 0 && bp_shape_ok(T, h, w) && r >= 0 && r <= JF_MAX_R && (long)P * T < (1L << 31) &&
         (long)K * T < (1L << 31) && (long)P * K * T * 3 < (1L << 31);
}

size_t jf_pairs_workspace_bytes(int n_seg, int n_ann, int n_frames, int h, int w, int radius) {
  if (!jfp_shape_ok(n_seg, n_ann, n_frames, h, w, radius)) return 0;
  return 3 * ((size_t)n_seg + (size_t)n_ann) * (size_t)n_frames * cdiv(h, 64) * (size_t)w * 8;
}

int jf_pairs_counts(const void* seg, int seg_kind, float seg_thr, const int* seg_values, const int* seg_planes, int n_seg, const void* ann,
                    int ann_kind, float ann_thr, const int* ann_values, const int* ann_planes, int n_ann, const unsigned char* void_px,
                    const int* void_planes, int n_frames, int h, int w, int radius, int* pair_out, int* seg_stat, int* ann_stat, void* ws,
                    size_t ws_bytes, hipStream_t s) {
  const int P = n_seg, K = n_ann, T = n_frames, r = radius;
  if (!jfp_shape_ok(P, K, T, h, w, r)) return SAMPT_ERR_ARG;
  BpSrc S, A, V = bp_no_source();
  if (!bp_source(S, seg, seg_kind, seg_thr, seg_values, seg_planes)) return SAMPT_ERR_ARG;
  if (!bp_source(A, ann, ann_kind, ann_thr, ann_values, ann_planes)) return SAMPT_ERR_ARG;
  if (void_px) bp_source(V, void_px, BP_KIND_BYTES, 0.f, nullptr, void_planes);
  if (!pair_out || !seg_stat || !ann_stat || !ws || ((uintptr_t)ws & 15)) return SAMPT_ERR_ARG;
  if (((uintptr_t)pair_out & 3) || ((uintptr_t)seg_stat & 3) || ((uintptr_t)ann_stat & 3)) return SAMPT_ERR_ARG;
  if (ws_bytes < jf_pairs_workspace_bytes(P, K, T, h, w, r)) return SAMPT_ERR_WORKSPACE;
  const JfDisk disk = jf_disk(r);
  hipError_t me = hipMemsetAsync(pair_out, 0, (size_t)T * P * K * 3 * sizeof(int), s);
  if (me == hipSuccess) me = hipMemsetAsync(seg_stat, 0, (size_t)T * P * 2 * sizeof(int), s);
  if (me == hipSuccess) me = hipMemsetAsync(ann_stat, 0, (size_t)T * K * 2 * sizeof(int), s);
  if (me != hipSuccess) {
    set_error("jf_pairs_counts memset", me);
    return SAMPT_ERR_HIP;
  }
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long W = (long)nb * w, planes = ((long)P + K) * T;
  u64* mb = (u64*)ws;
  u64* bb = mb + planes * W;
  u64* db = bb + planes * W;
  typedef void (*words_fn)(BpSrc, BpSrc, int, int, int, int, int, long, int, long, u64*, u64*, int*);
  static const words_fn table[3][2] = {{k_jfp_words<0, false>, k_jfp_words<0, true>},
                                       {k_jfp_words<1, false>, k_jfp_words<1, true>},
                                       {k_jfp_words<2, false>, k_jfp_words<2, true>}};
  for (int side = 0; side < 2; ++side) {
    const int per = side ? K : P;
    const long tiles = (long)per * T * nb * ncb;
    hipLaunchKernelGGL(table[side ? ann_kind : seg_kind][w >= 4 ? 1 : 0], dim3(bp_blocks(tiles, 4)), dim3(256), 0, s, side ? A : S, V, per, h, w, nb, ncb,
                       tiles, w % 4 == 0 ? 1 : 0, side ? (long)P * T : 0L, mb, bb, side ? ann_stat : seg_stat);
    SAMPT_CHECK_LAUNCH("jf_pairs_counts words");
  }
  const long dtiles = planes * nb * ncb;
  hipLaunchKernelGGL(k_jfp_dilate, dim3(bp_blocks(dtiles, 1)), dim3(256), 0, s, (const u64*)bb, db, h, w, nb,
                     ncb, r, disk, dtiles);
  SAMPT_CHECK_LAUNCH("jf_pairs_counts dilate");
  const int ptiles = cdiv(P, JP_TP), ktiles = cdiv(K, JP_TK), nsl = (int)((W + JP_SLICE - 1) / JP_SLICE);
  const long ptl = (long)T * ptiles * ktiles * nsl;
  hipLaunchKernelGGL(k_jfp_pairs, dim3(bp_blocks(ptl, 1)), dim3(256), 0, s, (const u64*)mb, (const u64*)bb,
                     (const u64*)db, P, K, T, W, ptiles, ktiles, nsl, ptl, pair_out);
  SAMPT_CHECK_LAUNCH("jf_pairs_counts pairs");
  return SAMPT_OK;
}

}  // namespace sampt
