// DAVIS region similarity J and boundary measure F on the device: six integer counts per (seg, ann) pair of binary images,
//   inter = |seg & ann|, union = |seg | ann|, n_seg = |B(seg)|, n_ann = |B(ann)|,
//   seg_match = |B(seg) & dil(B(ann))|, ann_match = |B(ann) & dil(B(seg))|,
// B = the boundary map seg2bmap (sam_pt_amd/vos_metrics.py), dil = binary dilation with the disk dy^2 + dx^2 <= r^2, everything
// outside the image 0.  An image is a plane [h][w] of bytes (set iff non-zero), of f32 values (set iff x > thr; NaN and x == thr
// are clear) or of a uint8 index map (set iff x == value[item]); an optional plane index per item lets several items share one
// plane.  An optional byte plane `void` clears its non-zero pixels in both images first.
//
//   k_jf_words  (pass A) one wave per tile of 64 rows x 256 columns: the tile reader of csrc/bitplane.h turns void, seg and ann into
//               64-bit column words held in registers (bit j = row y0 + j), 4 pixels per load from any pixel address (the rows of
//               a width that is no multiple of 4, 854 for one, are not aligned; images narrower than 4 take the element-load form).
//               The south neighbour of a word is word >> 1 with the pixel of the band below carried into bit 63; the east
//               neighbour is the next column's word: the next register, the next lane's first one (a shuffle) or, for the
//               tile's last column, a word that the wave builds with one pixel per lane and a ballot.  Writes the two boundary
//               bit-planes (workspace [item][seg | ann][band][x], 8 B per 64 pixels of a column) and adds the popcounts of
//               inter, union, n_seg, n_ann.  Every pixel of the tile is read once.
//   k_jf_match  (pass B) one workgroup per (item, side, tile), one thread per column.  The threads hold the other image's boundary
//               words of the tile's columns and of r columns to each side, with the words of the band above and below, and dilate
//               them with the disk (jf_halo / jf_dilate of jf_bits.h).  popcount(own word & dilation) is added to seg_match /
//               ann_match; the dilated map is never written.  Tiles whose own boundary is empty are skipped.
// All sums are integer atomics on int32 (h * w < 2^31): bitwise repeatable whatever the order.
#include "ops.h"
#include "jf_bits.h"

namespace sampt {

// tiles = n * nb * ncb in (item, band, column block) order; bw: boundary words [n][2][nb][w]; counts int32 [n][6] (zeroed)
// SK / AK: the kinds of seg and ann (void is bytes); VEC: 4 pixels per load (w >= 4)
template <int SK, int AK, bool VEC>
__global__ __launch_bounds__(256) void k_jf_words(BpSrc seg, BpSrc ann, BpSrc vd, int h, int w, int nb, int ncb, long tiles, int wvec,
                                                  u64* __restrict__ bw, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w;
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const BpTile k = bp_tile(t, nb, ncb, lane);
    JfBits S, A;
    jf_bits<SK, VEC>(seg, k.item, npix, k, h, w, lane, S);
    jf_bits<AK, VEC>(ann, k.item, npix, k, h, w, lane, A);
    if (vd.base) {
      JfBits V;
      jf_bits<BP_KIND_BYTES, VEC>(vd, k.item, npix, k, h, w, lane, V);
      jf_clear(S, V);
      jf_clear(A, V);
    }
    u64 bs[4], ba[4];
    jf_boundary(S, k.y0, k.x0, h, w, lane, bs);
    jf_boundary(A, k.y0, k.x0, h, w, lane, ba);
    int inter = 0, uni = 0, ns = 0, na = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      inter += __popcll(S.word[c] & A.word[c]), uni += __popcll(S.word[c] | A.word[c]);
      ns += __popcll(bs[c]), na += __popcll(ba[c]);
    }
    bp_store4(bw + ((k.item * 2) * nb + k.rb) * (long)w + k.x0, bs, k.x0, w, wvec);
    bp_store4(bw + ((k.item * 2 + 1) * nb + k.rb) * (long)w + k.x0, ba, k.x0, w, wvec);
    inter = bp_wave_sum(inter), uni = bp_wave_sum(uni), ns = bp_wave_sum(ns), na = bp_wave_sum(na);
    if (lane == 0) {
      int* o = counts + k.item * 6;
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
    const BpTile k = bp_tile(t, nb, ncb, 0);                   // k.item = item * 2 + side: the plane of bw that holds the own boundary
    const int x = k.cb * 256 + tid;
    const u64 mine = x < w ? bw[(k.item * nb + k.rb) * (long)w + x] : 0ull;
    // the barrier that jf_dilate asks for: past it, the previous tile's readers of lv and red are done
    if (!__syncthreads_or(mine != 0ull)) continue;
    u64 up[2], mid[2], dn[2];
    jf_halo(bw + ((k.item ^ 1) * nb) * (long)w, k, nb, w, r, tid, mid, up, dn);
    const u64 D = jf_dilate(mid, up, dn, r, disk, lv, tid);
    const int m = bp_wave_sum(__popcll(mine & D));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      const int tot = red[0] + red[1] + red[2] + red[3];
      if (tot) atomicAdd(counts + (k.item >> 1) * 6 + 4 + (k.item & 1), tot);
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------
static bool jf_shape_ok(int n, int h, int w, int r) { return n > 0 && bp_shape_ok(n, h, w) && r >= 0 && r <= JF_MAX_R; }

size_t jf_workspace_bytes(int n, int h, int w, int radius) {
  if (!jf_shape_ok(n, h, w, radius)) return 0;
  return (size_t)n * 2 * cdiv(h, 64) * (size_t)w * 8;
}

int jf_counts(const void* seg, int seg_kind, float seg_thr, const int* seg_values, const int* seg_planes, const void* ann, int ann_kind,
              float ann_thr, const int* ann_values, const int* ann_planes, const unsigned char* void_px, const int* void_planes, int n,
              int h, int w, int radius, int* counts, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!jf_shape_ok(n, h, w, radius)) return SAMPT_ERR_ARG;
  BpSrc S, A, V = bp_no_source();
  if (!bp_source(S, seg, seg_kind, seg_thr, seg_values, seg_planes)) return SAMPT_ERR_ARG;
  if (!bp_source(A, ann, ann_kind, ann_thr, ann_values, ann_planes)) return SAMPT_ERR_ARG;
  if (void_px) bp_source(V, void_px, BP_KIND_BYTES, 0.f, nullptr, void_planes);
  if (!counts || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)counts & 3)) return SAMPT_ERR_ARG;
  if (ws_bytes < jf_workspace_bytes(n, h, w, radius)) return SAMPT_ERR_WORKSPACE;
  const int r = radius;
  const JfDisk disk = jf_disk(r);
  const hipError_t me = hipMemsetAsync(counts, 0, (size_t)n * 6 * sizeof(int), s);
  if (me != hipSuccess) {
    set_error("jf_counts memset", me);
    return SAMPT_ERR_HIP;
  }
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long tiles = (long)n * nb * ncb;
  typedef void (*words_fn)(BpSrc, BpSrc, BpSrc, int, int, int, int, long, int, u64*, int*);
#define JF_W(sk, ak) {k_jf_words<sk, ak, false>, k_jf_words<sk, ak, true>}
  static const words_fn table[3][3][2] = {{JF_W(0, 0), JF_W(0, 1), JF_W(0, 2)}, {JF_W(1, 0), JF_W(1, 1), JF_W(1, 2)},
                                          {JF_W(2, 0), JF_W(2, 1), JF_W(2, 2)}};
#undef JF_W
  hipLaunchKernelGGL(table[seg_kind][ann_kind][w >= 4 ? 1 : 0], dim3(bp_blocks(tiles, 4)), dim3(256), 0, s, S, A, V, h, w, nb, ncb, tiles,
                     w % 4 == 0 ? 1 : 0, (u64*)ws, counts);
  SAMPT_CHECK_LAUNCH("jf_counts words");
  const long mtiles = tiles * 2;
  hipLaunchKernelGGL(k_jf_match, dim3(bp_blocks(mtiles, 1)), dim3(256), 0, s, (const u64*)ws, w, nb, ncb,
                     r, disk, mtiles, counts);
  SAMPT_CHECK_LAUNCH("jf_counts match");
  return SAMPT_OK;
}

}  // namespace sampt
