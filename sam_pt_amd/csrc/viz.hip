// Prediction overlays (sam_pt_amd/visualize.py): the frames of a clip with every mask's tint, its contour band and the point markers.
// The masks arrive as bit-planes (bits_pack of vis_eval.hip; mask m on frame t is item m * T + t).  All arithmetic of the blend was done
// on the host, in float64, into 256-entry byte tables: the kernels here only look bytes up.
//
//   k_viz_band     one workgroup per (item, band of 64 rows, 256 columns), one thread per column: band = dil(m) & dil(~m), dil = the
//                  disk dilation of jf_bits.h (jf_halo / jf_dilate), ~m taken inside the image only, everything outside it 0.  A tile
//                  whose reach holds one class only writes zeros and leaves early.
//   k_viz_compose  one wave per (frame, tile of 64 rows x 256 columns), bitplane.h's tile decode; a lane owns 4 adjacent columns and
//                  walks the tile in groups of 16 rows: 4 pixels of a channel per 4-byte load (planar frames) or 12 bytes of 4
//                  interleaved pixels, then per mask the 16-row slices of its column words (mask and band, read once overall), one
//                  table lookup per channel and mask, 12 contiguous bytes of interleaved output per row.  Then the markers: the wave
//                  takes 64 rows of the marker table at a time, a ballot keeps those whose bounding box meets the tile, and they are
//                  drawn in table order by the lane that owns the column - over its own earlier stores, so the last marker that covers
//                  a pixel wins without atomics.  The stacked panel writes the input half and the predictions half in the same pass.
// Integer work only: bitwise repeatable.
#include "ops.h"
#include "jf_bits.h"

namespace sampt {

namespace {
constexpr int VZ_ROWS = 16;                  // rows of a tile a lane holds at a time
constexpr int VZ_CLEAR = 60;                 // table rows: (colour * 3 + channel) * 2 + band for a set pixel, 60 + band for a clear one
constexpr int VZ_TABLES = 62;
constexpr int VZ_MARKER = 8;                 // int32 per marker: x, y, kind (0 ring, 1 cross), size, width, reach, colour, input colour
constexpr int VZ_PANEL_INPUT = 1, VZ_PANEL_PRED = 2;

typedef unsigned short vz_u16 __attribute__((aligned(2)));
typedef u32 vz_u32x3 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ u64 vz_rowmask(int h, int rb) {
  const int rows = h - rb * 64 < 64 ? h - rb * 64 : 64;
  return rows == 64 ? ~0ull : (1ull << rows) - 1ull;
}

// 4 pixels (y, xl .. xl + 3) of a frame as one word per channel (byte c = pixel xl + c); loads by bitplane.h's rules: xl <= w - 4 when
// VEC, element loads clamped to w - 1 otherwise
template <bool VEC>
__device__ __forceinline__ void vz_load(const unsigned char* __restrict__ f, int interleaved, long npix, int y, int xl, int w, u32* px) {
  if (interleaved) {
    const unsigned char* p = f + ((long)y * w) * 3;
    if (VEC) {
      const u32 a = *(const bp_u8x4*)(p + (long)xl * 3), b = *(const bp_u8x4*)(p + (long)xl * 3 + 4), c = *(const bp_u8x4*)(p + (long)xl * 3 + 8);
      px[0] = (a & 0xffu) | ((a >> 24) << 8) | (((b >> 16) & 0xffu) << 16) | (((c >> 8) & 0xffu) << 24);
      px[1] = ((a >> 8) & 0xffu) | ((b & 0xffu) << 8) | ((b >> 24) << 16) | (((c >> 16) & 0xffu) << 24);
      px[2] = ((a >> 16) & 0xffu) | (((b >> 8) & 0xffu) << 8) | ((c & 0xffu) << 16) | ((c >> 24) << 24);
    } else {
      px[0] = px[1] = px[2] = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int xc = xl + c < w ? xl + c : w - 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) px[ch] |= (u32)p[(long)xc * 3 + ch] << (8 * c);
      }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const unsigned char* p = f + ch * npix + (long)y * w;
      if (VEC) {
        px[ch] = *(const bp_u8x4*)(p + xl);
      } else {
        u32 v = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) v |= (u32)p[xl + c < w ? xl + c : w - 1] << (8 * c);
        px[ch] = v;
      }
    }
  }
}

// a lane's 4 pixels (one word per channel) to 12 interleaved bytes at dst = pixel (y, x0); wvec: w % 4 == 0 and a 4-byte aligned output,
// so dst is 4-byte aligned and x0 < w means all four columns
__device__ __forceinline__ void vz_store(unsigned char* __restrict__ dst, const u32* px, int x0, int w, int wvec) {
  const u32 r = px[0], g = px[1], b = px[2];
  if (wvec) {
    if (x0 < w) {
      vz_u32x3 v;
      v.x = (r & 0xffu) | ((g & 0xffu) << 8) | ((b & 0xffu) << 16) | (((r >> 8) & 0xffu) << 24);
      v.y = ((g >> 8) & 0xffu) | (((b >> 8) & 0xffu) << 8) | (((r >> 16) & 0xffu) << 16) | (((g >> 16) & 0xffu) << 24);
      v.z = ((b >> 16) & 0xffu) | ((r >> 24) << 8) | ((g >> 24) << 16) | ((b >> 24) << 24);
      *(vz_u32x3*)dst = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (x0 + c < w) {
        dst[c * 3] = (unsigned char)(r >> (8 * c)), dst[c * 3 + 1] = (unsigned char)(g >> (8 * c));
        dst[c * 3 + 2] = (unsigned char)(b >> (8 * c));
      }
  }
}

// does marker (kind, size, width) centred at (mx, my) cover pixel (u, v)?  The integer predicates of sam_pt_amd/visualize.py
__device__ __forceinline__ bool vz_covers(int kind, int size, int width, int mx, int my, int u, int v) {
  const long a = u - mx, b = v - my;
  if (kind == 0) {                                             // ring: max(2R - w, 0)^2 <= 4 d^2 <= (2R + w)^2
    const long d4 = 4 * (a * a + b * b), lo = 2 * size - width > 0 ? 2 * size - width : 0, hi = 2 * size + width;
    return lo * lo <= d4 && d4 <= hi * hi;
  }
  const long L2 = 2 * (long)size, w2 = (long)width * width;    // cross: the two diagonals of half-length L, thickness w
  long s = a + b;
  s = s < -L2 ? -L2 : s > L2 ? L2 : s;
  if ((2 * a - s) * (2 * a - s) + (2 * b - s) * (2 * b - s) <= w2) return true;
  s = a - b;
  s = s < -L2 ? -L2 : s > L2 ? L2 : s;
  return (2 * a - s) * (2 * a - s) + (2 * b + s) * (2 * b + s) <= w2;
}
}  // namespace

// tiles = n * nb * ncb in (item, band, column block) order; bits -> band, both [n][nb][w]
__global__ __launch_bounds__(256) void k_viz_band(const u64* __restrict__ bits, u64* __restrict__ band, int h, int w, int nb, int ncb, int r,
                                                  JfDisk disk, long tiles) {
  __shared__ u64 lv[2][256 + 2 * JF_MAX_R];
  const int tid = threadIdx.x;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {       // block-uniform
    const BpTile k = bp_tile(t, nb, ncb, 0);                   // k.item = the plane
    const int x = k.cb * 256 + tid;
    u64 up[2], mid[2], dn[2], cup[2], cmid[2], cdn[2];
    jf_halo(bits + k.item * nb * (long)w, k, nb, w, r, tid, mid, up, dn);
#pragma unroll
    for (int i = 0; i < 2; ++i) {                              // the complement inside the image: real columns, real rows
      const int hc = tid + i * 256, xx = k.cb * 256 - r + hc;
      const bool ok = hc < 256 + 2 * r && xx >= 0 && xx < w;
      cmid[i] = ok ? ~mid[i] & vz_rowmask(h, k.rb) : 0ull;
      cup[i] = ok && k.rb > 0 ? ~up[i] : 0ull;                 // (a band above the last one is full)
      cdn[i] = ok && k.rb + 1 < nb ? ~dn[i] & vz_rowmask(h, k.rb + 1) : 0ull;
    }
    u64* dst = band + (k.item * nb + k.rb) * (long)w;
    const u64 any = mid[0] | mid[1] | up[0] | up[1] | dn[0] | dn[1];
    const u64 cany = cmid[0] | cmid[1] | cup[0] | cup[1] | cdn[0] | cdn[1];
    // the barriers that jf_dilate asks for: past the first, the previous tile's readers of lv are done; past the last, this tile's
    // first dilation's are
    const int has = __syncthreads_or(any != 0ull), chas = __syncthreads_or(cany != 0ull);
    if (!has || !chas) {                                       // one class only within reach: no band
      if (x < w) dst[x] = 0ull;
      continue;
    }
    const u64 D = jf_dilate(mid, up, dn, r, disk, lv, tid);
    __syncthreads();
    const u64 C = jf_dilate(cmid, cup, cdn, r, disk, lv, tid);
    if (x < w) dst[x] = D & C & vz_rowmask(h, k.rb);           // the bits of rows >= h stay 0, as in every bit-plane
  }
}

// tiles = T * nb * ncb in (frame, band, column block) order.  frames [T][3][h][w] or, interleaved, [T][h][w][3]; bits / band
// [n_masks * T][nb][w] (mask m of frame t = item m * T + t); lut [VZ_TABLES][256]; markers int32 [T][n_markers][VZ_MARKER];
// out [T][rows_out][w][3] with rows_out = h, or 2 h for both panels (input above predictions)
template <bool VEC>
__global__ __launch_bounds__(256) void k_viz_compose(const unsigned char* __restrict__ frames, int interleaved, int T, int h, int w, int nb,
                                                     int ncb, const u64* __restrict__ bits, const u64* __restrict__ band, int n_masks,
                                                     const unsigned char* __restrict__ lut, const int* __restrict__ markers, int n_markers,
                                                     int panel, int wvec, long tiles, unsigned char* __restrict__ out) {
  __shared__ unsigned char tab[VZ_TABLES * 256];
  if (n_masks > 0 && (panel & VZ_PANEL_PRED)) {
    for (int i = threadIdx.x; i < VZ_TABLES * 64; i += 256) ((u32*)tab)[i] = ((const u32*)lut)[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long npix = (long)h * w, frame_out = npix * 3 * ((panel & VZ_PANEL_INPUT) && (panel & VZ_PANEL_PRED) ? 2 : 1);
  const long pred_off = (panel & VZ_PANEL_INPUT) ? npix * 3 : 0;   // the predictions half of the stacked panel
  for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (long)gridDim.x * 4) {   // wave-uniform
    const BpTile k = bp_tile(t, nb, ncb, lane);                // k.item = the frame
    const int x0 = k.x0, y0 = k.y0;
    const int xl = VEC ? (x0 + 4 <= w ? x0 : w - 4) : (x0 < w ? x0 : w - 1);
    const int d8 = VEC && x0 < w ? 8 * (x0 - xl) : 0;          // column x0 + c was loaded as byte c + d (beyond w: never stored)
    const int rows = h - y0 < 64 ? h - y0 : 64;
    const unsigned char* f = frames + k.item * npix * 3;
    unsigned char* o = out + k.item * frame_out;
    int xw[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) xw[c] = x0 + c < w ? x0 + c : w - 1;
    for (int g = 0; g * VZ_ROWS < rows; ++g) {                 // wave-uniform
      u32 px[VZ_ROWS][3];
#pragma unroll
      for (int j = 0; j < VZ_ROWS; ++j) {
        const int y = y0 + g * VZ_ROWS + j < h ? y0 + g * VZ_ROWS + j : h - 1;
        vz_load<VEC>(f, interleaved, npix, y, xl, w, px[j]);
      }
#pragma unroll
      for (int j = 0; j < VZ_ROWS; ++j) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) px[j][ch] >>= d8;
      }
      if (panel & VZ_PANEL_INPUT) {
#pragma unroll
        for (int j = 0; j < VZ_ROWS; ++j) {
          const int y = y0 + g * VZ_ROWS + j;
          if (y < h) vz_store(o + ((long)y * w + x0) * 3, px[j], x0, w, wvec);
        }
      }
      if (panel & VZ_PANEL_PRED) {
        for (int m = 0; m < n_masks; ++m) {
          const long wo = (((long)m * T + k.item) * nb + k.rb) * (long)w;
          const int cm = (m < 9 ? m : 9) * 6;
          u32 mb[4], bb[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {                        // rows 16 g .. 16 g + 15 of the column words
            mb[c] = ((const vz_u16*)(bits + wo + xw[c]))[g];
            bb[c] = ((const vz_u16*)(band + wo + xw[c]))[g];
          }
#pragma unroll
          for (int j = 0; j < VZ_ROWS; ++j) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              u32 v = px[j][ch], r = 0;
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const u32 on = (mb[c] >> j) & 1u, bd = (bb[c] >> j) & 1u;
                const u32 row = on ? cm + ch * 2 + bd : VZ_CLEAR + bd;
                r |= (u32)tab[row * 256 + ((v >> (8 * c)) & 0xffu)] << (8 * c);
              }
              px[j][ch] = r;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < VZ_ROWS; ++j) {
          const int y = y0 + g * VZ_ROWS + j;
          if (y < h) vz_store(o + pred_off + ((long)y * w + x0) * 3, px[j], x0, w, wvec);
        }
      }
    }
    // the markers of the frame, 64 at a time: the lane that owns a column overwrites its own stores, in table order
    const int xt0 = k.cb * 256, xt1 = (k.xe < w ? k.xe : w) - 1, yt1 = y0 + rows - 1;
    for (int c0 = 0; c0 < n_markers; c0 += 64) {               // wave-uniform
      const int i = c0 + lane < n_markers ? c0 + lane : n_markers - 1;
      const int* mk = markers + (k.item * n_markers + i) * VZ_MARKER;
      const int mx = mk[0], my = mk[1], kind = mk[2], size = mk[3], width = mk[4], reach = mk[5], col = mk[6], col_in = mk[7];
      const bool meets = c0 + lane < n_markers && mx + reach >= xt0 && mx - reach <= xt1 && my + reach >= y0 && my - reach <= yt1;
      u64 hits = __ballot(meets);
      while (hits) {                                           // wave-uniform
        const int s = __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int sx = __shfl(mx, s, 64), sy = __shfl(my, s, 64), sk = __shfl(kind, s, 64), ss = __shfl(size, s, 64);
        const int sw = __shfl(width, s, 64), sr = __shfl(reach, s, 64), sc = __shfl(col, s, 64), si = __shfl(col_in, s, 64);
        const int ya = sy - sr > y0 ? sy - sr : y0, yb = sy + sr < yt1 ? sy + sr : yt1;
        for (int y = ya; y <= yb; ++y) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (x0 + c < w && vz_covers(sk, ss, sw, sx, sy, x0 + c, y)) {
              unsigned char* p = o + ((long)y * w + x0 + c) * 3;
              if (panel & VZ_PANEL_INPUT) p[0] = (unsigned char)si, p[1] = (unsigned char)(si >> 8), p[2] = (unsigned char)(si >> 16);
              if (panel & VZ_PANEL_PRED) {
                p += pred_off;
                p[0] = (unsigned char)sc, p[1] = (unsigned char)(sc >> 8), p[2] = (unsigned char)(sc >> 16);
              }
            }
          }
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------
int viz_band(const unsigned long long* bits, int n, int h, int w, int radius, unsigned long long* band, hipStream_t s) {
  if (!bp_shape_ok(n, h, w) || radius < 0 || radius > JF_MAX_R) return SAMPT_ERR_ARG;
  if (n == 0) return SAMPT_OK;
  if (!bits || !band || ((uintptr_t)bits & 7) || ((uintptr_t)band & 7)) return SAMPT_ERR_ARG;
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long tiles = (long)n * nb * ncb;
  hipLaunchKernelGGL(k_viz_band, dim3(bp_blocks(tiles, 1)), dim3(256), 0, s, (const u64*)bits, (u64*)band, h, w, nb, ncb, radius,
                     jf_disk(radius), tiles);
  SAMPT_CHECK_LAUNCH("viz_band");
  return SAMPT_OK;
}

int viz_compose(const unsigned char* frames, int interleaved, int n_frames, int h, int w, const unsigned long long* bits,
                const unsigned long long* band, int n_masks, const unsigned char* lut, const int* markers, int n_markers, int panel,
                unsigned char* out, hipStream_t s) {
  const bool in = panel & VZ_PANEL_INPUT, pred = panel & VZ_PANEL_PRED;
  if (!bp_shape_ok(n_frames, h, w) || n_masks < 0 || n_markers < 0 || panel < 1 || panel > 3) return SAMPT_ERR_ARG;
  if (n_frames == 0) return SAMPT_OK;
  if (!frames || !out) return SAMPT_ERR_ARG;
  if (pred && n_masks > 0 && (!bits || !band || !lut || ((uintptr_t)bits & 7) || ((uintptr_t)band & 7) || ((uintptr_t)lut & 3)))
    return SAMPT_ERR_ARG;
  if (n_markers > 0 && (!markers || ((uintptr_t)markers & 3))) return SAMPT_ERR_ARG;
  const int nb = cdiv(h, 64), ncb = cdiv(w, 256);
  const long tiles = (long)n_frames * nb * ncb;
  const int wvec = w % 4 == 0 && !((uintptr_t)out & 3) ? 1 : 0;
  hipLaunchKernelGGL(w >= 4 ? k_viz_compose<true> : k_viz_compose<false>, dim3(bp_blocks(tiles, 4)), dim3(256), 0, s, frames, interleaved ? 1 : 0,
                     n_frames, h, w, nb, ncb, (const u64*)bits, (const u64*)band, in && !pred ? 0 : n_masks, lut, markers, n_markers, panel, wvec,
                     tiles, out);
  SAMPT_CHECK_LAUNCH("viz_compose");
  return SAMPT_OK;
}

}  // namespace sampt
