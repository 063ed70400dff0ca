// Prompt assembly of SamPt on the device: what SamPt._prepare_points followed by ResizeLongestSide.apply_coords computes per
// (frame, object) item (reference sam_pt.py:726-758), from point tracks that never left the device.  The specification is the host
// restatement sam_pt_amd/prompt_assembly.py (assemble_prompts_host); the results equal it word for word.
//
//   traj f32 [T][M][P][2]      vis f32 [T][M][P] visibility codes: a point is visible iff its code == 1.0f
//   ppe = min(pp, P): the leading points of an object that other objects receive as negatives
//
// An item's prompt: its own visible points in index order (label 1 for index < pp, else 0 when `negatives`, else 1), then - when
// M > 1 and `add_others` - the visible first-ppe points of every other object, object-major, label 0.  A coordinate is
// (float)((double)x * sx): NumPy's float64 product stored into a float32 array.
//
// Two stream-ordered calls, so that the host decides (which items run, how many point slots, which chunks) from the counts alone:
//   prompt_count   one workgroup per frame: the frame's visible leading points are summed once, every object's k and npos follow.
//   prompt_fill    one workgroup of 4 waves per item of a chunk.  The output order is defined, so there are no atomics: every
//                  round of 256 candidates is compacted with a ballot per wave (lane prefix = popcount of the lower lanes' bits) and
//                  the four wave totals meet in LDS.  The frame's candidate list is the same for all of its M items, each minus its
//                  own segment; a candidate's slot in THIS item's prompt is its rank in the frame's list, minus the item's own
//                  segment length when the candidate lies behind it - so the list itself is never stored, whatever M * pp is, and
//                  there is neither an LDS budget nor a scratch buffer to fall back to.  The price is that the M items of a frame
//                  each scan the frame's M * ppe codes (L2-resident: 100 objects x 8 points are 3.2 KB of codes).
//   mark_outside_frame   the four border comparisons of SamPt._mark_outside_frame (sam_pt.py:684-690), f32 IEEE divisions.
#include "ops.h"

namespace sampt {

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_WAVES = PA_THREADS / 64;

struct PaScan {
  int pos;       // number of `a` flags in front of this thread, in thread order
  int total_a;   // `a` flags of the workgroup
  int total_b;   // `b` flags of the workgroup
};

// Ordered workgroup scan of one flag and the count of a second one.  Every thread of the workgroup calls it; s_w is int[2 * PA_WAVES].
__device__ __forceinline__ PaScan pa_scan(bool a, bool b, int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ba = __ballot(a), bb = __ballot(b);
  if (lane == 0) s_w[wave] = __popcll(ba), s_w[PA_WAVES + wave] = __popcll(bb);
  __syncthreads();
  PaScan r;
  r.pos = __popcll(ba & ((1ull << lane) - 1ull));
  r.total_a = r.total_b = 0;
#pragma unroll
  for (int w = 0; w < PA_WAVES; ++w) {
    if (w < wave) r.pos += s_w[w];
    r.total_a += s_w[w], r.total_b += s_w[PA_WAVES + w];
  }
  __syncthreads();                                   // s_w is free for the next round
  return r;
}

}  // namespace

__global__ __launch_bounds__(PA_THREADS) void k_prompt_count(const float* __restrict__ vis, int M, int P, int ppe, int negatives,
                                                             int others, int* __restrict__ k_all, int* __restrict__ npos_all) {
  __shared__ int s_part[PA_WAVES];
  const int t = blockIdx.x, tid = threadIdx.x;
  const float* v = vis + (long)t * M * P;
  int lead = 0;                                      // visible leading points of the objects this thread owns
  if (others)
    for (int m = tid; m < M; m += PA_THREADS)
      for (int p = 0; p < ppe; ++p) lead += v[(long)m * P + p] == 1.f;
  for (int o = 32; o > 0; o >>= 1) lead += __shfl_xor(lead, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = lead;
  __syncthreads();
  int frame_lead = 0;
#pragma unroll
  for (int w = 0; w < PA_WAVES; ++w) frame_lead += s_part[w];
  for (int m = tid; m < M; m += PA_THREADS) {
    int own = 0, own_lead = 0;
    for (int p = 0; p < P; ++p) {
      const int on = v[(long)m * P + p] == 1.f;
      own += on, own_lead += (p < ppe) ? on : 0;
    }
    k_all[(long)t * M + m] = own + (others ? frame_lead - own_lead : 0);
    npos_all[(long)t * M + m] = negatives ? own_lead : own;
  }
}

__global__ __launch_bounds__(PA_THREADS) void k_prompt_fill(const float* __restrict__ traj, const float* __restrict__ vis, int T, int M,
                                                            int P, int pp, int ppe, int negatives, int others, double sx, double sy,
                                                            const int* __restrict__ items, int ld, float* __restrict__ pts,
                                                            int* __restrict__ labels, int* __restrict__ k_item,
                                                            int* __restrict__ npos_item) {
  __shared__ int s_w[2 * PA_WAVES];
  const int f = blockIdx.x, tid = threadIdx.x;
  float* out_xy = pts + (long)f * ld * 2;
  int* out_lab = labels + (long)f * ld;
  const int item = items[f];
  int k = 0, npos = 0;
  if (item >= 0 && item < T * M) {                   // (an item number outside the clip gets an empty prompt, never an address)
    const int t = item / M, m = item % M;
    const long frame = (long)t * M * P;
    int own_lead = 0;
    // ---- the item's own visible points, in index order
    for (int p0 = 0; p0 < P; p0 += PA_THREADS) {
      const int p = p0 + tid;
      const long src = frame + (long)m * P + p;
      const bool on = p < P && vis[src] == 1.f;
      const PaScan sc = pa_scan(on, on && p < ppe, s_w);
      const int slot = k + sc.pos;
      if (on && slot < ld) {
        out_xy[2 * slot] = (float)((double)traj[2 * src] * sx);
        out_xy[2 * slot + 1] = (float)((double)traj[2 * src + 1] * sy);
        out_lab[slot] = (p < pp || !negatives) ? 1 : 0;
      }
      k += sc.total_a, own_lead += sc.total_b;
    }
    npos = negatives ? own_lead : k;
    // ---- the other objects' visible leading points, object-major: rank in the frame's list, the item's own segment taken out
    if (others && ppe > 0) {
      const int n = M * ppe;
      const int own_k = k;
      int rank0 = 0;                                 // candidates of other objects placed so far
      for (int j0 = 0; j0 < n; j0 += PA_THREADS) {
        const int j = j0 + tid;
        const int mo = j / ppe, p = j - mo * ppe;
        const long src = frame + (long)mo * P + p;
        const bool on = j < n && mo != m && vis[src] == 1.f;
        const PaScan sc = pa_scan(on, false, s_w);
        const int slot = own_k + rank0 + sc.pos;
        if (on && slot < ld) {
          out_xy[2 * slot] = (float)((double)traj[2 * src] * sx);
          out_xy[2 * slot + 1] = (float)((double)traj[2 * src + 1] * sy);
          out_lab[slot] = 0;
        }
        rank0 += sc.total_a;
      }
      k = own_k + rank0;
    }
  }
  for (int i = k + tid; i < ld; i += PA_THREADS) out_xy[2 * i] = 0.f, out_xy[2 * i + 1] = 0.f, out_lab[i] = 0;   // as the host block
  if (tid == 0) k_item[f] = k, npos_item[f] = npos;
}

__global__ __launch_bounds__(PA_THREADS) void k_mark_outside_frame(const float* __restrict__ traj, const float* vis_in, long n, float hf,
                                                                   float wf, float* vis_out) {
  for (long i = (long)blockIdx.x * PA_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PA_THREADS) {
    const float x = traj[2 * i], y = traj[2 * i + 1];
    const bool out = __fdiv_rn(x, wf) < 0.01f || __fdiv_rn(y, hf) < 0.01f || __fdiv_rn(x, wf) > 0.99f || __fdiv_rn(y, hf) > 0.99f;
    vis_out[i] = out ? -2.f : vis_in[i];
  }
}

static bool pa_bad_shape(int T, int M, int P, int pp) {
  return T <= 0 || M <= 0 || P <= 0 || pp < 0 || (long)T * M * P * 2 > 0x7fffffffL;
}

int prompt_count(const float* vis, int T, int M, int P, int pp, int negatives, int add_others, int* k_all, int* npos_all, hipStream_t s) {
  if (pa_bad_shape(T, M, P, pp) || !vis || !k_all || !npos_all) return SAMPT_ERR_ARG;
  const int ppe = pp < P ? pp : P;
  hipLaunchKernelGGL(k_prompt_count, dim3(T), dim3(PA_THREADS), 0, s, vis, M, P, ppe, negatives ? 1 : 0, (add_others && M > 1) ? 1 : 0, k_all,
                     npos_all);
  SAMPT_CHECK_LAUNCH("prompt_count");
  return SAMPT_OK;
}

int prompt_fill(const float* traj, const float* vis, int T, int M, int P, int pp, int negatives, int add_others, double sx, double sy,
                const int* items, int F, int ld, float* pts, int* labels, int* k_item, int* npos_item, hipStream_t s) {
  if (pa_bad_shape(T, M, P, pp) || F <= 0 || ld <= 0 || (long)F * ld * 2 > 0x7fffffffL) return SAMPT_ERR_ARG;
  if (!traj || !vis || !items || !pts || !labels || !k_item || !npos_item) return SAMPT_ERR_ARG;
  const int ppe = pp < P ? pp : P;
  hipLaunchKernelGGL(k_prompt_fill, dim3(F), dim3(PA_THREADS), 0, s, traj, vis, T, M, P, pp, ppe, negatives ? 1 : 0,
                     (add_others && M > 1) ? 1 : 0, sx, sy, items, ld, pts, labels, k_item, npos_item);
  SAMPT_CHECK_LAUNCH("prompt_fill");
  return SAMPT_OK;
}

int mark_outside_frame(const float* traj, const float* vis_in, long n, int H, int W, float* vis_out, hipStream_t s) {
  if (n <= 0 || H <= 0 || W <= 0 || !traj || !vis_in || !vis_out) return SAMPT_ERR_ARG;
  const long blocks = (n + PA_THREADS - 1) / PA_THREADS;
  hipLaunchKernelGGL(k_mark_outside_frame, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(PA_THREADS), 0, s, traj, vis_in, n, (float)H,
                     (float)W, vis_out);
  SAMPT_CHECK_LAUNCH("mark_outside_frame");
  return SAMPT_OK;
}

}  // namespace sampt
