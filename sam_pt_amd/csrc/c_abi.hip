// extern "C" surface of libsampt_hip.so (declared in include/sampt_hip.h).
#include <string.h>

#include <exception>
#include <memory>
#include <string>
#include <unordered_map>

#include "../../include/sampt_hip.h"
#include "engine_layers.h"

namespace sampt {
static thread_local std::string g_err;
void set_error(const char* where, hipError_t e) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
}
const char* last_error() { return g_err.c_str(); }
static int fail(int rc, const std::string& msg) {
  g_err = msg;
  return rc;
}
// a caller's workspace for the fused InstanceNorm statistics (doubles, written by the convolution kernels)
static bool stats_ws_bad(const void* ws) { return !ws || ((uintptr_t)ws & 7); }
static WeightMap make_map(const char* const* names, const void* const* ptrs, int n) {
  WeightMap w;
  for (int i = 0; i < n; ++i) w.m[names[i]] = ptrs[i];
  return w;
}
// Builds a handle; no C++ exception (allocation failure, ...) may cross the C boundary.
template <class H, class Init>
static int create_handle(const char* what, H** out, Init init) {
  try {
    std::unique_ptr<H> h(new H());
    int rc = init(*h);
    if (rc != SAMPT_OK) return fail(rc, h->e.error.empty() ? std::string(what) + ": initialisation failed" : h->e.error);
    *out = h.release();
    return SAMPT_OK;
  } catch (const std::exception& ex) {
    return fail(SAMPT_ERR_ARG, std::string(what) + ": " + ex.what());
  } catch (...) {
    return fail(SAMPT_ERR_ARG, std::string(what) + ": unknown C++ exception");
  }
}
}  // namespace sampt

using namespace sampt;

struct sampt_pips {
  PipsEngine e;
  int* flag = nullptr;                       // pinned host int32[2]: active chains after the last two rounds (sampt_pips_track_f32)
  hipEvent_t flag_ev[2] = {nullptr, nullptr};
  ~sampt_pips() {
    if (flag) (void)hipHostFree(flag);
    for (auto& ev : flag_ev)
      if (ev) (void)hipEventDestroy(ev);
  }
};
struct sampt_pips2 { Pips2Engine e; };
struct sampt_cotracker { CotEngine e; };
struct sampt_raft { RaftEngine e; };
struct sampt_tapir {
  TapirEngine e;
  int max_queries = 0;   // > 0: at most this many queries per refinement chunk (sampt_tapir_set_max_queries)
};
struct sampt_tapnet { TapnetEngine e; };
struct sampt_sg { SgEngine e; };
struct sampt_vit { VitEngine e; };
struct sampt_tinyvit { TinyVitEngine e; };
// hipGraph cache of the per-(frame, object) decode chain (north_star: "hipGraph capture of the per-frame decode"): one
// instantiated graph per distinct call signature (every scalar AND every pointer of sampt_sam_track_decode_graph).
struct DecGraphKey {
  const void *features, *hq, *pts, *labels, *k_item, *npos_item, *logits, *score, *ws;
  size_t ws_bytes;
  int frames, k, ld_pts, n_pos_first, refine, in_h, in_w, oh, ow;
  int batch_invariant;   // DecEngine::batch_invariant at capture: a graph holds the kernels of ONE mode
  float iou_thr;
  bool operator==(const DecGraphKey& o) const { return memcmp(this, &o, sizeof(*this)) == 0; }
};
struct DecGraphKeyHash {
  size_t operator()(const DecGraphKey& k) const {
    const unsigned char* p = (const unsigned char*)&k;
    size_t h = 1469598103934665603ull;
    for (size_t i = 0; i < sizeof(k); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
  }
};
struct DecGraphEntry {
  hipGraphExec_t exec = nullptr;
  int seen = 0;       // calls with this signature so far (the first one runs eagerly: lazy one-time kernel attributes)
  long last_use = 0;
};
struct sampt_dec {
  DecEngine e;
  std::unordered_map<DecGraphKey, DecGraphEntry, DecGraphKeyHash> graphs;
  long graph_clock = 0, graph_launches = 0, graph_captures = 0;
  ~sampt_dec() {
    for (auto& kv : graphs)
      if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  }
};

extern "C" {

int sampt_version(void) { return 1; }
const char* sampt_last_error(void) { return last_error(); }

// ------------------------------------------------------------------------------------------- PIPS
int sampt_pips_create(const char* const* names, const void* const* ptrs, int n, int stride, int S, sampt_pips_t* out) {
  if (!names || !ptrs || !out || S != 8) return fail(SAMPT_ERR_ARG, "sampt_pips_create: bad arguments (S must be 8)");
  return create_handle<sampt_pips>("sampt_pips_create", out, [&](sampt_pips& h) {
    h.e.S = S, h.e.stride = stride;
    return h.e.init(make_map(names, ptrs, n));
  });
}
void sampt_pips_destroy(sampt_pips_t h) { delete h; }

int sampt_pips_fnet_workspace_bytes(sampt_pips_t h, int nf, int H, int W, size_t* bytes) {
  if (!h || !bytes) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  float* out[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = h->e.fnet(nullptr, nf, H, W, out, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_pips_fnet_f32(sampt_pips_t h, const uint8_t* frames, int nf, int H, int W, float* const pyr[4], void* ws,
                        size_t ws_bytes, sampt_stream_t stream) {
  // any frame size works (feature map = floor(H / stride), pyramid levels floor-halved like avg_pool2d); the coarsest
  // level must keep >= 2 pixels per axis because the sampler normalises by (size - 1) (pips.py:324-326)
  if (!h || !frames || !pyr || !ws || H < 16 * h->e.stride || W < 16 * h->e.stride)
    return fail(SAMPT_ERR_ARG, "sampt_pips_fnet_f32: bad arguments (H, W must be at least 16*stride)");
  Arena a(ws, ws_bytes);
  return h->e.fnet(frames, nf, H, W, pyr, a, (hipStream_t)stream);
}

int sampt_pips_sample_feat_f32(const float* fmap, int H0, int W0, const int32_t* frame_idx, const float* xy, int n,
                               float* out, sampt_stream_t stream) {
  return pips_sample_feat(fmap, H0, W0, 128, (const int*)frame_idx, xy, n, out, (hipStream_t)stream);
}

static PyramidLevels make_pyr(const float* const pyr[4], int H0, int W0) {
  PyramidLevels p;
  int h = H0, w = W0;
  for (int l = 0; l < 4; ++l) {
    p.base[l] = pyr[l], p.H[l] = h, p.W[l] = w;
    h /= 2, w /= 2;
  }
  return p;
}

int sampt_pips_track_workspace_bytes(sampt_pips_t h, int n, size_t* bytes) {
  if (!h || !bytes || n <= 0) return fail(SAMPT_ERR_ARG, "sampt_pips_track_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  PyramidLevels p = {};
  int rounds = 0;
  int rc = h->e.track(p, 2, n, nullptr, nullptr, nullptr, nullptr, 0.9f, 6, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                      nullptr, a, nullptr, &rounds);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_pips_track_f32(sampt_pips_t h, const float* const pyr[4], int H0, int W0, int T, int n, const float* q_dev,
                         const uint8_t* flip_dev, const float* q_host, const uint8_t* flip_host, float vis_threshold, int iters,
                         void* const* chunk_events, const int32_t* chunk_lo, const int32_t* chunk_hi, int nchunks,
                         float* traj_dev, float* vis_dev, void* ws, size_t ws_bytes, sampt_stream_t stream, int32_t* rounds) {
  if (!h || !pyr || !q_dev || !flip_dev || !q_host || !flip_host || !traj_dev || !vis_dev || !ws || !rounds || n <= 0 || T < 1 ||
      (nchunks > 0 && (!chunk_events || !chunk_lo || !chunk_hi)))
    return fail(SAMPT_ERR_ARG, "sampt_pips_track_f32: bad arguments");
  for (int i = 0; i < n; ++i)
    if (!(q_host[i * 3] >= 0.f && q_host[i * 3] <= (float)(T - 1)))
      return fail(SAMPT_ERR_ARG, "sampt_pips_track_f32: query frame outside the clip");
  // The pinned termination flags and their events belong to the handle: ONE track call at a time per handle (callers that want
  // concurrent clips create one tracker handle per stream).  Created on first use, all or nothing.
  if (!h->flag) {
    int* flag = nullptr;
    hipEvent_t evs[2] = {nullptr, nullptr};
    bool okay = hipHostMalloc((void**)&flag, 2 * sizeof(int), hipHostMallocDefault) == hipSuccess;
    for (int i = 0; okay && i < 2; ++i) okay = hipEventCreateWithFlags(&evs[i], hipEventDisableTiming) == hipSuccess;
    if (!okay) {
      for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
      if (flag) (void)hipHostFree(flag);
      return fail(SAMPT_ERR_HIP, "sampt_pips_track_f32: could not create the pinned flag / events");
    }
    h->flag = flag, h->flag_ev[0] = evs[0], h->flag_ev[1] = evs[1];
  }
  h->flag[0] = h->flag[1] = -1;
  Arena a(ws, ws_bytes);
  int r = 0;
  int rc = h->e.track(make_pyr(pyr, H0, W0), T, n, q_dev, flip_dev, q_host, flip_host, vis_threshold, iters, chunk_events,
                      (const int*)chunk_lo, (const int*)chunk_hi, nchunks, h->flag, h->flag_ev, traj_dev, vis_dev, a,
                      (hipStream_t)stream, &r);
  *rounds = r;
  if (rc != SAMPT_OK && !h->e.error.empty()) return fail(rc, h->e.error);
  return rc;
}

int sampt_pips_round_launches(sampt_pips_t h) { return h && h->e.window_launches ? h->e.window_launches + 2 : 0; }

int sampt_pips_update_workspace_bytes(sampt_pips_t h, int n, size_t* bytes) {
  if (!h || !bytes || n <= 0) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  PyramidLevels p = {};
  int rc = h->e.update(p, nullptr, n, nullptr, nullptr, 6, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_pips_update_f32(sampt_pips_t h, const float* const pyr[4], int H0, int W0, const int32_t* frame_idx, int n,
                          const float* xys, const float* feat_init, int iters, float* traj_out, float* vis_out, void* ws,
                          size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !pyr || !frame_idx || !xys || !feat_init || !traj_out || !vis_out || !ws || n <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips_update_f32: bad arguments");
  Arena a(ws, ws_bytes);
  return h->e.update(make_pyr(pyr, H0, W0), frame_idx, n, xys, feat_init, iters, traj_out, vis_out, a,
                     (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- CoTracker
int sampt_cotracker_create(const char* const* names, const void* const* ptrs, int n, int stride, int S,
                           sampt_cotracker_t* out) {
  if (!names || !ptrs || !out || S != 8 || stride != 4)
    return fail(SAMPT_ERR_ARG, "sampt_cotracker_create: bad arguments (the shipped checkpoint is stride 4, window 8)");
  return create_handle<sampt_cotracker>("sampt_cotracker_create", out, [&](sampt_cotracker& h) {
    h.e.S = S, h.e.stride = stride;
    return h.e.init(make_map(names, ptrs, n));
  });
}
void sampt_cotracker_destroy(sampt_cotracker_t h) { delete h; }

int sampt_resize_frames_f32(const void* frames, int src_u8, long planes, int H, int W, float* out, int out_h, int out_w,
                            sampt_stream_t stream) {
  if (!frames || !out || planes <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_resize_frames_f32: bad arguments (null pointer, a count <= 0 or a size above 16384)");
  return resize_planes(frames, src_u8, planes, H, W, out, out_h, out_w, (hipStream_t)stream);
}

int sampt_cotracker_fnet_workspace_bytes(sampt_cotracker_t h, int nf, int H, int W, size_t* bytes) {
  if (!h || !bytes) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  float* out[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = h->e.enc.fnet(nullptr, nf, H, W, out, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_cotracker_fnet_f32(sampt_cotracker_t h, const float* frames, int nf, int H, int W, float* const pyr[4], void* ws,
                             size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !pyr || !ws || H < 16 * h->e.stride || W < 16 * h->e.stride)
    return fail(SAMPT_ERR_ARG, "sampt_cotracker_fnet_f32: bad arguments (H, W must be at least 16*stride)");
  Arena a(ws, ws_bytes);
  return h->e.enc.fnet((const uint8_t*)frames, nf, H, W, pyr, a, (hipStream_t)stream);
}

int sampt_cotracker_track_workspace_bytes(sampt_cotracker_t h, int n, size_t* bytes) {
  if (!h || !bytes || n <= 0) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  PyramidLevels p = {};
  int rc = h->e.track(p, 8, nullptr, n, nullptr, nullptr, nullptr, nullptr, nullptr, 6, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_cotracker_track_f32(sampt_cotracker_t h, const float* const pyr[4], int H0, int W0, int T,
                              const int32_t* frame_map, int n, const int32_t* query_t_host, const int32_t* query_t,
                              const float* query_xy, const float* pos_x, const float* pos_y, int iters, float* traj_out,
                              float* vis_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !pyr || !frame_map || !query_t_host || !query_t || !query_xy || !pos_x || !pos_y || !traj_out || !vis_out ||
      !ws || n <= 0 || T < h->e.S || iters <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_cotracker_track_f32: bad arguments (T must be at least the window length 8)");
  Arena a(ws, ws_bytes);
  int rc = h->e.track(make_pyr(pyr, H0, W0), T, (const int*)frame_map, n, (const int*)query_t_host, (const int*)query_t,
                      query_xy, pos_x, pos_y, iters, traj_out, vis_out, a, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_cotracker_track_f32: query frames must be sorted ascending and inside [0, T)");
  return rc;
}

// ------------------------------------------------------------------------------------------- ViT
int sampt_vit_create(const sampt_vit_config* cfg, const char* const* names, const void* const* ptrs, int n,
                     int win_batches, sampt_vit_t* out) {
  if (!cfg || !names || !ptrs || !out || cfg->depth > 32) return fail(SAMPT_ERR_ARG, "sampt_vit_create: bad arguments");
  VitConfig c;
  c.D = cfg->embed_dim, c.depth = cfg->depth, c.heads = cfg->num_heads, c.grid = cfg->grid, c.window = cfg->window;
  c.patch = cfg->patch, c.out_chans = cfg->out_chans, c.mlp_ratio = cfg->mlp_ratio, c.img = cfg->img_size;
  c.global_mask = cfg->global_mask, c.f16 = cfg->f16;
  for (int i = 0; i < 3; ++i) c.mean[i] = cfg->pixel_mean[i], c.stdv[i] = cfg->pixel_std[i];
  return create_handle<sampt_vit>("sampt_vit_create", out,
                                  [&](sampt_vit& h) { return h.e.init(make_map(names, ptrs, n), c, win_batches); });
}
void sampt_vit_destroy(sampt_vit_t h) { delete h; }

int sampt_vit_set_gemm_workgroups(sampt_vit_t h, int per_xcd) {
  if (!h || per_xcd < 0 || per_xcd > 32) return fail(SAMPT_ERR_ARG, "sampt_vit_set_gemm_workgroups: per_xcd must be 0 .. 32");
  h->e.gemm_wgs = per_xcd;
  return SAMPT_OK;
}

int sampt_vit_set_gemm_workgroups_kind(sampt_vit_t h, int qkv, int proj, int fc1, int fc2) {
  const int v[4] = {qkv, proj, fc1, fc2};
  if (!h) return fail(SAMPT_ERR_ARG, "sampt_vit_set_gemm_workgroups_kind: null handle");
  for (int i = 0; i < 4; ++i)
    if (v[i] < 0 || v[i] > 32) return fail(SAMPT_ERR_ARG, "sampt_vit_set_gemm_workgroups_kind: counts must be 0 .. 32");
  for (int i = 0; i < 4; ++i) h->e.gemm_wgs_kind[i] = v[i];
  return SAMPT_OK;
}

int sampt_vit_set_attention_head_major(sampt_vit_t h, int on) {
  if (!h || (on != 0 && on != 1)) return fail(SAMPT_ERR_ARG, "sampt_vit_set_attention_head_major: need a handle and on = 0 | 1");
  h->e.attn_head_major = on;
  return SAMPT_OK;
}

int sampt_gemm_set_schedule(int sched) {
  if (sched < 0 || sched > 1) return fail(SAMPT_ERR_ARG, "sampt_gemm_set_schedule: 0 or 1");
  sampt::g_p8_sched = sched;
  return SAMPT_OK;
}

int sampt_gemm_set_thin_min_wgs(int n) {
  if (n < 1 || n > 4096) return fail(SAMPT_ERR_ARG, "sampt_gemm_set_thin_min_wgs: 1 .. 4096");
  sampt::g_thin_min_wgs = n;
  return SAMPT_OK;
}

int sampt_stream_create_cu_range(int cu_lo, int cu_hi, sampt_stream_t* out) {
  if (!out || cu_lo < 0 || cu_hi > 32 || cu_lo >= cu_hi) return fail(SAMPT_ERR_ARG, "sampt_stream_create_cu_range: need 0 <= cu_lo < cu_hi <= 32");
  hipDeviceProp_t p;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return fail(SAMPT_ERR_HIP, "sampt_stream_create_cu_range: no device");
  const int ncu = p.multiProcessorCount, nxcd = 8;
  if (ncu != nxcd * 32) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_stream_create_cu_range: written for 8 XCDs x 32 CUs");
  uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < ncu; ++i)              // bit i = CU i / 8 of XCD i % 8
    if (i / nxcd >= cu_lo && i / nxcd < cu_hi) mask[i / 32] |= 1u << (i % 32);
  hipStream_t s = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&s, 8, mask);
  if (e != hipSuccess) { sampt::set_error("hipExtStreamCreateWithCUMask", e); return SAMPT_ERR_HIP; }
  *out = (sampt_stream_t)s;
  return SAMPT_OK;
}

int sampt_stream_destroy(sampt_stream_t stream) {
  if (!stream) return SAMPT_OK;
  return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? SAMPT_OK : SAMPT_ERR_HIP;
}

int sampt_pips_set_mixer(int fused, int workgroups) {
  if (fused < 0 || fused > 2 || workgroups < 1 || workgroups > 1024)
    return fail(SAMPT_ERR_ARG, "sampt_pips_set_mixer: fused 0 / 1 / 2, workgroups 1 .. 1024");
  sampt::g_pips_mixer_fused = fused ? 1 : 0, sampt::g_pips_mixer_x3 = fused == 2, sampt::g_pips_mixer_wgs = workgroups;
  return SAMPT_OK;
}

int sampt_conv_set_halo(int on) {
  // 3: halo / stem kernels without the fused InstanceNorm statistics; 4: statistics from the halo kernel only; 5: from the stem only
  sampt::g_conv_in_stats = on == 3 ? 0 : (on == 4 ? 1 : (on == 5 ? 2 : 3));
  sampt::g_halo_dbg = on >= 6 && on <= 8 ? on : 0;
  sampt::g_conv_halo = on < 0 ? 0 : (on > 2 ? 1 : on);
  return SAMPT_OK;
}

int sampt_gemm_set_trim(int on) {
  sampt::g_p8_trim = on ? 1 : 0;
  return SAMPT_OK;
}

int sampt_gemm_set_wres(int on) {
  sampt::g_gemm_x3_wres = on ? 1 : 0;
  sampt::g_gemm_x3_epi = on == 2 ? 0 : 1;      // 2: the weights-resident kernel without the fused LayerNorm / dot-product tails
  return SAMPT_OK;
}

int sampt_gemm_set_stagger(int groups) {
  if (groups < 0 || groups > 8) return fail(SAMPT_ERR_ARG, "sampt_gemm_set_stagger: 0 .. 8 phase groups");
  sampt::g_p8_stagger = groups;
  return SAMPT_OK;
}

int sampt_vit_calibrate(sampt_vit_t h, float* colmeans_dev, int ld) {
  if (!h || (colmeans_dev && ld < h->e.c.mlp_ratio * h->e.c.D))
    return fail(SAMPT_ERR_ARG, "sampt_vit_calibrate: ld must be at least mlp_ratio * embed_dim");
  h->e.calib = colmeans_dev, h->e.calib_ld = colmeans_dev ? ld : 0;
  return SAMPT_OK;
}

int sampt_vit_profile_begin(sampt_vit_t h) {
  if (!h) return SAMPT_ERR_ARG;
  h->e.profiling = true;
  return SAMPT_OK;
}
int sampt_vit_profile_end(sampt_vit_t h, double* flop, double* ms, int* launches) {
  if (!h || !flop || !ms || !launches) return SAMPT_ERR_ARG;
  return h->e.profile_end(flop, ms, launches);
}

int sampt_vit_encode_workspace_bytes(sampt_vit_t h, int B, size_t* bytes) {
  if (!h || !bytes || B <= 0) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  int rc = h->e.encode(nullptr, 1, B, h->e.c.img, h->e.c.img, nullptr, nullptr, a, nullptr);
  // + the compact live-row stream of sampt_vit_encode_live (at most one more copy of the residual stream)
  *bytes = a.peak + 512 + (size_t)B * h->e.c.grid * h->e.c.grid * h->e.c.D * sizeof(float);
  return rc;
}

int sampt_vit_live_rows(sampt_vit_t h, int H, int W, int* live_rows, size_t* cache_bytes) {
  if (!h || !live_rows || !cache_bytes) return SAMPT_ERR_ARG;
  const int g = h->e.c.grid, lh = h->e.live_rows(H, W);
  *live_rows = lh;
  *cache_bytes = (size_t)(g - lh) * g * h->e.c.D * sizeof(float);
  return SAMPT_OK;
}

int sampt_vit_encode_live(sampt_vit_t h, const uint8_t* frames, int chw, int B, int H, int W, float* features,
                          float* interm_out, float* dead_cache, int build, void* ws, size_t ws_bytes,
                          sampt_stream_t stream) {
  if (!h || !frames || !dead_cache || !ws || B <= 0 || (!build && !features))
    return fail(SAMPT_ERR_ARG, "sampt_vit_encode_live: bad arguments");
  if (H > h->e.c.img || W > h->e.c.img || (H != h->e.c.img && W != h->e.c.img))
    return fail(SAMPT_ERR_UNSUPPORTED, "sampt_vit_encode_live: the frame's longest side must equal img_size");
  if (h->e.live_rows(H, W) >= h->e.c.grid)
    return fail(SAMPT_ERR_UNSUPPORTED,
                "sampt_vit_encode_live: this frame geometry has no frame-independent token rows (sampt_vit_live_rows)");
  Arena a(ws, ws_bytes);
  return h->e.encode(frames, chw, build ? 1 : B, H, W, features, interm_out, a, (hipStream_t)stream, dead_cache,
                     build ? 1 : 2);
}

int sampt_vit_encode(sampt_vit_t h, const uint8_t* frames, int chw, int B, int H, int W, float* features,
                     float* interm_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !features || !ws || B <= 0) return fail(SAMPT_ERR_ARG, "sampt_vit_encode: bad arguments");
  if (H > h->e.c.img || W > h->e.c.img || (H != h->e.c.img && W != h->e.c.img))
    return fail(SAMPT_ERR_UNSUPPORTED,
                "sampt_vit_encode: the frame's longest side must equal img_size (resize before SamPt, as the reference "
                "pipelines do)");
  Arena a(ws, ws_bytes);
  return h->e.encode(frames, chw, B, H, W, features, interm_out, a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- TinyViT
int sampt_tinyvit_create(const sampt_tinyvit_config* cfg, const char* const* names, const void* const* ptrs, int n, int max_batch,
                         sampt_tinyvit_t* out) {
  if (!cfg || !names || !ptrs || !out || n < 1 || max_batch < 1) return fail(SAMPT_ERR_ARG, "sampt_tinyvit_create: bad arguments");
  TinyVitConfig c;
  c.img = cfg->img_size, c.out_chans = cfg->out_chans, c.mlp_ratio = cfg->mlp_ratio, c.expand = cfg->mbconv_expand_ratio;
  for (int i = 0; i < 4; ++i)
    c.dims[i] = cfg->embed_dims[i], c.depths[i] = cfg->depths[i], c.heads[i] = cfg->num_heads[i], c.windows[i] = cfg->window_sizes[i];
  for (int i = 0; i < 3; ++i) c.mean[i] = cfg->pixel_mean[i], c.stdv[i] = cfg->pixel_std[i];
  return create_handle<sampt_tinyvit>("sampt_tinyvit_create", out,
                                      [&](sampt_tinyvit& h) { return h.e.init(make_map(names, ptrs, n), c, max_batch); });
}
void sampt_tinyvit_destroy(sampt_tinyvit_t h) { delete h; }

int sampt_tinyvit_encode_workspace_bytes(sampt_tinyvit_t h, int B, size_t* bytes) {
  if (!h || !bytes || B < 1) return fail(SAMPT_ERR_ARG, "sampt_tinyvit_encode_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  int rc = h->e.encode(nullptr, 1, B, h->e.c.img, h->e.c.img, nullptr, nullptr, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_tinyvit_encode_workspace_bytes: " + h->e.error);
}

int sampt_tinyvit_encode_stages(sampt_tinyvit_t h, const uint8_t* frames, int chw, int B, int H, int W, float* features, float* interm_out,
                                float* const stages[5], float* stage_ms, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !features || !ws || B < 1) return fail(SAMPT_ERR_ARG, "sampt_tinyvit_encode: bad arguments");
  // the engine carves its scratch stage by stage between launches, so the size is checked before the first one
  Arena dry(nullptr, 0);
  int rc = h->e.encode(nullptr, chw, B, H, W, nullptr, nullptr, nullptr, nullptr, dry, nullptr);
  if (rc != SAMPT_OK) return fail(rc, "sampt_tinyvit_encode: " + h->e.error);
  if (dry.peak + 256 > ws_bytes) return fail(SAMPT_ERR_WORKSPACE, "sampt_tinyvit_encode: workspace too small (sampt_tinyvit_encode_workspace_bytes)");
  Arena a(ws, ws_bytes);
  if (!stage_ms) return h->e.encode(frames, chw, B, H, W, features, interm_out, stages, nullptr, a, (hipStream_t)stream);
  hipEvent_t ev[7] = {};
  rc = SAMPT_OK;
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) rc = SAMPT_ERR_HIP;
  if (rc == SAMPT_OK) rc = h->e.encode(frames, chw, B, H, W, features, interm_out, stages, ev, a, (hipStream_t)stream);
  if (rc == SAMPT_OK && hipEventSynchronize(ev[6]) != hipSuccess) rc = SAMPT_ERR_HIP;
  for (int i = 0; i < 6 && rc == SAMPT_OK; ++i)
    if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = SAMPT_ERR_HIP;
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int sampt_tinyvit_encode(sampt_tinyvit_t h, const uint8_t* frames, int chw, int B, int H, int W, float* features, float* interm_out,
                         void* ws, size_t ws_bytes, sampt_stream_t stream) {
  return sampt_tinyvit_encode_stages(h, frames, chw, B, H, W, features, interm_out, nullptr, nullptr, ws, ws_bytes, stream);
}

int sampt_tinyvit_preprocess(const uint8_t* frames, int chw, int B, int H, int W, int img_size, const float* mean, const float* std_,
                             float* out, sampt_stream_t stream) {
  int rc = tinyvit_preprocess(frames, chw, B, H, W, img_size, mean, std_, out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tinyvit_preprocess: bad arguments (H, W <= img_size)") : rc;
}

int sampt_tinyvit_dwconv3x3_nhwc(const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int C, int stride, int gelu,
                                 sampt_stream_t stream) {
  int rc = tinyvit_dwconv3x3(x, w, bias, y, n, H, W, C, stride, gelu, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tinyvit_dwconv3x3_nhwc: bad arguments (C % 32 == 0, stride 1 | 2, 16-byte aligned pointers)") : rc;
}

int sampt_tinyvit_window_attention_f32(const float* qkv, const float* table, const float* pad_qkv, float* out, int B, int H, int W, int heads,
                                       int ws, sampt_stream_t stream) {
  int rc = tinyvit_window_attention(qkv, table, pad_qkv, out, B, H, W, heads, ws, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tinyvit_window_attention_f32: bad arguments (ws <= 14, 16-byte aligned pointers)") : rc;
}

// ------------------------------------------------------------------------------------------- PIPS++
int sampt_pips2_create(const char* const* names, const void* const* ptrs, int n, int stride, sampt_pips2_t* out) {
  if (!names || !ptrs || !out || stride <= 0) return fail(SAMPT_ERR_ARG, "sampt_pips2_create: bad arguments");
  return create_handle<sampt_pips2>("sampt_pips2_create", out,
                                    [&](sampt_pips2& h) { return h.e.init(make_map(names, ptrs, n), stride); });
}
void sampt_pips2_destroy(sampt_pips2_t h) { delete h; }

int sampt_pips2_fnet_workspace_bytes(sampt_pips2_t h, int nf, int H, int W, size_t* bytes) {
  if (!h || !bytes) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  float* out[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = h->e.enc.fnet(nullptr, nf, H, W, out, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_pips2_fnet_f32(sampt_pips2_t h, const void* frames, int frames_are_f32, int nf, int H, int W,
                         float* const pyr[4], void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !pyr || !ws || H < 16 * h->e.stride || W < 16 * h->e.stride)
    return fail(SAMPT_ERR_ARG, "sampt_pips2_fnet_f32: bad arguments (H, W must be at least 16*stride)");
  Arena a(ws, ws_bytes);
  h->e.enc.frames_f32 = frames_are_f32 ? 1 : 0;
  return h->e.enc.fnet((const uint8_t*)frames, nf, H, W, pyr, a, (hipStream_t)stream);
}

int sampt_pips2_update_workspace_bytes(sampt_pips2_t h, int n, int S, size_t* bytes) {
  if (!h || !bytes || n <= 0 || S <= 0) return SAMPT_ERR_ARG;
  Arena a(nullptr, 0);
  PyramidLevels p = {};
  float* feats[3] = {nullptr, nullptr, nullptr};
  int rc = h->e.update(p, nullptr, n, S, nullptr, 0, feats, 1, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

static PyramidLevels make_pyr(const float* const pyr[4], int H0, int W0);

int sampt_pips2_update_f32(sampt_pips2_t h, const float* const pyr[4], int H0, int W0, const int32_t* frame_idx, int n,
                           int S, const float* trajs0, int have_feat_init, float* const feats[3], int iters,
                           float* trajs_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !pyr || !frame_idx || !trajs0 || !feats || !feats[0] || !feats[1] || !feats[2] || !trajs_out || !ws ||
      n <= 0 || S <= 0 || iters <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips2_update_f32: bad arguments");
  Arena a(ws, ws_bytes);
  return h->e.update(make_pyr(pyr, H0, W0), (const int*)frame_idx, n, S, trajs0, have_feat_init, feats, iters, trajs_out,
                     a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- RAFT
static int raft_bad_size(const char* who, int H, int W) {
  const int Hp = (H + 7) / 8 * 8, Wp = (W + 7) / 8 * 8;
  if (Hp >= 128 && Wp >= 128) return SAMPT_OK;
  return fail(SAMPT_ERR_UNSUPPORTED, std::string(who) + ": RAFT needs frames of at least 128 pixels on both sides after padding to "
              "multiples of 8 (the coarsest of the 4 correlation levels must keep 2 x 2 cells); got " + std::to_string(H) + " x " +
              std::to_string(W) + " padded to " + std::to_string(Hp) + " x " + std::to_string(Wp));
}

int sampt_raft_create(const char* const* names, const void* const* ptrs, int n, sampt_raft_t* out) {
  if (!names || !ptrs || !out) return fail(SAMPT_ERR_ARG, "sampt_raft_create: bad arguments");
  return create_handle<sampt_raft>("sampt_raft_create", out, [&](sampt_raft& h) { return h.e.init(make_map(names, ptrs, n)); });
}
void sampt_raft_destroy(sampt_raft_t h) { delete h; }

int sampt_raft_workspace_bytes(sampt_raft_t h, int T, int H, int W, int max_pairs_in_flight, size_t* bytes) {
  if (!h || !bytes || T < 1 || H < 1 || W < 1 || max_pairs_in_flight < 1) return fail(SAMPT_ERR_ARG, "sampt_raft_workspace_bytes: bad arguments");
  SAMPT_TRY(raft_bad_size("sampt_raft_workspace_bytes", H, W));
  Arena a(nullptr, 0);
  int rc = h->e.flows(nullptr, T, H, W, 1, nullptr, nullptr, nullptr, max_pairs_in_flight, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_raft_flows_f32(sampt_raft_t h, const uint8_t* frames, int T, int H, int W, int iters, float* flows_fwd, float* flows_bwd,
                         float* flow_low, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || T < 1 || H < 1 || W < 1 || iters < 1 || !ws || (T > 1 && (!flows_fwd || !flows_bwd)))
    return fail(SAMPT_ERR_ARG, "sampt_raft_flows_f32: bad arguments");
  SAMPT_TRY(raft_bad_size("sampt_raft_flows_f32", H, W));
  if (T == 1) return SAMPT_OK;
  const int np = h->e.plan_pairs(T, H, W, T - 1, ws_bytes);
  if (np < 1) return fail(SAMPT_ERR_WORKSPACE, "sampt_raft_flows_f32: the workspace does not hold one pair (sampt_raft_workspace_bytes)");
  Arena a(ws, ws_bytes);
  return h->e.flows(frames, T, H, W, iters, flows_fwd, flows_bwd, flow_low, np, a, (hipStream_t)stream);
}

int sampt_raft_chain(const float* flows_fwd, const float* flows_bwd, int T, int H, int W, const float* q, int n, float* traj,
                     uint8_t* vis, sampt_stream_t stream) {
  int rc = raft_chain(flows_fwd, flows_bwd, T, H, W, q, n, traj, vis, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_raft_chain: bad arguments") : rc;
}

// ------------------------------------------------------------------------------------------- TAPIR
int sampt_tapir_create(const char* const* names, const void* const* ptrs, int n, sampt_tapir_t* out) {
  if (!names || !ptrs || !out || n < 1) return fail(SAMPT_ERR_ARG, "sampt_tapir_create: bad arguments");
  return create_handle<sampt_tapir>("sampt_tapir_create", out, [&](sampt_tapir& h) { return h.e.init(make_map(names, ptrs, n)); });
}
void sampt_tapir_destroy(sampt_tapir_t h) { delete h; }

int sampt_tapir_workspace_bytes(sampt_tapir_t h, int T, int n, int max_queries_in_flight, size_t* bytes) {
  if (!h || !bytes || T < 1 || n < 1 || max_queries_in_flight < 1) return fail(SAMPT_ERR_ARG, "sampt_tapir_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  int rc = h->e.track(nullptr, T, nullptr, n, 1, nullptr, nullptr, nullptr, nullptr, max_queries_in_flight, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_tapir_track_f32(sampt_tapir_t h, const float* frames, int T, const float* q, int n, int iters, float* tracks, float* occ,
                          float* expd, float* iter_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !q || !tracks || !occ || !expd || !ws || T < 1 || n < 1 || iters < 0)
    return fail(SAMPT_ERR_ARG, "sampt_tapir_track_f32: bad arguments");
  int qc = h->e.plan_queries(T, n, ws_bytes);
  if (qc < 1) return fail(SAMPT_ERR_WORKSPACE, "sampt_tapir_track_f32: the workspace does not hold one query (sampt_tapir_workspace_bytes)");
  if (h->max_queries > 0) qc = std::min(qc, h->max_queries);
  Arena a(ws, ws_bytes);
  return h->e.track(frames, T, q, n, iters, tracks, occ, expd, iter_out, qc, a, (hipStream_t)stream);
}

int sampt_tapir_launches(sampt_tapir_t h) { return h ? h->e.launches : 0; }

int sampt_tapir_set_max_queries(sampt_tapir_t h, int max_queries) {
  if (!h || max_queries < 0) return fail(SAMPT_ERR_ARG, "sampt_tapir_set_max_queries: bad arguments");
  h->max_queries = max_queries;
  return SAMPT_OK;
}

int sampt_tapir_backbone_workspace_bytes(sampt_tapir_t h, int nf, size_t* bytes) {
  if (!h || !bytes || nf < 1) return fail(SAMPT_ERR_ARG, "sampt_tapir_backbone_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  int rc = h->e.backbone(nullptr, nf, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_tapir_backbone_f32(sampt_tapir_t h, const float* frames, int nf, float* hires, float* lowres, void* ws, size_t ws_bytes,
                             sampt_stream_t stream) {
  if (!h || !frames || !hires || !lowres || !ws || nf < 1) return fail(SAMPT_ERR_ARG, "sampt_tapir_backbone_f32: bad arguments");
  Arena a(ws, ws_bytes);
  return h->e.backbone(frames, nf, hires, lowres, a, (hipStream_t)stream);
}

int sampt_tapir_query_feats_f32(const float* hires, const float* lowres, int T, const float* q, int n, float* qf, sampt_stream_t stream) {
  int rc = tapir_query_feats(hires, lowres, T, q, n, qf, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapir_query_feats_f32: bad arguments") : rc;
}

int sampt_tapir_heads_f32(const float* lowres, int T, const float* qf, int ldq, int qoff, const float* q, int n, const float* const weights[10],
                          float* points, float* occ, float* expd, sampt_stream_t stream) {
  if (!weights) return fail(SAMPT_ERR_ARG, "sampt_tapir_heads_f32: bad arguments");
  const TapirHeadW w{weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7], weights[8], weights[9]};
  int rc = tapir_heads(lowres, T, qf, ldq, qoff, q, n, w, points, occ, expd, nullptr, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapir_heads_f32: bad arguments") : rc;
}

int sampt_tapir_patch_corr_f32(const float* hires, const float* lowres, int T, int n, const float* pos, const float* occ, const float* expd,
                               const float* feat, int feat_per_row, float* x, int ldx, sampt_stream_t stream) {
  int rc = tapir_patch_corr(hires, lowres, T, n, pos, occ, expd, feat, feat_per_row, x, ldx, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapir_patch_corr_f32: bad arguments") : rc;
}

int sampt_tapir_temporal_mix_f32(const float* x, float* xo, const float* ln, const float* w1, const float* b1, const float* w2, const float* b2,
                                 int n, int T, sampt_stream_t stream) {
  int rc = tapir_temporal_mix(x, xo, ln, w1, b1, w2, b2, n, T, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapir_temporal_mix_f32: bad arguments") : rc;
}

int sampt_tapir_gemm_f32(const float* A, const float* W, const float* bias, const float* res, float* C, int M, int N, int K, int act,
                         sampt_stream_t stream) {
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_GELU_TANH) return fail(SAMPT_ERR_ARG, "sampt_tapir_gemm_f32: act must be 0, 1 or 3");
  int rc = tapir_gemm(A, K, W, bias, C, N, M, N, K, act, res, N, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapir_gemm_f32: bad arguments (K % 16 == 0, N % 4 == 0, 16-byte aligned pointers)") : rc;
}

int sampt_conv2d_same_nhwc(int dtype, const void* x, const void* w, float* y, int n, int H, int W, int Cin, int Cout, int K, int stride,
                           sampt_stream_t stream) {
  if (!x || !w || !y || n < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || K < 1 || stride < 1 || (dtype != 0 && dtype != 3 && dtype != 4))
    return fail(SAMPT_ERR_ARG, "sampt_conv2d_same_nhwc: bad arguments");
  ConvW c;
  c.w = (const float*)w, c.cin = Cin, c.cout = Cout, c.kh = c.kw = K, c.stride = stride;
  same_padding(H, K, stride, c.ph, c.ph_after);
  same_padding(W, K, stride, c.pw, c.pw_after);
  if (c.pw != c.ph) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_conv2d_same_nhwc: the padding before must be the same on both axes");
  GemmP p = gemm_conv(c, x, n, H, W, y);
  if (dtype == 0) return gemm_f32(p, (hipStream_t)stream);
  gemm_split_planes(p, (const half_t*)w);
  if (dtype == 4) p.A_lo = (const half_t*)x + (size_t)n * H * W * Cin;
  return conv_f16x3(p, (hipStream_t)stream);
}

int sampt_instance_norm_affine_nhwc(const float* x, const float* scale, const float* offset, float* y, void* y_hl, int n, int hw, int C,
                                    float eps, int relu, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!x || !scale || !offset || (!y && !y_hl) || !ws || n < 1 || hw < 1 || C < 4 || C % 4)
    return fail(SAMPT_ERR_ARG, "sampt_instance_norm_affine_nhwc: bad arguments");
  if (ws_bytes < sampt_instance_norm_workspace_bytes(n, hw, C))
    return fail(SAMPT_ERR_WORKSPACE, "sampt_instance_norm_affine_nhwc: workspace too small (sampt_instance_norm_workspace_bytes)");
  Arena a(ws, ws_bytes);
  double* part = (double*)a.get(instnorm_partial_doubles(n, hw, C) * sizeof(double));
  float* mr = a.f32((size_t)n * C * 2);
  SAMPT_TRY(instnorm_stats(x, n, hw, C, eps, part, mr, (hipStream_t)stream));
  half_t* hi = (half_t*)y_hl;
  return instnorm_affine_apply(x, mr, scale, offset, y, n, hw, C, relu, (hipStream_t)stream, hi, hi ? hi + (size_t)n * hw * C : nullptr);
}

// ------------------------------------------------------------------------------------------- TapNet
int sampt_tapnet_create(const char* const* names, const void* const* ptrs, int n, sampt_tapnet_t* out) {
  if (!names || !ptrs || !out || n < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_create: bad arguments");
  return create_handle<sampt_tapnet>("sampt_tapnet_create", out, [&](sampt_tapnet& h) { return h.e.init(make_map(names, ptrs, n)); });
}
void sampt_tapnet_destroy(sampt_tapnet_t h) { delete h; }

int sampt_tapnet_workspace_bytes(sampt_tapnet_t h, int T, int n, size_t* bytes) {
  if (!h || !bytes || T < 1 || n < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  int rc = h->e.track(nullptr, T, nullptr, n, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc == SAMPT_OK ? rc : fail(rc, ("sampt_tapnet_workspace_bytes: " + h->e.error).c_str());
}

int sampt_tapnet_track_f32(sampt_tapnet_t h, const float* frames, int T, const float* q, int n, float* tracks, float* occ, void* ws,
                           size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !q || !tracks || !occ || !ws || T < 1 || n < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_track_f32: bad arguments");
  Arena dry(nullptr, 0);
  int rc = h->e.track(nullptr, T, nullptr, n, nullptr, nullptr, dry, nullptr);
  if (rc != SAMPT_OK) return fail(rc, ("sampt_tapnet_track_f32: " + h->e.error).c_str());
  if (dry.peak + 256 > ws_bytes) return fail(SAMPT_ERR_WORKSPACE, "sampt_tapnet_track_f32: workspace too small (sampt_tapnet_workspace_bytes)");
  Arena a(ws, ws_bytes);
  return h->e.track(frames, T, q, n, tracks, occ, a, (hipStream_t)stream);
}

int sampt_tapnet_launches(sampt_tapnet_t h) { return h ? h->e.launches : 0; }

int sampt_tapnet_set_stem_chunk(sampt_tapnet_t h, int frames) {
  if (!h || frames < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_set_stem_chunk: bad arguments");
  h->e.stem_chunk = frames;
  return SAMPT_OK;
}

int sampt_tapnet_backbone_workspace_bytes(sampt_tapnet_t h, int nf, size_t* bytes) {
  if (!h || !bytes || nf < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_backbone_workspace_bytes: bad arguments");
  Arena a(nullptr, 0);
  int rc = h->e.backbone(nullptr, nf, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc == SAMPT_OK ? rc : fail(rc, ("sampt_tapnet_backbone_workspace_bytes: " + h->e.error).c_str());
}

int sampt_tapnet_backbone_f32(sampt_tapnet_t h, const float* frames, int nf, float* grid, float* const stages[4], void* ws, size_t ws_bytes,
                              sampt_stream_t stream) {
  if (!h || !frames || !grid || !ws || nf < 1) return fail(SAMPT_ERR_ARG, "sampt_tapnet_backbone_f32: bad arguments");
  Arena dry(nullptr, 0);
  int rc = h->e.backbone(nullptr, nf, nullptr, nullptr, dry, nullptr);
  if (rc != SAMPT_OK) return fail(rc, ("sampt_tapnet_backbone_f32: " + h->e.error).c_str());
  if (dry.peak + 256 > ws_bytes) return fail(SAMPT_ERR_WORKSPACE, "sampt_tapnet_backbone_f32: workspace too small (sampt_tapnet_backbone_workspace_bytes)");
  Arena a(ws, ws_bytes);
  h->e.launches = 0;
  return h->e.backbone(frames, nf, grid, stages, a, (hipStream_t)stream);
}

int sampt_tapnet_bn_shift_f32(const float* x, const float* a, const float* b, int T, int hw, int C, int n_shift, float* shifted,
                              void* shifted_hl, float* unshifted, void* unshifted_hl, sampt_stream_t stream) {
  if (!x || !a || !b || (!shifted && !shifted_hl) || T < 1 || hw < 1 || C < 4) return fail(SAMPT_ERR_ARG, "sampt_tapnet_bn_shift_f32: bad arguments");
  const size_t el = (size_t)T * hw * C;
  half_t *sh = (half_t*)shifted_hl, *uh = (half_t*)unshifted_hl;
  int rc = tapnet_bn_shift(x, a, b, T, hw, C, n_shift, shifted, sh, sh ? sh + el : nullptr, unshifted, uh, uh ? uh + el : nullptr,
                           (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapnet_bn_shift_f32: bad arguments (C % 4 == 0, n_shift % 4 == 0, 2 n_shift <= C)") : rc;
}

int sampt_tapnet_maxpool_nhwc(const float* x, float* y, int n, int H, int W, int C, sampt_stream_t stream) {
  int rc = tapnet_maxpool(x, y, n, H, W, C, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapnet_maxpool_nhwc: bad arguments (C % 4 == 0)") : rc;
}

int sampt_tapnet_query_feats_f32(const float* grid, int T, const float* q, int n, float* qf, sampt_stream_t stream) {
  int rc = tapnet_query_feats(grid, T, q, n, qf, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapnet_query_feats_f32: bad arguments") : rc;
}

int sampt_tapnet_heads_f32(const float* grid, int T, const float* qf, const float* q, int n, const float* const weights[10], float* points,
                           float* occ, sampt_stream_t stream) {
  if (!weights) return fail(SAMPT_ERR_ARG, "sampt_tapnet_heads_f32: bad arguments");
  const TapirHeadW w{weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6], weights[7], weights[8], weights[9]};
  int rc = tapnet_heads(grid, T, qf, q, n, w, points, occ, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_tapnet_heads_f32: bad arguments") : rc;
}

// ------------------------------------------------------------------------------------------- SuperGlue tracker
int sampt_sg_create(const char* const* names, const void* const* ptrs, int n, sampt_sg_t* out) {
  if (!names || !ptrs || !out) return fail(SAMPT_ERR_ARG, "sampt_sg_create: bad arguments");
  return create_handle<sampt_sg>("sampt_sg_create", out, [&](sampt_sg& h) { return h.e.init(make_map(names, ptrs, n)); });
}
void sampt_sg_destroy(sampt_sg_t h) { delete h; }

int sampt_sg_workspace_bytes(sampt_sg_t h, int T, int H, int W, int n0, int n1, size_t* detect_bytes, size_t* match_bytes) {
  if (!h || T < 1 || H < 8 || W < 8 || n0 < 0 || n1 < 0) return fail(SAMPT_ERR_ARG, "sampt_sg_workspace_bytes: bad arguments");
  if (detect_bytes) {
    Arena a(nullptr, 0);
    SgDetectCfg c;
    c.cap = 1;
    SAMPT_TRY(h->e.detect(nullptr, T, H, W, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a, nullptr));
    *detect_bytes = a.peak + 256;
  }
  if (match_bytes) {
    Arena a(nullptr, 0);
    SAMPT_TRY(h->e.match(nullptr, nullptr, nullptr, n0, nullptr, nullptr, nullptr, n1, H, W, 1, 0.f, nullptr, nullptr, nullptr, nullptr,
                         nullptr, a, nullptr));
    *match_bytes = a.peak + 256;
  }
  return SAMPT_OK;
}

static int sg_capacity(const char* who, const int* counts_host, int n, int cap) {
  for (int i = 0; i < n; ++i)
    if (counts_host[i] > cap)
      return fail(SAMPT_ERR_CAPACITY, std::string(who) + ": image " + std::to_string(i) + " has " + std::to_string(counts_host[i]) +
                                          " keypoints, the capacity is " + std::to_string(cap));
  return SAMPT_OK;
}

int sampt_sg_detect(sampt_sg_t h, const uint8_t* frames, int T, int H, int W, int nms_radius, float keypoint_threshold,
                    int remove_borders, int cap, float* kpts, float* kscores, float* desc, int32_t* counts_dev, int32_t* counts_host,
                    float* dense, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !frames || !kpts || !kscores || !desc || !counts_dev || !counts_host || !ws || T < 1 || H < 8 || W < 8 || cap < 1 ||
      nms_radius < 0)
    return fail(SAMPT_ERR_ARG, "sampt_sg_detect: bad arguments");
  SgDetectCfg c;
  c.nms_radius = nms_radius, c.threshold = keypoint_threshold, c.border = remove_borders, c.cap = cap;
  Arena a(ws, ws_bytes);
  int rc = h->e.detect(frames, T, H, W, c, kpts, kscores, desc, counts_dev, counts_host, dense, a, (hipStream_t)stream);
  if (rc == SAMPT_ERR_CAPACITY) return sg_capacity("sampt_sg_detect", counts_host, T, cap);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_sg_detect: workspace too small (sampt_sg_workspace_bytes)");
  if (rc == SAMPT_ERR_UNSUPPORTED) return fail(rc, "sampt_sg_detect: nms_radius above 16 or more than 4096 score rows");
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_detect: bad arguments") : rc;
}

int sampt_sg_match(sampt_sg_t h, const float* kp0, const float* sc0, const float* d0, int n0, const float* kp1, const float* sc1,
                   const float* d1, int n1, int H, int W, int iters, float thr, int32_t* matches0, float* mscores0, float* gnn_out,
                   float* scores_out, float* uv_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || n0 < 0 || n1 < 0 || iters < 0 || H < 1 || W < 1 || (n0 > 0 && (!matches0 || !mscores0)))
    return fail(SAMPT_ERR_ARG, "sampt_sg_match: bad arguments");
  if (n0 > 0 && n1 > 0 && (!kp0 || !sc0 || !d0 || !kp1 || !sc1 || !d1 || !ws)) return fail(SAMPT_ERR_ARG, "sampt_sg_match: null pointer");
  if (n0 == 0 || n1 == 0) return sg_no_match(n0, matches0, mscores0, (hipStream_t)stream);   // no workspace, no kernel
  Arena a(ws, ws_bytes);
  int rc = h->e.match(kp0, sc0, d0, n0, kp1, sc1, d1, n1, H, W, iters, thr, matches0, mscores0, gnn_out, scores_out, uv_out, a,
                      (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_sg_match: workspace too small (sampt_sg_workspace_bytes)");
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_match: bad arguments") : rc;
}

size_t sampt_sg_nms_workspace_bytes(int nimg, int Hs, int Ws) {
  return (nimg < 1 || Hs < 1 || Ws < 1) ? 0 : sg_nms_workspace_bytes(nimg, Hs, Ws);
}

int sampt_sg_nms(const float* scores, int nimg, int Hs, int Ws, int nms_radius, float keypoint_threshold, int remove_borders, int cap,
                 float* kpts, float* kscores, int32_t* counts_dev, int32_t* counts_host, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!counts_host) return fail(SAMPT_ERR_ARG, "sampt_sg_nms: bad arguments");
  int rc = sg_nms_compact(scores, nimg, Hs, Ws, nms_radius, keypoint_threshold, remove_borders, cap, kpts, kscores, counts_dev, ws,
                          ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_sg_nms: bad arguments");
  if (rc == SAMPT_ERR_UNSUPPORTED) return fail(rc, "sampt_sg_nms: nms_radius above 16 or more than 4096 rows");
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_sg_nms: workspace too small (sampt_sg_nms_workspace_bytes)");
  if (rc != SAMPT_OK) return rc;
  if (hipMemcpyAsync(counts_host, counts_dev, (size_t)nimg * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return fail(SAMPT_ERR_HIP, "sampt_sg_nms: copying the counts failed");
  return sg_capacity("sampt_sg_nms", counts_host, nimg, cap);
}

int sampt_sg_sample_descriptors(const float* dmap, int h8, int w8, const float* kpts, int n, float* out, sampt_stream_t stream) {
  if (n == 0) return SAMPT_OK;
  int rc = n < 0 ? SAMPT_ERR_ARG : sg_sample_descriptors(dmap, 1, h8, w8, kpts, nullptr, n, n, out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_sample_descriptors: bad arguments") : rc;
}

int sampt_sg_attention(const float* q, const float* k, const float* v, float* out, int N, int M, int heads, sampt_stream_t stream) {
  int rc = sg_attention(q, heads * 64, k, v, heads * 64, out, heads * 64, N, M, heads, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_attention: bad arguments (N, M, heads >= 1)") : rc;
}

int sampt_sg_sinkhorn(const float* scores, int N, int M, const float* bin, int iters, float* u, float* v, sampt_stream_t stream) {
  int rc = sg_sinkhorn(scores, M, N, M, bin, iters, u, v, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_sinkhorn: bad arguments (N, M >= 1)") : rc;
}

int sampt_sg_mutual_match(const float* scores, int N, int M, const float* u, const float* v, float thr, int32_t* matches0,
                          float* mscores0, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (N < 0 || M < 0) return fail(SAMPT_ERR_ARG, "sampt_sg_mutual_match: bad arguments");
  if (N == 0 || M == 0) return sg_no_match(N, matches0, mscores0, (hipStream_t)stream);
  if (!ws || ws_bytes < ((size_t)2 * N + M) * 4) return fail(SAMPT_ERR_WORKSPACE, "sampt_sg_mutual_match: workspace of (2 N + M) * 4 bytes");
  float* max0 = (float*)ws;
  int* idx0 = (int*)ws + N;
  int* idx1 = idx0 + N;
  int rc = sg_match_from_scores(scores, M, N, M, u, v, thr, max0, idx0, idx1, matches0, mscores0, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_mutual_match: bad arguments") : rc;
}

int sampt_sg_select(const int32_t* matches0, int n0, const float* kpts1, const float* masks, int n_masks, int H, int W, int cap,
                    int32_t* lists, int32_t* counts, sampt_stream_t stream) {
  int rc = sg_select_lists(matches0, n0, kpts1, masks, n_masks, H, W, cap, lists, counts, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_select: bad arguments") : rc;
}

int sampt_sg_gather(const float* query_xy, const float* kpts, int kp_cap, const int32_t* lists, int list_cap, const int32_t* counts,
                    const int32_t* draw, int T, int n_masks, int n_pos, int n_neg, float* traj, float* vis, sampt_stream_t stream) {
  int rc = sg_gather(query_xy, kpts, kp_cap, lists, list_cap, counts, draw, T, n_masks, n_pos, n_neg, traj, vis, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_sg_gather: bad arguments") : rc;
}

static void raft_level_sizes(int h8, int w8, int lh[4], int lw[4]) {
  lh[0] = h8, lw[0] = w8;
  for (int l = 1; l < 4; ++l) lh[l] = lh[l - 1] / 2, lw[l] = lw[l - 1] / 2;
}

size_t sampt_raft_corr_pyramid_workspace_bytes(int h8, int w8) {
  if (h8 < 1 || w8 < 1) return 0;
  int lh[4], lw[4];
  raft_level_sizes(h8, w8, lh, lw);
  size_t b = 256;
  for (int l = 1; l < 4; ++l) b += (size_t)lh[l] * lw[l] * 256 * 4 + 256;
  return b;
}

int sampt_raft_corr_pyramid(const float* fmap1, const float* fmap2, int h8, int w8, float* const levels[4], void* ws, size_t ws_bytes,
                            sampt_stream_t stream) {
  if (!fmap1 || !fmap2 || !levels || !ws || h8 < 8 || w8 < 8 || !levels[0] || !levels[1] || !levels[2] || !levels[3])
    return fail(SAMPT_ERR_ARG, "sampt_raft_corr_pyramid: bad arguments (the coarse grid must be at least 8 x 8)");
  if (ws_bytes < sampt_raft_corr_pyramid_workspace_bytes(h8, w8)) return fail(SAMPT_ERR_WORKSPACE, "sampt_raft_corr_pyramid: workspace too small");
  int lh[4], lw[4];
  raft_level_sizes(h8, w8, lh, lw);
  Arena a(ws, ws_bytes);
  const float* pooled[4] = {fmap2, nullptr, nullptr, nullptr};
  long s2[4] = {0, 0, 0, 0};
  for (int l = 1; l < 4; ++l) {
    float* p = a.f32((size_t)lh[l] * lw[l] * 256);
    SAMPT_TRY(avgpool2x2_nhwc(pooled[l - 1], 1, lh[l - 1], lw[l - 1], 256, p, (hipStream_t)stream));
    pooled[l] = p;
  }
  return raft_corr_levels(fmap1, 0, pooled, s2, 1, h8, w8, levels, (hipStream_t)stream);
}

int sampt_raft_lookup(const float* const levels[4], int h8, int w8, const float* coords, long m, float* out, sampt_stream_t stream) {
  if (!levels || h8 < 8 || w8 < 8 || m < 1) return fail(SAMPT_ERR_ARG, "sampt_raft_lookup: bad arguments (the coarse grid must be at least 8 x 8)");
  RaftLevels lv;
  int lh[4], lw[4];
  raft_level_sizes(h8, w8, lh, lw);
  for (int l = 0; l < 4; ++l) lv.base[l] = levels[l], lv.h[l] = lh[l], lv.w[l] = lw[l];
  int rc = raft_lookup(lv, coords, m, out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_raft_lookup: bad arguments") : rc;
}

int sampt_raft_upsample(const float* flow_low, const float* mask, float mask_scale, int pairs, int h8, int w8, int H, int W, float* out,
                        sampt_stream_t stream) {
  int rc = raft_upsample(flow_low, mask, mask_scale, h8, w8, H, W, 0, pairs, out, nullptr, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_raft_upsample: bad arguments") : rc;
}

// ------------------------------------------------------------------------------------------- decoder
int sampt_dec_create(const char* const* names, const void* const* ptrs, int n, int grid, int img_size, int max_frames,
                     int vit_dim, sampt_dec_t* out) {
  if (!names || !ptrs || !out || max_frames <= 0 || vit_dim < 0)
    return fail(SAMPT_ERR_ARG, "sampt_dec_create: bad arguments");
  DecConfig c;
  c.grid = grid, c.img = img_size, c.vit_dim = vit_dim;
  return create_handle<sampt_dec>("sampt_dec_create", out, [&](sampt_dec& h) {
    h.e.max_frames = max_frames;
    return h.e.init(make_map(names, ptrs, n), c);
  });
}
void sampt_dec_destroy(sampt_dec_t h) { delete h; }

int sampt_dec_set_batch_invariant(sampt_dec_t h, int on) {
  if (!h || on < 0 || on > 1) return fail(SAMPT_ERR_ARG, "sampt_dec_set_batch_invariant: null handle, or a value other than 0 / 1");
  h->e.batch_invariant = on != 0;     // (captured graphs are keyed by the mode: none is replayed across a change)
  return SAMPT_OK;
}

int sampt_dec_workspace_bytes_k(sampt_dec_t h, int frames, int k, int oh, int ow, size_t* bytes) {
  if (!h || !bytes) return fail(SAMPT_ERR_ARG, "sampt_dec_workspace_bytes_k: null handle / output");
  if (frames <= 0 || frames > h->e.max_frames)
    return fail(SAMPT_ERR_ARG, "sampt_dec_workspace_bytes_k: frames " + std::to_string(frames) + " outside 1.." +
                                   std::to_string(h->e.max_frames) + " (max_frames of sampt_dec_create)");
  if (k < 0 || k > SAMPT_DEC_MAX_POINTS)
    return fail(SAMPT_ERR_ARG, "sampt_dec_workspace_bytes_k: k = " + std::to_string(k) + " prompt points outside 0.." +
                                   std::to_string(SAMPT_DEC_MAX_POINTS) + " (SAMPT_DEC_MAX_POINTS)");
  Arena a(nullptr, 0);
  float dummy = 0.f;
  int rc = h->e.track_decode(frames, &dummy, h->e.is_hq() ? &dummy : nullptr, &dummy, nullptr, k, nullptr, nullptr, k, 0, 1, 0.f, oh, ow,
                             oh, ow, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_dec_workspace_bytes(sampt_dec_t h, int frames, int oh, int ow, size_t* bytes) {
  return sampt_dec_workspace_bytes_k(h, frames, 120, oh, ow, bytes);
}

int sampt_dec_hq_workspace_bytes(sampt_dec_t h, int frames, size_t* bytes) {
  if (!h || !bytes || frames <= 0 || frames > h->e.max_frames) return SAMPT_ERR_ARG;
  if (!h->e.is_hq()) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_dec_hq_workspace_bytes: not an HQ-SAM decoder handle");
  Arena a(nullptr, 0);
  int rc = h->e.hq_features(frames, nullptr, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_dec_hq_features(sampt_dec_t h, int frames, const float* features, const float* interm, float* hq_out, void* ws,
                          size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !features || !interm || !hq_out || !ws || frames <= 0 || frames > h->e.max_frames)
    return fail(SAMPT_ERR_ARG, "sampt_dec_hq_features: bad arguments");
  if (!h->e.is_hq()) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_dec_hq_features: not an HQ-SAM decoder handle");
  Arena a(ws, ws_bytes);
  return h->e.hq_features(frames, features, interm, hq_out, a, (hipStream_t)stream);
}

int sampt_sam_decode(sampt_dec_t h, const float* features, const float* hq_features, const float* pts,
                     const int32_t* labels, int k, const float* box, const float* mask_in, int in_h, int in_w, int oh, int ow, float* logits_out,
                     float* iou_out, float* low_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !features || !logits_out || !iou_out || !low_out || !ws || k < 0 || (k > 0 && (!pts || !labels)))
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode: bad arguments");
  if (h->e.is_hq() != (hq_features != nullptr))
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode: hq_features must be given for HQ-SAM handles and only for them");
  Arena a(ws, ws_bytes);
  return h->e.decode(1, features, hq_features, pts, labels, k, nullptr, k > 0 ? k : 1, box, mask_in, in_h, in_w, oh, ow, logits_out, iou_out,
                     low_out, nullptr, a, (hipStream_t)stream);
}

int sampt_sam_decode_multimask(sampt_dec_t h, const float* features, const float* pts, const int32_t* labels, int k,
                               const float* box, const float* mask_in, int in_h, int in_w, int oh, int ow,
                               float* logits_out, float* iou_out, float* low_out, void* ws, size_t ws_bytes,
                               sampt_stream_t stream) {
  if (!h || !features || !logits_out || !iou_out || !low_out || !ws || k < 0 || (k > 0 && (!pts || !labels)))
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_multimask: bad arguments");
  if (h->e.is_hq()) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_sam_decode_multimask: SAM decoder handles only");
  Arena a(ws, ws_bytes);
  h->e.multimask = true;
  int rc = h->e.decode(1, features, nullptr, pts, labels, k, nullptr, k > 0 ? k : 1, box, mask_in, in_h, in_w, oh, ow,
                       logits_out, iou_out, low_out, nullptr, a, (hipStream_t)stream);
  h->e.multimask = false;
  return rc;
}

int sampt_sam_decode_points_workspace_bytes(sampt_dec_t h, int n, int k, size_t* bytes) {
  if (!h || !bytes) return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points_workspace_bytes: null handle / output");
  if (n <= 0 || n > h->e.max_frames)
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points_workspace_bytes: n " + std::to_string(n) + " outside 1.." +
                                   std::to_string(h->e.max_frames) + " (max_frames of sampt_dec_create)");
  if (k <= 0 || k > SAMPT_DEC_MAX_POINTS)
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points_workspace_bytes: k = " + std::to_string(k) + " prompt points outside 1.." +
                                   std::to_string(SAMPT_DEC_MAX_POINTS) + " (SAMPT_DEC_MAX_POINTS)");
  Arena a(nullptr, 0);
  float dummy = 0.f;
  int rc = h->e.decode_points(n, &dummy, h->e.is_hq() ? &dummy : nullptr, &dummy, nullptr, k, true, nullptr, nullptr, a, nullptr);
  *bytes = a.peak + 256;
  return rc;
}

int sampt_sam_decode_points(sampt_dec_t h, int n, const float* features, const float* hq_features, const float* pts,
                            const int32_t* labels, int k, int multimask, float* low_out, float* iou_out, void* ws, size_t ws_bytes,
                            sampt_stream_t stream) {
  if (!h || !features || !pts || !labels || !low_out || !iou_out || !ws || k <= 0 || k > SAMPT_DEC_MAX_POINTS)
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points: bad arguments");
  if (n <= 0 || n > h->e.max_frames)
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points: n " + std::to_string(n) + " outside 1.." + std::to_string(h->e.max_frames) +
                                   " (max_frames of sampt_dec_create)");
  if (h->e.is_hq() != (hq_features != nullptr))
    return fail(SAMPT_ERR_ARG, "sampt_sam_decode_points: hq_features must be given for HQ-SAM handles and only for them");
  Arena a(ws, ws_bytes);
  return h->e.decode_points(n, features, hq_features, pts, labels, k, multimask != 0, low_out, iou_out, a, (hipStream_t)stream);
}

size_t sampt_amg_score_workspace_bytes(int n_masks) { return amg_score_workspace_bytes(n_masks); }

int sampt_amg_score(const float* low, int n_masks, int L, int img, int in_h, int in_w, int oh, int ow, double mask_threshold,
                    double offset, int32_t* out8, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  int rc = amg_score(low, n_masks, L, img, in_h, in_w, oh, ow, mask_threshold, offset, (int*)out8, ws, ws_bytes, (hipStream_t)stream);
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_amg_score: bad arguments or workspace too small");
}

int sampt_amg_binarize(const float* low, int n_masks, const int32_t* rows, int n_rows, int L, int img, int in_h, int in_w, int oh,
                       int ow, double mask_threshold, uint8_t* out, sampt_stream_t stream) {
  int rc = amg_binarize(low, n_masks, (const int*)rows, n_rows, L, img, in_h, in_w, oh, ow, mask_threshold, out, (hipStream_t)stream);
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_amg_binarize: bad arguments");
}

size_t sampt_amg_regions_workspace_bytes(int n_masks, int h, int w) { return amg_regions_workspace_bytes(n_masks, h, w); }

int sampt_amg_regions(const uint8_t* masks_in, int n, int h, int w, int min_area, uint8_t* masks_out, uint8_t* changed_out,
                      int32_t* area_out, int32_t* boxes_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (n < 0 || h <= 0 || w <= 0) return fail(SAMPT_ERR_ARG, "sampt_amg_regions: bad shape");
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, "sampt_amg_regions: h * w must be below 2^31");
  int rc = amg_regions(masks_in, n, h, w, min_area, masks_out, changed_out, (int*)area_out, (int*)boxes_out, ws, ws_bytes,
                       (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_amg_regions: workspace too small for one mask");
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_amg_regions: null or misaligned pointer");
}

size_t sampt_amg_nms_workspace_bytes(int n) { return amg_nms_workspace_bytes(n); }

int sampt_amg_nms(const float* boxes, const float* scores, int n, float iou_thr, int64_t* keep_out, int32_t* count_out, void* ws,
                  size_t ws_bytes, sampt_stream_t stream) {
  int rc = amg_nms(boxes, scores, n, iou_thr, (long long*)keep_out, (int*)count_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_amg_nms: workspace too small");
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_amg_nms: bad arguments (n outside 0..65535, null or misaligned pointer)");
}

size_t sampt_rle_workspace_bytes(int n, int h, int w) { return rle_workspace_bytes(n, h, w); }

static int rle_bad_shape(const char* who, int n, int h, int w) {
  if (n < 0 || h <= 0 || w <= 0) return fail(SAMPT_ERR_ARG, std::string(who) + ": bad shape");
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, std::string(who) + ": h * w must be below 2^31");
  return SAMPT_OK;
}

int sampt_rle_count(const void* x, int is_f32, float thr, int n, int h, int w, int64_t* offsets_out, int32_t* area_out, void* ws,
                    size_t ws_bytes, sampt_stream_t stream) {
  if (rle_bad_shape("sampt_rle_count", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  int rc = rle_count(x, is_f32, thr, n, h, w, (long long*)offsets_out, (int*)area_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_rle_count: workspace too small for n masks (split the stack by masks)");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_rle_count: null or misaligned pointer");
  return rc;
}

int sampt_rle_emit(int n, int h, int w, const int64_t* offsets, uint32_t* counts_out, const void* ws, size_t ws_bytes,
                   sampt_stream_t stream) {
  if (rle_bad_shape("sampt_rle_emit", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  int rc = rle_emit(n, h, w, (const long long*)offsets, counts_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_rle_emit: workspace smaller than the one sampt_rle_count filled");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_rle_emit: null or misaligned pointer");
  return rc;
}

size_t sampt_rle_string_workspace_bytes(int64_t total_counts) { return rle_string_workspace_bytes((long)total_counts); }

int sampt_rle_string_sizes(const uint32_t* counts, const int64_t* offsets, int n, int64_t total, int64_t* str_offsets, void* ws,
                           size_t ws_bytes, sampt_stream_t stream) {
  int rc = rle_string_sizes(counts, (const long long*)offsets, n, (long)total, (long long*)str_offsets, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_rle_string_sizes: workspace too small");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_rle_string_sizes: bad arguments (n < 1, total_counts < n, null or misaligned pointer)");
  return rc;
}

int sampt_rle_string_emit(const uint32_t* counts, const int64_t* offsets, int n, int64_t total, int64_t* str_offsets, uint8_t* chars_out,
                          const void* ws, size_t ws_bytes, sampt_stream_t stream) {
  int rc = rle_string_emit(counts, (const long long*)offsets, n, (long)total, (long long*)str_offsets, chars_out, ws, ws_bytes,
                           (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_rle_string_emit: workspace too small");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_rle_string_emit: bad arguments (n < 1, total_counts < n, null or misaligned pointer)");
  return rc;
}

static int ve_bad_shape(const char* who, int n, int h, int w) {
  if (n < 0 || h <= 0 || w <= 0) return fail(SAMPT_ERR_ARG, std::string(who) + ": bad shape");
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, std::string(who) + ": h * w must be below 2^31");
  return SAMPT_OK;
}

int sampt_bits_pack(const void* x, int kind, float thr, const int32_t* values, const int32_t* planes, int n, int h, int w, uint64_t* bits_out,
                    int32_t* area_out, sampt_stream_t stream) {
  if (ve_bad_shape("sampt_bits_pack", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (kind < 0 || kind > 2) return fail(SAMPT_ERR_ARG, "sampt_bits_pack: unknown kind (0 = bytes, 1 = f32 with a threshold, 2 = uint8 index map)");
  int rc = bits_pack(x, kind, thr, (const int*)values, (const int*)planes, n, h, w, (unsigned long long*)bits_out, (int*)area_out,
                     (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_bits_pack: null or misaligned pointer (an index map needs its values)");
  return rc;
}

size_t sampt_rle_decode_workspace_bytes(int64_t total_counts) { return rle_decode_workspace_bytes((long)total_counts); }

int sampt_rle_decode_bits(const uint32_t* counts, const int64_t* offsets, int n, int64_t total, int h, int w, uint64_t* bits_out,
                          int32_t* area_out, int32_t* status_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (ve_bad_shape("sampt_rle_decode_bits", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (total < 0) return fail(SAMPT_ERR_ARG, "sampt_rle_decode_bits: negative total_counts");
  int rc = rle_decode_bits(counts, (const long long*)offsets, n, (long)total, h, w, (unsigned long long*)bits_out, (int*)area_out,
                           (int*)status_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_rle_decode_bits: workspace smaller than sampt_rle_decode_workspace_bytes(total_counts)");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_rle_decode_bits: null or misaligned pointer");
  return rc;
}

int sampt_bits_unpack(const uint64_t* bits, int n, int h, int w, uint8_t* bytes_out, sampt_stream_t stream) {
  if (ve_bad_shape("sampt_bits_unpack", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  int rc = bits_unpack((const unsigned long long*)bits, n, h, w, bytes_out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_bits_unpack: null or misaligned pointer");
  return rc;
}

int sampt_bits_row_prefix(const uint64_t* bits, int n, int h, int w, int32_t* prefix_out, sampt_stream_t stream) {
  if (ve_bad_shape("sampt_bits_row_prefix", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  int rc = bits_row_prefix((const unsigned long long*)bits, n, h, w, (int*)prefix_out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_bits_row_prefix: null or misaligned pointer");
  return rc;
}

int sampt_bits_select(const uint64_t* bits, const int32_t* prefix, int n, int h, int w, const int32_t* queries, int nq, float* yx_out,
                      sampt_stream_t stream) {
  if (ve_bad_shape("sampt_bits_select", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (nq < 0) return fail(SAMPT_ERR_ARG, "sampt_bits_select: negative number of queries");
  int rc = bits_select((const unsigned long long*)bits, (const int*)prefix, n, h, w, (const int*)queries, nq, yx_out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_bits_select: null or misaligned pointer");
  return rc;
}

size_t sampt_seq_iou_workspace_bytes(int n_dt, int n_gt, int n_frames, int h, int w) {
  return seq_iou_workspace_bytes(n_dt, n_gt, n_frames, h, w);
}

int sampt_seq_iou_counts(const uint64_t* dt_bits, const int32_t* dt_area, const int32_t* dt_planes, int n_dt, int dt_n_planes,
                         const uint64_t* gt_bits, const int32_t* gt_area, const int32_t* gt_planes, int n_gt, int gt_n_planes, int n_frames,
                         int h, int w, int64_t* counts_out, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (n_dt <= 0 || n_gt <= 0 || n_frames <= 0) return fail(SAMPT_ERR_ARG, "sampt_seq_iou_counts: n_dt, n_gt and n_frames must be positive");
  if (ve_bad_shape("sampt_seq_iou_counts", 1, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  int rc = seq_iou_counts((const unsigned long long*)dt_bits, (const int*)dt_area, (const int*)dt_planes, n_dt, dt_n_planes,
                          (const unsigned long long*)gt_bits, (const int*)gt_area, (const int*)gt_planes, n_gt, gt_n_planes, n_frames, h, w,
                          (long long*)counts_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_seq_iou_counts: workspace smaller than sampt_seq_iou_workspace_bytes");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_seq_iou_counts: bad arguments (too many items, negative plane count, null or misaligned pointer)");
  return rc;
}

int sampt_vis_match(const int64_t* counts, int n_dt, int n_gt, int n_ranges, int n_thr, const double* thrs, const int32_t* gt_order,
                    const uint8_t* gt_ignore, const uint8_t* iscrowd, const uint8_t* dt_out, int32_t* dt_match_out, int32_t* gt_match_out,
                    uint8_t* dt_ignore_out, sampt_stream_t stream) {
  int rc = vis_match((const long long*)counts, n_dt, n_gt, n_ranges, n_thr, thrs, (const int*)gt_order, gt_ignore, iscrowd, dt_out,
                     (int*)dt_match_out, (int*)gt_match_out, dt_ignore_out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG)
    return fail(rc, "sampt_vis_match: bad arguments (n_dt >= 1, 1 <= n_gt <= 960, 1 <= n_thr <= 64, n_ranges >= 1, null or misaligned pointer)");
  return rc;
}

int sampt_viz_band(const uint64_t* bits, int n, int h, int w, int radius, uint64_t* band_out, sampt_stream_t stream) {
  if (ve_bad_shape("sampt_viz_band", n, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (radius < 0 || radius > 64) return fail(SAMPT_ERR_ARG, "sampt_viz_band: radius must be in 0 .. 64");
  int rc = viz_band((const unsigned long long*)bits, n, h, w, radius, (unsigned long long*)band_out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_viz_band: null or misaligned pointer");
  return rc;
}

static_assert(SAMPT_PATCH_FILTER_MAX_PATCH_SIZE == PATCH_FILTER_MAX_PATCH_SIZE, "header and kernel disagree");
int sampt_patch_filter(const uint8_t* rgb, int T, int H, int W, const float* query, const float* traj, const float* vis_in, int N,
                       int patch_size, float threshold, const double* companding, int border_rule, float* vis_out, float* sim_out,
                       sampt_stream_t stream) {
  if (T <= 0 || N <= 0 || H <= 0 || W <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_patch_filter: T, N, H and W must be positive; got T = " + std::to_string(T) + ", N = " +
                                   std::to_string(N) + ", H = " + std::to_string(H) + ", W = " + std::to_string(W));
  if (patch_size < 1 || patch_size > SAMPT_PATCH_FILTER_MAX_PATCH_SIZE)
    return fail(SAMPT_ERR_ARG, "sampt_patch_filter: patch_size must be in 1 .. " + std::to_string(SAMPT_PATCH_FILTER_MAX_PATCH_SIZE) +
                                   "; got " + std::to_string(patch_size));
  if (!rgb || !query || !traj || !vis_in || !companding || !vis_out)
    return fail(SAMPT_ERR_ARG, "sampt_patch_filter: null pointer (only sim_out may be null)");
  return patch_filter(rgb, T, H, W, query, traj, vis_in, N, patch_size, threshold, companding, border_rule, vis_out, sim_out,
                      (hipStream_t)stream);
}

static int pa_bad_shape(const char* who, int T, int M, int P, int pp) {
  if (T <= 0 || M <= 0 || P <= 0 || pp < 0 || (long)T * M * P * 2 > 0x7fffffffL)
    return fail(SAMPT_ERR_ARG, std::string(who) + ": T, M and P must be positive, pp non-negative and T * M * P * 2 below 2^31; got T = " +
                                   std::to_string(T) + ", M = " + std::to_string(M) + ", P = " + std::to_string(P) + ", pp = " +
                                   std::to_string(pp));
  return SAMPT_OK;
}

int sampt_prompt_count(const float* vis, int T, int M, int P, int pp, int negatives, int add_others, int32_t* k_all, int32_t* npos_all,
                       sampt_stream_t stream) {
  if (pa_bad_shape("sampt_prompt_count", T, M, P, pp) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (!vis || !k_all || !npos_all) return fail(SAMPT_ERR_ARG, "sampt_prompt_count: null pointer");
  return prompt_count(vis, T, M, P, pp, negatives, add_others, (int*)k_all, (int*)npos_all, (hipStream_t)stream);
}

int sampt_prompt_fill(const float* traj, const float* vis, int T, int M, int P, int pp, int negatives, int add_others, double sx, double sy,
                      const int32_t* items, int n_items, int ld, float* pts, int32_t* labels, int32_t* k_item, int32_t* npos_item,
                      sampt_stream_t stream) {
  if (pa_bad_shape("sampt_prompt_fill", T, M, P, pp) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (n_items <= 0 || ld <= 0 || (long)n_items * ld * 2 > 0x7fffffffL)
    return fail(SAMPT_ERR_ARG, "sampt_prompt_fill: n_items and ld must be positive and n_items * ld * 2 below 2^31; got n_items = " +
                                   std::to_string(n_items) + ", ld = " + std::to_string(ld));
  if (!traj || !vis || !items || !pts || !labels || !k_item || !npos_item) return fail(SAMPT_ERR_ARG, "sampt_prompt_fill: null pointer");
  return prompt_fill(traj, vis, T, M, P, pp, negatives, add_others, sx, sy, (const int*)items, n_items, ld, pts, (int*)labels, (int*)k_item,
                     (int*)npos_item, (hipStream_t)stream);
}

int sampt_mark_outside_frame(const float* traj, const float* vis_in, long n, int H, int W, float* vis_out, sampt_stream_t stream) {
  if (n <= 0 || H <= 0 || W <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_mark_outside_frame: n, H and W must be positive; got n = " + std::to_string(n) + ", H = " +
                                   std::to_string(H) + ", W = " + std::to_string(W));
  if (!traj || !vis_in || !vis_out) return fail(SAMPT_ERR_ARG, "sampt_mark_outside_frame: null pointer");
  return mark_outside_frame(traj, vis_in, n, H, W, vis_out, (hipStream_t)stream);
}

int sampt_viz_compose(const uint8_t* frames, int interleaved, int n_frames, int h, int w, const uint64_t* bits, const uint64_t* band,
                      int n_masks, const uint8_t* lut, const int32_t* markers, int n_markers, int panel, uint8_t* out,
                      sampt_stream_t stream) {
  if (ve_bad_shape("sampt_viz_compose", n_frames, h, w) != SAMPT_OK) return SAMPT_ERR_ARG;
  if (panel < 1 || panel > 3) return fail(SAMPT_ERR_ARG, "sampt_viz_compose: panel must be 1 (input), 2 (predictions) or 3 (stacked)");
  if (n_masks < 0 || n_markers < 0) return fail(SAMPT_ERR_ARG, "sampt_viz_compose: negative n_masks or n_markers");
  int rc = viz_compose(frames, interleaved, n_frames, h, w, (const unsigned long long*)bits, (const unsigned long long*)band, n_masks, lut,
                       (const int*)markers, n_markers, panel, out, (hipStream_t)stream);
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_viz_compose: null or misaligned pointer (masks need bits, band and lut; markers their table)");
  return rc;
}

size_t sampt_jf_workspace_bytes(int n, int h, int w, int radius) { return jf_workspace_bytes(n, h, w, radius); }

int sampt_jf_counts(const void* seg, int seg_kind, float seg_thr, const int32_t* seg_values, const int32_t* seg_planes, const void* ann,
                    int ann_kind, float ann_thr, const int32_t* ann_values, const int32_t* ann_planes, const uint8_t* void_px,
                    const int32_t* void_planes, int n, int h, int w, int radius, int32_t* counts_out, void* ws, size_t ws_bytes,
                    sampt_stream_t stream) {
  if (n <= 0 || h <= 0 || w <= 0) return fail(SAMPT_ERR_ARG, "sampt_jf_counts: bad shape (n, h and w must be positive)");
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, "sampt_jf_counts: h * w must be below 2^31");
  if (radius < 0 || radius > 64) return fail(SAMPT_ERR_ARG, "sampt_jf_counts: radius must be in 0 .. 64");
  if (seg_kind < 0 || seg_kind > 2 || ann_kind < 0 || ann_kind > 2)
    return fail(SAMPT_ERR_ARG, "sampt_jf_counts: unknown kind (0 = bytes, 1 = f32 with a threshold, 2 = uint8 index map)");
  int rc = jf_counts(seg, seg_kind, seg_thr, (const int*)seg_values, (const int*)seg_planes, ann, ann_kind, ann_thr, (const int*)ann_values,
                     (const int*)ann_planes, void_px, (const int*)void_planes, n, h, w, radius, (int*)counts_out, ws, ws_bytes,
                     (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_jf_counts: workspace too small for n items (split the stack by items)");
  if (rc == SAMPT_ERR_ARG) return fail(rc, "sampt_jf_counts: null or misaligned pointer (an index map needs its values)");
  return rc;
}

size_t sampt_jf_pairs_workspace_bytes(int n_seg, int n_ann, int n_frames, int h, int w, int radius) {
  return jf_pairs_workspace_bytes(n_seg, n_ann, n_frames, h, w, radius);
}

int sampt_jf_pairs_counts(const void* seg, int seg_kind, float seg_thr, const int32_t* seg_values, const int32_t* seg_planes, int n_seg,
                          const void* ann, int ann_kind, float ann_thr, const int32_t* ann_values, const int32_t* ann_planes, int n_ann,
                          const uint8_t* void_px, const int32_t* void_planes, int n_frames, int h, int w, int radius, int32_t* pair_out,
                          int32_t* seg_stat, int32_t* ann_stat, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (n_seg <= 0 || n_ann <= 0 || n_frames <= 0 || h <= 0 || w <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_jf_pairs_counts: bad shape (n_seg, n_ann, n_frames, h and w must be positive)");
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, "sampt_jf_pairs_counts: h * w must be below 2^31");
  if (radius < 0 || radius > 64) return fail(SAMPT_ERR_ARG, "sampt_jf_pairs_counts: radius must be in 0 .. 64");
  if (seg_kind < 0 || seg_kind > 2 || ann_kind < 0 || ann_kind > 2)
    return fail(SAMPT_ERR_ARG, "sampt_jf_pairs_counts: unknown kind (0 = bytes, 1 = f32 with a threshold, 2 = uint8 index map)");
  int rc = jf_pairs_counts(seg, seg_kind, seg_thr, (const int*)seg_values, (const int*)seg_planes, n_seg, ann, ann_kind, ann_thr,
                           (const int*)ann_values, (const int*)ann_planes, n_ann, void_px, (const int*)void_planes, n_frames, h, w, radius,
                           (int*)pair_out, (int*)seg_stat, (int*)ann_stat, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_jf_pairs_counts: workspace too small for n_frames frames (split the stack by frames)");
  if (rc == SAMPT_ERR_ARG)
    return fail(rc, "sampt_jf_pairs_counts: null or misaligned pointer (an index map needs its values), or 3 * n_seg * n_ann * n_frames >= 2^31");
  return rc;
}

int sampt_sam_track_decode(sampt_dec_t h, int frames, const float* features, const float* hq_features,
                           const float* pts, const int32_t* labels, int k, const int32_t* k_item,
                           const int32_t* npos_item, int ld_pts, int n_pos_first, int refine_iters, float iou_thr,
                           int in_h, int in_w, int oh, int ow, float* final_logits, float* score_out, void* ws,
                           size_t ws_bytes, sampt_stream_t stream) {
  if (!h || !features || !pts || !labels || !final_logits || !score_out || !ws || k <= 0 || n_pos_first > k ||
      ld_pts < k || frames <= 0 || frames > h->e.max_frames)
    return fail(SAMPT_ERR_ARG, "sampt_sam_track_decode: bad arguments");
  if (h->e.is_hq() != (hq_features != nullptr))
    return fail(SAMPT_ERR_ARG, "sampt_sam_track_decode: hq_features must be given for HQ-SAM handles and only for them");
  Arena a(ws, ws_bytes);
  if (npos_item && n_pos_first < 0)
    return fail(SAMPT_ERR_ARG, "sampt_sam_track_decode: npos_item needs the two-pass mode (n_pos_first >= 0)");
  return h->e.track_decode(frames, features, hq_features, pts, labels, k, k_item, npos_item, ld_pts, n_pos_first,
                           refine_iters, iou_thr, in_h, in_w, oh, ow, final_logits, score_out, a, (hipStream_t)stream);
}

int sampt_sam_track_decode_graph(sampt_dec_t h, int frames, const float* features, const float* hq_features,
                                 const float* pts, const int32_t* labels, int k, const int32_t* k_item,
                                 const int32_t* npos_item, int ld_pts, int n_pos_first, int refine_iters, float iou_thr,
                                 int in_h, int in_w, int oh, int ow, float* final_logits, float* score_out, void* ws,
                                 size_t ws_bytes, sampt_stream_t stream) {
  if (!h) return fail(SAMPT_ERR_ARG, "sampt_sam_track_decode_graph: null handle");
  hipStream_t s = (hipStream_t)stream;
  if (s == nullptr)    // the legacy default stream cannot be captured
    return sampt_sam_track_decode(h, frames, features, hq_features, pts, labels, k, k_item, npos_item, ld_pts, n_pos_first,
                                  refine_iters, iou_thr, in_h, in_w, oh, ow, final_logits, score_out, ws, ws_bytes, stream);
  DecGraphKey key;
  memset(&key, 0, sizeof(key));   // padding bytes are part of the hash / comparison
  key.features = features, key.hq = hq_features, key.pts = pts, key.labels = labels, key.k_item = k_item;
  key.npos_item = npos_item, key.logits = final_logits, key.score = score_out, key.ws = ws, key.ws_bytes = ws_bytes;
  key.frames = frames, key.k = k, key.ld_pts = ld_pts, key.n_pos_first = n_pos_first, key.refine = refine_iters;
  key.in_h = in_h, key.in_w = in_w, key.oh = oh, key.ow = ow, key.iou_thr = iou_thr;
  key.batch_invariant = h->e.batch_invariant ? 1 : 0;
  try {
    DecGraphEntry& ent = h->graphs[key];
    ent.last_use = ++h->graph_clock;
    while (h->graphs.size() > 64) {   // bound the cache: drop the least recently used signature, captured or only seen
      auto victim = h->graphs.end();
      for (auto it = h->graphs.begin(); it != h->graphs.end(); ++it)
        if (&it->second != &ent && (victim == h->graphs.end() || it->second.last_use < victim->second.last_use)) victim = it;
      if (victim == h->graphs.end()) break;
      if (victim->second.exec) (void)hipGraphExecDestroy(victim->second.exec);
      h->graphs.erase(victim);       // (references to other elements of an unordered_map stay valid)
    }
    if (ent.exec) {
      if (hipGraphLaunch(ent.exec, s) != hipSuccess) return fail(SAMPT_ERR_HIP, "sampt_sam_track_decode_graph: hipGraphLaunch failed");
      ++h->graph_launches;
      return SAMPT_OK;
    }
    if (ent.seen++ == 0)   // first sight of a signature: plain launches (validates the arguments, sets lazy attributes)
      return sampt_sam_track_decode(h, frames, features, hq_features, pts, labels, k, k_item, npos_item, ld_pts,
                                    n_pos_first, refine_iters, iou_thr, in_h, in_w, oh, ow, final_logits, score_out, ws,
                                    ws_bytes, stream);
    DecGraphEntry& e2 = h->graphs[key];
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess)
      return fail(SAMPT_ERR_HIP, "sampt_sam_track_decode_graph: hipStreamBeginCapture failed");
    int rc = sampt_sam_track_decode(h, frames, features, hq_features, pts, labels, k, k_item, npos_item, ld_pts, n_pos_first,
                                    refine_iters, iou_thr, in_h, in_w, oh, ow, final_logits, score_out, ws, ws_bytes, stream);
    hipGraph_t g = nullptr;
    hipError_t ce = hipStreamEndCapture(s, &g);
    if (rc != SAMPT_OK || ce != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      return rc != SAMPT_OK ? rc : fail(SAMPT_ERR_HIP, "sampt_sam_track_decode_graph: stream capture failed");
    }
    hipGraphExec_t exec = nullptr;
    hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess || !exec) return fail(SAMPT_ERR_HIP, "sampt_sam_track_decode_graph: hipGraphInstantiate failed");
    e2.exec = exec;
    ++h->graph_captures;
    if (hipGraphLaunch(exec, s) != hipSuccess) return fail(SAMPT_ERR_HIP, "sampt_sam_track_decode_graph: hipGraphLaunch failed");
    ++h->graph_launches;
    return SAMPT_OK;
  } catch (...) {
    return fail(SAMPT_ERR_ARG, "sampt_sam_track_decode_graph: C++ exception");
  }
}

int sampt_dec_graph_stats(sampt_dec_t h, long* cached, long* captures, long* launches) {
  if (!h || !cached || !captures || !launches) return SAMPT_ERR_ARG;
  *cached = (long)h->graphs.size(), *captures = h->graph_captures, *launches = h->graph_launches;
  return SAMPT_OK;
}

int sampt_postprocess_masks(const float* low, int L, int img, int in_h, int in_w, float* out, int oh, int ow,
                            sampt_stream_t stream) {
  return sam_postprocess(low, L, img, in_h, in_w, out, oh, ow, (hipStream_t)stream);
}

size_t sampt_bbox_workspace_bytes(int h, int w) { return bbox_partial_ints(h, w) * sizeof(int); }

int sampt_bbox_from_logits(const float* logits, int h, int w, int32_t* bbox_state, void* ws, size_t ws_bytes,
                           sampt_stream_t stream) {
  if (!logits || !bbox_state || !ws || ws_bytes < sampt_bbox_workspace_bytes(h, w)) return SAMPT_ERR_WORKSPACE;
  return bbox_from_logits_state(logits, h, w, (int*)bbox_state, (int*)ws, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- kernel-level
int sampt_gemm(int dtype, const void* A, const void* W, const float* bias, const float* res, void* C, int M, int N, int K,
               int act, float alpha, sampt_stream_t stream) {
  GemmP p = gemm_linear(A, K, W, bias, C, N, M, N, K, act, res);
  p.alpha = alpha, p.out_f16 = dtype == 2;
  return dtype == 0 ? gemm_f32(p, (hipStream_t)stream) : gemm_f16(p, (hipStream_t)stream);
}

int sampt_gemm_f32_rows(const float* A, int lda, const float* W, const float* bias, const float* res, int res_mod, float* C, int ldc,
                        int M, int N, int K, int act, int invariant, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (invariant < 0 || invariant > 1) return fail(SAMPT_ERR_ARG, "sampt_gemm_f32_rows: invariant is 0 or 1");
  GemmP p = gemm_linear(A, lda > 0 ? lda : K, W, bias, C, ldc > 0 ? ldc : N, M, N, K, act, res, N, res_mod);
  p.row_invariant = invariant;
  p.splitk_ws = (float*)ws, p.splitk_ws_floats = ws ? ws_bytes / sizeof(float) : 0;
  int rc = gemm_f32(p, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_gemm_f32_rows: null / misaligned operand, or K, lda not a multiple of 4") : rc;
}

int sampt_gemm_f32_route(int M, int N, int K, int lda, int ldc, int invariant, int* route, int* kparts) {
  if (M <= 0 || N <= 0 || K <= 0 || lda < 0 || ldc < 0 || invariant < 0 || invariant > 1 || !route || !kparts)
    return fail(SAMPT_ERR_ARG, "sampt_gemm_f32_route: bad arguments");
  // the decoder's call: 16-byte aligned operands, bias, no residual, its split-K workspace of 16 * M * 256 floats (never dereferenced)
  float* const aligned = (float*)(uintptr_t)4096;
  GemmP p = gemm_linear(aligned, lda > 0 ? lda : K, aligned, aligned, aligned, ldc > 0 ? ldc : N, M, N, K, ACT_NONE, nullptr, N, 0);
  p.row_invariant = invariant;
  p.splitk_ws = aligned, p.splitk_ws_floats = (size_t)16 * M * 256;
  int rc = gemm_f32_route(p, route, kparts);
  return rc == SAMPT_OK ? rc : fail(rc, "sampt_gemm_f32_route: K must be a multiple of 4");
}

int sampt_attn_t2i_plan(int F, int Nq, int Nk, int invariant, int* KS, int* kper) {
  if (F <= 0 || Nq <= 0 || Nk <= 0 || invariant < 0 || invariant > 1 || !KS || !kper)
    return fail(SAMPT_ERR_ARG, "sampt_attn_t2i_plan: bad arguments");
  attn_t2i_plan_query(F, Nq, Nk, invariant != 0, KS, kper);
  return SAMPT_OK;
}

int sampt_gemm_ex(int dtype, const void* A, const void* W, const float* bias, const float* res, void* C, int M, int N, int K,
                  int act, float alpha, const int32_t* rowmap, const int32_t* a_rowmap, int res_mod, int ldr,
                  sampt_stream_t stream) {
  GemmP p = gemm_linear(A, K, W, bias, C, N, M, N, K, act, res, ldr > 0 ? ldr : N, res_mod);
  p.alpha = alpha, p.rowmap = rowmap, p.a_rowmap = a_rowmap, p.out_f16 = dtype == 2;
  if (dtype == 3 || dtype == 4) {   // x3 rows in (A, W: 2K halves per row), f32 or x3 rows out
    p.x3 = 1, p.K = 2 * K, p.lda = 2 * K, p.ldw = 2 * K;
    if (dtype == 4) p.out_f16 = 2, p.ldc = 2 * N;
  }
  return dtype == 0 ? gemm_f32(p, (hipStream_t)stream) : gemm_f16(p, (hipStream_t)stream);
}

int sampt_gemm_f16_p8(int dtype, const void* A, const void* W, const float* bias, const float* res, void* C, int M, int N, int K,
                      int act, float alpha, const int32_t* rowmap, const int32_t* a_rowmap, int res_mod, int ldr, int heads, int hd,
                      int rows, int wgs_per_xcd, int stagger, sampt_stream_t stream) {
  const bool hm = heads != 0 || hd != 0 || rows != 0;
  if (dtype < 1 || dtype > 4 || !A || !W || !C || M <= 0 || N <= 0 || K <= 0 || res_mod < 0 || ldr < 0 || wgs_per_xcd < 0 ||
      wgs_per_xcd > 32 || stagger < 0 || stagger > 8)
    return fail(SAMPT_ERR_ARG, "sampt_gemm_f16_p8: dtype 1 .. 4, non-null operands, wgs_per_xcd 0 .. 32, stagger 0 .. 8");
  if (hm && (heads <= 0 || hd < 4 || hd % 4 || N % (heads * hd) || rows < (rowmap ? 1 : M)))
    return fail(SAMPT_ERR_ARG, "sampt_gemm_f16_p8: head-major needs hd % 4 == 0, N % (heads * hd) == 0, rows >= M without a rowmap");
  GemmP p = gemm_linear(A, K, W, bias, C, N, M, N, K, act, res, ldr > 0 ? ldr : N, res_mod);
  p.alpha = alpha, p.rowmap = rowmap, p.a_rowmap = a_rowmap, p.out_f16 = dtype == 2;
  if (dtype == 3 || dtype == 4) {
    p.x3 = 1, p.K = 2 * K, p.lda = 2 * K, p.ldw = 2 * K;
    if (dtype == 4) p.out_f16 = 2, p.ldc = 2 * N;
  }
  if (hm) {                          // a plain fp16 destination; the kernel has none for an x3 product and refuses it
    p.hm_heads = heads, p.hm_hd = hd, p.hm_rows = rows;
    if (dtype >= 2) p.out_f16 = 1, p.ldc = N;
  }
  p.p8_wgs = wgs_per_xcd, p.p8_stagger = stagger;
  // the epilogue's 16-byte accesses (the launcher checks A and W)
  if ((((uintptr_t)bias | (uintptr_t)res) & 15) || ((uintptr_t)C & (p.out_f16 ? 7 : 15))) return SAMPT_ERR_UNSUPPORTED;
  return gemm_f16_p8_launch(p, (hipStream_t)stream);
}

int sampt_gemm_f16_p8_plan(int M, int N, int wgs_per_xcd, int trim, int* workgroups_per_xcd, int* rounds, int* strip_rows) {
  if (M < 256 || N < 256 || N % 256 || wgs_per_xcd < 0 || wgs_per_xcd > 32 || trim < -1 || trim > 1 || !workgroups_per_xcd || !rounds ||
      !strip_rows)
    return fail(SAMPT_ERR_ARG, "sampt_gemm_f16_p8_plan: M >= 256, N a multiple of 256, wgs_per_xcd 0 .. 32, trim -1 / 0 / 1");
  gemm_f16_p8_plan(M, N, wgs_per_xcd, trim < 0 ? sampt::g_p8_trim : trim, workgroups_per_xcd, rounds, strip_rows);
  return SAMPT_OK;
}

int sampt_kmedoids_rowsums_f64(const float* xy, int n, double* out, sampt_stream_t stream) {
  int rc = kmedoids_rowsums(xy, n, out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_kmedoids_rowsums_f64: bad arguments (1 <= n <= 2048)") : rc;
}

int sampt_kmedoids_alternate(const float* xy, int n, int K, int32_t* medoids, int max_iter, int32_t* iters_out,
                             sampt_stream_t stream) {
  int rc = kmedoids_alternate(xy, n, K, (int*)medoids, max_iter, (int*)iters_out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_kmedoids_alternate: bad arguments (1 <= K <= min(n, 64), n <= 2048)") : rc;
}

size_t sampt_dbscan_workspace_bytes(int n) { return dbscan_workspace_bytes(n); }

int sampt_dbscan_labels(const float* xy, int n, int r2, int min_samples, int32_t* labels_out, void* ws, size_t ws_bytes,
                        sampt_stream_t stream) {
  int rc = dbscan_labels(xy, n, r2, min_samples, (int*)labels_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_dbscan_labels: workspace smaller than sampt_dbscan_workspace_bytes(n)");
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_dbscan_labels: bad arguments (1 <= n <= 2^20, r2 >= 0, min_samples >= 1, 16-byte aligned workspace)") : rc;
}

int sampt_dbscan_largest(const int32_t* labels, int n, int min_points, int32_t* members_out, int32_t* info_out, void* ws, size_t ws_bytes,
                         sampt_stream_t stream) {
  int rc = dbscan_largest((const int*)labels, n, min_points, (int*)members_out, (int*)info_out, ws, ws_bytes, (hipStream_t)stream);
  if (rc == SAMPT_ERR_WORKSPACE) return fail(rc, "sampt_dbscan_largest: workspace smaller than sampt_dbscan_workspace_bytes(n)");
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_dbscan_largest: bad arguments (1 <= n <= 2^20, 16-byte aligned workspace)") : rc;
}

int sampt_int_frame_state(const float* logits, const uint8_t* gt, int h, int w, const float* xy, const float* vis, const int32_t* label,
                          int n_points, int32_t* info_out, uint8_t* cat_out, uint8_t* fn_out, uint8_t* fp_out, sampt_stream_t stream) {
  if ((long)h * w >= (1L << 31)) return fail(SAMPT_ERR_ARG, "sampt_int_frame_state: h * w must be below 2^31");
  int rc = int_frame_state(logits, gt, h, w, xy, vis, (const int*)label, n_points, (int*)info_out, cat_out, fn_out, fp_out,
                           (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_int_frame_state: null pointer or bad shape") : rc;
}

int sampt_qp_corners_workspace_bytes(int H, int W, size_t* bytes) {
  if (!bytes || H < 3 || W < 3) return fail(SAMPT_ERR_ARG, "sampt_qp_corners_workspace_bytes: bad arguments");
  *bytes = qp_corners_workspace_bytes(H, W);
  return SAMPT_OK;
}

int sampt_qp_erode_u8(const uint8_t* mask, int H, int W, int k, uint8_t* tmp, uint8_t* out, sampt_stream_t stream) {
  int rc = qp_erode(mask, H, W, k, tmp, out, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_qp_erode_u8: bad arguments") : rc;
}

int sampt_qp_shi_tomasi(const uint8_t* image, const uint8_t* mask, int H, int W, int n_points, float quality_level, float* out_xy,
                        int32_t* out_info, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  int rc = qp_corners(image, mask, H, W, n_points, quality_level, out_xy, (int*)out_info, ws, ws_bytes, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_qp_shi_tomasi: bad arguments (H, W >= 3, 1 <= n_points <= 64, workspace of "
                                        "sampt_qp_corners_workspace_bytes)") : rc;
}

int sampt_split_rows_x3(const float* x, void* y, int M, int K, sampt_stream_t stream) {
  if (!x || !y) return fail(SAMPT_ERR_ARG, "sampt_split_rows_x3: bad arguments");
  return split_rows_x3(x, (half_t*)y, M, K, (hipStream_t)stream);
}

int sampt_conv2d_nhwc(int dtype, const void* x, const void* w, const float* bias, float* y, int n, int H, int W, int Cin,
                      int Cout, int KH, int KW, int stride, int pad, sampt_stream_t stream) {
  const ConvW c{(const float*)w, bias, nullptr, Cin, Cout, KH, KW, stride, pad, pad};
  GemmP p = gemm_conv(c, x, n, H, W, y);
  if (dtype == 3 || dtype == 4) {
    gemm_split_planes(p, (const half_t*)w);
    if (dtype == 4) p.A_lo = (const half_t*)x + (size_t)n * H * W * Cin;   // activations pre-split: [2][n][H][W][Cin] halves
    return conv_f16x3(p, (hipStream_t)stream);
  }
  return dtype == 0 ? gemm_f32(p, (hipStream_t)stream) : gemm_f16(p, (hipStream_t)stream);
}

int sampt_gemm_x3_rows(const float* A, const void* w_hl, const float* bias, const float* res, int res_mod, float* C, int M, int N,
                       int K, int act, int shuf_g, sampt_stream_t stream) {
  return sampt_gemm_x3_rows_epi(A, w_hl, bias, res, res_mod, C, M, N, K, act, shuf_g, 0, nullptr, nullptr, 0.f, 0, stream);
}

int sampt_gemm_x3_rows_epi(const float* A, const void* w_hl, const float* bias, const float* res, int res_mod, float* C, int M, int N,
                           int K, int act, int shuf_g, int epi, const float* epi_a, const float* epi_b, float epi_eps, int epi_ld,
                           sampt_stream_t stream) {
  GemmP p = gemm_linear(A, K, nullptr, bias, C, shuf_g ? N / 4 : N, M, N, K, act, res, shuf_g ? N / 4 : N, res_mod);
  gemm_split_planes(p, (const half_t*)w_hl);
  p.shuf_g = shuf_g, p.shuf_n = shuf_g ? N / 4 : 0;
  if (!epi) return conv_f16x3(p, (hipStream_t)stream);
  // the fused tails exist in the weights-resident kernel only: refuse rather than compute something else.  The operands are checked
  // as those of the plain launch, then the tail's own: both kernels read epi_a / epi_b one float at a time
  const int rc = x3_args_check(p);
  const bool tail_b = epi == 1 || epi == 3;
  if (rc == SAMPT_ERR_ARG || !epi_a || (tail_b && !epi_b) || (((uintptr_t)epi_a | (uintptr_t)epi_b) & 3))
    return fail(SAMPT_ERR_ARG, "sampt_gemm_x3_rows_epi: A, w_hl, C (and bias, res) non-null and 16-byte aligned, epi_a / epi_b non-null floats");
  p.epi = epi, p.epi_a = epi_a, p.epi_b = epi_b, p.epi_eps = epi_eps, p.epi_ld = epi_ld;
  if (epi == 2) p.ldc = 1;      // one float per output pixel
  if (rc != SAMPT_OK || !sampt::g_gemm_x3_wres || !(epi == 3 ? gemm_x3_wres_ln_eligible(p) : gemm_x3_wres_eligible(p)))
    return fail(SAMPT_ERR_UNSUPPORTED, "sampt_gemm_x3_rows_epi: shape without a fused tail");
  return gemm_x3_wres(p, (hipStream_t)stream);
}

int sampt_sam_mask_dot(const float* up, const float* hyper, int ld_hyper, float* low, int frames, int npix, int C, sampt_stream_t stream) {
  return sam_mask_dot(up, hyper, ld_hyper, nullptr, nullptr, 0, low, frames, npix, C, (hipStream_t)stream);
}

int sampt_move_rows(const void* src, void* dst, const int* idx, int rows, size_t row_bytes, int n_objects, int n_frames, int scatter,
                    sampt_stream_t stream) {
  if (!src || !dst || !idx) return fail(SAMPT_ERR_ARG, "sampt_move_rows: src, dst or idx is null");
  if (rows <= 0 || n_objects <= 0 || (scatter && n_frames <= 0))
    return fail(SAMPT_ERR_ARG, "sampt_move_rows: rows, n_objects (and n_frames of a scatter) must be positive");
  if (row_bytes == 0 || (row_bytes & 3) || (long)row_bytes <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_move_rows: row_bytes = " + std::to_string(row_bytes) + " is not a positive multiple of 4");
  if (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)idx) & 3) return fail(SAMPT_ERR_ARG, "sampt_move_rows: src, dst and idx must be 4-byte aligned");
  return move_rows(src, dst, idx, rows, (long)row_bytes, n_objects, n_frames, scatter, (hipStream_t)stream);
}

int sampt_fill_f32(float* dst, size_t n, float value, sampt_stream_t stream) {
  if (!dst || ((uintptr_t)dst & 3)) return fail(SAMPT_ERR_ARG, "sampt_fill_f32: dst must be non-null and 4-byte aligned");
  if (n == 0 || (long)n <= 0) return fail(SAMPT_ERR_ARG, "sampt_fill_f32: n must be positive");
  return fill_f32(dst, (long)n, value, (hipStream_t)stream);
}

int sampt_conv_stem7x7(const float* x_nhwc4, const float* w, const float* bias, float* y, int n, int H, int W, float eps,
                       float* mean_rstd, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  if (mean_rstd && stats_ws_bad(ws)) return fail(SAMPT_ERR_ARG, "sampt_conv_stem7x7: ws holds doubles: non-null, 8-byte aligned");
  const int chunks = conv_stem_tiles(H, W);
  if (mean_rstd && ws_bytes <(size_t)n * chunks * 64 * 2 * sizeof(double)) return SAMPT_ERR_WORKSPACE;
  SAMPT_TRY(conv_stem7x7_x3(x_nhwc4, w, bias, y, n, H, W, mean_rstd ? (double*)ws : nullptr, (hipStream_t)stream));
  if (!mean_rstd) return SAMPT_OK;
  const long hw = (long)((H + 6 - 7) / 2 + 1) * ((W + 6 - 7) / 2 + 1);
  return instnorm_finalize((const double*)ws, n, chunks, hw, 64, eps, mean_rstd, (hipStream_t)stream);
}

int sampt_conv3x3_planes_instnorm_stats(const void* x_hl, const void* w_hl, const float* bias, float* y, int n, int H, int W, int Cin,
                                        int Cout, float eps, float* mean_rstd, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  const ConvW c{nullptr, bias, (const half_t*)w_hl, Cin, Cout, 3, 3, 1, 1, 1};
  GemmP p = gemm_conv(c, x_hl, n, H, W, y);
  gemm_split_planes(p, c.w_hl);
  p.A_lo = (const half_t*)x_hl + (size_t)n * H * W * Cin;
  const int rc = x3_args_check(p);
  if (rc == SAMPT_ERR_ARG || !mean_rstd || stats_ws_bad(ws))
    return fail(SAMPT_ERR_ARG, "sampt_conv3x3_planes_instnorm_stats: x_hl, w_hl, y (and bias) non-null and 16-byte aligned, mean_rstd non-null, "
                               "ws non-null and 8-byte aligned");
  if (rc != SAMPT_OK || !conv3x3_halo_eligible(p)) return fail(SAMPT_ERR_UNSUPPORTED, "sampt_conv3x3_planes_instnorm_stats: Cin % 32, Cout % 4");
  const int chunks = conv3x3_halo_tiles(p);
  if (ws_bytes < (size_t)n * chunks * Cout * 2 * sizeof(double)) return SAMPT_ERR_WORKSPACE;
  p.in_part = (double*)ws;
  SAMPT_TRY(conv3x3_halo_x3(p, (hipStream_t)stream));
  return instnorm_finalize(p.in_part, n, chunks, (long)H * W, Cout, eps, mean_rstd, (hipStream_t)stream);
}

size_t sampt_instance_norm_workspace_bytes(int n, int hw, int C) {
  return instnorm_partial_doubles(n, hw, C) * sizeof(double) + (size_t)n * C * 2 * sizeof(float) + 512;
}

int sampt_instance_norm_nhwc(float* x, int n, int hw, int C, float eps, int relu, const float* skip, void* ws,
                             size_t ws_bytes, sampt_stream_t stream) {
  if (ws_bytes < sampt_instance_norm_workspace_bytes(n, hw, C)) return SAMPT_ERR_WORKSPACE;
  Arena a(ws, ws_bytes);
  double* part = (double*)a.get(instnorm_partial_doubles(n, hw, C) * sizeof(double));
  float* mr = a.f32((size_t)n * C * 2);
  SAMPT_TRY(instnorm_stats(x, n, hw, C, eps, part, mr, (hipStream_t)stream));
  return instnorm_apply(x, mr, skip, x, n, hw, C, relu, (hipStream_t)stream);
}

int sampt_layernorm(const float* x, const float* w, const float* b, void* y, int M, int D, float eps, int out_f16,
                    int act, sampt_stream_t stream) {
  return layernorm_rows(x, w, b, y, M, D, eps, nullptr, out_f16, act, (hipStream_t)stream);
}

int sampt_resize_bilinear_nhwc(const float* src, int n, int sh, int sw, int C, float* dst, int dh, int dw, int dstC,
                               int c_off, int align_corners, sampt_stream_t stream) {
  return resize_bilinear_nhwc(src, n, sh, sw, C, dst, dh, dw, dstC, c_off, align_corners, (hipStream_t)stream);
}

int sampt_avgpool2x2_nhwc(const float* src, int n, int h, int w, int C, float* dst, sampt_stream_t stream) {
  return avgpool2x2_nhwc(src, n, h, w, C, dst, (hipStream_t)stream);
}

int sampt_resize_logits(const float* src, int n, int sh, int sw, float* dst, int dh, int dw, sampt_stream_t stream) {
  if (!src || !dst || n <= 0) return SAMPT_ERR_ARG;
  return resize_logits(src, n, sh, sw, dst, dh, dw, (hipStream_t)stream);
}

int sampt_vos_index_masks(const float* logits, int M, int T, long hw, const int32_t* query_t, const uint8_t* gt_masks,
                          uint8_t* out, sampt_stream_t stream) {
  if (!logits || !out || !query_t || T <= 0 || hw <= 0) return SAMPT_ERR_ARG;
  return vos_index_masks(logits, M, T, hw, (const int*)query_t, gt_masks, out, (hipStream_t)stream);
}

int sampt_pil_resample_u8(const uint8_t* src, uint8_t* dst, long outer, int in_len, int out_len, int inner,
                          const int32_t* coef, const int32_t* bounds, int ksize, sampt_stream_t stream) {
  if (!src || !dst || !coef || !bounds || outer <= 0 || in_len <= 0 || out_len <= 0 || inner <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pil_resample_u8: bad arguments");
  return pil_resample_u8(src, dst, outer, in_len, out_len, inner, (const int*)coef, (const int*)bounds, ksize,
                         (hipStream_t)stream);
}

int sampt_vos_index_masks_resized(const float* logits, int M, int T, int h, int w, const int32_t* query_t,
                                  const uint8_t* gt_masks, int oh, int ow, uint8_t* out, sampt_stream_t stream) {
  if (!logits || !out || !query_t || T <= 0 || h <= 0 || w <= 0) return SAMPT_ERR_ARG;
  return vos_index_masks_resized(logits, M, T, h, w, (const int*)query_t, gt_masks, oh, ow, out, (hipStream_t)stream);
}

int sampt_index_masks(const float* logits, int M, long npix, uint8_t* out, sampt_stream_t stream) {
  if (!logits || !out || npix <= 0) return SAMPT_ERR_ARG;
  return index_masks(logits, M, npix, out, (hipStream_t)stream);
}

int sampt_corr_sample_f32(const float* const pyr[4], int H0, int W0, const int32_t* frame_idx, int S, int n,
                          const float* ffeats, const float* coords, float* out, sampt_stream_t stream) {
  return pips_corr_sample(make_pyr(pyr, H0, W0), frame_idx, S, n, 128, ffeats, coords, out, 196, 0, (hipStream_t)stream);
}

// Handle-free wrappers of the trackers' window kernels for the kernel tests (tests/test_gpu_tracker_kernels.py): every one refuses
// null pointers and non-positive counts before any launch.
int sampt_pips_corr_sample_ex(const float* const pyr[4], int H0, int W0, const int32_t* frame_idx, int S, int n, const float* ffeats,
                              const float* coords, float* x, int ldx, int xoff, const float* times, sampt_stream_t stream) {
  if (!pyr || !pyr[0] || !pyr[1] || !pyr[2] || !pyr[3] || !frame_idx || !ffeats || !coords || !x || S <= 0 || n <= 0 || H0 < 16 ||
      W0 < 16 || xoff < 0 || ldx < xoff + 196)
    return fail(SAMPT_ERR_ARG, "sampt_pips_corr_sample_ex: bad arguments (null pointer, S, n <= 0, H0, W0 < 16 or ldx < xoff + 196)");
  if (times && (xoff != 128 || ldx < 519 || ldx > 580))
    return fail(SAMPT_ERR_ARG, "sampt_pips_corr_sample_ex: the fused tail needs xoff == 128 and 519 <= ldx <= 580");
  return pips_corr_sample(make_pyr(pyr, H0, W0), (const int*)frame_idx, S, n, 128, ffeats, coords, x, ldx, xoff, (hipStream_t)stream,
                          times);
}

int sampt_pips_build_input_f32(const float* ffeats, const float* coords, const float* times, int S, int n, float* x, int ldx,
                               sampt_stream_t stream) {
  if (!ffeats || !coords || !times || !x || S <= 0 || n <= 0 || ldx < 519 || ldx > 580)
    return fail(SAMPT_ERR_ARG, "sampt_pips_build_input_f32: bad arguments (null pointer, S, n <= 0 or ldx outside [519, 580])");
  return pips_build_input(ffeats, coords, times, S, n, x, ldx, (hipStream_t)stream);
}

int sampt_pips_init_state_f32(const float* xys, const float* feat_init, float stride, int S, int n, float* coords, float* coords0,
                              float* ffeats, sampt_stream_t stream) {
  if (!xys || !feat_init || !coords || !coords0 || !ffeats || S <= 0 || n <= 0 || !(stride > 0.f))
    return fail(SAMPT_ERR_ARG, "sampt_pips_init_state_f32: bad arguments");
  return pips_init_state(xys, feat_init, stride, S, n, coords, coords0, ffeats, (hipStream_t)stream);
}

int sampt_pips_apply_update_f32(const float* delta, const float* gn_w, const float* gn_b, const float* up_wT, const float* up_b,
                                float* ffeats, float* coords, const float* coords0, int S, int n, sampt_stream_t stream) {
  if (!delta || !gn_w || !gn_b || !up_wT || !up_b || !ffeats || !coords || S <= 0 || n <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips_apply_update_f32: bad arguments");
  return pips_update(delta, gn_w, gn_b, up_wT, up_b, ffeats, coords, coords0, S, n, (hipStream_t)stream);
}

int sampt_pips_finalize_f32(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride, int S,
                            int n, float* traj, float* vis, sampt_stream_t stream) {
  if (!ffeats || !vis_w || !vis_b || !coords || !traj || !vis || S <= 0 || n <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips_finalize_f32: bad arguments");
  return pips_finalize(ffeats, vis_w, vis_b, coords, stride, S, n, traj, vis, (hipStream_t)stream);
}

int sampt_pips_chain_init(const float* q, int n, int T, int32_t* cur, float* traj, float* vis, sampt_stream_t stream) {
  if (!q || !cur || !traj || !vis || n <= 0 || T <= 0) return fail(SAMPT_ERR_ARG, "sampt_pips_chain_init: bad arguments");
  return pips_chain_init(q, n, T, (int*)cur, traj, vis, (hipStream_t)stream);
}

int sampt_pips_round_begin(const int32_t* cur, const uint8_t* flip, const float* traj, int T, int n, int S, int32_t* fidx, float* xys,
                           float* xy_feat, int32_t* f0, float stride, sampt_stream_t stream) {
  if (!cur || !flip || !traj || !fidx || !xys || T <= 0 || n <= 0 || S <= 0 || !xy_feat != !f0 || (xy_feat && !(stride > 0.f)))
    return fail(SAMPT_ERR_ARG, "sampt_pips_round_begin: bad arguments (xy_feat and f0 come together)");
  return pips_round_begin((const int*)cur, flip, traj, T, n, S, (int*)fidx, xys, xy_feat, (int*)f0, stride, (hipStream_t)stream);
}

int sampt_pips_round_end(int32_t* cur, const float* tr, const float* vi, int T, int n, int S, float thr0, float* traj, float* vis,
                         int32_t* n_active, sampt_stream_t stream) {
  if (!cur || !tr || !vi || !traj || !vis || !n_active || T <= 0 || n <= 0 || S <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips_round_end: bad arguments");
  return pips_round_end((int*)cur, tr, vi, T, n, S, thr0, traj, vis, (int*)n_active, (hipStream_t)stream);
}

int sampt_pips2_init_f32(const float* trajs0, const float* fmap, int H, int W, const int32_t* frame_idx, float stride, int S, int n,
                         int have_init, float* coords, float* bak, float* f1, float* f2, float* f4, sampt_stream_t stream) {
  if (!trajs0 || !coords || !bak || S <= 0 || n <= 0 || !(stride > 0.f) ||
      (!have_init && (!fmap || !frame_idx || !f1 || !f2 || !f4 || H <= 0 || W <= 0)))
    return fail(SAMPT_ERR_ARG, "sampt_pips2_init_f32: bad arguments");
  return pips2_init(trajs0, fmap, H, W, (const int*)frame_idx, stride, S, n, have_init, coords, bak, f1, f2, f4, (hipStream_t)stream);
}

int sampt_pips2_templates_f32(const float* fmap, int H, int W, const int32_t* frame_idx, const float* coords, int S, int n, float* f2,
                              float* f4, sampt_stream_t stream) {
  if (!fmap || !frame_idx || !coords || !f2 || !f4 || H <= 0 || W <= 0 || S <= 0 || n <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips2_templates_f32: bad arguments");
  return pips2_templates(fmap, H, W, (const int*)frame_idx, coords, S, n, f2, f4, (hipStream_t)stream);
}

int sampt_pips2_build_input_f32(const float* coords, const float* omega, int S, int n, float* x, int ldx, sampt_stream_t stream) {
  if (!coords || !omega || !x || S <= 0 || n <= 0 || ldx != 720)
    return fail(SAMPT_ERR_ARG, "sampt_pips2_build_input_f32: bad arguments (null pointer, S, n <= 0 or ldx != 720)");
  return pips2_build_input(coords, omega, S, n, x, ldx, (hipStream_t)stream);
}

int sampt_instnorm1d_relu_f32(const float* x, float* y, int n, int S, int C, sampt_stream_t stream) {
  if (!x || !y || n <= 0 || S <= 0 || C <= 0) return fail(SAMPT_ERR_ARG, "sampt_instnorm1d_relu_f32: bad arguments");
  return instnorm1d_relu(x, y, n, S, C, (hipStream_t)stream);
}

int sampt_add_chanpad_f32(float* out, const float* identity, long rows, int cin, int cout, int relu, sampt_stream_t stream) {
  if (!out || !identity || rows <= 0 || cin <= 0 || cout < cin) return fail(SAMPT_ERR_ARG, "sampt_add_chanpad_f32: bad arguments");
  return add_chanpad(out, identity, rows, cin, cout, relu, (hipStream_t)stream);
}

int sampt_pips2_apply_delta_f32(const float* delta, const float* bak, float stride, int S, int n, int last, float* coords, float* trajs,
                                sampt_stream_t stream) {
  if (!delta || !bak || !coords || (last && !trajs) || S <= 0 || n <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_pips2_apply_delta_f32: bad arguments");
  return pips2_apply_delta(delta, bak, stride, S, n, last, coords, trajs, (hipStream_t)stream);
}

int sampt_cot_prepare(const float* qxy, const int32_t* qt, const int32_t* frame_map, float stride, int n, int T, float* xy0,
                      int32_t* fidx_pt, float* traj_out, float* vis_out, sampt_stream_t stream) {
  if (!qxy || !qt || !frame_map || !xy0 || !fidx_pt || !traj_out || !vis_out || n <= 0 || T <= 0 || !(stride > 0.f))
    return fail(SAMPT_ERR_ARG, "sampt_cot_prepare: bad arguments");
  return cot_prepare(qxy, (const int*)qt, (const int*)frame_map, stride, n, T, xy0, (int*)fidx_pt, traj_out, vis_out, (hipStream_t)stream);
}

int sampt_cot_window_init(int ind, int S_local, int prev, int na, int S, const int32_t* qt, const float* xy0, const int32_t* frame_map,
                          const float* coords_prev, const float* vis_prev, const float* feat_init, float* coords, float* visin,
                          float* mask, int32_t* fidx, float* ffeats, sampt_stream_t stream) {
  if (!qt || !xy0 || !frame_map || !feat_init || !coords || !visin || !mask || !fidx || !ffeats || ind < 0 || S <= 0 || S_local <= 0 ||
      S_local > S || na <= 0 || prev < 0 || prev > na || (prev > 0 && (!coords_prev || !vis_prev)))
    return fail(SAMPT_ERR_ARG, "sampt_cot_window_init: bad arguments (0 <= prev <= na, 1 <= S_local <= S, carries needed when prev > 0)");
  return cot_window_init(ind, S_local, prev, na, S, (const int*)qt, xy0, (const int*)frame_map, coords_prev, vis_prev, feat_init, coords,
                         visin, mask, (int*)fidx, ffeats, (hipStream_t)stream);
}

int sampt_cot_pos_embed_f32(const float* coords, const float* pos_x, const float* pos_y, int H, int W, int E, int na, float* pos,
                            sampt_stream_t stream) {
  if (!coords || !pos_x || !pos_y || !pos || H <= 0 || W <= 0 || E <= 0 || (E & 1) || na <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_cot_pos_embed_f32: bad arguments");
  return cot_pos_embed(coords, pos_x, pos_y, H, W, E, na, pos, (hipStream_t)stream);
}

int sampt_cot_build_input_f32(const float* ffeats, const float* coords, const float* visin, const float* mask, const float* pos,
                              const float* times, int S, int na, float* x, sampt_stream_t stream) {
  if (!ffeats || !coords || !visin || !mask || !pos || !times || !x || S <= 0 || na <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_cot_build_input_f32: bad arguments");
  return cot_build_input(ffeats, coords, visin, mask, pos, times, S, na, x, (hipStream_t)stream);
}

int sampt_cot_window_store_f32(const float* ffeats, const float* vis_w, const float* vis_b, const float* coords, float stride, int S,
                               int na, int ind, int S_local, int n_total, float* coords_prev, float* vis_prev, float* traj_out,
                               float* vis_out, sampt_stream_t stream) {
  if (!ffeats || !vis_w || !vis_b || !coords || !coords_prev || !vis_prev || !traj_out || !vis_out || S <= 0 || na <= 0 || ind < 0 ||
      S_local <= 0 || S_local > S || n_total < na)
    return fail(SAMPT_ERR_ARG, "sampt_cot_window_store_f32: bad arguments (1 <= S_local <= S, na <= n_total)");
  return cot_window_store(ffeats, vis_w, vis_b, coords, stride, S, na, ind, S_local, n_total, coords_prev, vis_prev, traj_out, vis_out,
                          (hipStream_t)stream);
}

int sampt_pips_mix_mlp_f32(const float* x, const float* lnw, const float* lnb, const float* w1, const float* b1, const float* w2,
                           float* part, int nseq, int slices, sampt_stream_t stream) {
  if (!x || !lnw || !lnb || !w1 || !b1 || !w2 || !part) return fail(SAMPT_ERR_ARG, "sampt_pips_mix_mlp_f32: null pointer");
  return pips_mix_mlp(x, lnw, lnb, w1, b1, w2, part, nseq, slices, (hipStream_t)stream);
}

int sampt_pips_mix_reduce_f32(const float* part, int slices, const float* bias, const float* res, int nseq, int mode,
                              const float* lnw, const float* lnb, const float* tw1, const float* tb1, const float* tw2,
                              const float* tb2, float* out, sampt_stream_t stream) {
  if (!lnw || !lnb || (mode != 0 && mode != 1) || (mode == 0 && (!tw1 || !tb1 || !tw2 || !tb2)))
    return fail(SAMPT_ERR_ARG, "sampt_pips_mix_reduce_f32: bad arguments");
  return pips_mix_reduce(part, slices, bias, res, nseq, mode, lnw, lnb, tw1, tb1, tw2, tb2, out, (hipStream_t)stream);
}

size_t sampt_pips_mix_xop_halves(int nseq) { return nseq > 0 ? pips_mix_xop_halves(nseq) : 0; }

int sampt_pips_mix_pre_f32(const float* part, int slices, const float* bias, const float* res, int nseq, const float* ln1w,
                           const float* ln1b, const float* tw1, const float* tb1, const float* tw2, const float* tb2,
                           const float* ln2w, const float* ln2b, float* xout, void* xop, sampt_stream_t stream) {
  if (!ln1w || !ln1b || !tw1 || !tb1 || !tw2 || !tb2 || !ln2w || !ln2b) return fail(SAMPT_ERR_ARG, "sampt_pips_mix_pre_f32: null pointer");
  return pips_mix_pre(part, slices, bias, res, nseq, ln1w, ln1b, tw1, tb1, tw2, tb2, ln2w, ln2b, xout, (half_t*)xop, (hipStream_t)stream);
}

int sampt_pips_mix_mlp_x3(const void* xop, const void* wstream, const float* b1, float* part, int nseq, int slices,
                          sampt_stream_t stream) {
  return pips_mix_mlp_x3((const half_t*)xop, (const half_t*)wstream, b1, part, nseq, slices, (hipStream_t)stream);
}

int sampt_vit_attention_f16(const void* qkv, const float* rel_h, const float* rel_w, void* out, int B, int S, int heads,
                            int hd, void* ws, size_t ws_bytes, sampt_stream_t stream) {
  (void)ws, (void)ws_bytes;  // the decomposed rel-pos bias is computed inside the kernel: no scratch needed any more
  return vit_flash_attention_f16((const half_t*)qkv, rel_h, rel_w, (half_t*)out, B, S, heads, hd, (hipStream_t)stream);
}

int sampt_vit_attention_f16_head_major(const void* qkv, const float* rel_h, const float* rel_w, void* out, int B, int S, int heads,
                                       int hd, const void* bias_row, int nwx, int nwy, int grid_h, int grid_w, sampt_stream_t stream) {
  if (!qkv || !rel_h || !rel_w || !out || B <= 0 || (bias_row && (nwx <= 0 || nwy <= 0 || B % (nwx * nwy))))
    return fail(SAMPT_ERR_ARG, "sampt_vit_attention_f16_head_major: bad arguments");
  FlashPad fp;
  fp.head_major = 1;
  if (bias_row) fp.bias_row = (const half_t*)bias_row, fp.nwx = nwx, fp.nwin = nwx * nwy, fp.gh = grid_h, fp.gw = grid_w;
  return vit_flash_attention_f16((const half_t*)qkv, rel_h, rel_w, (half_t*)out, B, S, heads, hd, (hipStream_t)stream, fp);
}

int sampt_gemm_f16_head_major(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int heads, int hd,
                              int rows, const int32_t* rowmap, sampt_stream_t stream) {
  if (!A || !W || !C || heads <= 0 || hd <= 0 || rows <= 0) return fail(SAMPT_ERR_ARG, "sampt_gemm_f16_head_major: bad arguments");
  GemmP p = gemm_linear(A, K, W, bias, C, N, M, N, K);
  p.rowmap = rowmap, p.out_f16 = 1, p.hm_heads = heads, p.hm_hd = hd, p.hm_rows = rows;
  int rc = gemm_f16(p, (hipStream_t)stream);
  return rc == SAMPT_ERR_ARG ? fail(rc, "sampt_gemm_f16_head_major: need hd % 4 == 0, N % (heads * hd) == 0, rows >= M without a rowmap")
                             : rc;
}

int sampt_vit_attention_x3(const void* qkv, const float* rel_h, const float* rel_w, void* out, int B, int S, int heads,
                           int hd, sampt_stream_t stream) {
  if (!qkv || !rel_h || !rel_w || !out) return fail(SAMPT_ERR_ARG, "sampt_vit_attention_x3: bad arguments");
  return vit_flash_attention_x3((const half_t*)qkv, rel_h, rel_w, (half_t*)out, B, S, heads, hd, (hipStream_t)stream);
}

int sampt_vit_window_attention(int precision, const void* qkv, const float* rel_h, const float* rel_w, void* out, int frames,
                               int S, int heads, int hd, const void* bias_row, int nwx, int nwy, int grid_h, int grid_w,
                               sampt_stream_t stream) {
  if (!qkv || !rel_h || !rel_w || !out || !bias_row || frames <= 0 || nwx <= 0 || nwy <= 0)
    return fail(SAMPT_ERR_ARG, "sampt_vit_window_attention: bad arguments");
  FlashPad fp;
  fp.bias_row = (const half_t*)bias_row, fp.nwx = nwx, fp.nwin = nwx * nwy, fp.gh = grid_h, fp.gw = grid_w;
  const int B = frames * nwx * nwy;
  if (precision == 1)
    return vit_flash_attention_f16((const half_t*)qkv, rel_h, rel_w, (half_t*)out, B, S, heads, hd, (hipStream_t)stream, fp);
  if (precision == 2)
    return vit_flash_attention_x3((const half_t*)qkv, rel_h, rel_w, (half_t*)out, B, S, heads, hd, (hipStream_t)stream, fp);
  return fail(SAMPT_ERR_ARG, "sampt_vit_window_attention: precision must be 1 (fp16) or 2 (x3 rows)");
}

int sampt_attention_f32(int kind, const float* q, const float* k, const float* v, float* out, int F, int Nq, int Nk,
                        int heads, int hd, const int32_t* nk_item, sampt_stream_t stream) {
  if (!q || !k || !v || !out) return fail(SAMPT_ERR_ARG, "sampt_attention_f32: bad arguments");
  if (kind == 0) return attn_rowblock(q, k, v, out, F, Nq, Nk, heads, hd, (const int*)nk_item, (hipStream_t)stream);
  if (kind == 1) return attn_fewkeys(q, k, v, out, F, Nq, Nk, heads, hd, (const int*)nk_item, (hipStream_t)stream);
  return SAMPT_ERR_UNSUPPORTED;
}

int sampt_attention_t2i_workspace_bytes(int F, int Nq, int Nk, size_t* bytes) {
  if (!bytes || F <= 0 || Nq <= 0 || Nk <= 0) return SAMPT_ERR_ARG;
  *bytes = attn_t2i_workspace_floats(F, Nq, Nk) * sizeof(float) + 16;
  return SAMPT_OK;
}

int sampt_attention_t2i_f32(const float* q, const float* k, const float* v, float* out, int F, int Nq, int Nk, void* ws,
                            size_t ws_bytes, sampt_stream_t stream) {
  if (!q || !k || !v || !out) return fail(SAMPT_ERR_ARG, "sampt_attention_t2i_f32: bad arguments");
  return attn_t2i(q, k, v, out, F, Nq, Nk, (float*)ws, ws_bytes / sizeof(float), (hipStream_t)stream);
}

int sampt_cotracker_attention_f32(const float* qkv, float* out, int nbatch, int L, int batch_stride_rows,
                                  int token_stride_rows, int heads, int hd, sampt_stream_t stream) {
  if (!qkv || !out) return fail(SAMPT_ERR_ARG, "sampt_cotracker_attention_f32: bad arguments");
  return cot_attention(qkv, out, nbatch, L, batch_stride_rows, token_stride_rows, heads, hd, (hipStream_t)stream);
}

}  // extern "C"
