// amhip_api.hip -- C ABI of libaerial_mapper_hip.so (see
// include/aerial_mapper_hip.h): context, layers, parameter set-up, host
// staging, timing.  Kernels live in amhip_dsm.hip / amhip_ortho.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "amhip_common.h"
#include "amhip_ortho_blend.h"
#include "amhip_ortho_plan.h"

namespace amhip {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

void set_last_error(const std::string& msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "HIP error %d (%s) in `%s` at %s:%d", (int)e,
                hipGetErrorString(e), what, file, line);
  set_last_error(buf);
  return e == hipErrorOutOfMemory ? AMHIP_ERR_NOMEM : AMHIP_ERR_HIP;
}

static int arg_fail(const char* msg) {
  set_last_error(msg);
  return AMHIP_ERR_ARG;
}

// ---------------------------------------------------------------------------
// memory
// ---------------------------------------------------------------------------
int ensure_bytes(void** ptr, size_t* cap_bytes, size_t need_bytes) {
  if (*cap_bytes >= need_bytes && *ptr) return AMHIP_OK;
  if (*ptr) {
    AMHIP_TRY(hipFree(*ptr));
    *ptr = nullptr;
    *cap_bytes = 0;
  }
  // grow by 1/8 so that slightly larger follow-up clouds do not reallocate
  size_t want = need_bytes + need_bytes / 8 + 256;
  hipError_t e = hipMalloc(ptr, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    want = need_bytes;
    AMHIP_TRY(hipMalloc(ptr, want));
  }
  *cap_bytes = want;
  return AMHIP_OK;
}

template <typename T>
int ensure_capacity(T** ptr, size_t* cap, size_t need) {
  size_t cap_bytes = *cap * sizeof(T);
  void* p = *ptr;
  const int rc = ensure_bytes(&p, &cap_bytes, need * sizeof(T));
  *ptr = static_cast<T*>(p);
  *cap = cap_bytes / sizeof(T);
  return rc;
}
template int ensure_capacity<double>(double**, size_t*, size_t);
template int ensure_capacity<uint32_t>(uint32_t**, size_t*, size_t);
template int ensure_capacity<uint8_t>(uint8_t**, size_t*, size_t);
template int ensure_capacity<int32_t>(int32_t**, size_t*, size_t);
template int ensure_capacity<FramePose>(FramePose**, size_t*, size_t);

// ---------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------
ScopedTimer::ScopedTimer(Ctx* ctx, int slot) : c(ctx), on(ctx->timing) {
  if (!on) return;
  if (!c->free_regions.empty()) {
    r = c->free_regions.back();
    c->free_regions.pop_back();
  } else {
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
      on = false;
      return;
    }
  }
  r.slot = slot;
  (void)hipEventRecord(r.a, c->stream);
}

ScopedTimer::~ScopedTimer() {
  if (!on) return;
  (void)hipEventRecord(r.b, c->stream);
  c->regions.push_back(r);
}

static void drain_timers(Ctx* c) {
  for (TimedRegion& r : c->regions) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess &&
        hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->slot_ms[r.slot] += ms;
      c->slot_launches[r.slot] += 1;
    }
    c->free_regions.push_back(r);
  }
  c->regions.clear();
}

// ---------------------------------------------------------------------------
// parameter set-up
// ---------------------------------------------------------------------------
// grid_bases: amhip_dsm_plan.h.  The mosaic's poses, view bounds and plan: amhip_ortho_plan.h

// The opt-in single-precision mode protects itself on rough terrain.  A
// tile whose height range leaves no room under the error bound is done by the FP64 kernel, which
// in that mode stages its points from the caller's UNSORTED cloud through the records' row
// indices (24 of every 64 bytes it touches); beyond about half the tiles that costs more than the
// records save in the sort.  The context knows the previous call's share (the pinned mirror of
// its tile counters, never waited for -- a value one or two calls late is as good): above one
// half, this call and the next 15 run the FP64 pipeline outright (sorted doubles), then the
// single-precision pipeline is tried once more.  Results: FP64 is the stricter arithmetic, every
// bar of the single-precision mode holds.  tuning knob dsm_no_rough_switch disables the switch.
static void dsm_rough_policy(Ctx* c) {
  const bool off = tuning_on("dsm_no_rough_switch");  // (looked up per call: tests toggle it)
  RoughState s = {c->rough_hold, c->last_call_f32, c->last_ntiles};
  c->dsm_exact_now = rough_policy_step(&s, !(c->dsm_exact || c->dsm_knn || off), c->host_tile_stats);
  c->rough_hold = s.hold;
}

// The plan of a DSM call on window (i0, j0, rows, cols) of the context's map (amhip_dsm_plan.h: plan_dsm;
// mode and pcl_lambda as there): the context's precision state and the tuning knobs of this moment.
static int make_dsm_plan(const Ctx& c, int i0, int j0, int rows, int cols, int radius_sq, double center_easting,
                         double center_northing, DsmParams* out, int mode, int pcl_lambda, size_t num_points) {
  DsmPlanInput in = {};
  in.grid = c.grid;
  in.win_i0 = i0;
  in.win_j0 = j0;
  in.win_rows = rows;
  in.win_cols = cols;
  in.radius_sq = radius_sq;
  in.center_easting = center_easting;
  in.center_northing = center_northing;
  in.mode = mode;
  in.pcl_lambda = pcl_lambda;
  in.num_points = num_points;
  in.dsm_exact = c.dsm_exact;
  in.dsm_exact_now = c.dsm_exact_now;
  in.dsm_knn = c.dsm_knn;
  in.canon_all = tuning_on("dsm_canon_all") ? 1 : 0;
  in.p3_min_points = (size_t)tuning("p3_min_points", (double)(1u << 20));
  in.p3_target = tuning("p3_target", 1536.0);
  in.p3_cap = (int)tuning("p3_cap", 2048.0);
  in.knn_global_bins = tuning_on("knn_global_bins") ? 1 : 0;
#ifdef AMHIP_TIMING_PROBES
  in.gather_tj = tuning("gather_tj", 0.0);
  in.fx_theta = tuning("fx_theta", 0.0);
#endif
  const char* why = "";
  return plan_dsm(in, out, &why) ? arg_fail(why) : AMHIP_OK;
}
// ... on the context's whole window
static int make_dsm_params(const Ctx& c, int radius_sq, double center_easting, double center_northing,
                           DsmParams* out, int mode, int pcl_lambda, size_t num_points) {
  return make_dsm_plan(c, c.win_i0, c.win_j0, c.win_rows, c.win_cols, radius_sq, center_easting, center_northing,
                       out, mode, pcl_lambda, num_points);
}

// A SMALL cloud onto a LARGE resident map (the incremental demo: one stereo pair's 360 K points
// per call onto a map of 1e8 .. 1.6e9 cells, main-ortho-backward-grid-incremental.cc:143-157).
// Binned over the context's whole window the call costs O(map): a 400 MB memset and scan of the
// bin table of a 40 000 x 40 000 map, an occupancy pre-pass over its 1.5 M gather tiles -- 0.75 ms
// for 0.05 ms of work.  Instead: the bounding box of the points the binning would accept (one
// pass over the cloud, five integers back to the host: the one synchronisation of such a call),
// grown by the last fallback radius -- no cell outside it can receive a value -- becomes the
// window of THIS call; the kernels run unchanged on it and write into the full layer
// (DsmParams::out_*).  Only while the layer is materialized (a lazily reset layer has to be
// written everywhere).  tuning knob dsm_no_subwindow: never.
// Returns 1: *p_sub is the call's parameter set; 0: run on the whole window; 2: no point near the
// window, nothing to do; < 0: error.
static int dsm_subwindow(Ctx* c, const double* dev_xyz, size_t n, int radius_sq, double center_easting,
                         double center_northing, const DsmParams& p_full, DsmParams* p_sub) {
  if (n > (1u << 20) || c->cells < (size_t)(4u << 20) || !c->dev_bbox || !c->host_bbox ||
      tuning_on("dsm_no_subwindow"))
    return 0;
  int rc;
  if ((rc = dsm_bbox_run(c, dev_xyz, n, p_full, c->dev_bbox))) return -rc;
  if (hipMemcpyAsync(c->host_bbox, c->dev_bbox, 5 * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return -hip_fail(hipGetLastError(), "bounding box of the cloud", __FILE__, __LINE__);
  if (c->host_bbox[4] == 0) return 2;
  // (k_dsm_bbox's biased words: an all-zero buffer is the empty box)
  const int b[4] = {kBboxBias - c->host_bbox[0], c->host_bbox[1] - kBboxBias,
                    kBboxBias - c->host_bbox[2], c->host_bbox[3] - kBboxBias};
  const int grow = p_full.w[p_full.nlevels - 1] + 2;   // last radius of the ladder, in cells (+ slack)
  const int i_lo = std::max(0, b[0] - grow), i_hi = std::min(p_full.rows - 1, b[1] + grow);
  const int j_lo = std::max(0, b[2] - grow), j_hi = std::min(p_full.cols - 1, b[3] + grow);
  if (i_lo > i_hi || j_lo > j_hi) return 2;             // (every binned point lies beyond the border by more than the radius)
  const size_t sub = (size_t)(i_hi - i_lo + 1) * (size_t)(j_hi - j_lo + 1);
  if (sub * 4 > c->cells) return 0;                     // not small against the map: nothing to win
  // the same context, seen through the sub-window
  rc = make_dsm_plan(*c, c->win_i0 + i_lo, c->win_j0 + j_lo, i_hi - i_lo + 1, j_hi - j_lo + 1, radius_sq,
                     center_easting, center_northing, p_sub, 0, 1, n);
  if (rc) return -rc;
  p_sub->out_i0 = i_lo;
  p_sub->out_j0 = j_lo;
  p_sub->out_pitch = c->win_rows;
  return 1;
}

static float layer_init_value(int layer) {
  // aerial-mapper-grid-map.cc:40-48
  switch (layer) {
    case AMHIP_LAYER_ORTHO:
      return 255.0f;
    case AMHIP_LAYER_ELEVATION_ANGLE:
    case AMHIP_LAYER_NUM_OBSERVATIONS:
      return 0.0f;
    default:
      return std::numeric_limits<float>::quiet_NaN();
  }
}

static int use_device(Ctx* c) {
  AMHIP_TRY(hipSetDevice(c->device));
  return AMHIP_OK;
}

static int fetch_status(Ctx* c) {
  // dev_err -> pinned mirror, then clear
  AMHIP_TRY(hipMemcpyAsync(c->host_err, c->dev_err, sizeof(unsigned),
                           hipMemcpyDeviceToHost, c->stream));
  AMHIP_TRY(hipMemsetAsync(c->dev_err, 0, sizeof(unsigned), c->stream));
  AMHIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned e = *c->host_err;
  if (e & kDevErrExactHit) {
    set_last_error(
        "a point coincides with a cell centre (reference: dsm.cc:165 "
        "CHECK(distances[i] > 0.0))");
    return AMHIP_ERR_EXACT_HIT;
  }
  if (e & kDevErrAlphaNonPos) {
    set_last_error(
        "observation angle alpha <= 0 (reference: ortho-backward-grid.cc:178 "
        "CHECK(alpha > 0.0))");
    return AMHIP_ERR_ALPHA_NONPOS;
  }
  if (e & kDevErrRectifyZeroW) {
    set_last_error("rectification: w == 0 (reference: rectifier.cpp:93,99 CHECK_NE(xyw(2), 0.0))");
    return AMHIP_ERR_ARG;
  }
  if (e & kDevErrHaloOverflow) {
    set_last_error(
        "tiled DSM: more halo points for a neighbouring window than send rows were reserved "
        "(cap_per_dest): the elevation near that edge is incomplete");
    return AMHIP_ERR_HALO_OVERFLOW;
  }
  return AMHIP_OK;
}

// tiled DSM: a selection that did not fit its send rows must fail the step (the points beyond
// the capacity were not shipped), without a host round trip inside the step
__global__ void k_halo_overflow_check(const unsigned long long* __restrict__ counts, int nd,
                                      unsigned long long cap, unsigned* __restrict__ dev_err) {
  if ((int)threadIdx.x < nd && counts[threadIdx.x] > cap) atomicOr(dev_err, kDevErrHaloOverflow);
}

static bool valid_layer(int l) { return l >= 0 && l < AMHIP_NUM_LAYERS; }

}  // namespace amhip

using namespace amhip;

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int amhip_abi_version(void) { return AMHIP_ABI_VERSION; }

const char* amhip_last_error(void) { return g_last_error.c_str(); }

void amhip_make_grid(double length_x, double length_y, double resolution,
                     double pos_x, double pos_y, amhip_grid_desc* out) {
  if (!out) return;
  out->rows = static_cast<int>(std::round(length_x / resolution));
  out->cols = static_cast<int>(std::round(length_y / resolution));
  out->resolution = resolution;
  out->length_x = static_cast<double>(out->rows) * resolution;
  out->length_y = static_cast<double>(out->cols) * resolution;
  out->pos_x = pos_x;
  out->pos_y = pos_y;
}

void amhip_cell_position(const amhip_grid_desc* grid, int i, int j, double* x,
                         double* y) {
  double bx, by;
  grid_bases(*grid, &bx, &by);
  if (x) *x = bx + grid->resolution * (-static_cast<double>(i));
  if (y) *y = by + grid->resolution * (-static_cast<double>(j));
}

int amhip_ctx_create(const amhip_grid_desc* grid, int device, amhip_ctx** out) {
  if (!grid) return arg_fail("amhip_ctx_create: null argument");
  return amhip_ctx_create_window(grid, 0, 0, grid->rows, grid->cols, device, out);
}

int amhip_ctx_create_window(const amhip_grid_desc* grid, int i0, int j0, int rows, int cols,
                            int device, amhip_ctx** out) {
  if (!grid || !out) return arg_fail("amhip_ctx_create: null argument");
  if (grid->rows <= 0 || grid->cols <= 0 || !(grid->resolution > 0.0))
    return arg_fail("amhip_ctx_create: empty grid");
  if (i0 < 0 || j0 < 0 || rows <= 0 || cols <= 0 || i0 + rows > grid->rows ||
      j0 + cols > grid->cols)
    return arg_fail("amhip_ctx_create_window: window outside the map");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    set_last_error("no HIP device visible (libaerial_mapper_hip needs a gfx950 GPU)");
    return AMHIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return arg_fail("amhip_ctx_create: bad device index");
  amhip_ctx* h = new (std::nothrow) amhip_ctx();
  if (!h) return AMHIP_ERR_NOMEM;
  Ctx* c = &h->impl;
  c->grid = *grid;
  c->device = device;
  c->win_i0 = i0;
  c->win_j0 = j0;
  c->win_rows = rows;
  c->win_cols = cols;
  c->windowed = rows != grid->rows || cols != grid->cols;
  c->cells = static_cast<size_t>(rows) * static_cast<size_t>(cols);
  // reference-identical by default; FAST is opt-in (setter, or AMHIP_DSM_FAST=1 for hosts that
  // cannot be recompiled; AMHIP_DSM_EXACT=1 wins over it)
  {
    c->dsm_exact = amhip_default_dsm_precision() == AMHIP_DSM_EXACT ? 1 : 0;
  }
  int rc = AMHIP_OK;
  do {
    if ((rc = use_device(c))) break;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
      rc = hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
      break;
    }
    c->stream = c->own_stream;
    hipError_t e = hipSuccess;
    for (int l = 0; l < AMHIP_NUM_LAYERS && e == hipSuccess; ++l)
      e = hipMalloc(reinterpret_cast<void**>(&c->layers[l]), c->cells * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->dev_err), 4 * sizeof(unsigned));
    if (e == hipSuccess)
      e = hipMalloc(reinterpret_cast<void**>(&c->dev_zrange), 4 * sizeof(unsigned long long));  // [2], [3]: the last DSM call's own range
    if (e == hipSuccess)
      e = hipHostMalloc(reinterpret_cast<void**>(&c->host_err), sizeof(unsigned), 0);
    if (e == hipSuccess) {
      e = hipHostMalloc(reinterpret_cast<void**>(&c->host_tile_stats), 8 * sizeof(unsigned), 0);
      if (e == hipSuccess) std::memset(c->host_tile_stats, 0, 8 * sizeof(unsigned));
    }
    if (e == hipSuccess) {
      e = hipHostMalloc(reinterpret_cast<void**>(&c->host_sort_stats), 4 * sizeof(unsigned), 0);
      if (e == hipSuccess) std::memset(c->host_sort_stats, 0xFF, 4 * sizeof(unsigned));  // ("unknown")
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->dev_tickets), 16 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemsetAsync(c->dev_tickets, 0, 16 * sizeof(unsigned), c->stream);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->dev_bbox), 8 * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->host_bbox), 8 * sizeof(int), 0);
    if (e == hipSuccess) e = hipMemsetAsync(c->dev_err, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) {
      rc = hip_fail(e, "context allocation", __FILE__, __LINE__);
      break;
    }
    rc = amhip_layers_reset(h);
  } while (0);
  if (rc != AMHIP_OK) {
    const std::string keep = g_last_error;
    amhip_ctx_destroy(h);
    set_last_error(keep);
    return rc;
  }
  *out = h;
  return AMHIP_OK;
}

void amhip_ctx_destroy(amhip_ctx* h) {
  if (!h) return;
  Ctx* c = &h->impl;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drain_timers(c);
  for (TimedRegion& r : c->free_regions) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l)
    if (c->layers[l]) (void)hipFree(c->layers[l]);
  void* bufs[] = {c->dev_bbox, c->ortho_list, c->zpart, c->dev_zrange, c->tile_list, c->tile_occ, c->fill_mask, c->stage_values, c->dev_err, c->sorted,       c->rank,        c->bin_start, c->bin_z, c->rec_a, c->rec_b, c->rec16, c->sidx, c->zref, c->zall, c->tmp_points, c->stripe_ws,
                  c->scan_partials, c->stage_points, c->frame_poses, c->stage_frames, c->stereo_ws,
                  c->blend_sums[0], c->blend_sums[1]};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  jpeg_scratch_free(&c->jpeg);
  if (c->host_err) (void)hipHostFree(c->host_err);
  if (c->host_tile_stats) (void)hipHostFree(c->host_tile_stats);
  if (c->host_sort_stats) (void)hipHostFree(c->host_sort_stats);
  if (c->dev_tickets) (void)hipFree(c->dev_tickets);
  if (c->host_bbox) (void)hipHostFree(c->host_bbox);
  if (c->order_event) (void)hipEventDestroy(c->order_event);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete h;
}

int amhip_ctx_set_dsm_precision(amhip_ctx* h, int mode) {
  if (!h) return arg_fail("null context");
  if (mode != AMHIP_DSM_FAST && mode != AMHIP_DSM_EXACT) return arg_fail("unknown DSM precision mode");
  h->impl.dsm_exact = mode == AMHIP_DSM_EXACT ? 1 : 0;
  return AMHIP_OK;
}

int amhip_ctx_set_dsm_knn(amhip_ctx* h, int k) {
  if (!h) return arg_fail("null context");
  if (k < 0 || k > 8) return arg_fail("amhip_ctx_set_dsm_knn: k must be 0 (off) .. 8");
  h->impl.dsm_knn = k;
  return AMHIP_OK;
}

int amhip_ctx_set_stream(amhip_ctx* h, void* hip_stream) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  AMHIP_TRY(hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
  return AMHIP_OK;
}

int amhip_ctx_synchronize(amhip_ctx* h) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  return fetch_status(c);
}

// every elevation is NaN again: empty height range
static int zrange_reset(Ctx* c) {
  static const unsigned long long empty[2] = {0xFFF0000000000000ull, 0x000FFFFFFFFFFFFFull};
  AMHIP_TRY(hipMemcpyAsync(c->dev_zrange, empty, sizeof(empty), hipMemcpyHostToDevice, c->stream));
  c->zrange_valid = true;
  return AMHIP_OK;
}

// a transition of amhip_session_plan.h: the fill it asks for, then the state it gives
static int apply_step(Ctx* c, int layer, LayerStep step) {
  if (step.fill) {
    const int rc = launch_fill(c, c->layers[layer], c->cells, layer_init_value(layer));
    if (rc) return rc;
  }
  c->layer_state[layer] = step.state;
  return AMHIP_OK;
}

int amhip_layers_reset(amhip_ctx* h) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  // Lazy: nothing is written here.  A layer that is already in its initial
  // state (physically or logically) stays as it is; a written one becomes
  // "logically initial": the next kernel that produces it writes the initial
  // value into the cells it leaves alone (fused fill), anything else that
  // needs the memory (download, device pointer, a partial writer) fills it
  // first (materialize()).  Layers whose device pointer was handed out are
  // refilled eagerly.  tuning knob eager_reset restores the plain fills.
  const bool eager = tuning_on("eager_reset");
  if ((rc = zrange_reset(c))) return rc;
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l) {
    if ((rc = apply_step(c, l, layer_reset(c->layer_state[l], eager)))) return rc;
  }
  return AMHIP_OK;
}

// the layer's memory is about to be read or partially written by someone who
// does not know about the lazy state
static int materialize(Ctx* c, int layer) {
  return apply_step(c, layer, layer_materialize(c->layer_state[layer]));
}

// What the last writing call can have written: the whole window, unless the call narrows it
// afterwards (a small cloud's sub-window, a small batch's tile list).  Every writer passes here --
// touch() / overwrite() / the fused-fill branches -- so a rectangle never outlives its call
// (the tiled / OrthoFromPcl / empty-cloud entry points used to leave the previous one).
static void dirty_full(Ctx* c) {
  c->dirty_on_device = false;
  c->dirty[0] = c->dirty[1] = 0;
  c->dirty[2] = c->win_rows;
  c->dirty[3] = c->win_cols;
}

// partial writer: materialize, then dirty
static int touch(Ctx* c, int layer) {
  dirty_full(c);
  return apply_step(c, layer, layer_touch(c->layer_state[layer]));
}

// a kernel that produces the whole layer claims it; true: the layer was logically initial and the
// kernel has to write the initial value into the cells it leaves alone (fused fill)
static bool claim_output(Ctx* c, int layer) {
  dirty_full(c);
  const LayerStep step = layer_claim_output(c->layer_state[layer]);
  c->layer_state[layer] = step.state;
  return step.fill;
}

// full overwrite (upload): no need to fill first
static void overwrite(Ctx* c, int layer) {
  dirty_full(c);
  c->layer_state[layer] = layer_overwrite(c->layer_state[layer]);
  if (layer == AMHIP_LAYER_ELEVATION) c->zrange_valid = false;  // heights from outside
}

}  // extern "C"

namespace amhip {
int ctx_use_device(Ctx* c) { return use_device(c); }
int ctx_last_dirty(Ctx* c, int rect[4]) {
  if (c->dirty_on_device) {
    // (k_ortho_tile_list left [min tx, max tx, min ty, max ty] of the listed tiles behind the count)
    if (!c->ortho_list || !c->host_bbox) return arg_fail("no tile list");
    AMHIP_TRY(hipMemcpyAsync(c->host_bbox, c->ortho_list, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    AMHIP_TRY(hipStreamSynchronize(c->stream));
    const int* b = c->host_bbox;
    if (b[0] == 0 || b[4] > b[5] || b[6] > b[7]) {
      c->dirty[0] = c->dirty[1] = c->dirty[2] = c->dirty[3] = 0;
    } else {
      const int i0 = b[4] * 64, j0 = b[6] * 64;   // (the mosaic's tiles: 64 x 64 cells)
      c->dirty[0] = i0;
      c->dirty[1] = j0;
      c->dirty[2] = std::min(c->win_rows, (b[5] + 1) * 64) - i0;
      c->dirty[3] = std::min(c->win_cols, (b[7] + 1) * 64) - j0;
    }
    c->dirty_on_device = false;
  }
  for (int k = 0; k < 4; ++k) rect[k] = c->dirty[k];
  return AMHIP_OK;
}
int ctx_materialize(Ctx* c, int layer) { return materialize(c, layer); }
void ctx_overwrite(Ctx* c, int layer) { overwrite(c, layer); }
int ctx_fetch_status(Ctx* c) { return fetch_status(c); }
float ctx_layer_init_value(int layer) { return layer_init_value(layer); }
bool ctx_layer_is_initial(const Ctx* c, int layer) {
  return layer_is_initial(c->layer_state[layer]);
}
int arg_failure(const char* msg) { return arg_fail(msg); }
int ctx_stage_cloud(Ctx* c, const double* host_xyz, const int32_t* host_values, size_t n) {
  int rc = ensure_capacity(&c->stage_points, &c->stage_points_cap, 3 * n);
  if (rc == AMHIP_OK && host_values) rc = ensure_capacity(&c->stage_values, &c->stage_values_cap, n);
  if (rc) return rc;
  AMHIP_TRY(hipMemcpyAsync(c->stage_points, host_xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (host_values)
    AMHIP_TRY(hipMemcpyAsync(c->stage_values, host_values, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return AMHIP_OK;
}
int ctx_stage_frames(Ctx* c, const uint8_t* const* images, const size_t* steps, size_t F, size_t row, size_t height) {
  for (size_t f = 0; f < F; ++f) {
    if (!images[f]) return arg_fail("null image");
    if (steps[f] < row) return arg_fail("image step smaller than a row");
  }
  const size_t frame = row * height;
  const int rc = ensure_capacity(&c->stage_frames, &c->stage_frames_cap, frame * F);
  if (rc) return rc;
  for (size_t f = 0; f < F; ++f) {
    if (steps[f] == row)
      AMHIP_TRY(hipMemcpyAsync(c->stage_frames + f * frame, images[f], frame, hipMemcpyHostToDevice, c->stream));
    else
      AMHIP_TRY(hipMemcpy2DAsync(c->stage_frames + f * frame, row, images[f], steps[f], row, height,
                                 hipMemcpyHostToDevice, c->stream));
  }
  return AMHIP_OK;
}
int ctx_layer_set_initial(Ctx* c, int layer) {
  if (layer == AMHIP_LAYER_ELEVATION) {
    const int rc = zrange_reset(c);
    if (rc) return rc;
  }
  return apply_step(c, layer, layer_set_initial(c->layer_state[layer]));  // (handed out: eager)
}
}  // namespace amhip

extern "C" {

int amhip_layer_upload(amhip_ctx* h, int layer, const float* host) {
  if (!h || !host || !valid_layer(layer)) return arg_fail("amhip_layer_upload: bad argument");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  overwrite(c, layer);
  AMHIP_TRY(hipMemcpyAsync(c->layers[layer], host, c->cells * sizeof(float),
                           hipMemcpyHostToDevice, c->stream));
  AMHIP_TRY(hipStreamSynchronize(c->stream));
  return AMHIP_OK;
}

int amhip_layer_download(amhip_ctx* h, int layer, float* host) {
  if (!h || !host || !valid_layer(layer)) return arg_fail("amhip_layer_download: bad argument");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  if ((rc = materialize(c, layer))) return rc;
  AMHIP_TRY(hipMemcpyAsync(host, c->layers[layer], c->cells * sizeof(float),
                           hipMemcpyDeviceToHost, c->stream));
  AMHIP_TRY(hipStreamSynchronize(c->stream));
  return AMHIP_OK;
}

void* amhip_layer_device_ptr(amhip_ctx* h, int layer) {
  if (!h || !valid_layer(layer)) return nullptr;
  Ctx* c = &h->impl;
  if (use_device(c) != AMHIP_OK || materialize(c, layer) != AMHIP_OK) return nullptr;
  c->layer_state[layer] = kLayerHandedOut;  // the caller may write through the pointer at any time
  if (layer == AMHIP_LAYER_ELEVATION) c->zrange_valid = false;
  return c->layers[layer];
}

// ---- DSM ------------------------------------------------------------------

int amhip_dsm_process_dev(amhip_ctx* h, const double* dev_xyz, size_t n,
                          int radius_sq, double center_easting,
                          double center_northing) {
  if (!h) return arg_fail("null context");  // CHECK(map), dsm.cc:194
  if (n == 0) {                               // empty cloud: warning + return -- nothing written
    h->impl.dirty_on_device = false;
    h->impl.dirty[0] = h->impl.dirty[1] = h->impl.dirty[2] = h->impl.dirty[3] = 0;
    return AMHIP_OK;
  }
  if (!dev_xyz) return arg_fail("amhip_dsm_process_dev: null point pointer");
  if (radius_sq <= 0)
    return arg_fail("interpolation_radius must be >= 1 (the reference loops forever on 0)");
  if (n >= 0x7FFFFFFFull)
    return arg_fail("more than 2^31-1 points (the reference indexes results with int)");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  DsmParams p;
  dsm_rough_policy(c);
  if ((rc = make_dsm_params(*c, radius_sq, center_easting, center_northing, &p, 0, 1, n)))
    return rc;
  // a logically-initial elevation layer is filled by the gather itself
  const bool fused_fill = claim_output(c, AMHIP_LAYER_ELEVATION);
  if (!fused_fill) {  // a small cloud onto a large materialized map: its bounding box is the window
    DsmParams ps;
    const int sw = dsm_subwindow(c, dev_xyz, n, radius_sq, center_easting, center_northing, p, &ps);
    if (sw < 0) return -sw;
    if (sw == 2) {  // (no point within the last radius of any cell: every cell stays)
      c->dirty[2] = c->dirty[3] = 0;
      return AMHIP_OK;
    }
    if (sw == 1) {
      p = ps;
      c->dirty[0] = ps.out_i0;
      c->dirty[1] = ps.out_j0;
      c->dirty[2] = ps.rows;
      c->dirty[3] = ps.cols;
    }
  }
  return dsm_run(c, dev_xyz, nullptr, n, p, c->layers[AMHIP_LAYER_ELEVATION], nullptr, nullptr,
                 fused_fill, layer_init_value(AMHIP_LAYER_ELEVATION),
                 c->zrange_valid ? c->dev_zrange : nullptr);
}

int amhip_dsm_process(amhip_ctx* h, const double* host_xyz, size_t n,
                      int radius_sq, double center_easting,
                      double center_northing, float* elevation) {
  if (!h) return arg_fail("null context");
  if (n == 0) return AMHIP_OK;
  if (!host_xyz || !elevation) return arg_fail("amhip_dsm_process: null buffer");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  overwrite(c, AMHIP_LAYER_ELEVATION);
  AMHIP_TRY(hipMemcpyAsync(c->layers[AMHIP_LAYER_ELEVATION], elevation,
                           c->cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if ((rc = ctx_stage_cloud(c, host_xyz, nullptr, n))) return rc;
  if ((rc = amhip_dsm_process_dev(h, c->stage_points, n, radius_sq, center_easting,
                                  center_northing)))
    return rc;
  AMHIP_TRY(hipMemcpyAsync(elevation, c->layers[AMHIP_LAYER_ELEVATION],
                           c->cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  return fetch_status(c);
}

// ---- OrthoFromPcl -------------------------------------------------------------

int amhip_ortho_from_pcl_process_dev(amhip_ctx* h, const double* dev_xyz,
                                     const int32_t* dev_intensities, size_t n, int radius_sq,
                                     int adaptive) {
  if (!h) return arg_fail("null context");                    // CHECK(map)
  if (n == 0 || !dev_xyz || !dev_intensities)
    return arg_fail("empty point cloud (CHECK(!pointcloud.empty()))");
  if (radius_sq <= 0) return arg_fail("interpolation_radius must be >= 1");
  if (n >= 0x7FFFFFFFull) return arg_fail("more than 2^31-1 points");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  float* out = c->layers[AMHIP_LAYER_ORTHO];
  DsmParams p;
  if ((rc = make_dsm_params(*c, radius_sq, 0.0, 0.0, &p, 1, 1, n))) return rc;
  if (!adaptive) {
    const bool fused_fill = claim_output(c, AMHIP_LAYER_ORTHO);
    return dsm_run(c, dev_xyz, dev_intensities, n, p, out, nullptr, nullptr, fused_fill,
                   layer_init_value(AMHIP_LAYER_ORTHO));
  }
  if ((rc = touch(c, AMHIP_LAYER_ORTHO))) return rc;

  // use_adaptive_interpolation: cells whose search is empty retry with the
  // squared radius x10, x100, ... (int lambda, ortho-from-pcl.cc:63-71).  Every
  // retry is a full pass restricted to the cells no earlier pass has filled.
  if ((rc = ensure_capacity(&c->fill_mask, &c->fill_mask_cap, c->cells))) return rc;
  unsigned* unfilled = c->dev_err + 1;  // second word of the device status block
  AMHIP_TRY(hipMemsetAsync(c->fill_mask, 0, c->cells, c->stream));
  AMHIP_TRY(hipMemsetAsync(unfilled, 0, sizeof(unsigned), c->stream));
  if ((rc = dsm_run(c, dev_xyz, dev_intensities, n, p, out, c->fill_mask, unfilled))) return rc;
  long long lambda = 10;
  for (;;) {
    unsigned left = 0;
    AMHIP_TRY(hipMemcpyAsync(&left, unfilled, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    AMHIP_TRY(hipStreamSynchronize(c->stream));
    if (left == 0) break;
    if (lambda * radius_sq > 0x7FFFFFFFll) break;  // the reference's int product overflows here
    if ((rc = make_dsm_params(*c, radius_sq, 0.0, 0.0, &p, 1, static_cast<int>(lambda), n))) return rc;
    p.only_unfilled = 1;
    AMHIP_TRY(hipMemsetAsync(unfilled, 0, sizeof(unsigned), c->stream));
    if ((rc = dsm_run(c, dev_xyz, dev_intensities, n, p, out, c->fill_mask, unfilled))) return rc;
    lambda *= 10;
  }
  return AMHIP_OK;
}

int amhip_ortho_from_pcl_process(amhip_ctx* h, const double* host_xyz,
                                 const int32_t* host_intensities, size_t n, int radius_sq,
                                 int adaptive, float* ortho) {
  if (!h) return arg_fail("null context");
  if (n == 0 || !host_xyz || !host_intensities || !ortho)
    return arg_fail("empty point cloud / null buffer (CHECK(!pointcloud.empty()))");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  overwrite(c, AMHIP_LAYER_ORTHO);
  AMHIP_TRY(hipMemcpyAsync(c->layers[AMHIP_LAYER_ORTHO], ortho, c->cells * sizeof(float),
                           hipMemcpyHostToDevice, c->stream));
  if ((rc = ctx_stage_cloud(c, host_xyz, host_intensities, n))) return rc;
  if ((rc = amhip_ortho_from_pcl_process_dev(h, c->stage_points, c->stage_values, n, radius_sq,
                                             adaptive)))
    return rc;
  AMHIP_TRY(hipMemcpyAsync(ortho, c->layers[AMHIP_LAYER_ORTHO], c->cells * sizeof(float),
                           hipMemcpyDeviceToHost, c->stream));
  return fetch_status(c);
}

// ---- densifier reprojection -----------------------------------------------------

int amhip_densify_dev(amhip_ctx* h, const float* dev_disparity, size_t disp_step,
                      const uint8_t* dev_image_left, size_t img_step, int width, int height,
                      const double* K, double baseline, const double* R_G_C,
                      const double* t_G_C1, double* dev_xyz_out, int32_t* dev_intensity_out,
                      size_t capacity, int64_t* dev_count) {
  if (!h) return arg_fail("null context");
  if (!dev_disparity || !dev_image_left || !K || !R_G_C || !t_G_C1 || !dev_xyz_out ||
      !dev_intensity_out || !dev_count)
    return arg_fail("amhip_densify_dev: null argument");
  if (width <= 0 || height <= 0 || disp_step < (size_t)width * sizeof(float) ||
      img_step < (size_t)width)
    return arg_fail("amhip_densify_dev: bad image geometry");
  if (baseline == 0.0) return arg_fail("CHECK_NE(baseline, 0.0)");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  const DensifyParams p = densify_params(K, baseline, R_G_C, t_G_C1, width, height, disp_step, img_step);
  return densify_run(c, p, dev_disparity, dev_image_left, dev_xyz_out, dev_intensity_out,
                     capacity, reinterpret_cast<long long*>(dev_count));
}

// ---- multi-GPU halo ----------------------------------------------------------

}  // extern "C"
namespace amhip {
int make_halo_params(const Ctx& c, double center_easting, double center_northing,
                     const int32_t* dest_windows, int nd, double margin_m,
                     size_t cap_per_dest, HaloParams* out) {
  HaloParams hp;
  std::memset(&hp, 0, sizeof(hp));
  grid_bases(c.grid, &hp.base_x, &hp.base_y);
  hp.inv_res = 1.0 / c.grid.resolution;
  hp.sub_x = center_northing;  // dsm.cc:42
  hp.sub_y = center_easting;   // dsm.cc:43
  hp.nd = nd;
  hp.cap = cap_per_dest;
  const double mc = margin_m / c.grid.resolution;  // margin in cells
  for (int d = 0; d < nd; ++d) {
    const int32_t* w = dest_windows + 4 * d;
    if (w[2] <= 0 || w[3] <= 0) return arg_fail("halo selection: empty window");
    hp.lo_i[d] = (double)w[0] - 0.5 - mc;
    hp.hi_i[d] = (double)(w[0] + w[2]) - 0.5 + mc;
    hp.lo_j[d] = (double)w[1] - 0.5 - mc;
    hp.hi_j[d] = (double)(w[1] + w[3]) - 0.5 + mc;
    hp.off[d] = (unsigned long long)d * (unsigned long long)cap_per_dest;
    hp.cap_d[d] = cap_per_dest;
  }
  // the context's own window shrunk by the margin, if no destination reaches into it
  // (windows of one tiling never do)
  hp.in_lo_i = (double)c.win_i0 - 0.5 + mc + 1.0;
  hp.in_hi_i = (double)(c.win_i0 + c.win_rows) - 0.5 - mc - 1.0;
  hp.in_lo_j = (double)c.win_j0 - 0.5 + mc + 1.0;
  hp.in_hi_j = (double)(c.win_j0 + c.win_cols) - 0.5 - mc - 1.0;
  bool clear = hp.in_lo_i < hp.in_hi_i && hp.in_lo_j < hp.in_hi_j;
  for (int d = 0; d < nd && clear; ++d)
    clear = hp.hi_i[d] < hp.in_lo_i || hp.lo_i[d] > hp.in_hi_i || hp.hi_j[d] < hp.in_lo_j ||
            hp.lo_j[d] > hp.in_hi_j;
  if (!clear) {
    hp.in_lo_i = hp.in_lo_j = 1.0;
    hp.in_hi_i = hp.in_hi_j = 0.0;
  }
  *out = hp;
  return AMHIP_OK;
}
}  // namespace amhip
extern "C" {

int amhip_halo_select_dev(amhip_ctx* h, const double* dev_xyz, size_t n,
                          double center_easting, double center_northing,
                          const int32_t* dest_windows, int nd, double margin_m,
                          double* dev_out, size_t cap_per_dest, int64_t* dev_counts) {
  if (!h) return arg_fail("null context");
  if (nd < 0 || nd > kMaxHaloDests) return arg_fail("amhip_halo_select_dev: 0..8 destinations");
  if (nd == 0) return AMHIP_OK;
  if ((n && !dev_xyz) || !dest_windows || !dev_out || !dev_counts || !(margin_m >= 0.0))
    return arg_fail("amhip_halo_select_dev: bad argument");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  HaloParams hp;
  if ((rc = make_halo_params(*c, center_easting, center_northing, dest_windows, nd, margin_m,
                             cap_per_dest, &hp)))
    return rc;
  return halo_select_run(c, dev_xyz, n, hp, dev_out,
                         reinterpret_cast<unsigned long long*>(dev_counts));
}

int amhip_dsm_tiled_begin_dev(amhip_ctx* h, const double* dev_xyz, size_t n_owned,
                              size_t n_total, int radius_sq, double center_easting,
                              double center_northing, const int32_t* dest_windows, int nd,
                              double margin_m, double* dev_out, size_t cap_per_dest,
                              int64_t* dev_counts) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  c->tiled_pending = false;
  if (!dev_xyz || n_total == 0 || n_owned > n_total)
    return arg_fail("amhip_dsm_tiled_begin_dev: bad point arguments");
  if (radius_sq <= 0) return arg_fail("interpolation_radius must be >= 1");
  if (n_total >= 0x7FFFFFFFull) return arg_fail("more than 2^31-1 points");
  if (nd < 1 || nd > kMaxHaloDests || !dest_windows || !dev_out || !dev_counts ||
      !(margin_m >= 0.0) || cap_per_dest == 0)
    return arg_fail("amhip_dsm_tiled_begin_dev: bad halo arguments (1..8 destinations)");
  int rc = use_device(c);
  if (rc) return rc;
  SortSplit sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.phase = 1;
  sp.n_prefix = n_owned;
  if ((rc = make_halo_params(*c, center_easting, center_northing, dest_windows, nd, margin_m,
                             cap_per_dest, &sp.hp)))
    return rc;
  sp.halo_out = dev_out;
  sp.halo_counts = reinterpret_cast<unsigned long long*>(dev_counts);
  DsmParams p;
  dsm_rough_policy(c);
  if ((rc = make_dsm_params(*c, radius_sq, center_easting, center_northing, &p, 0, 1, n_total)))
    return rc;
  if ((rc = dsm_run(c, dev_xyz, nullptr, n_total, p, nullptr, nullptr, nullptr, false, 0.0f,
                    nullptr, &sp)))
    return rc;
  c->tiled_pending = true;
  c->tiled_xyz = dev_xyz;
  c->tiled_n = n_total;
  c->tiled_radius_sq = radius_sq;
  c->tiled_ce = center_easting;
  c->tiled_cn = center_northing;
  c->tiled_split = sp;
  c->tiled_params = p;
  return AMHIP_OK;
}

int amhip_dsm_tiled_finish_dev(amhip_ctx* h) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  if (!c->tiled_pending)
    return arg_fail("amhip_dsm_tiled_finish_dev without amhip_dsm_tiled_begin_dev");
  c->tiled_pending = false;
  int rc = use_device(c);
  if (rc) return rc;
  // (the plan of the begin call, not a fresh one: amhip_ctx_set_dsm_precision / _knn between the
  // two calls must not make the gather disagree with the binning of phase 1)
  const DsmParams p = c->tiled_params;
  SortSplit sp = c->tiled_split;
  sp.phase = 2;
  hipLaunchKernelGGL(k_halo_overflow_check, dim3(1), dim3(64), 0, c->stream, sp.halo_counts,
                     sp.hp.nd, sp.hp.cap, c->dev_err);
  const bool fused_fill = claim_output(c, AMHIP_LAYER_ELEVATION);
  return dsm_run(c, c->tiled_xyz, nullptr, c->tiled_n, p, c->layers[AMHIP_LAYER_ELEVATION],
                 nullptr, nullptr, fused_fill, layer_init_value(AMHIP_LAYER_ELEVATION),
                 c->zrange_valid ? c->dev_zrange : nullptr, &sp);
}

// ---- ortho ----------------------------------------------------------------

void amhip_compose_T_G_C(const double* T_G_B, const double* T_C_B, size_t F,
                         double* T_G_C) {
  const HPose T_B_C = hpose_inverse(hpose_from7(T_C_B));
  for (size_t f = 0; f < F; ++f) {
    const HPose p = hpose_compose(hpose_from7(T_G_B + 7 * f), T_B_C);
    double* o = T_G_C + 7 * f;
    o[0] = p.tx;
    o[1] = p.ty;
    o[2] = p.tz;
    o[3] = p.qw;
    o[4] = p.qx;
    o[5] = p.qy;
    o[6] = p.qz;
  }
}

int amhip_camera_view_bounds(const amhip_camera* cam, double* out4) {
  if (!cam || !out4) return arg_fail("amhip_camera_view_bounds: null argument");
  if (!(cam->fu > 0.0) || !(cam->fv > 0.0) || cam->width <= 0 || cam->height <= 0)
    return arg_fail("amhip_camera_view_bounds: bad camera");
  const ViewBounds b = camera_view_bounds(*cam);
  out4[0] = b.cone;
  out4[1] = b.ax;
  out4[2] = b.ay;
  out4[3] = b.rin;
  return AMHIP_OK;
}

// The occlusion-tested mosaic's own refusals (before any device work): the margin, and a context
// that holds a window of the map -- the ray leaves the window.
static int occl_args_check(const amhip_ctx* h, double margin_m) {
  if (!h) return arg_fail("null context / camera");
  if (!(margin_m >= 0.0))
    return arg_fail("occlusion test: margin_m must be >= 0 (+inf is legal: nothing occludes), not negative or NaN");
  if (h->impl.windowed)
    return arg_fail(
        "occlusion test: the context holds a window of the map (amhip_ctx_create_window) and the ray "
        "towards the camera leaves it; windows need an elevation halo, which is not built yet");
  return AMHIP_OK;
}

// The blended mosaic's own refusals (before any device work): the options, and with the occlusion
// test on that mode's.  Without it a window is served: no ray leaves it, and its context holds its
// own cells' sums.
static int blend_args_check(const amhip_ctx* h, const amhip_ortho_blend_opts* opts) {
  if (!h) return arg_fail("null context / camera");
  if (!opts) return arg_fail("blended mosaic: null options (amhip_ortho_blend_opts)");
  if (opts->sharpness < 0 || opts->sharpness > kBlendMaxSharpness)
    return arg_fail("blended mosaic: sharpness must be 0 .. 4 (the weight is sin^2 .. sin^32 of the view angle)");
  return opts->occlusion_test ? occl_args_check(h, opts->occlusion_margin_m) : AMHIP_OK;
}

// occl_margin: null = the reference's visibility rule; else the occlusion-tested one with that
// margin (checked by the caller: occl_args_check).  blend: null = the winning view's pixel; else
// the weighted mean of every visible view's (checked by the caller: blend_args_check; its
// occlusion switch is what occl_margin says).
static int ortho_backward_dev(amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
                              const uint8_t* dev_frames, size_t frame_stride, size_t row_step,
                              int channels, int colored, const double* occl_margin,
                              const amhip_ortho_blend_opts* blend = nullptr) {
  if (!h || !cam) return arg_fail("null context / camera");
  if (F == 0 || !host_T_G_C) return arg_fail("empty pose list (CHECK(!T_G_Bs.empty()))");
  if (!dev_frames) return arg_fail("null frame pointer");
  if (colored ? channels != 3 : channels != 1)
    return arg_fail("colored_ortho needs 8UC3 frames, gray needs 8UC1");
  if (cam->width <= 0 || cam->height <= 0) return arg_fail("bad image size");
  if (row_step < (size_t)cam->width * (size_t)channels ||
      frame_stride < row_step * (size_t)cam->height)
    return arg_fail("frame strides smaller than the image");
  if (F >= (1u << 24)) return arg_fail("too many frames for a float observation_index");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  // ---- what the plan depends on: the context's window, the layers' states, the knobs of this moment
  const int out_layer = colored ? AMHIP_LAYER_COLORED_ORTHO : AMHIP_LAYER_ORTHO;
  OrthoPlanInput in = {};
  in.grid = c->grid;
  in.win_i0 = c->win_i0;
  in.win_j0 = c->win_j0;
  in.win_rows = c->win_rows;
  in.win_cols = c->win_cols;
  in.cam = *cam;
  in.F = F;
  in.frame_stride = frame_stride;
  in.row_step = row_step;
  in.channels = channels;
  in.colored = colored;
  in.zrange_valid = c->zrange_valid;
  in.state_angle = c->layer_state[AMHIP_LAYER_ELEVATION_ANGLE];
  in.state_index = c->layer_state[AMHIP_LAYER_OBSERVATION_INDEX];
  in.state_out = c->layer_state[out_layer];
  in.state_nobs = c->layer_state[AMHIP_LAYER_NUM_OBSERVATIONS];
  in.knobs.no_distorted_cull = tuning_on("no_distorted_cull");
  in.knobs.no_distorted_prune = tuning_on("no_distorted_prune");
  in.knobs.distorted_square_cull = tuning_on("distorted_square_cull");
  in.knobs.ortho_exact_fold = occl_margin != nullptr || blend != nullptr || tuning_on("ortho_exact_fold");
  in.knobs.no_coarse_cull = tuning_on("no_coarse_cull");
  in.knobs.ortho_no_prune = tuning_on("ortho_no_prune");
  in.knobs.ortho_no_tile_list = tuning_on("ortho_no_tile_list");
  // ---- the frame table and the plan (amhip_ortho_plan.h)
  // (the occlusion test: the camera centres -- the translations of T_G_C -- and one word for the
  // map's largest elevation, key(-inf) until reduced, ride behind the table)
  const size_t table_slots = frame_table_slots(F);
  const size_t occl_slots = occl_margin ? (3 * F * sizeof(double) + sizeof(FramePose) - 1) / sizeof(FramePose) + 1 : 0;
  const size_t slots = table_slots + occl_slots;
  std::vector<FramePose> table(slots);
  const FrameTable frames = build_frame_table(*cam, host_T_G_C, F, in.knobs.ortho_exact_fold, table.data());
  OrthoPlan plan = plan_ortho_call(in, frames, &c->view_bounds);
  if (occl_margin) {
    double* centres = reinterpret_cast<double*>(table.data() + table_slots);
    for (size_t f = 0; f < F; ++f)
      for (int k = 0; k < 3; ++k) centres[3 * f + k] = host_T_G_C[7 * f + k];
    static const unsigned long long minus_inf_key = 0x000FFFFFFFFFFFFFull;  // (amhip_device.h)
    std::memcpy(table.data() + slots - 1, &minus_inf_key, sizeof(minus_inf_key));
  }
  if (occl_margin || blend) {
    // dominated() assumes that a fully visible frame beats the pruned one at every landmark: not
    // once the dominator can be occluded -- and a dominated view still contributes to a blend.
    // The kernel writes into real memory, tile by tile.
    plan.p.prune = 0;
    plan.p.virt_out = 0;
    plan.launch.tile_list = false;
  }
  // ---- the blended mosaic's sums: allocated, zero, by the first call of their kind
  const int sums = colored ? 1 : 0;
  if (blend && !c->blend_sums[sums]) {
    const size_t bytes = (colored ? 4 : 2) * c->cells * sizeof(double);
    AMHIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->blend_sums[sums]), bytes));
    AMHIP_TRY(hipMemsetAsync(c->blend_sums[sums], 0, bytes, c->stream));
  }
  // ---- one buffer, one upload (pageable source: hipMemcpyAsync returns once it has been staged)
  if ((rc = ensure_capacity(&c->frame_poses, &c->frame_pose_cap, slots))) return rc;
  AMHIP_TRY(hipMemcpyAsync(c->frame_poses, table.data(), slots * sizeof(FramePose),
                           hipMemcpyHostToDevice, c->stream));
  // ---- layer states (lazy reset): the kernel reads elevation; elevation_angle, observation_index
  // and the output layer are either all produced with a fused fill or all materialized;
  // num_observations stays in its state while it is logically 0.  (The dirty box is ortho_run's
  // to set: every error return before it comes out of materialize -- nothing written yet -- or out
  // of touch(), which has marked the whole window by then.)
  if ((rc = materialize(c, AMHIP_LAYER_ELEVATION))) return rc;
  const int outs[3] = {AMHIP_LAYER_ELEVATION_ANGLE, AMHIP_LAYER_OBSERVATION_INDEX, out_layer};
  for (int k = 0; k < 3; ++k) {
    if (plan.p.virt_out)
      c->layer_state[outs[k]] = kLayerWritten;
    else if ((rc = touch(c, outs[k])))
      return rc;
  }
  if (!plan.p.virt_nobs && (rc = touch(c, AMHIP_LAYER_NUM_OBSERVATIONS))) return rc;
  OcclParams q = {0.0, nullptr, nullptr};
  unsigned long long* own_key = nullptr;
  if (occl_margin) {
    q.margin = *occl_margin;
    q.centres = reinterpret_cast<const double*>(c->frame_poses + table_slots);
    // the height cut-off of the march: the range the DSM calls wrote, or the layer's own maximum
    own_key = reinterpret_cast<unsigned long long*>(c->frame_poses + slots - 1);
    q.zmax_key = c->zrange_valid ? c->dev_zrange + 1 : own_key;
    if (c->zrange_valid) own_key = nullptr;
  }
  if (blend) {
    BlendParams b;
    b.sharpness = blend->sharpness;
    b.plane = c->cells;
    b.wsum = c->blend_sums[sums];
    b.acc = c->blend_sums[sums] + c->cells;
    return ortho_blend_run(c, plan, occl_margin ? &q : nullptr, b, c->frame_poses, dev_frames, own_key);
  }
  if (occl_margin) return ortho_occl_run(c, plan, q, c->frame_poses, dev_frames, own_key);
  return ortho_run(c, plan, c->frame_poses, reinterpret_cast<const FrameFast*>(c->frame_poses + F),
                   dev_frames);
}

int amhip_ortho_backward_process_dev(amhip_ctx* h, const amhip_camera* cam,
                                     const double* host_T_G_C, size_t F,
                                     const uint8_t* dev_frames,
                                     size_t frame_stride, size_t row_step,
                                     int channels, int colored) {
  return ortho_backward_dev(h, cam, host_T_G_C, F, dev_frames, frame_stride, row_step, channels, colored,
                            nullptr);
}

int amhip_ortho_backward_process_occl_dev(amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C,
                                          size_t F, const uint8_t* dev_frames, size_t frame_stride,
                                          size_t row_step, int channels, int colored, double margin_m) {
  const int rc = occl_args_check(h, margin_m);
  if (rc) return rc;
  return ortho_backward_dev(h, cam, host_T_G_C, F, dev_frames, frame_stride, row_step, channels, colored,
                            &margin_m);
}

int amhip_ortho_backward_process_blend_dev(amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C,
                                           size_t F, const uint8_t* dev_frames, size_t frame_stride,
                                           size_t row_step, int channels, int colored,
                                           const amhip_ortho_blend_opts* opts) {
  const int rc = blend_args_check(h, opts);
  if (rc) return rc;
  return ortho_backward_dev(h, cam, host_T_G_C, F, dev_frames, frame_stride, row_step, channels, colored,
                            opts->occlusion_test ? &opts->occlusion_margin_m : nullptr, opts);
}

static int ortho_backward_host(
    amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho, const double* occl_margin, const amhip_ortho_blend_opts* blend = nullptr) {
  if (!h || !cam) return arg_fail("null context / camera");
  if (F == 0 || !host_T_G_C || !images || !steps)
    return arg_fail("empty pose / image list (CHECK(!T_G_Bs.empty()))");
  if (cam->width <= 0 || cam->height <= 0) return arg_fail("bad image size");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  const size_t bytes = c->cells * sizeof(float);
  const float* ups[AMHIP_NUM_LAYERS] = {ortho,           elevation,
                                        elevation_angle, num_observations,
                                        observation_index, colored_ortho};
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l)
    if (ups[l]) {
      overwrite(c, l);
      AMHIP_TRY(hipMemcpyAsync(c->layers[l], ups[l], bytes, hipMemcpyHostToDevice,
                               c->stream));
    }
  const size_t row = (size_t)cam->width * (size_t)channels;
  const size_t frame = row * (size_t)cam->height;
  if ((rc = ctx_stage_frames(c, images, steps, F, row, (size_t)cam->height))) return rc;
  if ((rc = ortho_backward_dev(h, cam, host_T_G_C, F, c->stage_frames, frame, row, channels, colored,
                               occl_margin, blend)))
    return rc;
  float* downs[AMHIP_NUM_LAYERS] = {ortho,           nullptr,
                                    elevation_angle, num_observations,
                                    observation_index, colored_ortho};
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l)
    if (downs[l]) {
      if ((rc = materialize(c, l))) return rc;
      AMHIP_TRY(hipMemcpyAsync(downs[l], c->layers[l], bytes, hipMemcpyDeviceToHost,
                               c->stream));
    }
  return fetch_status(c);
}

int amhip_ortho_backward_process(
    amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho) {
  return ortho_backward_host(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                             elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                             nullptr);
}

int amhip_ortho_backward_process_occl(
    amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho, double margin_m) {
  const int rc = occl_args_check(h, margin_m);
  if (rc) return rc;
  return ortho_backward_host(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                             elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                             &margin_m);
}

int amhip_ortho_backward_process_blend(
    amhip_ctx* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho, const amhip_ortho_blend_opts* opts) {
  const int rc = blend_args_check(h, opts);
  if (rc) return rc;
  return ortho_backward_host(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                             elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                             opts->occlusion_test ? &opts->occlusion_margin_m : nullptr, opts);
}

// ---- measurement ------------------------------------------------------------

int amhip_ctx_enable_timing(amhip_ctx* h, int on) {
  if (!h) return arg_fail("null context");
  h->impl.timing = on != 0;
  return AMHIP_OK;
}

int amhip_ctx_timing_reset(amhip_ctx* h) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  drain_timers(c);
  for (int k = 0; k < AMHIP_NUM_KERNELS; ++k) {
    c->slot_ms[k] = 0.0;
    c->slot_launches[k] = 0;
  }
  return AMHIP_OK;
}

int amhip_ctx_kernel_time(amhip_ctx* h, int kernel, double* total_ms,
                          int64_t* launches) {
  if (!h || kernel < 0 || kernel >= AMHIP_NUM_KERNELS) return arg_fail("bad kernel slot");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  drain_timers(c);
  if (total_ms) *total_ms = c->slot_ms[kernel];
  if (launches) *launches = c->slot_launches[kernel];
  return AMHIP_OK;
}

const char* amhip_kernel_name(int kernel) {
  switch (kernel) {
    // sort slots: named after the kernels of the default path for large clouds
    // (three-pass partition sort); the one-level sort of small clouds reports its
    // count / scan / scatter launches in the same slots
    case AMHIP_K_DSM_BIN_COUNT:
      return "k_dsm_p3_count";    // + k_dsm_p3_reduce, k_dsm_p3_scan
    case AMHIP_K_DSM_SCATTER:
      return "k_dsm_p3_scatter";  // both scatter passes
    case AMHIP_K_DSM_SCAN:
      return "k_dsm_p3_place";
    case AMHIP_K_DSM_GATHER:
      return "k_dsm_gather";
    case AMHIP_K_ORTHO:
      return "k_ortho_backward";
    case AMHIP_K_MISC:
      return "memset/fill";
    case AMHIP_K_HALO_SELECT:
      return "k_halo_select";
    case AMHIP_K_STEREO:
      return "k_stereo";          // every kernel of amhip_sgbm_disparity_dev / amhip_bm_disparity_dev
    default:
      return "?";
  }
}

int amhip_set_tuning(const char* key, double value) {
  if (!tuning_set(key, value)) return arg_fail("amhip_set_tuning: unknown key (include/aerial_mapper_hip.h lists them)");
  return AMHIP_OK;
}

double amhip_get_tuning(const char* key, double dflt) { return key ? tuning(key, dflt) : dflt; }

int amhip_default_dsm_precision(void) {
  // AMHIP_DSM_FAST=1 (and not AMHIP_DSM_EXACT): hosts that cannot be recompiled opt in to the
  // single-precision gather; everything else starts in the reference's arithmetic
  const char* fast = std::getenv("AMHIP_DSM_FAST");
  return (fast && fast[0] && fast[0] != '0' && !std::getenv("AMHIP_DSM_EXACT")) ? AMHIP_DSM_FAST : AMHIP_DSM_EXACT;
}

int amhip_ctx_order_after(amhip_ctx* h, void* other_stream) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  hipStream_t other = static_cast<hipStream_t>(other_stream);
  if (other == c->stream) return AMHIP_OK;  // (already ordered)
  if (!c->order_event) AMHIP_TRY(hipEventCreateWithFlags(&c->order_event, hipEventDisableTiming));
  AMHIP_TRY(hipEventRecord(c->order_event, c->stream));
  AMHIP_TRY(hipStreamWaitEvent(other, c->order_event, 0));
  return AMHIP_OK;
}

int amhip_ctx_dsm_gather_stats(amhip_ctx* h, int64_t* out8) {
  if (!h || !out8) return arg_fail("amhip_ctx_dsm_gather_stats: null argument");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  for (int k = 0; k < 8; ++k) out8[k] = 0;
  if (!c->tile_list || c->last_ntiles == 0) return AMHIP_OK;
  unsigned hdr[8];
  AMHIP_TRY(hipMemcpyAsync(hdr, c->tile_list, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
  AMHIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 7; ++k) out8[k] = hdr[k];
  out8[4] += hdr[7];  // (pre-classified tiles the dense FP64 launch took instead of list 4)
  out8[7] = c->last_ntiles;
  return AMHIP_OK;
}

int amhip_ctx_dsm_stats(amhip_ctx* h, int64_t* points_binned, int64_t* num_bins,
                        int32_t* bin_cells) {
  if (!h) return arg_fail("null context");
  Ctx* c = &h->impl;
  int rc = use_device(c);
  if (rc) return rc;
  if (points_binned) {
    *points_binned = 0;
    if (c->bin_start && c->last_num_bins > 0) {
      uint32_t total = 0;
      AMHIP_TRY(hipMemcpyAsync(&total, c->bin_start + c->last_num_bins,
                               sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      AMHIP_TRY(hipStreamSynchronize(c->stream));
      *points_binned = total;
    }
  }
  if (num_bins) *num_bins = c->last_num_bins;
  if (bin_cells) *bin_cells = c->last_bin_cells;
  return AMHIP_OK;
}

int amhip_ctx_dsm_sort_pipeline(amhip_ctx* h, int32_t* pipeline) {
  if (!h || !pipeline) return arg_fail("amhip_ctx_dsm_sort_pipeline: null argument");
  *pipeline = h->impl.last_sort_pipeline;
  return AMHIP_OK;
}

}  // extern "C"
