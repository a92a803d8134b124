// amhip_stereo_seq.hip -- stereo::Stereo (aerial_mapper_dense_pcl/src/stereo.cpp): a frame
// sequence -> one dense cloud, resident in HBM from the uploaded frame to the concatenated cloud.
//
// Host side only: the kernels are the rectifier's (amhip_rectify.hip), the matchers'
// (amhip_stereo.hip), the mapped undistorter's (amhip_forward.hip) and the append-mode densify
// (amhip_densify.hip).  What this file adds is the order of things:
//   frames     nslots raw slots in rotation (frame j of a sequence lives in slot j mod nslots; 2 slots,
//              or n + 1 once amhip_stereo_set_pairs_in_flight(n) has asked for more): a frame is
//              staged once and undistorted once although it is the right image of one pair and the
//              left image of the next.  Host frames go through pinned buffers and a second stream;
//              the upload of a frame waits only for the rectifier of the pair that last read its
//              slot, so it runs beside the matching of the pairs before it.
//   groups     seq_run_group is the one way a pair runs: g consecutive frames behind the left frame
//              that is in place (add_frame: g = 1; add_frames: groups of up to pairs_in_flight, for
//              every n) -- each frame staged and its pair rectified into the next entry of the
//              stacks, ONE matcher call for the g pairs, then the appends pair by pair in order,
//              all enqueued on the context's stream.  The point count stays on the device
//              (SeqState) and is read once, by amhip_stereo_cloud.  In a group of more than one,
//              each pair copies the context's sticky error word behind its own rectifier (stream
//              order) and its append reads that copy: a zero w silences its own pair and the later
//              ones, never an earlier one.  A group of one reads the context's word itself.
//   capacity   settled before the first pair of a call (pairs x W x H points).
#include <algorithm>
#include <cstring>
#include <new>

#include "amhip_common.h"
#include "amhip_ortho_plan.h"  // HPose, hpose_*

namespace amhip {

constexpr int kSeqMaxSlots = AMHIP_STEREO_MAX_BATCH + 1;

// T_G_C of a frame: rotation matrix and position
struct SeqPose {
  double R[9], t[3];
};
// one frame handed to the sequence: its T_G_B (7 doubles), its rows, `step` bytes apart
struct SeqFrame {
  const double* T_G_B7;
  const uint8_t* src;
  size_t step;
};

struct Stereo {
  amhip_ctx* ctx = nullptr;
  amhip_camera cam = {};
  amhip_stereo_settings settings = {};
  HPose T_B_C = {};
  double K[9] = {};
  int W = 0, H = 0;
  size_t npix = 0;
  bool undistort = false;

  hipStream_t up_stream = nullptr;
  int nslots = 0;                      // frame slots allocated: 2, or (the largest n asked for) + 1
  int in_flight = 1;                   // pairs per group of add_frames
  hipEvent_t ev_up[kSeqMaxSlots] = {};    // the upload into slot s has finished
  hipEvent_t ev_free[kSeqMaxSlots] = {};  // the last kernel reading raw[s] has finished
  bool up_used[kSeqMaxSlots] = {};
  uint8_t* pin[kSeqMaxSlots] = {};
  uint8_t* raw[kSeqMaxSlots] = {};
  uint8_t* und[kSeqMaxSlots] = {};

  bool first_frame = true;
  int left_slot = 0;
  SeqPose left_pose = {};

  // stacks of `stack` rectified pairs, masks and disparity maps, npix elements apart
  int stack = 0;
  uint8_t *rect_l = nullptr, *rect_r = nullptr, *mask = nullptr;
  float* disp = nullptr;
  unsigned* flags = nullptr;  // per pair of a group: the device error word behind its rectifier
  double* xyz = nullptr;
  int32_t* inten = nullptr;
  size_t cap = 0;  // points
  SeqState* state = nullptr;
  SeqState* host_state = nullptr;  // pinned
  void* pc2 = nullptr;
};

static int seq_arg_fail(const char* msg) { return arg_failure(msg); }

// Eigen::Quaterniond::toRotationMatrix (the formula is part of the contract: aerial_mapper_hip.h)
static void quat_to_matrix(const HPose& p, double R[9]) {
  const double tx = 2.0 * p.qx, ty = 2.0 * p.qy, tz = 2.0 * p.qz;
  const double twx = tx * p.qw, twy = ty * p.qw, twz = tz * p.qw;
  const double txx = tx * p.qx, txy = ty * p.qx, txz = tz * p.qx;
  const double tyy = ty * p.qy, tyz = tz * p.qy, tzz = tz * p.qz;
  R[0] = 1.0 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}

static int dev_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    *p = nullptr;
    set_last_error("amhip_stereo: out of device memory");
    return AMHIP_ERR_NOMEM;
  }
  AMHIP_TRY(e);
  return AMHIP_OK;
}

static void seq_free(Stereo* s) {
  if (s->up_stream) (void)hipStreamSynchronize(s->up_stream);
  if (s->ctx) (void)hipStreamSynchronize(s->ctx->impl.stream);
  for (int k = 0; k < kSeqMaxSlots; ++k) {
    if (s->ev_up[k]) (void)hipEventDestroy(s->ev_up[k]);
    if (s->ev_free[k]) (void)hipEventDestroy(s->ev_free[k]);
    if (s->pin[k]) (void)hipHostFree(s->pin[k]);
    if (s->raw[k]) (void)hipFree(s->raw[k]);
    if (s->und[k]) (void)hipFree(s->und[k]);
  }
  if (s->up_stream) (void)hipStreamDestroy(s->up_stream);
  void* dev[] = {s->rect_l, s->rect_r, s->mask, s->disp, s->flags, s->xyz, s->inten, s->state, s->pc2};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  if (s->host_state) (void)hipHostFree(s->host_state);
}

// the cloud can take `points` points (contents are not kept: callers empty or replace the cloud)
static int seq_reserve(Stereo* s, size_t points) {
  if (points <= s->cap) return AMHIP_OK;
  // (hipFree waits for the kernels that still use the old buffers)
  if (s->xyz) AMHIP_TRY(hipFree(s->xyz));
  if (s->inten) AMHIP_TRY(hipFree(s->inten));
  s->xyz = nullptr;
  s->inten = nullptr;
  s->cap = 0;
  int rc;
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->xyz), points * 3 * sizeof(double)))) return rc;
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->inten), points * sizeof(int32_t)))) return rc;
  s->cap = points;
  return AMHIP_OK;
}

static int seq_clear(Stereo* s) {
  AMHIP_TRY(hipMemsetAsync(s->state, 0, sizeof(SeqState), s->ctx->impl.stream));
  return AMHIP_OK;
}

// frame slots 0 .. n - 1 exist (events, pinned staging, raw and, if used, undistorted frame)
static int seq_grow_slots(Stereo* s, int n) {
  for (int k = s->nslots; k < n; ++k) {
    AMHIP_TRY(hipEventCreateWithFlags(&s->ev_up[k], hipEventDisableTiming));
    AMHIP_TRY(hipEventCreateWithFlags(&s->ev_free[k], hipEventDisableTiming));
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&s->pin[k]), s->npix, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      s->pin[k] = nullptr;
      set_last_error("amhip_stereo: out of pinned host memory");
      return AMHIP_ERR_NOMEM;
    }
    AMHIP_TRY(e);
    int rc;
    if ((rc = dev_alloc(reinterpret_cast<void**>(&s->raw[k]), s->npix))) return rc;
    if (s->undistort && (rc = dev_alloc(reinterpret_cast<void**>(&s->und[k]), s->npix))) return rc;
    s->nslots = k + 1;  // (a slot that failed half-way is freed with the object)
  }
  return AMHIP_OK;
}

// the stacks hold n rectified pairs, masks and disparity maps (contents are not kept)
static int seq_grow_stacks(Stereo* s, int n) {
  if (n <= s->stack) return AMHIP_OK;
  uint8_t *l = nullptr, *r = nullptr, *m = nullptr;
  float* d = nullptr;
  int rc;
  if ((rc = dev_alloc(reinterpret_cast<void**>(&l), s->npix * n)) ||
      (rc = dev_alloc(reinterpret_cast<void**>(&r), s->npix * n)) ||
      (rc = dev_alloc(reinterpret_cast<void**>(&m), s->npix * n)) ||
      (rc = dev_alloc(reinterpret_cast<void**>(&d), s->npix * n * sizeof(float)))) {
    void* got[] = {l, r, m, d};
    for (void* p : got)
      if (p) (void)hipFree(p);
    return rc;
  }
  // (hipFree waits for the kernels that still use the old stacks)
  void* old[] = {s->rect_l, s->rect_r, s->mask, s->disp};
  for (void* p : old)
    if (p) AMHIP_TRY(hipFree(p));
  s->rect_l = l;
  s->rect_r = r;
  s->mask = m;
  s->disp = d;
  s->stack = n;
  return AMHIP_OK;
}

// stereo.cpp:129-137: T_G_C = T_G_B * T_B_C, its position and rotation matrix
static SeqPose seq_pose(const Stereo* s, const double* T_G_B7) {
  const HPose T_G_C = hpose_compose(hpose_from7(T_G_B7), s->T_B_C);
  SeqPose p;
  quat_to_matrix(T_G_C, p.R);
  p.t[0] = T_G_C.tx;
  p.t[1] = T_G_C.ty;
  p.t[2] = T_G_C.tz;
  return p;
}

static const uint8_t* seq_frame(const Stereo* s, int slot) { return s->undistort ? s->und[slot] : s->raw[slot]; }

// a frame into its slot: staged and, if asked for, undistorted -- once, whichever pairs it serves
static int seq_stage(Stereo* s, int slot, const SeqFrame& f, bool on_device) {
  Ctx* c = &s->ctx->impl;
  hipStream_t main = c->stream;
  const size_t W = (size_t)s->W, H = (size_t)s->H;
  if (on_device) {
    AMHIP_TRY(hipMemcpy2DAsync(s->raw[slot], W, f.src, f.step, W, H, hipMemcpyDeviceToDevice, main));
  } else {
    if (s->up_used[slot]) AMHIP_TRY(hipEventSynchronize(s->ev_up[slot]));  // pin[slot] is free again
    for (size_t v = 0; v < H; ++v) std::memcpy(s->pin[slot] + v * W, f.src + v * f.step, W);
    AMHIP_TRY(hipStreamWaitEvent(s->up_stream, s->ev_free[slot], 0));
    AMHIP_TRY(hipMemcpyAsync(s->raw[slot], s->pin[slot], s->npix, hipMemcpyHostToDevice, s->up_stream));
    AMHIP_TRY(hipEventRecord(s->ev_up[slot], s->up_stream));
    s->up_used[slot] = true;
    AMHIP_TRY(hipStreamWaitEvent(main, s->ev_up[slot], 0));
  }
  if (s->undistort) {
    ScopedTimer t(c, AMHIP_K_MISC);
    int rc = undistort_frames_run(main, s->cam, s->raw[slot], s->npix, W, 1, 1, s->und[slot]);
    if (rc) return rc;
    AMHIP_TRY(hipEventRecord(s->ev_free[slot], main));
  }
  return AMHIP_OK;
}

// the pair (frame in slot `left`, pose p1; frame in slot `right`, pose p2) rectified into entry k
// of the stacks
static int seq_rectify(Stereo* s, int k, int left, const SeqPose& p1, int right, const SeqPose& p2,
                       double* R_G_C, double* baseline) {
  const size_t W = (size_t)s->W;
  int rc = amhip_rectify_stereo_pair_dev(s->ctx, s->K, p1.R, p2.R, p1.t, p2.t, s->W, s->H, seq_frame(s, left), W,
                                         seq_frame(s, right), W, R_G_C, baseline, nullptr,
                                         s->rect_l + k * s->npix, s->rect_r + k * s->npix,
                                         s->mask + k * s->npix);
  if (rc) return rc;
  // (the slot of a pair's left frame is the next one to be staged into)
  if (!s->undistort) AMHIP_TRY(hipEventRecord(s->ev_free[left], s->ctx->impl.stream));
  return AMHIP_OK;
}

// entry k of the stacks -> the cloud; err_word: the device error word this pair answers to
static int seq_append(Stereo* s, int k, const double* R_G_C, double baseline, const double* t1,
                      bool replace, const unsigned* err_word) {
  const size_t W = (size_t)s->W;
  const DensifyParams p = densify_params(s->K, baseline, R_G_C, t1, s->W, s->H, W * sizeof(float), W);
  return densify_append_run(&s->ctx->impl, p, s->disp + k * s->npix, s->rect_l + k * s->npix, s->xyz,
                            s->inten, s->cap, s->state, s->pc2, replace, err_word);
}

// the first frame of a sequence has no left partner: it is staged and becomes the left frame
static int seq_first_frame(Stereo* s, const SeqFrame& f, bool on_device) {
  int rc;
  if ((rc = seq_stage(s, 0, f, on_device))) return rc;
  s->left_pose = seq_pose(s, f.T_G_B7);
  s->left_slot = 0;
  s->first_frame = false;
  return AMHIP_OK;
}

// g (1 .. stack) consecutive frames of a sequence whose left frame is in place: g pairs, matched by
// ONE call.  Frame k of the group is staged, then its pair with the frame before it is rectified
// into entry k.  A pair that is refused -- both frames at one position, or a baseline the rectifier
// finds to be zero -- cuts the group in front of it: its frame has been staged (and, for the zero
// baseline, rectified), the pairs before it go through and roll the left frame, then the call fails
// with that pair's error.  `replace`: the (one) pair replaces the cloud instead of joining it.
static int seq_run_group(Stereo* s, const SeqFrame* f, int g, bool on_device, bool replace) {
  Ctx* c = &s->ctx->impl;
  SeqPose pose[AMHIP_STEREO_MAX_BATCH + 1];  // pose / slot [k + 1]: frame k; [0]: the left frame
  int slot[AMHIP_STEREO_MAX_BATCH + 1];
  double R_G_C[AMHIP_STEREO_MAX_BATCH][9], baseline[AMHIP_STEREO_MAX_BATCH];
  pose[0] = s->left_pose;
  slot[0] = s->left_slot;
  const char* refused = nullptr;
  int m = 0, rc;  // m: pairs that go through
  for (; m < g; ++m) {
    const SeqPose& l = pose[m];
    SeqPose& r = pose[m + 1] = seq_pose(s, f[m].T_G_B7);
    slot[m + 1] = (slot[m] + 1) % s->nslots;
    if ((rc = seq_stage(s, slot[m + 1], f[m], on_device))) return rc;
    if (r.t[0] == l.t[0] && r.t[1] == l.t[1] && r.t[2] == l.t[2]) {
      refused = "CHECK_NE(baseline, 0.0) (densifier.cpp:39): both frames have the same position";
      break;
    }
    baseline[m] = 0.0;
    if ((rc = seq_rectify(s, m, slot[m], l, slot[m + 1], r, R_G_C[m], &baseline[m]))) return rc;
    if (baseline[m] == 0.0) {
      refused = "CHECK_NE(baseline, 0.0) (densifier.cpp:39)";
      break;
    }
    // the error word as it stands behind this pair's rectifier (the next pair's comes later)
    if (g > 1)
      AMHIP_TRY(hipMemcpyAsync(s->flags + m, c->dev_err, sizeof(unsigned), hipMemcpyDeviceToDevice, c->stream));
  }
  if (m > 0) {
    const size_t W = (size_t)s->W, np = s->npix;
    const StereoImages im = {s->rect_l, W, s->rect_r, W, s->mask, W, s->disp, W * sizeof(float), nullptr, 0, m,
                             {np, np, np, np * sizeof(float), 0}};
    if ((rc = stereo_match(c, s->settings, s->W, s->H, im))) return rc;
    for (int k = 0; k < m; ++k)
      if ((rc = seq_append(s, k, R_G_C[k], baseline[k], pose[k].t, replace, g > 1 ? s->flags + k : nullptr)))
        return rc;
    // stereo.cpp:142-146: the right frame is the next pair's left frame
    s->left_pose = pose[m];
    s->left_slot = slot[m];
  }
  return refused ? seq_arg_fail(refused) : AMHIP_OK;
}

static int check_channels(int channels) {
  if (channels == 3)
    return seq_arg_fail("amhip_stereo: 8UC3 frames are refused: the reference stores the RAW colour "
                        "image (stereo.cpp:131,138), which OpenCV's block matchers reject");
  if (channels != 1) return seq_arg_fail("amhip_stereo: image type not supported (stereo.cpp:123): 8UC1 only");
  return AMHIP_OK;
}

}  // namespace amhip

struct amhip_stereo {
  amhip::Stereo impl;
};

namespace amhip {

static int add_one(amhip_stereo* h, const double* T, const uint8_t* image, size_t step, int channels,
                   bool on_device) {
  int rc;
  if ((rc = check_channels(channels))) return rc;
  if (!T || !image) return seq_arg_fail("amhip_stereo_add_frame: null argument");
  if (!h) return seq_arg_fail("null stereo object");
  Stereo* s = &h->impl;
  if (step < (size_t)s->W) return seq_arg_fail("amhip_stereo_add_frame: step smaller than the camera's width");
  if ((rc = ctx_use_device(&s->ctx->impl))) return rc;
  const SeqFrame f = {T, image, step};
  if (s->first_frame) return seq_first_frame(s, f, on_device);
  if ((rc = seq_reserve(s, s->npix))) return rc;
  return seq_run_group(s, &f, 1, on_device, /*replace=*/true);
}

static int add_many(amhip_stereo* h, const double* T, const uint8_t* const* images,
                    const size_t* steps, const uint8_t* dev_frames, size_t frame_stride,
                    size_t row_step, int channels, size_t F) {
  int rc;
  if ((rc = check_channels(channels))) return rc;
  const bool on_device = images == nullptr;
  if (F > 0 && (!T || (on_device ? !dev_frames : !steps)))
    return seq_arg_fail("amhip_stereo_add_frames: null argument");
  if (!h) return seq_arg_fail("null stereo object");
  Stereo* s = &h->impl;
  const size_t nth = (size_t)s->settings.use_every_nth_image;
  size_t used = 0;
  for (size_t i = 0; i < F; ++i) {
    if ((i + 1) % nth != 0) continue;
    ++used;
    if (on_device) continue;
    if (!images[i]) return seq_arg_fail("amhip_stereo_add_frames: null image");
    if (steps[i] < (size_t)s->W) return seq_arg_fail("amhip_stereo_add_frames: step smaller than the camera's width");
  }
  if (on_device && F > 0 && (row_step < (size_t)s->W || (F > 1 && frame_stride < row_step * (size_t)s->H)))
    return seq_arg_fail("amhip_stereo_add_frames_dev: row_step / frame_stride smaller than a row / a frame");
  if ((rc = ctx_use_device(&s->ctx->impl))) return rc;
  const size_t pairs = used == 0 ? 0 : (s->first_frame ? used - 1 : used);
  if ((rc = seq_reserve(s, pairs * s->npix))) return rc;
  const size_t n = (size_t)s->in_flight;
  // (the matcher's scratch for a whole group, before the first pair)
  if (n > 1 && pairs > 0 &&
      (rc = stereo_scratch_reserve(&s->ctx->impl, s->settings, s->W, s->H, (int)std::min(n, pairs))))
    return rc;
  if ((rc = seq_clear(s))) return rc;  // point_cloud->clear() (stereo.cpp:86)
  SeqFrame group[AMHIP_STEREO_MAX_BATCH];
  int g = 0;
  for (size_t i = 0; i < F; ++i) {
    if ((i + 1) % nth != 0) continue;  // ++skip % use_every_nth_image == 0 (:93)
    const SeqFrame f = {T + 7 * i, on_device ? dev_frames + i * frame_stride : images[i],
                        on_device ? row_step : steps[i]};
    if (s->first_frame) {
      if ((rc = seq_first_frame(s, f, on_device))) return rc;
      continue;
    }
    group[g] = f;
    if (++g == (int)n) {
      if ((rc = seq_run_group(s, group, g, on_device, /*replace=*/false))) return rc;
      g = 0;
    }
  }
  // (the last, shorter group)
  return g > 0 ? seq_run_group(s, group, g, on_device, /*replace=*/false) : AMHIP_OK;
}

}  // namespace amhip

using namespace amhip;

extern "C" {

void amhip_stereo_default_settings(amhip_stereo_settings* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->use_every_nth_image = 1;  // stereo::Settings (common.h:31-35)
  out->images_need_undistortion = 0;
  out->use_bm = 0;               // BlockMatchingParameters::use_BM (common.h:83)
  amhip_sgbm_default_params(&out->sgbm);
  amhip_bm_default_params(&out->bm);
}

int amhip_stereo_create(amhip_ctx* ctx, const amhip_camera* cam, const double* T_C_B7,
                        const amhip_stereo_settings* settings, amhip_stereo** out) {
  if (out) *out = nullptr;
  if (!cam || !T_C_B7 || !settings || !out) return seq_arg_fail("amhip_stereo_create: null argument");
  if (settings->use_every_nth_image == 0)
    return seq_arg_fail("amhip_stereo_create: use_every_nth_image == 0 (stereo.cpp:93 divides by it)");
  if (cam->width < 1 || cam->height < 1 || cam->width > 32767 || cam->height > 32767)
    return seq_arg_fail("amhip_stereo_create: camera width and height must be in [1, 32767]");
  if (cam->distortion != AMHIP_DIST_NONE && cam->distortion != AMHIP_DIST_RADTAN &&
      cam->distortion != AMHIP_DIST_EQUIDISTANT)
    return seq_arg_fail("amhip_stereo_create: unknown distortion model");
  int rc;
  if ((rc = stereo_params_check(*settings, cam->width, cam->height))) return rc;
  if (!ctx) return seq_arg_fail("null context");
  if ((rc = ctx_use_device(&ctx->impl))) return rc;
  amhip_stereo* h = new (std::nothrow) amhip_stereo();
  if (!h) return AMHIP_ERR_NOMEM;
  Stereo* s = &h->impl;
  s->ctx = ctx;
  s->cam = *cam;
  s->settings = *settings;
  s->T_B_C = hpose_inverse(hpose_from7(T_C_B7));  // stereo.cpp:43
  const double K[9] = {cam->fu, 0.0, cam->cu, 0.0, cam->fv, cam->cv, 0.0, 0.0, 1.0};  // :37-40
  std::memcpy(s->K, K, sizeof(K));
  s->W = cam->width;
  s->H = cam->height;
  s->npix = (size_t)s->W * s->H;
  s->undistort = settings->images_need_undistortion != 0 && cam->distortion != AMHIP_DIST_NONE;
  auto fail = [&](int code) {
    seq_free(s);
    delete h;
    return code;
  };
#define SEQ_TRY(expr)                                                         \
  do {                                                                        \
    const hipError_t _e = (expr);                                             \
    if (_e != hipSuccess) return fail(hip_fail(_e, #expr, __FILE__, __LINE__)); \
  } while (0)
  SEQ_TRY(hipStreamCreateWithFlags(&s->up_stream, hipStreamNonBlocking));
  if ((rc = seq_grow_slots(s, 2))) return fail(rc);
  if ((rc = seq_grow_stacks(s, 1))) return fail(rc);
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->flags), AMHIP_STEREO_MAX_BATCH * sizeof(unsigned)))) return fail(rc);
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->state), sizeof(SeqState)))) return fail(rc);
  if ((rc = dev_alloc(&s->pc2, s->npix * 16))) return fail(rc);
  SEQ_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->host_state), sizeof(SeqState), hipHostMallocDefault));
  std::memset(s->host_state, 0, sizeof(SeqState));
  SEQ_TRY(hipMemsetAsync(s->state, 0, sizeof(SeqState), ctx->impl.stream));
  SEQ_TRY(hipMemsetAsync(s->pc2, 0, s->npix * 16, ctx->impl.stream));
#undef SEQ_TRY
  *out = h;
  return AMHIP_OK;
}

int amhip_stereo_destroy(amhip_stereo* h) {
  if (!h) return seq_arg_fail("null stereo object");
  (void)ctx_use_device(&h->impl.ctx->impl);
  seq_free(&h->impl);
  delete h;
  return AMHIP_OK;
}

int amhip_stereo_reset(amhip_stereo* h) {
  if (!h) return seq_arg_fail("null stereo object");
  Stereo* s = &h->impl;
  int rc = ctx_use_device(&s->ctx->impl);
  if (rc) return rc;
  s->first_frame = true;
  s->left_slot = 0;
  if ((rc = seq_clear(s))) return rc;
  AMHIP_TRY(hipMemsetAsync(s->pc2, 0, s->npix * 16, s->ctx->impl.stream));
  return AMHIP_OK;
}

int amhip_stereo_set_pairs_in_flight(amhip_stereo* h, int n) {
  if (n < 1 || n > AMHIP_STEREO_MAX_BATCH)
    return seq_arg_fail("amhip_stereo_set_pairs_in_flight: n must be in [1, 16]");
  if (!h) return seq_arg_fail("null stereo object");
  Stereo* s = &h->impl;
  int rc = ctx_use_device(&s->ctx->impl);
  if (rc) return rc;
  // (slots and stacks only grow: a frame carried over from earlier calls stays in its slot)
  if ((rc = seq_grow_slots(s, n + 1))) return rc;
  if ((rc = seq_grow_stacks(s, n))) return rc;
  s->in_flight = n;
  return AMHIP_OK;
}

int amhip_stereo_add_frame(amhip_stereo* h, const double* T_G_B7, const uint8_t* host_image,
                           size_t step, int channels) {
  return add_one(h, T_G_B7, host_image, step, channels, false);
}

int amhip_stereo_add_frame_dev(amhip_stereo* h, const double* T_G_B7, const uint8_t* dev_image,
                               size_t step, int channels) {
  return add_one(h, T_G_B7, dev_image, step, channels, true);
}

int amhip_stereo_add_frames(amhip_stereo* h, const double* T_G_B7xF, const uint8_t* const* host_images,
                            const size_t* steps, int channels, size_t F) {
  if (F > 0 && !host_images) {
    const int rc = check_channels(channels);
    return rc ? rc : seq_arg_fail("amhip_stereo_add_frames: null argument");
  }
  static const uint8_t* const none[1] = {nullptr};
  return add_many(h, T_G_B7xF, host_images ? host_images : none, steps, nullptr, 0, 0, channels, F);
}

int amhip_stereo_add_frames_dev(amhip_stereo* h, const double* T_G_B7xF, const uint8_t* dev_frames,
                                size_t frame_stride, size_t row_step, int channels, size_t F) {
  return add_many(h, T_G_B7xF, nullptr, nullptr, dev_frames, frame_stride, row_step, channels, F);
}

int amhip_stereo_cloud(amhip_stereo* h, const double** dev_xyz, const int32_t** dev_intensities,
                       size_t* n, size_t* pairs) {
  if (!h) return seq_arg_fail("null stereo object");
  Stereo* s = &h->impl;
  Ctx* c = &s->ctx->impl;
  int rc = ctx_use_device(c);
  if (rc) return rc;
  AMHIP_TRY(hipMemcpyAsync(s->host_state, s->state, sizeof(SeqState), hipMemcpyDeviceToHost, c->stream));
  rc = ctx_fetch_status(c);  // (synchronises)
  const size_t total = (size_t)s->host_state->running;
  if (dev_xyz) *dev_xyz = s->xyz;
  if (dev_intensities) *dev_intensities = s->inten;
  if (n) *n = total < s->cap ? total : s->cap;
  if (pairs) *pairs = s->host_state->pairs;
  return rc;
}

int amhip_stereo_point_cloud2_dev(amhip_stereo* h, const void** dev_data, size_t* bytes) {
  if (!h) return seq_arg_fail("null stereo object");
  if (dev_data) *dev_data = h->impl.pc2;
  if (bytes) *bytes = h->impl.npix * 16;
  return AMHIP_OK;
}

}  // extern "C"
