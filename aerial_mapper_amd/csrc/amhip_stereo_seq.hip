// amhip_stereo_seq.hip -- stereo::Stereo (aerial_mapper_dense_pcl/src/stereo.cpp): a frame
// sequence -> one dense cloud, resident in HBM from the uploaded frame to the concatenated cloud.
//
// Host side only: the kernels are the rectifier's (amhip_rectify.hip), the matchers'
// (amhip_stereo.hip), the mapped undistorter's (amhip_forward.hip) and the append-mode densify
// (amhip_densify.hip).  What this file adds is the order of things:
//   frames     two raw slots that swap roles (frame j lives in slot j & 1): a frame is staged once
//              and undistorted once although it is the right image of one pair and the left image
//              of the next.  Host frames go through two pinned buffers and a second stream; the
//              upload of frame j + 1 waits only for the rectifier of the pair that last read its
//              slot, so it runs beside the matching of pair j.
//   pairs      rectify -> match -> append, all enqueued on the context's stream; the point count
//              stays on the device (SeqState) and is read once, by amhip_stereo_cloud.
//   capacity   settled before the first pair of a sequence (pairs x W x H points).
#include <cstring>
#include <new>

#include "amhip_common.h"

namespace amhip {

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
  hipEvent_t ev_up[2] = {nullptr, nullptr};    // the upload into slot s has finished
  hipEvent_t ev_free[2] = {nullptr, nullptr};  // the last kernel reading raw[s] has finished
  bool up_used[2] = {false, false};
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* raw[2] = {nullptr, nullptr};
  uint8_t* und[2] = {nullptr, nullptr};

  bool first_frame = true;
  int left_slot = 0;
  double R1[9] = {}, t1[3] = {};

  uint8_t *rect_l = nullptr, *rect_r = nullptr, *mask = nullptr;
  float* disp = nullptr;
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

// The selected matcher's own argument check, run without a context: it reports every parameter
// error before it looks at the context, so "null context" means the parameters passed.
static int check_matcher_params(const amhip_stereo_settings& s, int W, int H) {
  const uint8_t* img = reinterpret_cast<const uint8_t*>(&s);  // (never dereferenced: no context)
  float* out = reinterpret_cast<float*>(const_cast<amhip_stereo_settings*>(&s));
  const int rc = s.use_bm
      ? amhip_bm_disparity_dev(nullptr, &s.bm, W, H, img, (size_t)W, img, (size_t)W, nullptr, 0, out,
                               (size_t)W * sizeof(float), nullptr, 0)
      : amhip_sgbm_disparity_dev(nullptr, &s.sgbm, W, H, img, (size_t)W, img, (size_t)W, nullptr, 0,
                                 out, (size_t)W * sizeof(float), nullptr, 0);
  if (rc == AMHIP_ERR_ARG && std::strstr(amhip_last_error(), "null context")) {
    set_last_error("");
    return AMHIP_OK;
  }
  return rc;
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
  for (int k = 0; k < 2; ++k) {
    if (s->ev_up[k]) (void)hipEventDestroy(s->ev_up[k]);
    if (s->ev_free[k]) (void)hipEventDestroy(s->ev_free[k]);
    if (s->pin[k]) (void)hipHostFree(s->pin[k]);
    if (s->raw[k]) (void)hipFree(s->raw[k]);
    if (s->und[k]) (void)hipFree(s->und[k]);
  }
  if (s->up_stream) (void)hipStreamDestroy(s->up_stream);
  void* dev[] = {s->rect_l, s->rect_r, s->mask, s->disp, s->xyz, s->inten, s->state, s->pc2};
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

// One frame of the sequence: stage, undistort, and -- unless it is the first -- run the pair.
static int seq_push(Stereo* s, const double* T_G_B7, const uint8_t* src, size_t step, bool on_device,
                    bool replace) {
  Ctx* c = &s->ctx->impl;
  hipStream_t main = c->stream;
  // stereo.cpp:129-137: T_G_C = T_G_B * T_B_C, its position and rotation matrix
  const HPose T_G_C = hpose_compose(hpose_from7(T_G_B7), s->T_B_C);
  double R2[9];
  quat_to_matrix(T_G_C, R2);
  const double t2[3] = {T_G_C.tx, T_G_C.ty, T_G_C.tz};
  const int slot = s->first_frame ? 0 : (s->left_slot ^ 1);
  const size_t W = (size_t)s->W, H = (size_t)s->H;
  if (on_device) {
    AMHIP_TRY(hipMemcpy2DAsync(s->raw[slot], W, src, step, W, H, hipMemcpyDeviceToDevice, main));
  } else {
    if (s->up_used[slot]) AMHIP_TRY(hipEventSynchronize(s->ev_up[slot]));  // pin[slot] is free again
    for (size_t v = 0; v < H; ++v) std::memcpy(s->pin[slot] + v * W, src + v * step, W);
    AMHIP_TRY(hipStreamWaitEvent(s->up_stream, s->ev_free[slot], 0));
    AMHIP_TRY(hipMemcpyAsync(s->raw[slot], s->pin[slot], s->npix, hipMemcpyHostToDevice, s->up_stream));
    AMHIP_TRY(hipEventRecord(s->ev_up[slot], s->up_stream));
    s->up_used[slot] = true;
    AMHIP_TRY(hipStreamWaitEvent(main, s->ev_up[slot], 0));
  }
  const uint8_t* img[2] = {s->raw[0], s->raw[1]};
  if (s->undistort) {
    ScopedTimer t(c, AMHIP_K_MISC);
    int rc = undistort_frames_run(main, s->cam, s->raw[slot], s->npix, W, 1, 1, s->und[slot]);
    if (rc) return rc;
    AMHIP_TRY(hipEventRecord(s->ev_free[slot], main));
    img[0] = s->und[0];
    img[1] = s->und[1];
  }
  if (s->first_frame) {
    std::memcpy(s->R1, R2, sizeof(R2));
    std::memcpy(s->t1, t2, sizeof(t2));
    s->left_slot = slot;
    s->first_frame = false;
    return AMHIP_OK;
  }
  const int left = s->left_slot;
  if (t2[0] == s->t1[0] && t2[1] == s->t1[1] && t2[2] == s->t1[2])
    return seq_arg_fail("CHECK_NE(baseline, 0.0) (densifier.cpp:39): both frames have the same position");
  double R_G_C[9], baseline = 0.0;
  int rc = amhip_rectify_stereo_pair_dev(s->ctx, s->K, s->R1, R2, s->t1, t2, s->W, s->H, img[left], W,
                                         img[slot], W, R_G_C, &baseline, nullptr, s->rect_l, s->rect_r,
                                         s->mask);
  if (rc) return rc;
  // (the next frame is staged into the left frame's slot)
  if (!s->undistort) AMHIP_TRY(hipEventRecord(s->ev_free[left], main));
  if (baseline == 0.0) return seq_arg_fail("CHECK_NE(baseline, 0.0) (densifier.cpp:39)");
  const size_t dstep = W * sizeof(float);
  rc = s->settings.use_bm
      ? amhip_bm_disparity_dev(s->ctx, &s->settings.bm, s->W, s->H, s->rect_l, W, s->rect_r, W, s->mask,
                               W, s->disp, dstep, nullptr, 0)
      : amhip_sgbm_disparity_dev(s->ctx, &s->settings.sgbm, s->W, s->H, s->rect_l, W, s->rect_r, W,
                                 s->mask, W, s->disp, dstep, nullptr, 0);
  if (rc) return rc;
  DensifyParams p;
  std::memset(&p, 0, sizeof(p));
  p.width = s->W;
  p.height = s->H;
  p.disp_step = dstep;
  p.img_step = W;
  // stereo projection matrix Q (densifier.cpp:39-46), as amhip_densify_dev builds it
  const double fx = s->K[0], fy = s->K[4], cx = s->K[2], cy = s->K[5];
  p.Q03 = -cx;
  p.Q11 = fx / fy;
  p.Q13 = -cy * (fx / fy);
  p.Q23 = fx;
  p.Q32 = 1.0 / baseline;
  for (int k = 0; k < 9; ++k) p.R[k] = R_G_C[k];
  for (int k = 0; k < 3; ++k) p.t[k] = s->t1[k];
  if ((rc = densify_append_run(c, p, s->disp, s->rect_l, s->xyz, s->inten, s->cap, s->state, s->pc2,
                               replace)))
    return rc;
  // stereo.cpp:142-146: the right frame is the next pair's left frame
  std::memcpy(s->R1, R2, sizeof(R2));
  std::memcpy(s->t1, t2, sizeof(t2));
  s->left_slot = slot;
  return AMHIP_OK;
}

static int check_channels(int channels) {
  if (channels == 3)
    return seq_arg_fail("amhip_stereo: 8UC3 frames are refused: the reference stores the RAW colour "
                        "image (stereo.cpp:131,138), which OpenCV's block matchers reject");
  if (channels != 1) return seq_arg_fail("amhip_stereo: image type not supported (stereo.cpp:123): 8UC1 only");
  return AMHIP_OK;
}

static int add_one(amhip_stereo* h, const double* T, const uint8_t* image, size_t step, int channels,
                   bool on_device);
static int add_many(amhip_stereo* h, const double* T, const uint8_t* const* images,
                    const size_t* steps, const uint8_t* dev_frames, size_t frame_stride,
                    size_t row_step, int channels, size_t F);

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
  if (!s->first_frame && (rc = seq_reserve(s, s->npix))) return rc;
  return seq_push(s, T, image, step, on_device, /*replace=*/true);
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
  if ((rc = seq_clear(s))) return rc;  // point_cloud->clear() (stereo.cpp:86)
  for (size_t i = 0; i < F; ++i) {
    if ((i + 1) % nth != 0) continue;  // ++skip % use_every_nth_image == 0 (:93)
    const uint8_t* src = on_device ? dev_frames + i * frame_stride : images[i];
    if ((rc = seq_push(s, T + 7 * i, src, on_device ? row_step : steps[i], on_device, /*replace=*/false)))
      return rc;
  }
  return AMHIP_OK;
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
  if ((rc = check_matcher_params(*settings, cam->width, cam->height))) return rc;
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
  for (int k = 0; k < 2; ++k) {
    SEQ_TRY(hipEventCreateWithFlags(&s->ev_up[k], hipEventDisableTiming));
    SEQ_TRY(hipEventCreateWithFlags(&s->ev_free[k], hipEventDisableTiming));
    SEQ_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->pin[k]), s->npix, hipHostMallocDefault));
    if ((rc = dev_alloc(reinterpret_cast<void**>(&s->raw[k]), s->npix))) return fail(rc);
    if (s->undistort && (rc = dev_alloc(reinterpret_cast<void**>(&s->und[k]), s->npix))) return fail(rc);
  }
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->rect_l), s->npix))) return fail(rc);
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->rect_r), s->npix))) return fail(rc);
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->mask), s->npix))) return fail(rc);
  if ((rc = dev_alloc(reinterpret_cast<void**>(&s->disp), s->npix * sizeof(float)))) return fail(rc);
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
