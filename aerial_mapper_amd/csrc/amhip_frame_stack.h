// amhip_frame_stack.h -- the host side the image decoders share (amhip_jpeg_decode.hip,
// amhip_png_decode.hip): F files in host memory -> ONE stack of frames in HBM.
// decode_frame_stack<Codec> owns the contract -- the order of the checks, the error texts, the groups,
// the stack's layout, the five out-parameters -- and a codec fills in what a file is:
//
//   struct Codec {                                   (one object per call; it owns its device scratch)
//     using Frame = ...;                             the per-frame descriptor the kernels read: width, height
//     static constexpr const char* kDecode, *kInfo;  the exports' names, the prefix of every error text
//     static constexpr const char* kBudgetKey;       tuning key: MB of group scratch
//     static constexpr double kBudgetMB;             ... and its default
//     static constexpr size_t kGroupFrames;          most frames per group (a grid dimension)
//     static bool info(file, len, &w, &h, &channels, err, errcap);
//     static const char* status_text(uint32_t);
//     bool parse(file, len, Frame*, err, errcap);    host only; stages the frame's bytes, in call order
//     size_t cost_bytes(const Frame&);               the frame's share of a group's scratch
//     void place(Frame*, size_t base_bytes, int colored);   ... and where it starts
//     int upload(files, lens, F, max_group_bytes, colored, stream);   allocates, copies the staged bytes
//     void launch_group(first, n, const StackLaunch<Frame>&);
//   };
//
// Also here: DevBuf, open_device and budget_bytes, for every entry point that is one synchronous call
// on the default stream (amhip_io.hip's text parser as well).
#ifndef AMHIP_FRAME_STACK_H_
#define AMHIP_FRAME_STACK_H_

#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_frame_plan.h"
#include "amhip_tuning.h"

namespace amhip {

// device memory of one call: freed on every way out unless released to the caller
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    AMHIP_TRY(hipMalloc(&p, bytes ? bytes : 16));
    return AMHIP_OK;
  }
  template <typename T>
  T* as() {
    return static_cast<T*>(p);
  }
  void* release() {
    void* q = p;
    p = nullptr;
    return q;
  }
};

// the first touch of the device in an entry point: is there one, is `device` one, make it current
inline int open_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    set_last_error("no HIP device available (libaerial_mapper_hip has no CPU fallback)");
    return AMHIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) {
    set_last_error(std::string(who) + ": bad device index");
    return AMHIP_ERR_ARG;
  }
  AMHIP_TRY(hipSetDevice(device));
  return AMHIP_OK;
}

// a tuning key in MB -> bytes; a value outside [0, 1 TB] means the default
inline size_t budget_bytes(const char* key, double default_mb) {
  const double mb = tuning(key, default_mb);
  return (size_t)((mb >= 0.0 && mb <= 1048576.0 ? mb : default_mb) * 1048576.0);
}

// what a group's launches get besides the codec's own buffers
template <typename Frame>
struct StackLaunch {
  const Frame* frames;   // device: all F descriptors
  uint32_t* status;      // device: one word per frame, 0 = fine
  uint8_t* out;          // device: the stack
  size_t frame_stride, row_step;
  int width, height, colored;
  hipStream_t stream;
};

template <typename Codec>
int image_info(const uint8_t* file, size_t len, int* width, int* height, int* channels) {
  if (!file || !width || !height || !channels) {
    set_last_error(std::string(Codec::kInfo) + ": null argument");
    return AMHIP_ERR_ARG;
  }
  char text[160];
  if (!Codec::info(file, len, width, height, channels, text, sizeof(text))) {
    set_last_error(std::string(Codec::kInfo) + ": " + text);
    return AMHIP_ERR_ARG;
  }
  return AMHIP_OK;
}

template <typename Codec>
int decode_frame_stack(int device, const uint8_t* const* files, const size_t* lens, size_t F, int colored,
                       uint8_t** dev_frames, int* width, int* height, size_t* row_step, size_t* frame_stride) {
  typedef typename Codec::Frame Frame;
  auto fail_arg = [](const std::string& msg) {
    set_last_error(std::string(Codec::kDecode) + ": " + msg);
    return AMHIP_ERR_ARG;
  };
  if (dev_frames) *dev_frames = nullptr;
  if (!files || !lens || !dev_frames || !width || !height || !row_step || !frame_stride)
    return fail_arg("null argument");
  if (F == 0) return fail_arg("no frames (F = 0)");
  // ---- everything the host can see, before any device is touched ---------------------------
  Codec codec;
  std::vector<Frame> frames(F);
  std::vector<size_t> cost(F), base(F);
  char text[160];
  for (size_t i = 0; i < F; ++i) {
    if (!files[i]) return fail_arg("frame " + std::to_string(i) + ": null file");
    if (!codec.parse(files[i], lens[i], &frames[i], text, sizeof(text)))
      return fail_arg("frame " + std::to_string(i) + ": " + text);
    if (frames[i].width != frames[0].width || frames[i].height != frames[0].height)
      return fail_arg("frame " + std::to_string(i) + " is " + std::to_string(frames[i].width) + " x " +
                      std::to_string(frames[i].height) + ", frame 0 is " + std::to_string(frames[0].width) +
                      " x " + std::to_string(frames[0].height));
    cost[i] = codec.cost_bytes(frames[i]);
  }
  const int W = frames[0].width, H = frames[0].height, ch = colored ? 3 : 1;
  // groups of consecutive frames whose scratch fits the budget (at least one frame each)
  std::vector<size_t> group_begin;
  size_t max_group_bytes = 0;
  plan_groups(cost.data(), F, budget_bytes(Codec::kBudgetKey, Codec::kBudgetMB), Codec::kGroupFrames,
              &group_begin, base.data(), &max_group_bytes);
  for (size_t i = 0; i < F; ++i) codec.place(&frames[i], base[i], colored);
  // ---- the device ----------------------------------------------------------------------------
  int rc;
  if ((rc = open_device(device, Codec::kDecode))) return rc;
  hipStream_t stream = nullptr;   // the default stream: this entry point is synchronous
  const size_t rstep = (size_t)W * ch, fstride = rstep * (size_t)H;
  DevBuf desc, status, out;
  if ((rc = codec.upload(files, lens, F, max_group_bytes, colored, stream))) return rc;
  if ((rc = desc.alloc(F * sizeof(Frame)))) return rc;
  if ((rc = status.alloc(F * sizeof(uint32_t)))) return rc;
  if ((rc = out.alloc(F * fstride))) return rc;
  AMHIP_TRY(hipMemcpyAsync(desc.p, frames.data(), F * sizeof(Frame), hipMemcpyHostToDevice, stream));
  AMHIP_TRY(hipMemsetAsync(status.p, 0, F * sizeof(uint32_t), stream));
  const StackLaunch<Frame> launch = {desc.as<Frame>(), status.as<uint32_t>(), out.as<uint8_t>(), fstride, rstep,
                                     W, H, colored ? 1 : 0, stream};
  for (size_t g = 0; g + 1 < group_begin.size(); ++g) {
    codec.launch_group(group_begin[g], group_begin[g + 1] - group_begin[g], launch);
    AMHIP_TRY(hipGetLastError());
  }
  std::vector<uint32_t> st(F);
  AMHIP_TRY(hipMemcpyAsync(st.data(), status.p, F * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  for (size_t i = 0; i < F; ++i)
    if (st[i]) return fail_arg("frame " + std::to_string(i) + ": " + Codec::status_text(st[i]));
  *dev_frames = static_cast<uint8_t*>(out.release());
  *width = W;
  *height = H;
  *row_step = rstep;
  *frame_stride = fstride;
  return AMHIP_OK;
}

}  // namespace amhip

#endif  // AMHIP_FRAME_STACK_H_
