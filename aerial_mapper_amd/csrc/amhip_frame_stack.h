// amhip_frame_stack.h -- the host side the image decoders share, and the one the encoders share.
// The decoders (amhip_jpeg_decode.hip, amhip_png_decode.hip): F files in host memory -> ONE stack of
// frames in HBM.
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
// The other direction (amhip_jpeg.hip, amhip_png_encode.hip, amhip_tiff_encode.hip):
// one stack of F frames -> F files.  encode_frame_stack<Enc> and write_frame_stack<Enc> own the contract
// of the four stack exports -- the null checks, *dev_files = NULL on every failure, "filenames[f] is
// null", the device, host frames staged a group at a time, the download slices, files written in order
// up to the first that cannot be, offsets as prefix sums, the final synchronise -- and encode_groups is
// the two-pass loop the GeoTIFF and the single-image PNG encoders run as well.  An encoder derives from
// EncodeGroups (the groups, the scratch, the stream, every file's size) and fills in the format:
//
//   struct Enc : EncodeGroups {                      (one object per call; it owns its device scratch)
//     void plan(...);                                host only: geometry, then plan_uniform(F, a frame's
//                                                    scratch, the format's tuning key and default, cap)
//     int open();                                    allocates the scratch of most_group_frames() frames
//     int front(gi, ...);                            every pass of group gi up to its files' sizes, which
//                                                    it reads back into sizes[group_begin[gi] ..]
//     int back(gi, out, at);                         group gi's files to out + at, group_bytes(gi) bytes;
//                                                    front(gi) ran last
//     size_t frame_stride() const;                   the stack drivers only: bytes from frame to frame,
//     size_t group_span(gi) const;                   ... and the bytes of the stack group gi spans;
//                                                    front(gi, px) takes the group's first frame
//   };
//
// The format's argument check and plan() reach a driver as one callback, which sets the error text
// itself: the drivers never see `quality` and never ask which format they serve.
//
// Also here: DevBuf, open_device and budget_bytes, for every entry point that is one synchronous call
// on the default stream (amhip_io.hip's text parser as well), and capacity_failure.
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

// ---- the encoders ------------------------------------------------------------------------------------

// a file that does not fit the caller's buffer: `who` is the export's name, or "jpeg" / "png"
inline int capacity_failure(const char* who, unsigned long long need, unsigned long long cap) {
  return arg_failure((std::string(who) + ": the file takes " + std::to_string(need) + " bytes, the buffer holds " +
                      std::to_string(cap) + " (nothing written)").c_str());
}

// What a grouped encoder keeps of one call besides its own geometry: the groups, the scratch of the
// largest group (which lives for the call) and the sizes of all files.
struct EncodeGroups {
  size_t F = 0;
  std::vector<size_t> group_begin;   // the first frame of every group, then F
  std::vector<uint64_t> sizes;       // every frame's file, once front() of its group ran
  DevBuf scratch;
  hipStream_t stream = nullptr;      // the default stream: the stack entry points are synchronous

  size_t groups() const { return group_begin.size() - 1; }
  size_t group_frames(size_t gi) const { return group_begin[gi + 1] - group_begin[gi]; }
  uint64_t group_bytes(size_t gi) const {
    uint64_t sum = 0;
    for (size_t f = group_begin[gi]; f < group_begin[gi + 1]; ++f) sum += sizes[f];
    return sum;
  }
  uint64_t largest_file(size_t gi) const {
    uint64_t most = 0;
    for (size_t f = group_begin[gi]; f < group_begin[gi + 1]; ++f) most = sizes[f] > most ? sizes[f] : most;
    return most;
  }
  size_t most_group_frames() const {
    size_t most = 0;
    for (size_t gi = 0; gi < groups(); ++gi) most = group_frames(gi) > most ? group_frames(gi) : most;
    return most;
  }
  // host only: `frames` frames that cost `cost` bytes of scratch each, cut by plan_groups
  void plan_uniform(size_t frames, size_t cost, const char* budget_key, double default_mb, size_t max_per_group) {
    F = frames;
    std::vector<size_t> costs(F, cost), base(F);
    size_t max_group_bytes = 0;
    plan_groups(costs.data(), F, budget_bytes(budget_key, default_mb), max_per_group, &group_begin, base.data(),
                &max_group_bytes);
    sizes.assign(F, 0);
  }
};

constexpr size_t kMaxGroupFrames = 65535;   // (grid.y of the per-frame launches)
constexpr size_t kWriteSlice = 8u << 20;    // bytes of files downloaded at a time by a writing call

// The output of a call is one buffer of exactly the files' bytes (or the caller's, which nothing may
// be written to unless the whole fits), so the sizes come first: front(gi) runs every group up to its
// sizes, place(&out, &at) sizes or checks the output from enc.sizes, then every group goes straight
// to its place, out + at onwards.  front(gi) runs again first when there is more than one group (the
// groups share the scratch): no second buffer and no copy; twice the arithmetic, in calls whose
// scratch exceeds the budget only.
template <typename Enc, typename Front, typename Place>
int encode_groups(Enc& enc, Front front, Place place) {
  const size_t G = enc.groups();
  int rc;
  for (size_t gi = 0; gi < G; ++gi)
    if ((rc = front(gi))) return rc;
  uint8_t* out = nullptr;
  uint64_t at = 0;
  if ((rc = place(&out, &at))) return rc;
  for (size_t gi = 0; gi < G; ++gi) {
    if (G > 1 && (rc = front(gi))) return rc;
    if ((rc = enc.back(gi, out, at))) return rc;
    at += enc.group_bytes(gi);
  }
  return AMHIP_OK;
}

// amhip_io_encode_*_frames: F frames in HBM -> one device buffer of the F files, back to back.
// plan(&enc): the format's own argument check, then enc.plan(..); it sets the error text itself.
template <typename Enc, typename Plan>
int encode_frame_stack(const char* who, int device, const uint8_t* dev_frames, uint8_t** dev_files, size_t* offsets,
                       Plan plan) {
  if (dev_files) *dev_files = nullptr;
  if (!dev_frames || !dev_files || !offsets) {
    set_last_error(std::string(who) + ": null argument");
    return AMHIP_ERR_ARG;
  }
  Enc enc;
  int rc;
  if ((rc = plan(&enc))) return rc;
  if ((rc = open_device(device, who))) return rc;
  if ((rc = enc.open())) return rc;
  DevBuf out;
  rc = encode_groups(
      enc, [&](size_t gi) { return enc.front(gi, dev_frames + enc.group_begin[gi] * enc.frame_stride()); },
      [&](uint8_t** to, uint64_t*) {
        uint64_t total = 0;
        for (size_t gi = 0; gi < enc.groups(); ++gi) total += enc.group_bytes(gi);
        const int r = out.alloc((size_t)total);
        *to = out.as<uint8_t>();
        return r;
      });
  if (rc) return rc;
  AMHIP_TRY(hipStreamSynchronize(enc.stream));
  prefix_offsets(enc.sizes.data(), enc.F, offsets);
  *dev_files = static_cast<uint8_t*>(out.release());
  return AMHIP_OK;
}

// amhip_io_write_*_frames: the same files, frame f written to filenames[f].  Group by group: encode,
// download the group's bytes, write its files in order; the first file that cannot be written ends
// the call.  Host frames are uploaded a group at a time.
template <typename Enc, typename Plan>
int write_frame_stack(const char* who, int device, const uint8_t* frames, int on_device,
                      const char* const* filenames, Plan plan) {
  auto fail_arg = [who](const std::string& msg) {
    set_last_error(std::string(who) + ": " + msg);
    return AMHIP_ERR_ARG;
  };
  if (!frames || !filenames) return fail_arg("null argument");
  Enc enc;
  int rc;
  if ((rc = plan(&enc))) return rc;
  for (size_t f = 0; f < enc.F; ++f)
    if (!filenames[f]) return fail_arg("filenames[" + std::to_string(f) + "] is null");
  if ((rc = open_device(device, who))) return rc;
  if ((rc = enc.open())) return rc;
  DevBuf staged;   // a group of host frames, uploaded
  if (!on_device) {
    size_t most = 0;
    for (size_t gi = 0; gi < enc.groups(); ++gi) most = enc.group_span(gi) > most ? enc.group_span(gi) : most;
    if ((rc = staged.alloc(most))) return rc;
  }
  std::vector<uint8_t> host;
  for (size_t gi = 0; gi < enc.groups(); ++gi) {
    const size_t last = enc.group_begin[gi + 1];
    const uint8_t* px = frames + enc.group_begin[gi] * enc.frame_stride();
    if (!on_device) {
      AMHIP_TRY(hipMemcpyAsync(staged.p, px, enc.group_span(gi), hipMemcpyHostToDevice, enc.stream));
      px = staged.as<const uint8_t>();
    }
    if ((rc = enc.front(gi, px))) return rc;
    DevBuf out;
    if ((rc = out.alloc((size_t)enc.group_bytes(gi)))) return rc;
    if ((rc = enc.back(gi, out.as<uint8_t>(), 0))) return rc;
    // Down in slices of consecutive files, kWriteSlice bytes at the most (one file at the least): the
    // host buffer is touched once and reused, where one buffer for a group of 200 MB would be fresh
    // pages, faulted in and zeroed, on every call.
    size_t at = 0;
    for (size_t f = enc.group_begin[gi]; f < last;) {
      size_t slice = 0;
      const size_t end = slice_end(enc.sizes.data(), f, last, kWriteSlice, &slice);
      if (host.size() < slice) host.resize(slice);
      AMHIP_TRY(hipMemcpyAsync(host.data(), out.as<uint8_t>() + at, slice, hipMemcpyDeviceToHost, enc.stream));
      AMHIP_TRY(hipStreamSynchronize(enc.stream));
      size_t in_slice = 0;
      for (; f < end; ++f) {
        if ((rc = write_file(who, filenames[f], host.data() + in_slice, (size_t)enc.sizes[f]))) return rc;
        in_slice += (size_t)enc.sizes[f];
      }
      at += slice;
    }
  }
  return AMHIP_OK;
}

}  // namespace amhip

#endif  // AMHIP_FRAME_STACK_H_
