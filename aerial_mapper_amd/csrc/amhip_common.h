// amhip_common.h -- internal declarations shared by the HIP translation units
// of libaerial_mapper_hip.so (gfx950 only; not part of the public C ABI).
#ifndef AMHIP_COMMON_H_
#define AMHIP_COMMON_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "aerial_mapper_hip.h"
#include "amhip_tuning.h"
#include "amhip_dsm_plan.h"
#include "amhip_ortho_fold.h"
#include "amhip_ortho_plan.h"
#include "amhip_session_plan.h"

namespace amhip {

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
void set_last_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define AMHIP_TRY(expr)                                                  \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) return ::amhip::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

// ---------------------------------------------------------------------------
// device-side constants
// ---------------------------------------------------------------------------
// kMaxLevels, kMaxW0, kTileI, kMaxRegionRows, DsmParams (geometry + search parameters of one DSM call,
// passed by value to kernels), the tile lists' numbers: amhip_dsm_plan.h

// The binned cloud as the gather sees it (amhip_dsm.hip: pts_x / pts_y / pts_z; filled by
// dsm_sort): the doubles pipeline (sorted), the record pipeline of the single-precision
// gather (rec + sidx + cloud), or both.
struct PtsView {
  const double* sorted;   // 3 doubles per sorted point (px, py, z), or null
  const uint4* rec;       // 16-byte record per sorted point, or null: x = cell ix | iy << 16
                          // (map cells + margin M), y / z = offsets from the cell centre in
                          // units of 2^-fx_S cells (int32), w = f32 bits of z - zref[0]
  const uint32_t* sidx;   // row of the caller's cloud behind sorted point g (with rec)
  const double* cloud;    // the caller's cloud (AoS x, y, z), untouched
  const double* zref;     // device: [0] the reference height of the records' offsets
  double sub_x, sub_y;    // dsm.cc:42-43's centre offsets (applied when reading `cloud`)
};

// FramePose / FrameFast (per-frame inverse pose T_C_G = T_G_C^-1): amhip_ortho_fold.h
// OrthoParams (geometry, camera and switches of one mosaic call, passed by value to kernels), HPose and
// the host pose arithmetic: amhip_ortho_plan.h

// Device error word bits (sticky until amhip_ctx_synchronize).
enum : unsigned { kDevErrExactHit = 1u, kDevErrAlphaNonPos = 2u, kDevErrHaloOverflow = 4u,
                  kDevErrRectifyZeroW = 8u };

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
constexpr int kMaxHaloDests = 8;
struct HaloParams {
  double base_x, base_y, inv_res, sub_x, sub_y;
  int nd;
  double lo_i[kMaxHaloDests], hi_i[kMaxHaloDests], lo_j[kMaxHaloDests], hi_j[kMaxHaloDests];
  unsigned long long cap;
  // where destination d's rows start in the output (in points) and how many it may take:
  // d * cap / cap for the equal-split layout of the RCCL exchange; prefix sums of the counts /
  // the counts themselves for the session's count-then-compact routing (cap_d = 0: count only)
  unsigned long long off[kMaxHaloDests], cap_d[kMaxHaloDests];
  // a box (open) no destination reaches into -- the inside of the context's own window --
  // or an empty one: a point in it is done after four comparisons
  double in_lo_i, in_hi_i, in_lo_j, in_hi_j;
};
// Multi-GPU tiling (amhip_dsm_tiled_begin_dev / _finish_dev): the sort's count pass in two
// parts around the caller's halo exchange.  phase 1: count rows [0, n_prefix) of the cloud
// and copy the points other windows need into their send rows, then stop; phase 2: count
// rows [n_prefix, n) (what the exchange delivered) and carry on.
struct SortSplit {
  int phase;
  size_t n_prefix;
  HaloParams hp;
  double* halo_out;
  unsigned long long* halo_counts;
};

// The JPEG encoder's scratch (amhip_jpeg.hip), owned by a context or a mosaic, grown on demand and
// kept: coefficients, bit counts, scan partials and the packed words of one call in `dev`; the
// header and the two words read back in `pinned`; the raster a layer is turned into before it is
// encoded in `image`; the file before it goes to the host in `out`.
struct JpegScratch {
  uint8_t* dev = nullptr;
  size_t cap = 0;
  uint8_t* pinned = nullptr;
  uint8_t* image = nullptr;
  size_t image_cap = 0;
  uint8_t* out = nullptr;
  size_t out_cap = 0;
};
enum { kJpegGray8 = 0, kJpegBgr8 = 1, kJpegBgr16s = 2 };   // 8UC1 / 8UC3 / CV_16SC3 clamped to 0..255
struct JpegSource {
  const void* dev;
  size_t step;     // bytes per row
  int width, height;
  int mode;
};
void jpeg_scratch_free(JpegScratch* ws);
int jpeg_scratch_image(JpegScratch* ws, size_t bytes, uint8_t** out);
// true: rows x cols pixels are what a JPEG file, or a PNG file of this encoder, holds
inline bool image_size_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535; }
// the whole file into dev_out (at most cap bytes, nothing written when it does not fit:
// AMHIP_ERR_ARG); asynchronous on `stream` up to the read-back of *bytes.  Arguments checked by
// the callers (jpeg::check_image_args); quality 0 = 95.
int jpeg_encode_run(hipStream_t stream, JpegScratch* ws, const JpegSource& src, int quality,
                    uint8_t* dev_out, size_t cap, size_t* bytes);
// encode, download, write `filename`
int jpeg_write_run(const char* what, hipStream_t stream, JpegScratch* ws, const JpegSource& src,
                   int quality, const char* filename);
// the whole of `data` to `filename`; a failure is AMHIP_ERR_ARG with `what`, the name and errno's text
int write_file(const char* what, const char* filename, const uint8_t* data, size_t size);

// The PNG encoder (amhip_png_encode.hip) on the same sources: the file into dev_out (at most cap
// bytes, nothing written when it does not fit: AMHIP_ERR_ARG), or downloaded and written.  Its
// scratch lives for the call.  Arguments checked by the callers (pnge::check_image_args).
int png_encode_run(hipStream_t stream, const JpegSource& src, uint8_t* dev_out, size_t cap, size_t* bytes);
int png_write_run(const char* what, hipStream_t stream, const JpegSource& src, const char* filename);

// What the JPEG and the PNG entry points share (amhip_jpeg.hip).  stage_host_image: a host image (*src)
// -> the context's image scratch, rows packed; *src then names the copy.  layer_image_source: the
// context's window of `layer` as an image in that scratch -> *src; `limit`: the whole refusal of a
// window no file of the format holds.
struct Ctx;
int stage_host_image(Ctx* c, int channels, JpegSource* src);
int layer_image_source(amhip_ctx* h, const char* limit, int layer, int bgr, float lower, float upper, JpegSource* src);

// The GeoTIFF reader (amhip_tiff_decode.hip) under a layer, in two halves, so that a session can run the
// first on every window before the second on any: prepare parses the file and decodes the pixels under
// the context's window into a raster of its own (no layer is touched; an error leaves nothing behind),
// place writes the layer.  The job is freed by the caller, after either.
// level: which level of the file: k >= 0, -1 the automatic choice for the map's
// resolution, kTiffFirstIfd the exports without the argument (IFD 0, the chain not looked at).
struct TiffLayerJob;
struct Ctx;
constexpr int kTiffFirstIfd = -2;
int tiff_layer_prepare(Ctx* c, const char* who, int layer, const uint8_t* file, size_t len, int level,
                       TiffLayerJob** job);
int tiff_layer_place(Ctx* c, TiffLayerJob* job);
void tiff_layer_job_free(TiffLayerJob* job);
// the whole of `filename`; a failure is AMHIP_ERR_ARG with `what`, the name and errno's text
int read_file(const char* what, const char* filename, std::vector<uint8_t>* out);

struct TimedRegion {
  hipEvent_t a, b;
  int slot;
};

struct Ctx {
  amhip_grid_desc grid;       // the (global) map
  int win_i0 = 0, win_j0 = 0; // window of it this context owns
  int win_rows = 0, win_cols = 0;
  bool windowed = false;      // created as a proper part of the map (a tile of a tiling)
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t order_event = nullptr;  // amhip_ctx_order_after
  size_t cells = 0;
  int dsm_exact = 0;          // amhip_ctx_set_dsm_precision
  // single-precision mode on rough terrain (amhip_api.hip: dsm_rough_policy): when a call filed
  // more than half of its tiles for the FP64 kernel, the next calls run the FP64 pipeline
  // outright (sorted doubles instead of records + the caller's unsorted cloud)
  int dsm_exact_now = 0;      // this call
  int rough_hold = 0;         // calls left before the single-precision pipeline is tried again
  bool last_call_f32 = false; // the last DSM call ran the record pipeline with bin ranges
  int dsm_knn = 0;            // amhip_ctx_set_dsm_knn

  float* layers[AMHIP_NUM_LAYERS] = {nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr};
  // the lazy-reset state of every layer (amhip_session_plan.h: LayerState and its transitions)
  LayerState layer_state[AMHIP_NUM_LAYERS] = {kLayerWritten, kLayerWritten, kLayerWritten,
                                              kLayerWritten, kLayerWritten, kLayerWritten};
  // [min, max] of the heights every DSM call since the last reset could have
  // written (ordered 64-bit keys, amhip_device.h); lets the mosaic kernel drop
  // tiles no frame of a small batch can see before it reads their elevation.
  // Not valid once the elevation layer was written from outside.
  unsigned long long* dev_zrange = nullptr;
  bool zrange_valid = false;
  double* zpart = nullptr;       // per-workgroup partials of one call
  size_t zpart_cap = 0;
  unsigned* dev_err = nullptr;   // device error word
  unsigned* host_err = nullptr;  // pinned mirror

  // DSM workspaces (grow on demand)
  PtsView pts = {};              // what the last dsm_sort left for the gather
  double* sorted = nullptr;      // 3 doubles per binned point (px, py, z)
  size_t sorted_cap = 0;         // in points
  uint32_t* rank = nullptr;      // per input point: rank inside its bin
  size_t rank_cap = 0;
  uint32_t* bin_start = nullptr; // nbins + 1 (+ scan partials behind it)
  size_t bin_cap = 0;
  // record pipeline (single-precision gather): 20-byte records between the sort passes, the
  // 16-byte records + rows the gather reads, the records' reference height
  uint32_t* rec_a = nullptr;
  size_t rec_a_cap = 0;
  uint32_t* rec_b = nullptr;
  size_t rec_b_cap = 0;
  uint32_t* rec16 = nullptr;     // (uint4 per point)
  size_t rec16_cap = 0;
  uint32_t* sidx = nullptr;
  size_t sidx_cap = 0;
  double* zref = nullptr;        // [0] reference height, [1] / [2] range of the cloud's heights
  size_t zref_cap = 0;
  double* zall = nullptr;        // per-wave [min, max] partials of the count pass
  size_t zall_cap = 0;
  uint32_t* bin_z = nullptr;     // per bin: ordered keys of its lowest / highest height (uint2)
  size_t bin_z_cap = 0;
  bool bin_z_valid = false;      // written by the last sort (three-pass, single-precision mode)
  uint32_t* scan_partials = nullptr;
  size_t partial_cap = 0;
  double* tmp_points = nullptr;    // stripe-ordered points (level 1 of the sort)
  size_t tmp_points_cap = 0;
  uint32_t* stripe_ws = nullptr;   // stripe counts / starts / cursors
  size_t stripe_ws_cap = 0;
  uint8_t* tile_occ = nullptr;         // per gather tile: any point within the last radius
  size_t tile_occ_cap = 0;
  int* tile_list = nullptr;            // sparse gather: [count (4 ints)] [occupied tile ids]
  size_t tile_list_cap = 0;
  unsigned char* fill_mask = nullptr;  // OrthoFromPcl adaptive passes
  size_t fill_mask_cap = 0;
  int32_t* stage_values = nullptr;     // H2D staging of host intensities
  size_t stage_values_cap = 0;
  double* stage_points = nullptr;  // H2D staging of host clouds
  size_t stage_points_cap = 0;

  // ortho workspaces
  ViewBoundsCache view_bounds;   // of the last camera with a distortion model (plan_ortho_call)
  FramePose* frame_poses = nullptr;
  size_t frame_pose_cap = 0;
  uint8_t* stage_frames = nullptr;
  size_t stage_frames_cap = 0;
  // the blended mosaic's per-cell FP64 sums (amhip_ortho_blend.hip): [0] gray, 2 planes of
  // `cells` doubles (wsum, acc); [1] colour, 4 planes (wsum, B, G, R).  Allocated, zero, by the
  // first blended call of that kind.
  double* blend_sums[2] = {nullptr, nullptr};
  // The cells of the window the LAST DSM / mosaic call can have written (window coordinates):
  // the whole window, the sub-window of a small cloud, or the bounding box of the mosaic's tile
  // list (then still on the device: dirty_on_device, read back by ctx_last_dirty()).  What the
  // session downloads after the call (amhip_session.hip) instead of whole layers.
  int dirty[4] = {0, 0, 0, 0};   // i0, j0, rows, cols
  bool dirty_on_device = false;
  int* dev_bbox = nullptr;       // k_dsm_bbox: [min i, max i, min j, max j, count] of a small cloud
  int* host_bbox = nullptr;      // pinned mirror
  int* ortho_list = nullptr;     // [count (4 ints)] [tiles some frame of a small batch can see]
  size_t ortho_list_cap = 0;

  // amhip_dsm_tiled_begin_dev .. amhip_dsm_tiled_finish_dev
  bool tiled_pending = false;
  const double* tiled_xyz = nullptr;
  size_t tiled_n = 0;
  int tiled_radius_sq = 0;
  double tiled_ce = 0.0, tiled_cn = 0.0;
  SortSplit tiled_split = {};
  DsmParams tiled_params = {};  // the begin call's plan: the finish call must bin with the same

  // stats of the last DSM call
  int64_t last_points_binned = 0;
  int64_t last_num_bins = 0;
  int32_t last_bin_cells = 0;
  int last_sort_pipeline = -1;    // AMHIP_SORT_* of the last dsm_sort (-1: none yet)
  int64_t last_ntiles = 0;        // gather tiles of the last call (0: not the LDS-tiled gather)
  // Launch bookkeeping (round 5): what the sort's single-workgroup kernel resets for the gather
  // (SortAux), where the scatter waves' height partials end, the ticket of the count pass's
  // reduce-then-scan kernel, and the pinned words the device leaves for the NEXT call's launch
  // policy (never waited for): [0] sub-partitions beyond the placement workgroup's registers.
  uint32_t* aux_zero_words = nullptr;
  int aux_nzero = 0;
  bool aux_done = false;
  size_t range_parts = 0;
  unsigned long long* range_running = nullptr;
  unsigned* dev_tickets = nullptr;      // 16 words, zero between launches
  unsigned* host_sort_stats = nullptr;  // pinned, 4 words
  unsigned long long sort_stats_sig = 0, tile_stats_sig = 0;  // the geometry the pinned counters describe
  unsigned* host_tile_stats = nullptr;  // pinned mirror of the last call's tile-list counters

  // the stereo matchers (amhip_stereo.hip): the cost volumes or prefiltered images, the maps and
  // the speckle labels of one call, carved out of one block that grows on demand
  uint8_t* stereo_ws = nullptr;
  size_t stereo_ws_cap = 0;
  JpegScratch jpeg;

  // timing
  bool timing = false;
  std::vector<TimedRegion> regions;
  std::vector<TimedRegion> free_regions;
  double slot_ms[AMHIP_NUM_KERNELS] = {};
  int64_t slot_launches[AMHIP_NUM_KERNELS] = {};
};

// RAII-less helper: bracket a launch sequence with events when timing is on.
struct ScopedTimer {
  Ctx* c;
  TimedRegion r;
  bool on;
  ScopedTimer(Ctx* ctx, int slot);
  ~ScopedTimer();
};

template <typename T>
int ensure_capacity(T** ptr, size_t* cap, size_t need);

int ensure_bytes(void** ptr, size_t* cap_bytes, size_t need_bytes);

// ---------------------------------------------------------------------------
// launchers (defined in amhip_dsm.hip / amhip_ortho.hip)
// ---------------------------------------------------------------------------
int launch_fill(Ctx* c, float* dst, size_t n, float value);

// stereo densifier reprojection (amhip_densify.hip)
struct DensifyParams {
  int width, height;
  size_t disp_step, img_step;  // bytes per row
  double Q03, Q11, Q13, Q23, Q32;
  double R[9], t[3];
};
// the stereo projection matrix Q (densifier.cpp:39-46; K row-major) and the pose of one W x H pair
inline DensifyParams densify_params(const double* K, double baseline, const double* R_G_C,
                                    const double* t_G_C1, int width, int height, size_t disp_step,
                                    size_t img_step) {
  DensifyParams p = {};
  p.width = width;
  p.height = height;
  p.disp_step = disp_step;
  p.img_step = img_step;
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  p.Q03 = -cx;
  p.Q11 = fx / fy;
  p.Q13 = -cy * (fx / fy);
  p.Q23 = fx;
  p.Q32 = 1.0 / baseline;
  for (int k = 0; k < 9; ++k) p.R[k] = R_G_C[k];
  for (int k = 0; k < 3; ++k) p.t[k] = t_G_C1[k];
  return p;
}
int densify_run(Ctx* c, const DensifyParams& p, const float* dev_disparity,
                const uint8_t* dev_image_left, double* dev_xyz_out, int32_t* dev_intensity_out,
                size_t capacity, long long* dev_count);

// Append mode (amhip_stereo_seq.hip): the device-resident bookkeeping of one frame sequence.
// running = points of the sequence so far, base = where the current pair's points start,
// pairs = pairs in the cloud, skip = the current pair adds nothing (its rectification failed).
struct SeqState {
  unsigned long long running, base;
  unsigned pairs, skip;
};
// densify_run at dev_state->running (0 with `replace`), advancing it on the device, plus the pair's
// PointCloud2 payload (width * height slots of 16 bytes) into dev_pc2
int densify_append_run(Ctx* c, const DensifyParams& p, const float* dev_disparity,
                       const uint8_t* dev_image_left, double* dev_xyz, int32_t* dev_intensities,
                       size_t capacity, SeqState* dev_state, void* dev_pc2, bool replace,
                       const unsigned* dev_err_word = nullptr);  // (null: the context's own word)
// What one matcher call reads and writes (amhip_stereo.hip): `batch` pairs of images, pair b at
// base + b * batch stride.  Steps and strides in bytes; mask and raw may be null.
struct BatchStrides {
  size_t left, right, mask, disp, raw;
};
struct StereoImages {
  const uint8_t* left;
  size_t left_step;
  const uint8_t* right;
  size_t right_step;
  const uint8_t* mask;
  size_t mask_step;
  float* disp;
  size_t disp_step;
  int16_t* raw;
  size_t raw_step;
  int batch;
  BatchStrides bs;
};
// the parameter rules of the selected matcher for width x height images, with the texts of its
// one-pair export; no context, no device (amhip_stereo.hip)
int stereo_params_check(const amhip_stereo_settings& s, int width, int height);
// the context's stereo scratch holds `batch` pairs of the selected matcher
int stereo_scratch_reserve(Ctx* c, const amhip_stereo_settings& s, int width, int height, int batch);
// the selected matcher on images and parameters that passed the checks
int stereo_match(Ctx* c, const amhip_stereo_settings& s, int width, int height, const StereoImages& im);
// aslam MappedUndistorter::processImage for G frames (amhip_forward.hip: k_fwd_undistort), packed
// output (G x height x width x channels); asynchronous on `stream`
int undistort_frames_run(hipStream_t stream, const amhip_camera& cam, const uint8_t* dev_frames,
                         size_t frame_stride, size_t row_step, int channels, int G, uint8_t* dev_out);

// multi-GPU halo selection
int halo_select_run(Ctx* c, const double* dev_xyz, size_t n, const HaloParams& hp,
                    double* dev_out, unsigned long long* dev_counts);
// cells (of p's window, point_bin's arithmetic) the points of a cloud fall into: dev_bbox5 =
// [kBboxBias - min i, max i + kBboxBias, kBboxBias - min j, max j + kBboxBias, points inside the
// binned area] (amhip_sort.hip; all zero = the empty box)
constexpr int kBboxBias = 1 << 30;
int dsm_bbox_run(Ctx* c, const double* dev_xyz, size_t n, const DsmParams& p, int* dev_bbox5);
// geometry of a selection for `nd` destination windows (amhip_api.hip); off / cap_d are set to
// the equal-split layout (d * cap_per_dest, cap_per_dest)
int make_halo_params(const Ctx& c, double center_easting, double center_northing,
                     const int32_t* dest_windows, int nd, double margin_m, size_t cap_per_dest,
                     HaloParams* out);
// values: nullptr -> interpolate the points' z; else one int per point
// (OrthoFromPcl intensities).  out: the layer to write.  mask (may be null): one
// byte per cell, set where this call wrote a value; unfilled (may be null):
// device counter of cells left without a value.
// amhip_sort.hip: bin-sort the cloud into c->sorted / c->bin_start
bool no_launch_skips();            // amhip_sort.hip: tuning knob no_launch_skips
int dsm_sort(Ctx* c, const double* dev_xyz, const int32_t* dev_values, size_t n,
             const DsmParams& p, unsigned long long* zrange, const SortSplit* split = nullptr);
int dsm_run(Ctx* c, const double* dev_xyz, const int32_t* dev_values, size_t n,
            const DsmParams& p, float* out, unsigned char* mask, unsigned* unfilled,
            bool fill_untouched = false, float init_value = 0.0f,
            unsigned long long* zrange = nullptr, const SortSplit* split = nullptr);
// the launches of one mosaic call as plan_ortho_call (amhip_ortho_plan.h) decided them.  dev_fast:
// FrameFast[num_frames] followed by the camera and the atan table (build_frame_table); only read when p.fast
int ortho_run(Ctx* c, const OrthoPlan& plan, const FramePose* dev_poses, const FrameFast* dev_fast,
              const uint8_t* dev_frames);
// The occlusion-tested mosaic (amhip_ortho_occl.hip): what its kernel gets
// beside the mosaic's own parameter set.
struct OcclParams {
  double margin;                       // metres a sample must rise above the ray (>= 0, +inf legal)
  const double* centres;               // device: the camera centre of frame f in the map frame at [3 f]
  const unsigned long long* zmax_key;  // device: ordered key of (a bound of) the map's largest elevation
};
// plan: plan_ortho_call's with the exact fold, no pruning, no lazily initial output layer and the
// dense launch.  own_zmax_key: null, or q.zmax_key as a word to reduce the elevation layer into
// first (it holds key(-inf)).
int ortho_occl_run(Ctx* c, const OrthoPlan& plan, const OcclParams& q, const FramePose* dev_poses,
                   const uint8_t* dev_frames, unsigned long long* own_zmax_key);
// The blended mosaic (amhip_ortho_blend.hip): what its kernel gets beside
// the mosaic's own parameter set and, with the occlusion test on, the occlusion-tested mosaic's.
struct BlendParams {
  int sharpness;  // the weight is sin^2 of the view angle squared this many times (0 .. 4)
  double* wsum;   // device, per cell of the window (i + j * rows): the sum of the weights ...
  double* acc;    // ... and of weight * pixel: one plane of `plane` cells, or three (B, G, R)
  size_t plane;
};
// plan: as for ortho_occl_run.  q: null = no occlusion test (own_zmax_key is not looked at then).
int ortho_blend_run(Ctx* c, const OrthoPlan& plan, const OcclParams* q, const BlendParams& b,
                    const FramePose* dev_poses, const uint8_t* dev_frames,
                    unsigned long long* own_zmax_key);

// context internals shared with amhip_session.hip (defined in amhip_api.hip)
// i0, j0, rows, cols (window coordinates) of what the last DSM / mosaic call can have written;
// synchronises the stream when the box is still on the device.  rows == 0: nothing.
int ctx_last_dirty(Ctx* c, int rect[4]);
int ctx_use_device(Ctx* c);
int ctx_materialize(Ctx* c, int layer);      // lazy-initial -> filled
void ctx_overwrite(Ctx* c, int layer);       // about to be fully overwritten from outside
int ctx_layer_set_initial(Ctx* c, int layer);  // one layer back to its (lazy) initial state
int ctx_fetch_status(Ctx* c);                // synchronize + sticky device status
float ctx_layer_init_value(int layer);
bool ctx_layer_is_initial(const Ctx* c, int layer);
// host cloud -> stage_points (and stage_values, where the points carry intensities), asynchronously
int ctx_stage_cloud(Ctx* c, const double* host_xyz, const int32_t* host_values, size_t n);
// F host images of `height` rows of `row` bytes -> stage_frames, dense [F][height][row]: one linear
// copy per frame with dense rows (the usual cv::Mat), a pitched one otherwise
int ctx_stage_frames(Ctx* c, const uint8_t* const* images, const size_t* steps, size_t F, size_t row, size_t height);
int arg_failure(const char* msg);

}  // namespace amhip

struct amhip_ctx {
  amhip::Ctx impl;
};

#endif  // AMHIP_COMMON_H_
