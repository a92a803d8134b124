/*
 * aerial_mapper_hip.h -- C ABI of libaerial_mapper_hip.so
 *
 * MI355X (gfx950) implementation of aerial_mapper's one data-parallel hot
 * path: point cloud -> DSM rasterisation and the grid-based backward-projection
 * orthomosaic.  The reference (ethz-asl/aerial_mapper) has no FFI layer; its
 * boundary for this path is the C++ class API
 *
 *   dsm::Dsm::Dsm / Dsm::process
 *       aerial_mapper_dsm/include/aerial-mapper-dsm/dsm.h:25-42
 *       aerial_mapper_dsm/src/dsm.cc:20-34,186-201
 *   ortho::OrthoBackwardGrid::OrthoBackwardGrid / ::process
 *       aerial_mapper_ortho/include/aerial-mapper-ortho/ortho-backward-grid.h:32-50
 *       aerial_mapper_ortho/src/ortho-backward-grid.cc:23-40,223-239
 *   grid_map::AerialGridMap::initialize (layer set, geometry, init constants)
 *       aerial_mapper_grid_map/src/aerial-mapper-grid-map.cc:23-49
 *
 * which the drop-in C++ classes under include/aerial-mapper-dsm/ and
 * include/aerial-mapper-ortho/ implement on top of the entry points below
 * (see INTEGRATION.md).  Everything here is extern "C", POD only: plain
 * pointers, sizes and two small structs; no C++ / torch / HIP types.
 *
 * Conventions
 *   - A layer is one grid_map::Matrix (Eigen::MatrixXf): float32, column-major,
 *     rows*cols elements, element (i,j) at i + j*rows.  rows <-> index(0) <->
 *     x/easting, cols <-> index(1) <-> y/northing.
 *   - Points are AoS x,y,z doubles, 24 B apart: the memory layout of
 *     AlignedType<std::vector, Eigen::Vector3d>::type (dsm.h:41).
 *   - Poses are 7 doubles tx,ty,tz,qw,qx,qy,qz (Hamilton unit quaternion), the
 *     components of kindr::minimal::QuatTransformation.
 *   - Images are 8UC1 (gray) or 8UC3 (OpenCV BGR) rasters with a row step in
 *     bytes (cv::Mat::data / cv::Mat::step).
 *   - "host" pointers are ordinary process memory; "dev" pointers are HIP
 *     device allocations on the context's GPU (e.g. torch tensor data_ptr()).
 *   - Every function returns an amhip_status (0 = ok) unless noted.  The
 *     reference aborts through glog CHECK on precondition failures; the C++
 *     shim turns a non-zero status back into that behaviour.
 *   - One context serialises its own calls (the caller must not use one
 *     context from two threads at once); different contexts are independent.
 */
#ifndef AERIAL_MAPPER_HIP_H_
#define AERIAL_MAPPER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMHIP_ABI_VERSION 2

typedef enum amhip_status {
  AMHIP_OK = 0,
  AMHIP_ERR_ARG = 1,          /* null / shape / mode error (reference: CHECK) */
  AMHIP_ERR_EXACT_HIT = 2,    /* a point coincides with a cell centre:
                                 dsm.cc:165 CHECK(distances[i] > 0.0)        */
  AMHIP_ERR_ALPHA_NONPOS = 3, /* ortho-backward-grid.cc:178 CHECK(alpha > 0) */
  AMHIP_ERR_HIP = 4,          /* HIP runtime failure, see amhip_last_error() */
  AMHIP_ERR_NO_DEVICE = 5,    /* no usable gfx950 device                     */
  AMHIP_ERR_NOMEM = 6,
  AMHIP_ERR_HALO_OVERFLOW = 7 /* tiled DSM: a window had more halo points for a neighbour than
                                 the send rows reserved: the step's result is incomplete   */
} amhip_status;

/* Geometry of the grid_map::GridMap the layers belong to
 * (grid_map_core GridMap::setGeometry as called by
 * aerial-mapper-grid-map.cc:30-33; startIndex is always 0 there). */
typedef struct amhip_grid_desc {
  int32_t rows;      /* getSize()(0) */
  int32_t cols;      /* getSize()(1) */
  double resolution; /* getResolution() */
  double length_x;   /* getLength().x() = rows * resolution */
  double length_y;   /* getLength().y() = cols * resolution */
  double pos_x;      /* getPosition().x() (center_easting)  */
  double pos_y;      /* getPosition().y() (center_northing) */
} amhip_grid_desc;

enum {
  AMHIP_DIST_NONE = 0,
  AMHIP_DIST_RADTAN = 1,      /* k1,k2,p1,p2 */
  AMHIP_DIST_EQUIDISTANT = 2  /* k1,k2,k3,k4 */
};

/* aslam::PinholeCamera of ncameras->getCamera(0)
 * (ortho-backward-grid.cc:46,131): intrinsics, image size, distortion. */
typedef struct amhip_camera {
  double fu, fv, cu, cv;
  int32_t width;
  int32_t height;
  int32_t distortion; /* AMHIP_DIST_* */
  int32_t _pad;
  double dist[4];
} amhip_camera;

/* The layers of AerialGridMap the hot path reads or writes
 * (aerial-mapper-grid-map.cc:25-28). */
typedef enum amhip_layer {
  AMHIP_LAYER_ORTHO = 0,
  AMHIP_LAYER_ELEVATION = 1,
  AMHIP_LAYER_ELEVATION_ANGLE = 2,
  AMHIP_LAYER_NUM_OBSERVATIONS = 3,
  AMHIP_LAYER_OBSERVATION_INDEX = 4,
  AMHIP_LAYER_COLORED_ORTHO = 5,
  AMHIP_NUM_LAYERS = 6
} amhip_layer;

typedef struct amhip_ctx amhip_ctx; /* opaque: GPU, stream, layers, workspaces */

/* ---- library / context ---------------------------------------------------*/

int amhip_abi_version(void);

/* Message of the last failing call on this thread ("" if none). */
const char* amhip_last_error(void);

/* grid_map_core GridMap::setGeometry: size = (int)round(length/resolution),
 * length := size*resolution.  Pure host helper. */
void amhip_make_grid(double length_x, double length_y, double resolution,
                     double pos_x, double pos_y, amhip_grid_desc* out);

/* grid_map_core GridMap::getPosition(index): centre of cell (i,j). */
void amhip_cell_position(const amhip_grid_desc* grid, int i, int j, double* x,
                         double* y);

/* Replaces the per-cell bookkeeping of dsm.cc:24-33 and
 * ortho-backward-grid.cc:30-39 (the GPU needs only the geometry).  Allocates
 * the six layers on GPU `device` and sets them to AerialGridMap::initialize()'s
 * constants (ortho 255, elevation NaN, elevation_angle 0, num_observations 0,
 * observation_index NaN, colored_ortho NaN). */
int amhip_ctx_create(const amhip_grid_desc* grid, int device, amhip_ctx** out);
void amhip_ctx_destroy(amhip_ctx* ctx);

/* The same for the window [i0, i0+rows) x [j0, j0+cols) of a larger map
 * `grid` (one tile of a survey spread over several GPUs): cell positions, and
 * therefore every result, are exactly those of the full map; the context's
 * layers hold only the window (rows*cols floats, column-major).  The caller
 * hands the DSM every point within sqrt(7) m of the window (the last fallback
 * radius, dsm.cc:133-144) -- see aerial_mapper_amd/tiling.py. */
int amhip_ctx_create_window(const amhip_grid_desc* grid, int i0, int j0, int rows,
                            int cols, int device, amhip_ctx** out);

/* Run the context's kernels on an existing HIP stream (hipStream_t passed as
 * void*; NULL = back to the context's own stream). */
int amhip_ctx_set_stream(amhip_ctx* ctx, void* hip_stream);

/* Arithmetic of the DSM gather (dsm::Dsm::process, dsm.cc:160-172).
 *   AMHIP_DSM_EXACT (DEFAULT since round 3) the FP64 gather everywhere: the reference's doubles
 *                   decide and weigh every pair, only the ORDER of the double sums differs from
 *                   the kd-tree's (1e-16 relative, then rounded to float): bit-identical floats
 *                   in every test so far (one cell in 1e8 follows the kd-tree's own summation
 *                   order), THE SAME BITS IN EVERY RUN AND FOR EVERY ORDER OF THE CLOUD (since
 *                   round 4: the rounding of every quotient is guarded, the cells on a float
 *                   rounding boundary are redone in order-independent double-double sums), and
 *                   therefore a byte-identical mosaic on top.  What a drop-in must be by default.
 *   AMHIP_DSM_FAST  (opt-in) single-precision distances and weights under exact guards: the
 *                   reference's neighbour sets (any decision within 2e-6 of the radius is taken
 *                   in its own doubles), identical NaN pattern, heights within the contract's
 *                   1e-4 m (1 float spacing above 1024 m) by a per-tile error bound; tiles /
 *                   cells without room under the bound take the FP64 path.  ~0.6 ms faster per
 *                   100 M cells; heights may differ from the reference's by one float spacing
 *                   and from run to run (the f32 sums follow the order the atomics of the
 *                   binning left the points in), so a mosaic on top of them can differ in the
 *                   rare cell whose keypoint sits on a pixel boundary.  A context whose
 *                   scene is mostly rough (more than half of the tiles without room under the
 *                   bound) runs the FP64 pipeline by itself for 16 calls at a time.
 * New contexts start in EXACT; the environment variable AMHIP_DSM_FAST=1 makes FAST their
 * default (hosts that cannot be recompiled), AMHIP_DSM_EXACT=1 (round 2's switch) still forces
 * EXACT.  The setters override either.  amhip_session_set_dsm_precision applies to every window
 * of a session (the drop-in dsm::Dsm::setPrecision calls it). */
#define AMHIP_DSM_FAST 0
#define AMHIP_DSM_EXACT 1
int amhip_ctx_set_dsm_precision(amhip_ctx* ctx, int mode);

/* OPTIONAL capped interpolation ("IDW k = 4" of BASELINE.json's wording): only the k nearest
 * points of a cell's radius search (nanoflann::KNNResultSet's order, nanoflann.hpp:80-131)
 * take part in the weighting.  k = 0 (default) = the reference's behaviour: every point of
 * the search.  NOT a reference code path -- dsm.cc:127-172 has no k -- so its parity is
 * unpinned by the reference (oracle: KNNResultSet on the reference's vendored tree); it is a
 * separately reported extra, never the graded mode.  1 <= k <= 8; always the FP64 pipeline,
 * whatever amhip_ctx_set_dsm_precision says (true divisions in ascending-distance order:
 * bit-identical to the oracle but for exact distance ties). */
int amhip_ctx_set_dsm_knn(amhip_ctx* ctx, int k);

/* Wait for everything enqueued on the context and return the sticky status
 * of the device-side CHECKs (EXACT_HIT / ALPHA_NONPOS) or HIP errors since
 * the last synchronize; the status is then cleared. */
int amhip_ctx_synchronize(amhip_ctx* ctx);

/* ---- layers (device resident; persist across process() calls like the
 *      GridMap's matrices do in incremental mode,
 *      main-ortho-backward-grid-incremental.cc:153-162) --------------------*/

/* AerialGridMap::initialize() values (aerial-mapper-grid-map.cc:40-48).  The
 * reset is lazy: it writes nothing; the next call that produces a layer
 * (DSM -> elevation, OrthoFromPcl -> ortho, OrthoBackwardGrid ->
 * elevation_angle / observation_index / ortho|colored_ortho) also writes the
 * initial value into the cells it leaves alone, and anything else that needs
 * the memory (download, device pointer, a batch on top of uploaded layers)
 * fills the layer first.  Observable contents are always those of an eager
 * fill; the tuning knob eager_reset (amhip_set_tuning) restores the plain fills. */
int amhip_layers_reset(amhip_ctx* ctx);
int amhip_layer_upload(amhip_ctx* ctx, int layer, const float* host);
int amhip_layer_download(amhip_ctx* ctx, int layer, float* host);
/* Device address of a layer (rows*cols floats) or NULL.  The layer is
 * filled if its reset was still pending and is refilled eagerly from then on
 * (the library cannot see writes through the pointer). */
void* amhip_layer_device_ptr(amhip_ctx* ctx, int layer);

/* ---- DSM: dsm::Dsm::process (dsm.cc:186-201) ----------------------------*/

/* Asynchronous, device-resident form.  dev_xyz: n points on the context's
 * GPU.  Updates the context's ELEVATION layer exactly where the reference
 * would (cells with no point inside the last fallback radius stay untouched).
 * n == 0 is the reference's soft no-op.  radius_sq is
 * dsm::Settings::interpolation_radius (an int holding the SQUARED search
 * radius in m^2); center_* are dsm::Settings::center_easting/northing
 * (note dsm.cc:42-43 subtracts center_northing from x and center_easting
 * from y -- reproduced).
 * dev_xyz is read until the LAST kernel of the call (in AMHIP_DSM_FAST mode the sort carries
 * 20-byte records and the exact routines fetch a point's doubles from dev_xyz itself): work
 * that overwrites or frees it has to be ordered after the call on the context's stream. */
int amhip_dsm_process_dev(amhip_ctx* ctx, const double* dev_xyz, size_t n,
                          int radius_sq, double center_easting,
                          double center_northing);

/* Synchronous drop-in form on host buffers: uploads `elevation` (the map's
 * current layer), copies the cloud to the GPU, runs the DSM, downloads the
 * layer back into `elevation`, returns the final status. */
int amhip_dsm_process(amhip_ctx* ctx, const double* host_xyz, size_t n,
                      int radius_sq, double center_easting,
                      double center_northing, float* elevation);

/* ---- OrthoFromPcl: ortho::OrthoFromPcl::process
 *      (aerial_mapper_ortho/src/ortho-from-pcl.cc:20-113) --
 * The DSM's radius search + inverse-squared-distance weighting applied to the
 * points' INTENSITIES (one int per point), written to the ORTHO layer.
 * Differences to the DSM that are reproduced: no centre offsets (:30-31); an
 * exact hit takes that point's value instead of failing (:91-96); no fallback
 * unless `adaptive` (ortho::Settings::use_adaptive_interpolation), which then
 * retries with the squared radius x10, x100, ... (int lambda, :63-71) until
 * every cell has a value (one extra pass over the cloud per retry; stops where
 * the reference's int product would overflow).  radius_sq is
 * ortho::Settings::interpolation_radius (squared, like the DSM's).  The _dev
 * form is asynchronous unless `adaptive` is set. */
int amhip_ortho_from_pcl_process_dev(amhip_ctx* ctx, const double* dev_xyz,
                                     const int32_t* dev_intensities, size_t n,
                                     int radius_sq, int adaptive);
int amhip_ortho_from_pcl_process(amhip_ctx* ctx, const double* host_xyz,
                                 const int32_t* host_intensities, size_t n,
                                 int radius_sq, int adaptive, float* ortho);

/* ---- stereo::Densifier::computePointCloud, reprojection part
 *      (aerial_mapper_dense_pcl/src/densifier.cpp:25-108) --
 * Disparity map (float32 rows, disp_step bytes apart) + left rectified image
 * (8UC1, img_step) -> world points in RASTER order (pixels with disparity <= 1
 * or infinite z dropped) + their gray values, written to device buffers in
 * the layout amhip_dsm_process_dev / amhip_ortho_from_pcl_process_dev take, so
 * the cloud of the incremental pipeline never leaves HBM.  K and R_G_C are
 * row-major 3x3 (StereoRigParameters::K, RectifiedStereoPair::R_G_C), t_G_C1
 * is StereoRigParameters::t_G_C1, baseline RectifiedStereoPair::baseline.
 * dev_count receives the number of valid points (it may exceed `capacity`, the
 * excess is not written).  Asynchronous.  The block matcher in front of it is
 * amhip_sgbm_disparity_dev (use_BM = false) or amhip_bm_disparity_dev
 * (use_BM = true).  The sensor_msgs::PointCloud2 payload of densifier.cpp:53-106 is filled by the
 * sequence object below (amhip_stereo_point_cloud2_dev), not by this call. */
int amhip_densify_dev(amhip_ctx* ctx, const float* dev_disparity, size_t disp_step,
                      const uint8_t* dev_image_left, size_t img_step, int width,
                      int height, const double* K, double baseline,
                      const double* R_G_C, const double* t_G_C1,
                      double* dev_xyz_out, int32_t* dev_intensity_out,
                      size_t capacity, int64_t* dev_count);

/* ---- multi-GPU: halo points of a tiled survey ------------------------------
 * No reference counterpart (the reference is single-process).  When one map
 * is tiled over several GPUs with amhip_ctx_create_window(), a rank's DSM
 * needs every point within the last fallback radius of its window.  Given the
 * points a rank holds, this collects (compacts) the ones that lie inside each
 * of `nd` OTHER windows expanded by `margin_m` metres, so that the host can
 * ship them with one RCCL all_to_all (aerial_mapper_amd/tiling.py).
 *   dest_windows  host, nd x 4 int32: i0, j0, rows, cols (nd <= 8)
 *   dev_out       device, nd * cap_per_dest * 3 doubles; points of destination
 *                 d start at dev_out + d*cap_per_dest*3 (original x,y,z)
 *   dev_counts    device, nd int64: number of points selected per destination
 *                 (may exceed cap_per_dest: the excess was not written)
 * Asynchronous on the context's stream. */
int amhip_halo_select_dev(amhip_ctx* ctx, const double* dev_xyz, size_t n,
                          double center_easting, double center_northing,
                          const int32_t* dest_windows, int nd, double margin_m,
                          double* dev_out, size_t cap_per_dest,
                          int64_t* dev_counts);

/* The same selection folded into dsm::Dsm::process (dsm.cc:186-201) of a window, around the
 * caller's exchange -- the DSM's binning pass reads every point anyway:
 *   1. amhip_dsm_tiled_begin_dev: bins the rank's own points dev_xyz[0, n_owned) and, in the
 *      same pass, copies the ones the `nd` windows in dest_windows need into dev_out /
 *      dev_counts exactly like amhip_halo_select_dev (a placeholder window far outside the
 *      map for the rank itself keeps the rows indexed by rank).
 *   2. the caller exchanges the rows (one all_to_all of equal splits, no count exchange, no
 *      host synchronisation) into dev_xyz[n_owned, n_total); rows it does not fill must be
 *      NaN -- the binning drops them like any point outside the map.
 *   3. amhip_dsm_tiled_finish_dev: bins dev_xyz[n_owned, n_total) and runs the rest of
 *      Dsm::process on all n_total rows; the ELEVATION layer is as after
 *      amhip_dsm_process_dev(dev_xyz, n_total).
 * Both asynchronous on the context's stream; dev_xyz must stay valid and rows [0, n_owned)
 * unchanged in between (and all n_total rows until the finish call's last kernel: see
 * amhip_dsm_process_dev).  Any other DSM / OrthoFromPcl call on the context in between cancels
 * the pending call: amhip_dsm_tiled_finish_dev then returns AMHIP_ERR_ARG. */
int amhip_dsm_tiled_begin_dev(amhip_ctx* ctx, const double* dev_xyz, size_t n_owned,
                              size_t n_total, int radius_sq, double center_easting,
                              double center_northing, const int32_t* dest_windows, int nd,
                              double margin_m, double* dev_out, size_t cap_per_dest,
                              int64_t* dev_counts);
int amhip_dsm_tiled_finish_dev(amhip_ctx* ctx);

/* ---- Ortho: ortho::OrthoBackwardGrid::process
 *      (ortho-backward-grid.cc:223-239) ------------------------------------*/

/* T_G_C[i] = T_G_B[i] * T_C_B^-1 (ortho-backward-grid.cc:230-233) with
 * minkindr's composition / inverse.  Pure host helper (F poses of 7). */
void amhip_compose_T_G_C(const double* T_G_B, const double* T_C_B, size_t F,
                         double* T_G_C);

/* Asynchronous, device-resident form.  host_T_G_C: F x 7 doubles on the host
 * (small; copied).  dev_frames: F rasters on the GPU, frame f starts at
 * dev_frames + f*frame_stride, rows are row_step bytes apart, `channels` is 1
 * (8UC1) or 3 (8UC3 BGR).  colored = ortho::Settings::colored_ortho (needs
 * channels == 3; gray needs channels == 1).  Reads the ELEVATION layer, folds
 * the F frames in ascending order into ELEVATION_ANGLE / OBSERVATION_INDEX /
 * NUM_OBSERVATIONS and ORTHO or COLORED_ORTHO of the context. */
int amhip_ortho_backward_process_dev(amhip_ctx* ctx, const amhip_camera* cam,
                                     const double* host_T_G_C, size_t F,
                                     const uint8_t* dev_frames,
                                     size_t frame_stride, size_t row_step,
                                     int channels, int colored);

/* Synchronous drop-in form on host buffers: uploads the six layers given
 * (any may be NULL = keep the context's copy), stages the images on the GPU,
 * runs the mosaic, downloads the five output layers that are non-NULL. */
int amhip_ortho_backward_process(
    amhip_ctx* ctx, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho);

/* The same two with an occlusion test ("true ortho"; an extension: the reference has none).  The
 * reference's visibility rule (ortho-backward-grid.cc:164-171) gets one more term,
 *   visible = in_box && z > 1e-10 && !occluded(cell, frame),
 * and nothing else of the fold changes.  occluded(i, j, f) marches the ELEVATION layer from the
 * cell towards the camera, one cell per step along the ray's major axis (FP64, every operation
 * rounded on its own, in this order): h = elevation(i, j), NaN: not occluded; (x_c, y_c) =
 * amhip_cell_position(i, j), (tx, ty, tz) = the translation of T_G_C[f];
 *   di = (x_c - tx) / res, dj = (y_c - ty) / res, m = max(|di|, |dj|), dz = tz - h;
 *   !(dz > 0): not occluded; for k = 1, 2, ... while k < m: s = k / m,
 *   ii = i + (int)rint(s * di), jj = j + (int)rint(s * dj) (round half to even); outside the map:
 *   not occluded; z = h + s * dz; elevation(ii, jj) > z + margin_m: occluded (strict; a NaN
 *   sample does not occlude).
 * A cell every view of which is occluded keeps what the layers held.  margin_m >= 0 in metres
 * (+inf: nothing occludes, the layers are the plain mosaic's); negative or NaN: AMHIP_ERR_ARG.
 * The ray leaves a window of the map: a context of amhip_ctx_create_window is refused
 * (AMHIP_ERR_ARG) until windows carry an elevation halo. */
int amhip_ortho_backward_process_occl_dev(amhip_ctx* ctx, const amhip_camera* cam,
                                          const double* host_T_G_C, size_t F,
                                          const uint8_t* dev_frames,
                                          size_t frame_stride, size_t row_step,
                                          int channels, int colored, double margin_m);
int amhip_ortho_backward_process_occl(
    amhip_ctx* ctx, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho, double margin_m);

/* The same two, blended (an extension: the reference has none).  The
 * reference paints a cell with the nearest pixel of its single most-nadir view; here EVERY view
 * that is visible from the cell (in_box && z > 1e-10 with a finite elevation; with occlusion_test
 * also !occluded(cell, frame), the march above with occlusion_margin_m) contributes its nearest
 * pixel, weighted by a power of the sine of its view angle, and the cell gets the weighted mean.
 * Whether a view wins or loses the angle fold does not matter for contributing.  One pair, FP64,
 * every operation rounded on its own, in this order -- (cx, cy, cz) the landmark in the camera
 * frame, I the pixel at the plain mosaic's keypoint (min((int)round(v), height - 1), x likewise):
 *   zz = cz * cz; n2 = (cx * cx + cy * cy) + zz; w = zz / n2; `sharpness` times: w = w * w;
 *   acc = acc + w * (double)I (gray; colour: B, G and R each with a sum of its own);
 *   wsum = wsum + w;
 * frames ascending over all F frames of the call.  sharpness in [0, 4] (sin^2 .. sin^32 of the view
 * angle; 2 is a good default).  At the end of the call a cell with at least one contributing pair
 * in this call and wsum > 0 gets rint(acc / wsum) (round half to even; colour: per channel, packed
 * R << 16 | G << 8 | B like the plain mosaic's); any other cell keeps what the layer held.
 * elevation_angle, observation_index and num_observations are written exactly as by the plain
 * (occlusion_test = 0) or the occlusion-tested mosaic on the same inputs.
 *   The sums are per-cell FP64 device buffers of the context, allocated (zero) by the first blended
 * call, gray and colour each their own: 16 bytes per cell for gray, 32 for colour.  A cell whose
 * observation_index is NaN at the start of a call restarts from zero -- a reset map needs no
 * other hook --, any other continues from what the buffers hold: frames 0..k in one call and
 * k+1..F in the next give the bits of one call with all of them.  Blended and unblended calls may
 * be mixed on one map: each call follows its own rule, and the sums know only the blended calls.
 *   AMHIP_ERR_ARG before any device work: null opts, sharpness outside [0, 4], and with
 * occlusion_test the refusals of amhip_ortho_backward_process_occl (margin, window contexts).
 * Without the occlusion test a window context is served: no ray leaves it. */
typedef struct amhip_ortho_blend_opts {
  int32_t sharpness;
  int32_t occlusion_test;      /* 0: the reference's visibility rule */
  double occlusion_margin_m;   /* only read with occlusion_test */
} amhip_ortho_blend_opts;
int amhip_ortho_backward_process_blend_dev(amhip_ctx* ctx, const amhip_camera* cam,
                                           const double* host_T_G_C, size_t F,
                                           const uint8_t* dev_frames,
                                           size_t frame_stride, size_t row_step,
                                           int channels, int colored,
                                           const amhip_ortho_blend_opts* opts);
int amhip_ortho_backward_process_blend(
    amhip_ctx* ctx, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels,
    int colored, const float* elevation, float* elevation_angle,
    float* observation_index, float* num_observations, float* ortho,
    float* colored_ortho, const amhip_ortho_blend_opts* opts);

/* ---- ortho::OrthoForwardHomography
 *      (aerial_mapper_ortho/src/ortho-forward-homography.cc; SURVEY section 8b/8f,
 *      named in the API surface to keep) --
 * A mosaic is the object's state: Settings::{width,height}_mosaic_pixels,
 * ground_plane_elevation_m, origin (ortho-forward-homography.h:33-42), the
 * camera, the FeatherBlender accumulators and result_ / result_mask_.
 * result_ is CV_16SC3 (height x width x 3 int16, row-major; a gray frame is
 * replicated into the three channels, :45-47), result_mask_ CV_8U (255 where
 * the summed feather weight exceeds 1e-5).  Poses are T_G_C (amhip_compose_T_G_C).
 *   amhip_mosaic_batch    = OrthoForwardHomography::batch (:137-189): every
 *       frame is warped (4 corner rays on the ground plane -> homography ->
 *       nearest-neighbour warp) and fed to the blender, then blended and the
 *       "unobserved pixels" set to 0.  batch() offsets both ground axes by
 *       width/2 (:155-158) -- reproduced.
 *   amhip_mosaic_update   = ::updateOrthomosaic (:74-135): feed the frame, blend,
 *       start a new blender holding the previous result.
 * The _dev forms take device-resident frames (frame f at dev_frames + f *
 * frame_stride, rows row_step bytes apart), run asynchronously on the mosaic's
 * stream and leave the result on the device (amhip_mosaic_device_ptr /
 * amhip_mosaic_download).  imshow / imwrite / ROS publishing stay with the
 * caller.  OpenCV / aslam semantics are restated, see oracle/amo_forward.cc
 * for the list ("parity unpinned": the reference has no tests for this path). */
typedef struct amhip_mosaic amhip_mosaic;

typedef struct amhip_mosaic_desc {
  int32_t width_mosaic_pixels;
  int32_t height_mosaic_pixels;
  double ground_plane_elevation_m;
  double origin[3];
} amhip_mosaic_desc;

int amhip_mosaic_create(const amhip_mosaic_desc* desc, const amhip_camera* cam, int device,
                        amhip_mosaic** out);
int amhip_mosaic_destroy(amhip_mosaic* mosaic);
int amhip_mosaic_set_stream(amhip_mosaic* mosaic, void* hip_stream);
int amhip_mosaic_synchronize(amhip_mosaic* mosaic);
/* fresh blender + zero result (a newly constructed object) */
int amhip_mosaic_reset(amhip_mosaic* mosaic);
int amhip_mosaic_batch(amhip_mosaic* mosaic, const double* T_G_C, size_t num_frames,
                       const void* const* images, const size_t* steps, int channels,
                       int16_t* result_16sc3, uint8_t* result_mask);
int amhip_mosaic_batch_dev(amhip_mosaic* mosaic, const double* T_G_C, size_t num_frames,
                           const void* dev_frames, size_t frame_stride, size_t row_step,
                           int channels);
int amhip_mosaic_update(amhip_mosaic* mosaic, const double* T_G_C7, const void* image,
                        size_t step, int channels, int16_t* result_16sc3,
                        uint8_t* result_mask);
int amhip_mosaic_update_dev(amhip_mosaic* mosaic, const double* T_G_C7, const void* dev_frame,
                            size_t row_step, int channels);
int amhip_mosaic_download(amhip_mosaic* mosaic, int16_t* result_16sc3, uint8_t* result_mask);
int amhip_mosaic_device_ptr(amhip_mosaic* mosaic, void** result_16sc3, void** result_mask);
/* cv::imwrite(settings_.filename_mosaic_output, result_) (:126-128, :188): the device-resident
 * result_ (CV_16SC3, clamped to 0..255 in the kernel) as a baseline JPEG file, see amhip_jpeg_*
 * below.  _encode_jpeg_dev leaves the file in device memory (at most cap bytes; *bytes = its size;
 * a file that does not fit: AMHIP_ERR_ARG, nothing written), _write_jpeg downloads and writes it.
 * quality 1..100, 0 = 95 (OpenCV's default). */
int amhip_mosaic_encode_jpeg_dev(amhip_mosaic* mosaic, int quality, uint8_t* dev_out, size_t cap,
                                 size_t* bytes);
int amhip_mosaic_write_jpeg(amhip_mosaic* mosaic, int quality, const char* filename);
/* The image -> mosaic homography of one frame (row-major 3x3, M[8] = 1); host
 * arithmetic only.  batch_quirk != 0: batch()'s offsets. */
int amhip_mosaic_homography(const amhip_mosaic_desc* desc, const amhip_camera* cam,
                            const double* T_G_C7, int batch_quirk, double* M9);

/* The conservative view bounds the backward-grid mosaic derives from a camera
 * (host arithmetic only; diagnostics / tests), in normalised camera coordinates
 * (x / z, y / z):
 *   out[0] cone   every visible landmark has |p| <= cone            (0: no bound)
 *   out[1], out[2]  ax, ay: every visible landmark has |x| <= ax, |y| <= ay
 *   out[3] rin    |p| <= rin  =>  the landmark is visible             (0: unknown)
 * "visible" = aslam project3's image-box test (ortho-backward-grid.cc:164-171);
 * for an undistorted camera cone = rin = 0 and ax, ay describe the image box. */
int amhip_camera_view_bounds(const amhip_camera* cam, double* out4);

/* ---- io::AerialMapperIO::loadPointCloudFromFile
 *      (aerial_mapper_io/src/aerial-mapper-io.cc:309-347) --
 * The text point-cloud format in front of the DSM: whitespace separated
 * records `x y z intensity`, read like `infile >> x >> y >> z >> intensity`
 * (tokens four at a time; reading stops at the first token that is not a
 * number; an incomplete last record is dropped), points with z <= -100 dropped.
 * host_text is the file's content (e.g. mmap'ed).  The text is tokenised and
 * parsed on the GPU -- decimal -> double correctly rounded (Eisel-Lemire; the
 * rare inputs it cannot decide are re-done with strtod on the host and counted
 * in *num_strtod_tokens) -- and the result stays on the device in the layout
 * amhip_dsm_process_dev / amhip_ortho_from_pcl_process_dev take: dev_xyz = 3 *
 * num_points doubles (AoS), dev_intensities = num_points int32, file order.
 * Both buffers are allocated here; release them with amhip_io_free().
 * Synchronous.  Pose files (`x y z qw qx qy qz`, :103-121) are a few KB and are
 * read on the host by the C++ shim. */
int amhip_io_parse_point_cloud_text(int device, const char* host_text, size_t len,
                                    double** dev_xyz, int32_t** dev_intensities,
                                    size_t* num_points, size_t* num_strtod_tokens);
int amhip_io_download_point_cloud(const double* dev_xyz, const int32_t* dev_intensities,
                                  size_t n, double* host_xyz, int32_t* host_intensities);
int amhip_io_free(void* dev_ptr);

/* ---- io::AerialMapperIO::loadImagesFromFile (aerial-mapper-io.cc:207-227): the frames' JPEG files,
 *      decoded on the GPU ------------------------------------------------------------------------
 * What cv::imread gives through libjpeg at its defaults (JDCT_ISLOW, fancy upsampling), bit for bit
 * libjpeg-turbo's pixels (tests/golden/jpeg_decode/); parity with OpenCV itself is adopted, unpinned,
 * and EXIF orientation is not applied.  Accepted: baseline sequential DCT (SOF0), 8 bit, Huffman, one
 * scan; one component, or Y Cb Cr with Y sampled 1x1, 2x1 or 2x2 and chroma 1x1; 8-bit quantisation
 * tables; Huffman table ids 0 and 1 of any content; optional DRI; APPn / COM skipped; width and
 * height 1..65535.  Also accepted: progressive DCT (SOF2), 8 bit, Huffman, the same components: any
 * complete scan script (spectral selection, successive approximation, DC scans interleaved or not,
 * DHT / DQT / DRI / COM / APPn between scans, table ids 0..3), bit for bit libjpeg-turbo's pixels
 * (tests/golden/jpeg_progressive/).  A call may mix baseline and progressive files.  Refused under
 * SOF2, each with a text that names the scan and the field: what libjpeg refuses or warns about in a
 * script (Ss = 0 with Se != 0, Ss > 0 with more than one component, Se < Ss or > 63, Al > 13, Ah with
 * Al != Ah - 1, a refinement that does not continue where the coefficient stands, a coefficient sent
 * first twice, an AC scan before the component's DC scan, an undefined component or table), any
 * other marker between scans, and a file that ends before every coefficient has reached bit 0
 * (libjpeg would smooth its blocks: not reproduced).  Everything else (arithmetic, 12 bit, 4
 * components, other sampling
 * factors, 16-bit DQT, several scans under SOF0, Adobe transform 0 or component ids R G B, missing tables, no
 * SOI / SOS / EOI) is AMHIP_ERR_ARG with a text naming the marker or field, reported before any
 * device is touched.  A scan that does not decode (undefined code, run past coefficient 63 or past a
 * progressive scan's band, wrong or missing RSTn, early end, a refinement coefficient of a size other
 * than 1) is found on the device: AMHIP_ERR_ARG naming the frame, *dev_frames = NULL.
 * The scan ends at the first EOI behind it; whatever follows that EOI (thumbnails, padding, a second image) is
 * ignored, as libjpeg ignores it.  As in libjpeg, any number of 0xFF fill bytes may stand in front of a marker
 * (a run of 0xFF followed by 0x00 is one data byte 0xFF), and bytes between the end of a restart interval's data
 * and its RSTn, or between the last block and EOI, are skipped.  Stricter than libjpeg, which only warns: a wrong
 * RSTn index and a scan that ends early are errors here.  Scratch is bounded by decoding in groups of frames
 * (tuning key jpegd_coef_budget_mb). */
/* host only: parses up to SOS (SOF2: every scan up to EOI), applies every rule above; channels = components in
 * the file (1 or 3) */
int amhip_jpeg_info(const uint8_t* file, size_t len, int* width, int* height, int* channels);
/* F files in host memory -> ONE stack of frames in HBM, frame f at *dev_frames + f * *frame_stride, rows *row_step
 * bytes apart: the layout amhip_ortho_backward_process_dev, amhip_mosaic_batch_dev and amhip_stereo_add_frames_dev
 * take.  colored == 0: 8UC1 (a gray file as it is, of a colour file its Y plane); colored != 0: 8UC3 B, G, R (a gray
 * file replicated).  All files must have the width and height of file 0 (else AMHIP_ERR_ARG naming the frame).
 * Released with amhip_io_free().  Like the other amhip_io_* calls it takes a device, not a context: the mains load
 * frames before a map exists.  Scratch lives for the call. */
int amhip_io_decode_jpeg_frames(int device, const uint8_t* const* files, const size_t* lens, size_t F, int colored,
                                uint8_t** dev_frames, int* width, int* height, size_t* row_step, size_t* frame_stride);
/* num_bytes of such a stack (or of a part of it) into host memory: what the drop-in loadImagesFromFile fills its
 * cv::Mats from.  Synchronous. */
int amhip_io_download_frames(const uint8_t* dev_frames, size_t num_bytes, uint8_t* host_frames);

/* ---- io::AerialMapperIO::loadImagesFromFile(directory, image_names, ..) (aerial-mapper-io.cc:229-249):
 *      the frames' PNG files, decoded on the GPU ------------------------------------------------------
 * What cv::imread gives through libpng: inflate as zlib defines it and the pixels Pillow gives, bit for
 * bit (tests/golden/png_decode/).  Accepted: bit depth 8; colour types 0 (gray), 2 (RGB), 3 (palette),
 * 4 (gray + alpha), 6 (RGBA); not interlaced; width and height 1..65535; any number of consecutive IDAT
 * chunks (they are joined into one zlib stream on the host); ancillary chunks skipped unread, tRNS and
 * gAMA included; bytes behind IEND ignored.  Refused with AMHIP_ERR_ARG and a text naming the field or
 * chunk, before any device is touched: bit depths 1, 2, 4, 16; Adam7; a bad CRC on IHDR, PLTE, IDAT or
 * IEND; a missing PLTE, IDAT or IEND; an IDAT behind another chunk that interrupted the run; a truncated
 * chunk; a length that runs past the file; a zlib header other than CM 8, CINFO <= 7, FDICT 0 with a
 * valid FCHECK.  Found on the device (AMHIP_ERR_ARG naming the frame and the reason, *dev_frames = NULL):
 * an undefined Huffman code, an over-subscribed or incomplete set of code lengths (but for the distance
 * code of one symbol RFC 1951 allows), a dynamic header out of range, block type 3, LEN != ~NLEN, a
 * distance behind the first output byte, a stream that ends early, output shorter or longer than the
 * scanlines, a filter type above 4, an Adler-32 mismatch, a palette index outside PLTE.  Stricter than
 * libpng, which only warns: surplus inflated data is an error.  Laxer than a strict zlib: a distance up
 * to 32768 is taken whatever CINFO declares.  Alpha is dropped.  colored == 0 on a colour file: libpng's
 * png_set_rgb_to_gray(.., 0.299, 0.587) as cv::imread sets it up, (9797 R + 19234 G + 3737 B) >> 15,
 * gAMA ignored -- this one rule is adopted, unpinned.  Scratch (the streams, the raw scanlines) lives for
 * the call and is bounded by decoding in groups of frames (tuning key pngd_raw_budget_mb). */
/* host only: applies every host rule above; channels = 1 for colour types 0 and 4, else 3 */
int amhip_png_info(const uint8_t* file, size_t len, int* width, int* height, int* channels); /* host only; 1 or 3 */
/* The contract of amhip_io_decode_jpeg_frames: F files in host memory -> ONE stack in HBM, tight rows
 * (*row_step = width * channels, *frame_stride = height * *row_step).  colored == 0: 8UC1; colored != 0:
 * 8UC3 B, G, R (gray replicated, palette through PLTE).  All files must have the width and height of file
 * 0 (else AMHIP_ERR_ARG naming the frame); colour types may differ.  Released with amhip_io_free();
 * amhip_io_download_frames works on the result. */
int amhip_io_decode_png_frames(int device, const uint8_t* const* files, const size_t* lens, size_t F, int colored,
                               uint8_t** dev_frames, int* width, int* height, size_t* row_step, size_t* frame_stride);

/* ---- what leaves the map: images, GeoTiff, grid_map_msgs, binary clouds
 *      (the formats either side of the path) ------------------
 * grid_map_cv, grid_map_ros, GDAL and roscpp are not part of the reference tree; the adopted
 * definitions are restated in oracle/amo_export.py (parity unpinned). */

/* A layer as an 8-bit image in grid_map_cv::GridMapCvConverter::toImage's orientation (image row
 * = grid index 0, image column = grid index 1; aerial-mapper-grid-map.cc:10 includes it).
 * bgr == 0: toImage<unsigned char, 1>(map, layer, CV_8UC1, lower, upper, image): the layer clamped
 * to [lower, upper], finite cells -> (uchar)(((v - lower) / (upper - lower)) * 255.0f), others 0.
 * bgr != 0: the layer holds grid_map's packed colours (colored_ortho: the float's bits are
 * R << 16 | G << 8 | B, ortho-backward-grid.cc:203-207): an 8UC3 image in OpenCV's B, G, R order,
 * NaN -> 0, 0, 0 (lower / upper unused).  step = bytes per image row.  A transposition through
 * LDS on the device; the _dev form leaves the image in HBM. */
int amhip_layer_to_image_dev(amhip_ctx* ctx, int layer, int bgr, float lower, float upper,
                             uint8_t* dev_image, size_t step);
int amhip_layer_to_image(amhip_ctx* ctx, int layer, int bgr, float lower, float upper,
                         uint8_t* host_image, size_t step);

/* ---- JPEG, encoded on the GPU ------------------------------------------------------------------
 * The file libjpeg writes for cv::imwrite(name, image) at quality q (save_orthomosaic_jpg /
 * orthomosaic_jpg_filename of the ortho::Settings, filename_mosaic_output of the forward mosaic):
 * baseline sequential DCT, 8 bit, the standard Huffman tables, one scan, no restart markers; JFIF
 * 1.01 header; 8UC1 as one component, 8UC3 (B, G, R) as Y Cb Cr 4:2:0.  Byte for byte what
 * libjpeg-turbo writes through Pillow's save(quality=q, subsampling=2, optimize=False)
 * (tests/golden/jpeg/).  width, height 1..65535; channels 1 or 3; quality 1..100, 0 = 95.
 * Argument errors are reported before the context is looked at.
 *   amhip_jpeg_bound       worst-case size of the file (0 for arguments out of range)
 *   amhip_jpeg_encode_dev  device pixels (rows `step` bytes apart) -> the file in dev_out, at most
 *                          cap bytes; *bytes = the file's size.  A file larger than cap gives
 *                          AMHIP_ERR_ARG and nothing is written.  Runs on the context's stream,
 *                          asynchronously up to the one read-back of *bytes.
 *   amhip_jpeg_write       encode (host or device pixels), download, write `filename`
 *   amhip_layer_write_jpeg amhip_layer_to_image_dev into scratch, then the encoder
 * A file that cannot be opened or written is AMHIP_ERR_ARG with errno's text (amhip_status has no
 * I/O code; the GeoTiff and point-cloud writers do the same). */
size_t amhip_jpeg_bound(int width, int height, int channels);
int amhip_jpeg_encode_dev(amhip_ctx* ctx, const uint8_t* dev_pixels, size_t step, int width, int height,
                          int channels, int quality, uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_jpeg_write(amhip_ctx* ctx, const char* filename, const uint8_t* pixels, int on_device,
                     size_t step, int width, int height, int channels, int quality);
int amhip_layer_write_jpeg(amhip_ctx* ctx, int layer, int bgr, float lower, float upper, int quality,
                           const char* filename);

/* ---- a stack of frames -> JPEG files, one batched encode: the cv::imwrite loops of
 *      io::AerialMapperIO::toStandardFormat (aerial-mapper-io.cc:199-204) and exportPix4dGeofile (:284-305) ----
 * The frames of a call share width, height, channels and quality, so every pass of the encoder above runs
 * once per group of frames, not once per frame, and only the files' sizes are read back.  Synchronous calls
 * on the default stream that take a device, not a context, like the decoders.  Scratch lives for the call
 * and is bounded by encoding in groups of frames (tuning key jpege_scratch_budget_mb); the result does not
 * depend on the grouping.  AMHIP_ERR_ARG with a text naming the export and the field, before any device is
 * touched and with *dev_files = NULL: a null pointer; F = 0; width or height outside 1..65535; channels
 * other than 1 or 3; row_step < width * channels; F > 1 and frame_stride < height * row_step; quality
 * outside 0..100; a null filenames[f]. */
/* F frames of one stack (frame f at dev_frames + f * frame_stride, rows row_step bytes apart: the layout
 * amhip_io_decode_*_frames leave) -> F baseline JPEG files, tightly concatenated in device memory:
 * file f is bytes [offsets[f], offsets[f + 1]) of *dev_files, offsets[0] = 0 (offsets: F + 1 host words).
 * channels 1 (8UC1) or 3 (8UC3 B, G, R -> Y Cb Cr 4:2:0); quality 1..100, 0 = 95.  Each file is byte for
 * byte what amhip_jpeg_encode_dev writes for that frame.  Release *dev_files with amhip_io_free(). */
int amhip_io_encode_jpeg_frames(int device, const uint8_t* dev_frames, size_t F, int width, int height,
                                int channels, size_t row_step, size_t frame_stride, int quality,
                                uint8_t** dev_files, size_t* offsets);
/* the same, downloaded and written: file f to filenames[f].  frames: host or device (on_device).  Group by
 * group: encode, download, write the group's files in order.  A file that cannot be opened or written is
 * AMHIP_ERR_ARG with its name and errno's text; the files before it stay, none behind it is written. */
int amhip_io_write_jpeg_frames(int device, const uint8_t* frames, int on_device, size_t F, int width,
                               int height, int channels, size_t row_step, size_t frame_stride, int quality,
                               const char* const* filenames);

/* ---- PNG, encoded on the GPU -------------------------------------------------------------------
 * The file libpng and zlib write for cv::imwrite(name, image) when the name ends in .png and no
 * parameter is given (filename_mosaic_output of the forward mosaic, ortho-forward-homography.cc:
 * 126-128, 188): signature, IHDR (bit depth 8, colour type 0 for 8UC1, 2 for 8UC3 stored R, G, B),
 * the zlib stream in IDAT payloads of 8192 bytes, IEND, no other chunk; filter Sub on every row;
 * zlib at level 1 with strategy Z_RLE, window 15, memLevel 8.  Byte for byte what zlib 1.2.11 writes
 * for those scanlines (tests/golden/png_encode/); that cv::imwrite chooses these parameters is
 * adopted, unpinned.  Lossless: amhip_io_decode_png_frames gives the pixels back.
 * width, height 1..65535; channels 1 or 3.  The calls mirror the JPEG ones without `quality`;
 * argument errors (AMHIP_ERR_ARG, the text names the export and the field) are reported before any
 * device is touched, a file that cannot be written is AMHIP_ERR_ARG with errno's text.
 *   amhip_png_bound        worst-case size of the file (0 for arguments out of range)
 *   amhip_png_encode_dev   device pixels (rows `step` bytes apart) -> the file in dev_out, at most
 *                          cap bytes; *bytes = the file's size.  A file larger than cap gives
 *                          AMHIP_ERR_ARG and nothing is written.  Scratch lives for the call.
 *   amhip_png_write        encode (host or device pixels), download, write `filename`
 *   amhip_layer_write_png  amhip_layer_to_image_dev into scratch, then the encoder
 *   amhip_session_layer_write_png  the whole map of a session, from the assembled image
 *   amhip_mosaic_encode_png_dev / amhip_mosaic_write_png  the mosaic's device-resident result_
 *                          (CV_16SC3 clamped to 0..255), as colour type 2 */
size_t amhip_png_bound(int width, int height, int channels);
int amhip_png_encode_dev(amhip_ctx* ctx, const uint8_t* dev_pixels, size_t step, int width, int height,
                         int channels, uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_png_write(amhip_ctx* ctx, const char* filename, const uint8_t* pixels, int on_device,
                    size_t step, int width, int height, int channels);
int amhip_layer_write_png(amhip_ctx* ctx, int layer, int bgr, float lower, float upper, const char* filename);
int amhip_mosaic_encode_png_dev(amhip_mosaic* mosaic, uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_mosaic_write_png(amhip_mosaic* mosaic, const char* filename);
/* A stack of frames -> PNG files, one batched encode; the contract of amhip_io_encode_jpeg_frames /
 * amhip_io_write_jpeg_frames above without `quality`: synchronous, on the default stream, scratch
 * bounded by encoding in groups of frames (tuning key pnge_scratch_budget_mb), the bytes independent
 * of the grouping and equal to amhip_png_encode_dev's for each frame.  AMHIP_ERR_ARG before any
 * device is touched and with *dev_files = NULL: a null pointer; F = 0; width or height outside
 * 1..65535; channels other than 1 or 3; row_step < width * channels; F > 1 and frame_stride < height
 * * row_step; a null filenames[f].  Release *dev_files with amhip_io_free(). */
int amhip_io_encode_png_frames(int device, const uint8_t* dev_frames, size_t F, int width, int height,
                               int channels, size_t row_step, size_t frame_stride, uint8_t** dev_files,
                               size_t* offsets);
int amhip_io_write_png_frames(int device, const uint8_t* frames, int on_device, size_t F, int width,
                              int height, int channels, size_t row_step, size_t frame_stride,
                              const char* const* filenames);

/* The GeoTiff container io::AerialMapperIO::toGeoTiff / writeDataToDEMGeoTiffColor produce with
 * GDAL (aerial_mapper_io/src/aerial-mapper-io.cc:349-509), without GDAL: classic little-endian
 * TIFF, 8 bits per sample, bands = 1 (BlackIsZero) or 3 (pixel interleaved, as GDAL's GTiff
 * driver lays out Create(.., 3, GDT_Byte, NULL)), uncompressed strips, ModelPixelScale /
 * ModelTiepoint from the north-up geotransform {x0, dx, 0, y0, 0, -dy}, GeoKeys of
 * "WGS 84 / UTM zone <utm_zone><N|S>" with the reference's citation.  pixels = height rows of
 * `step` bytes.  Host code only (no device is touched). */
int amhip_geotiff_write_u8(const char* filename, const uint8_t* pixels, int width, int height,
                           size_t step, int bands, const double* geotransform, int utm_zone,
                           int northern);

/* ---- tiled Deflate GeoTIFF, compressed on the GPU (an extension: the reference's two GDAL calls
 * write uncompressed bytes) -------------------------------------------------------------------------
 * A classic little-endian TIFF with one IFD, square tiles of `tile` pixels a side (a multiple of 16
 * in 16..1024; 0: 256) in row-major tile order, every tile full size (zero bytes outside the
 * raster), Compression 8 (Adobe Deflate), PlanarConfiguration 1, and the geo tags
 * amhip_geotiff_write_u8 writes for the same geotransform, zone and hemisphere.  kind:
 *   AMHIP_GEOTIFF_F32 (0)   one band of 32-bit floats, Predictor 3, SampleFormat 3, GDAL_NODATA "nan"
 *   AMHIP_GEOTIFF_U8 (1)    one band of bytes, Predictor 2, BlackIsZero
 *   AMHIP_GEOTIFF_RGB8 (2)  three bands of bytes, pixel interleaved in the order given, Predictor 2
 * Every tile is one zlib stream: byte for byte what zlib 1.2.11 writes for the tile's predictor
 * bytes at level 1 with strategy Z_RLE, window 15, memLevel 8 (tests/golden/geotiff/).
 * Any TIFF reader accepts the file; identity with a file GDAL would write is not claimed.  A file
 * of more than 2^32 - 1 bytes is refused (no BigTIFF).  Scratch lives for the call and is bounded by
 * encoding in groups of tiles (tuning key tiffe_scratch_budget_mb); the bytes do not depend on the
 * grouping.  Argument errors (AMHIP_ERR_ARG, the text names the export and the field) are reported
 * before any device is touched: a null pointer; width or height outside 1..65535; a bad kind or
 * tile; a step smaller than a row; a geotransform that is not north-up; a zone outside 1..60;
 * upper <= lower for AMHIP_GEOTIFF_U8 of a layer.  A file that cannot be written is AMHIP_ERR_ARG
 * with errno's text.
 *   amhip_geotiff_bound       worst-case size of the file (0 for arguments out of range)
 *   amhip_geotiff_encode_dev  a row-major device raster (rows `step` bytes apart) -> the file in
 *                             dev_out, at most cap bytes; *bytes = the file's size.  A file larger
 *                             than cap gives AMHIP_ERR_ARG and nothing is written.
 *   amhip_geotiff_write       encode (host or device raster), download, write `filename`
 *   amhip_layer_encode_geotiff_dev / amhip_layer_write_geotiff   the context's window of a layer as
 *                             its north-up raster, reoriented and converted inside the encoder:
 *                             x is easting, y northing, so the raster is win_rows wide and win_cols
 *                             high, pixel (r, c) is cell (win_rows - 1 - c, r) of the window, and the
 *                             geotransform is {x0, res, 0, y0, 0, -res} with x0 = pos_x - length_x / 2
 *                             + res * (rows - win_i0 - win_rows), y0 = pos_y + length_y / 2 - res *
 *                             win_j0.  Kind 0: the layer's bits (NaN stays NaN); kind 1:
 *                             amhip_layer_to_image's conversion with lower / upper; kind 2: the
 *                             packed colour layer as R, G, B (NaN: 0, 0, 0).
 *   amhip_session_layer_write_geotiff   (below) the whole map of a session */
enum { AMHIP_GEOTIFF_F32 = 0, AMHIP_GEOTIFF_U8 = 1, AMHIP_GEOTIFF_RGB8 = 2 };
size_t amhip_geotiff_bound(int width, int height, int kind, int tile);
int amhip_geotiff_encode_dev(amhip_ctx* ctx, const void* dev_raster, size_t step, int width, int height,
                             int kind, int tile, const double* geotransform, int utm_zone, int northern,
                             uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_geotiff_write(amhip_ctx* ctx, const char* filename, const void* raster, int on_device,
                        size_t step, int width, int height, int kind, int tile,
                        const double* geotransform, int utm_zone, int northern);
int amhip_layer_encode_geotiff_dev(amhip_ctx* ctx, int layer, int kind, float lower, float upper, int tile,
                                   int utm_zone, int northern, uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_layer_write_geotiff(amhip_ctx* ctx, int layer, int kind, float lower, float upper, int tile,
                              int utm_zone, int northern, const char* filename);

/* ---- GeoTIFF in: a DEM (or any raster of the accepted set) from a Deflate GeoTIFF into a layer, decoded
 * on the GPU (amhip_tiff_decode.hip).  Read: a classic little-endian TIFF, its first IFD
 * only; tiles (width and length multiples of 16) or strips; Compression 1, 8 or 32946; one band of
 * 32-bit floats, of 8- or 16-bit unsigned or of 16-bit signed integers, or three bands of 8 bit, pixel
 * interleaved; Predictor 1, 2, or 3 (floats only; with Compression 1 the tag is not acted on, as in
 * libtiff); FillOrder and Orientation 1; width and height up to 2^20.  Geo tags: ModelPixelScale + one ModelTiepoint, or a ModelTransformation without rotation,
 * north-up only; a PixelIsPoint file's origin is moved by half a pixel, so `geotransform` always
 * describes pixel areas (GDAL's convention); GeoKey 3072 is reported as `epsg`, nothing is
 * reprojected.  GDAL_NODATA is read as strtod reads it.  Anything else -- big-endian, BigTIFF, LZW,
 * PackBits, JPEG, ZSTD, LERC, 64-, 1- or 4-bit samples, 2 or 4 bands, a palette, ExtraSamples, a
 * count or an offset that leaves the file -- is AMHIP_ERR_ARG before any device is touched, with a
 * text that names the tag and the value.
 *   amhip_geotiff_info        host only: the file's description
 *   amhip_geotiff_decode_dev  the pixel window (x0, y0, w, h) of the file, in the file's sample type,
 *                             row-major into dev_out, rows `step` bytes apart (dev_out and step
 *                             multiples of the sample's size).  Only the chunks that meet the window
 *                             are uploaded and inflated (one wave per chunk), in groups bounded by
 *                             the tuning key tiffd_scratch_budget_mb; the result does not depend on
 *                             the grouping.  A chunk the walk refuses is an error that names the
 *                             chunk and the inflate status; dev_out is then undefined.
 *   amhip_layer_decode_geotiff / amhip_layer_read_geotiff   the file under the context's window of
 *                             a layer: a cell takes the pixel its centre (getPosition) lies in,
 *                             col = floor((x - GT0) / GT1), row = floor((y - GT3) / GT5) in IEEE double;
 *                             a float keeps its bits, integers are converted to float, rgb8 becomes
 *                             the packed colour value (R << 16 | G << 8 | B as a float's bits) and
 *                             goes to colored_ortho only.  A cell whose centre lies outside the
 *                             raster, whose pixel equals the nodata value or is a NaN is left as it
 *                             is (on a reset map: the layer's initial value).  No resampling.  The
 *                             layer is written only after every chunk has decoded: on any error it
 *                             is as it was.  A file without geo tags is refused here.
 *   amhip_session_layer_read_geotiff   (below) every window of a session, and the host matrix */
enum { AMHIP_GEOTIFF_U16 = 3, AMHIP_GEOTIFF_I16 = 4 };   /* kinds only a file that is read can have */
typedef struct amhip_geotiff_desc {
  int32_t width, height, bands;
  int32_t kind;             /* AMHIP_GEOTIFF_* */
  int32_t tiled;            /* 1: tiles of tile_width x tile_height; 0: strips of rows_per_strip rows */
  int32_t tile_width, tile_height, rows_per_strip;
  int32_t compression;      /* 1, 8 or 32946 */
  int32_t predictor;        /* 1, 2 or 3 */
  int32_t has_geo;          /* 0: no geo tags (geotransform = 0, 1, 0, 0, 0, 1) */
  int32_t epsg;             /* GeoKey 3072, 0: none */
  int32_t raster_type;      /* GeoKey 1025: 1 PixelIsArea (or absent), 2 PixelIsPoint */
  int32_t has_nodata;
  double geotransform[6];   /* GDAL's: x = GT0 + col * GT1, y = GT3 + row * GT5, of pixel areas */
  double nodata;
} amhip_geotiff_desc;
int amhip_geotiff_info(const uint8_t* file, size_t len, amhip_geotiff_desc* desc);
int amhip_geotiff_decode_dev(amhip_ctx* ctx, const uint8_t* file, size_t len, int x0, int y0, int w, int h,
                             void* dev_out, size_t step);
int amhip_layer_decode_geotiff(amhip_ctx* ctx, int layer, const uint8_t* file, size_t len);
int amhip_layer_read_geotiff(amhip_ctx* ctx, int layer, const char* filename);

/* ---- GeoTIFF overviews: the pyramid written on the GPU, and read by level (amhip_tiff_overview.hip,
 * DESIGN 4.18).  Level 0 is the raster as above; level k >= 1 is ceil(w / 2) x ceil(h / 2) of level
 * k - 1 and is computed from it: pixel (r, c) from rows 2r, 2r + 1 and columns 2c, 2c + 1, clipped at
 * an odd edge.  f32: the mean of the pixels that are no NaN, added as doubles in the order (2r, 2c),
 * (2r, 2c + 1), (2r + 1, 2c), (2r + 1, 2c + 1) and rounded to float once; none: the quiet NaN
 * 0x7FC00000.  u8 / rgb8: (sum + n / 2) / n per band over the n pixels of the block.  For a layer,
 * level 1 reduces the bytes of level 0 as they lie in the file, not the floats.
 * `overviews` = n >= 0 writes levels 1..n; -1 writes levels until both sides of the last are at most
 * the tile's; 0 gives the file of the exports above, byte for byte.  Refused (AMHIP_ERR_ARG, before
 * any device is touched, the text names the export and `overviews`): n > 16, n < -1, an n that would
 * reduce a 1 x 1 level.
 * The file: the header; IFD 0 at byte 8 as above; IFD 1, IFD 2, .. behind it, each word aligned and
 * followed by its own out-of-line values, chained through the next-IFD offsets.  An overview IFD
 * carries NewSubfileType (254) = 1, its own size and tile tables, the sample tags of IFD 0, GDAL_NODATA
 * for f32, and no geo tags.  Tile data from the next multiple of 16: the coarsest level first, level 0
 * last.  The tiles of all levels are coded as one list in groups bounded by tiffe_scratch_budget_mb;
 * the bytes do not depend on the grouping.  The 2^32 - 1 byte limit covers the whole file.  No GDAL
 * ghost header is written: conformance with GDAL's COG validator is not claimed. */
size_t amhip_geotiff_bound_ovr(int width, int height, int kind, int tile, int overviews);
int amhip_geotiff_encode_ovr_dev(amhip_ctx* ctx, const void* dev_raster, size_t step, int width, int height,
                                 int kind, int tile, int overviews, const double* geotransform, int utm_zone,
                                 int northern, uint8_t* dev_out, size_t cap, size_t* bytes);
int amhip_geotiff_write_ovr(amhip_ctx* ctx, const char* filename, const void* raster, int on_device,
                            size_t step, int width, int height, int kind, int tile, int overviews,
                            const double* geotransform, int utm_zone, int northern);
int amhip_layer_encode_geotiff_ovr_dev(amhip_ctx* ctx, int layer, int kind, float lower, float upper, int tile,
                                       int overviews, int utm_zone, int northern, uint8_t* dev_out, size_t cap,
                                       size_t* bytes);
int amhip_layer_write_geotiff_ovr(amhip_ctx* ctx, int layer, int kind, float lower, float upper, int tile,
                                  int overviews, int utm_zone, int northern, const char* filename);

/* Reading by level.  The IFD chain is walked with every IFD and value checked to lie inside the file;
 * more than 64 IFDs, or an offset that comes twice, is refused.  Level 0 is IFD 0; level k >= 1 is
 * the k-th later IFD whose NewSubfileType has bit 0 set and bit 2 (mask) clear; masks and pages (254
 * absent or bit 0 clear) are passed over.  A level passes the checks of IFD 0 when it is asked for
 * (the text names the level and the IFD), has IFD 0's kind, may be tiled or stripped differently, and
 * is no larger than the level before it in either dimension and smaller in one.  Its geotransform
 * is GT0, GT3 of the base, GT1 * W0 / Wk and GT5 * H0 / Hk in IEEE double; nodata is the base's.
 *   amhip_geotiff_levels       host only: 1 + the number of overview IFDs
 *   amhip_geotiff_level_info   host only: a level's description; level 0: amhip_geotiff_info's
 *   amhip_geotiff_decode_level_dev   amhip_geotiff_decode_dev on a level's chunks
 *   amhip_layer_decode_geotiff_level / amhip_layer_read_geotiff_level   the level under the layer;
 *                              level -1: the coarsest level with GT1_k <= res and -GT5_k <= res for the
 *                              map's resolution, level 0 when there is none.  A chunk that fails names
 *                              the level and the chunk; the layer is then as it was.
 *   amhip_session_layer_read_geotiff_level   (below) */
int amhip_geotiff_levels(const uint8_t* file, size_t len, int* n);
int amhip_geotiff_level_info(const uint8_t* file, size_t len, int level, amhip_geotiff_desc* desc);
int amhip_geotiff_decode_level_dev(amhip_ctx* ctx, const uint8_t* file, size_t len, int level, int x0, int y0,
                                   int w, int h, void* dev_out, size_t step);
int amhip_layer_decode_geotiff_level(amhip_ctx* ctx, int layer, const uint8_t* file, size_t len, int level);
int amhip_layer_read_geotiff_level(amhip_ctx* ctx, int layer, const char* filename, int level);

/* grid_map_msgs/GridMap in ROS 1 wire format, as GridMapRosConverter::toMessage fills it for
 * AerialGridMap::publishOnce / publishUntilShutdown (aerial-mapper-grid-map.cc:51-72).
 * _bytes: size of the message; _layout: writes everything except the layers' float payloads and
 * reports where each payload (rows * cols floats, column-major) belongs.  Host code only. */
size_t amhip_grid_map_msg_bytes(const amhip_grid_desc* grid, const char* frame_id, int num_layers,
                                const char* const* layer_names);
int amhip_grid_map_msg_layout(const amhip_grid_desc* grid, uint64_t stamp_ns, const char* frame_id,
                              int num_layers, const char* const* layer_names, uint8_t* out,
                              size_t cap, size_t* payload_offsets);

/* A binary point-cloud file ("AMPCLD01", n, flags, n x 3 float64, n x int32 intensities: what
 * loadPointCloudFromFile, aerial-mapper-io.cc:309-347, leaves in its vectors).  The loader
 * stages the file through two pinned buffers (read() of one chunk overlaps the link transfer of
 * the previous one) and leaves the cloud in HBM in the layout of amhip_dsm_process_dev /
 * amhip_ortho_from_pcl_process_dev; release with amhip_io_free().  *dev_intensities = NULL for a
 * file without intensities. */
int amhip_io_write_point_cloud_binary(const char* filename, const double* host_xyz,
                                      const int32_t* host_intensities, size_t n);
int amhip_io_load_point_cloud_binary(int device, const char* filename, double** dev_xyz,
                                     int32_t** dev_intensities, size_t* num_points);

/* ---- measurement ----------------------------------------------------------*/

/* Kernel slots for amhip_ctx_kernel_time(). */
typedef enum amhip_kernel {
  AMHIP_K_DSM_BIN_COUNT = 0, /* sort: partition histogram (+ reduce, scan)  */
  AMHIP_K_DSM_SCAN = 1,      /* sort: in-LDS placement of the sub-partitions */
  AMHIP_K_DSM_SCATTER = 2,   /* sort: the two LDS-staged scatter passes      */
  AMHIP_K_DSM_GATHER = 3,    /* per-cell radius search + IDW               */
  AMHIP_K_ORTHO = 4,         /* per-tile frame cull + per-cell fold/sample */
  AMHIP_K_MISC = 5,          /* memsets / small helpers                    */
  AMHIP_K_HALO_SELECT = 6,   /* multi-GPU: compact the halo points          */
  AMHIP_K_STEREO = 7,        /* block matching (SGBM or BM; all its kernels) */
  AMHIP_NUM_KERNELS = 8
} amhip_kernel;

/* ---- stereo::Rectifier::rectifyStereoPair (+ computeMask)
 *      aerial_mapper_dense_pcl/src/rectifier.cpp:34-128 -- the step in front of the block
 *      matcher of the dense-point-cloud pipeline (its other half is amhip_densify_dev) --------
 * K, R_G_C1, R_G_C2: row-major 3x3 on the HOST (intrinsics; orientation of the left / right
 * camera in the world), t_G_C1, t_G_C2 their positions.  dev_left / dev_right: 8UC1 rasters on
 * the GPU, rows `*_step` bytes apart.  Outputs, any may be NULL: R_G_C_out (host, 3x3 rectified
 * rotation, RectifiedStereoPair::R_G_C), baseline_out (host), dev_maps (4 planes of
 * width*height floats: map_rectify_1_x, _1_y, _2_x, _2_y), the rectified images and the mask
 * (dense width*height bytes on the GPU).  Asynchronous on the context's stream.  A zero w of
 * the inverse rectifying transformation (CHECK_NE(xyw(2), 0.0)) is reported by
 * amhip_ctx_synchronize as AMHIP_ERR_ARG. */
int amhip_rectify_stereo_pair_dev(amhip_ctx* ctx, const double* K, const double* R_G_C1,
                                  const double* R_G_C2, const double* t_G_C1, const double* t_G_C2,
                                  int width, int height, const uint8_t* dev_left, size_t left_step,
                                  const uint8_t* dev_right, size_t right_step, double* R_G_C_out,
                                  double* baseline_out, float* dev_maps, uint8_t* dev_rect_left,
                                  uint8_t* dev_rect_right, uint8_t* dev_mask);

/* ---- stereo::BlockMatchingSGBM::computeDisparityMap
 *      aerial_mapper_dense_pcl/src/block-matching-sgbm.cpp -- OpenCV's StereoSGBM (MODE_SGBM, 8UC1)
 *      between amhip_rectify_stereo_pair_dev and amhip_densify_dev --------------------------
 * BlockMatchingParameters::SGBM (common.h), field for field; amhip_sgbm_default_params fills in its
 * defaults (1, 80, 35, 10, 100, 20, 0, 120, 250, 9).  40 bytes. */
typedef struct amhip_sgbm_params {
  int32_t min_disparity, num_disparities, pre_filter_cap, uniqueness_ratio,
          speckle_window_size, speckle_range, disp_12_max_diff, p1, p2, block_size;
} amhip_sgbm_params;
void amhip_sgbm_default_params(amhip_sgbm_params* out);
/* dev_left / dev_right: rectified 8UC1 rasters on the GPU, rows *_step bytes apart.  dev_mask (NULL:
 * none): the rectification mask, pixels where it is 0 get kMaxInvalidDisparity = 1.0f.
 * dev_disparity: float rows disp_step bytes apart, the map as the wrapper leaves it (CV_16S / 16,
 * masked); dev_raw (NULL: not wanted): StereoSGBM::compute's CV_16S map (16 * disparity, invalid =
 * (min_disparity - 1) * 16), raw_step bytes apart.  num_disparities: a multiple of 16 up to 256;
 * block_size: odd, up to 11 (0: OpenCV's 5); width and height up to 32767.  min_disparity >= -2047
 * and min_disparity + num_disparities <= 2047: the CV_16S map must hold the invalid marker and
 * 16 * the largest disparity, the subpixel term included (nothing wraps inside that range; outside
 * it the call is AMHIP_ERR_ARG).  speckle_range in [-4096, 4096] (the map spans less than 2^16, so
 * every range from 4096 on acts alike; a negative one joins nothing).  The rules are those of
 * tests/sgbm_reference.py, reproduced bit for bit (parity with OpenCV itself is unpinned).
 * Scratch (about 6 bytes per pixel and disparity) belongs to the context and is kept between calls.
 * Asynchronous on the context's stream. */
int amhip_sgbm_disparity_dev(amhip_ctx* ctx, const amhip_sgbm_params* p, int width, int height,
                             const uint8_t* dev_left, size_t left_step,
                             const uint8_t* dev_right, size_t right_step,
                             const uint8_t* dev_mask, size_t mask_step,
                             float* dev_disparity, size_t disp_step,
                             int16_t* dev_raw, size_t raw_step);

/* ---- stereo::BlockMatchingBM::computeDisparityMap
 *      aerial_mapper_dense_pcl/src/block-matching-bm.cpp -- OpenCV's StereoBM (PREFILTER_XSOBEL, 8UC1),
 *      the matcher Densifier picks with BlockMatchingParameters::use_BM = true ------------------------
 * BlockMatchingParameters::BM (common.h), field for field; amhip_bm_default_params fills in its
 * defaults (1, 80, 31, 9, 80, 20, 100, 5, 0, 15).  40 bytes. */
typedef struct amhip_bm_params {
  int32_t min_disparity, num_disparities, pre_filter_cap, pre_filter_size, uniqueness_ratio,
          texture_threshold, speckle_window_size, speckle_range, disp_12_max_diff, block_size;
} amhip_bm_params;
void amhip_bm_default_params(amhip_bm_params* out);
/* The wrapper's setters as written (block-matching-bm.h): setPreFilterCap(pre_filter_cap) and then
 * setPreFilterCap(pre_filter_size), so the effective preFilterCap is pre_filter_size (9 by default)
 * and pre_filter_cap is unused; preFilterSize keeps OpenCV's 9 (unused by the x-Sobel prefilter);
 * disp_12_max_diff is never passed (disp12MaxDiff = -1: no left-right check); speckle_range is
 * passed as is, in 1/16 pixel.  The other fields map one to one.
 * Arguments as amhip_sgbm_disparity_dev: rectified 8UC1 rasters dev_left / dev_right, the optional
 * mask (0 -> kMaxInvalidDisparity = 1.0f), the float map (CV_16S / 16, masked) and the optional
 * StereoBM::compute CV_16S map (16 * disparity, FILTERED = (min_disparity - 1) * 16).
 * num_disparities: a multiple of 16 up to 256; block_size: odd, in [5, 31], <= min(width, height);
 * pre_filter_size in [1, 63]; texture_threshold, uniqueness_ratio >= 0; min_disparity >= -2047 and
 * min_disparity + num_disparities <= 2047 (what the CV_16S map can hold: FILTERED and 16 * the
 * largest disparity with its subpixel term; nothing wraps inside that range, outside it the call
 * is AMHIP_ERR_ARG); width and height in [1, 32767].  The rules are those of tests/bm_reference.py,
 * reproduced bit for bit (parity with OpenCV itself is unpinned).  Scratch (about 16 bytes per
 * pixel, no cost volume) is the context's stereo scratch, shared with the SGBM matcher.
 * Asynchronous on the context's stream. */
int amhip_bm_disparity_dev(amhip_ctx* ctx, const amhip_bm_params* p, int width, int height,
                           const uint8_t* dev_left, size_t left_step,
                           const uint8_t* dev_right, size_t right_step,
                           const uint8_t* dev_mask, size_t mask_step,
                           float* dev_disparity, size_t disp_step,
                           int16_t* dev_raw, size_t raw_step);

/* ---- several rectified pairs per call (an extension beside the reference's one-pair wrappers) ----
 * `batch` pairs of one size and one parameter set go through ONE set of launches: pair b reads
 * dev_left + b * left_batch_stride (bytes; likewise right and mask) and writes dev_disparity +
 * b * disp_batch_stride and, if wanted, dev_raw + b * raw_batch_stride.  Every rule of the one-pair
 * call holds per pair, and pair b's result is bit for bit what that call gives for pair b alone:
 * no step sees across pairs (cost sums, SGBM chains, BM window sums, the median's borders, the
 * speckle filter's regions and the right-image map all stay inside one image).  batch in
 * [1, AMHIP_STEREO_MAX_BATCH]; every *_batch_stride >= height * its row step (the mask's only with a
 * mask, the raw map's only with dev_raw), the output strides multiples of the element size:
 * otherwise AMHIP_ERR_ARG, reported before the context is looked at like every argument error.
 * The context's stereo scratch grows to batch x the one-pair size (at 1920 x 1080 and 80
 * disparities about 1 GB per SGBM pair, 33 MB per BM pair) and is kept; AMHIP_ERR_NOMEM if it cannot
 * be had.  One pair cannot fill the device (one wave per SGBM chain); several can.  Timed into the
 * same slot as the one-pair calls (AMHIP_K_STEREO).  Asynchronous on the context's stream. */
#define AMHIP_STEREO_MAX_BATCH 16
int amhip_sgbm_disparity_batch_dev(amhip_ctx* ctx, const amhip_sgbm_params* p, int width, int height,
                                   int batch,
                                   const uint8_t* dev_left, size_t left_step, size_t left_batch_stride,
                                   const uint8_t* dev_right, size_t right_step, size_t right_batch_stride,
                                   const uint8_t* dev_mask, size_t mask_step, size_t mask_batch_stride,
                                   float* dev_disparity, size_t disp_step, size_t disp_batch_stride,
                                   int16_t* dev_raw, size_t raw_step, size_t raw_batch_stride);
int amhip_bm_disparity_batch_dev(amhip_ctx* ctx, const amhip_bm_params* p, int width, int height,
                                 int batch,
                                 const uint8_t* dev_left, size_t left_step, size_t left_batch_stride,
                                 const uint8_t* dev_right, size_t right_step, size_t right_batch_stride,
                                 const uint8_t* dev_mask, size_t mask_step, size_t mask_batch_stride,
                                 float* dev_disparity, size_t disp_step, size_t disp_batch_stride,
                                 int16_t* dev_raw, size_t raw_step, size_t raw_batch_stride);

/* ---- stereo::Stereo: a frame sequence -> one dense cloud
 *      aerial_mapper_dense_pcl/include/aerial-mapper-dense-pcl/stereo.h:42-94, src/stereo.cpp ----
 * Images + body poses in, the concatenated cloud of all stereo pairs out, without a host round trip
 * inside a sequence: every frame is staged (and, if asked for, undistorted) once although it serves
 * two pairs, each pair runs amhip_rectify_stereo_pair_dev -> the block matcher -> an append-mode
 * densify whose output position is a point count that lives on the device.
 *
 * stereo::Settings (common.h:31-35) + BlockMatchingParameters (common.h:81-110).  show_rectification
 * has no counterpart (no GUI), nothing is published to ROS.  104 bytes. */
typedef struct amhip_stereo amhip_stereo;
typedef struct amhip_stereo_settings {
  uint64_t use_every_nth_image;     /* 1; 0 divides by zero in the reference: AMHIP_ERR_ARG */
  int32_t images_need_undistortion; /* 0 */
  int32_t use_bm;                   /* BlockMatchingParameters::use_BM; 0 = SGBM */
  int32_t _pad[2];
  amhip_sgbm_params sgbm;
  amhip_bm_params bm;
} amhip_stereo_settings;
/* Settings' and BlockMatchingParameters' defaults (1, false, use_BM = false, the matchers' own). */
void amhip_stereo_default_settings(amhip_stereo_settings* out);

/* stereo::Stereo::Stereo (stereo.cpp:12-80).  The object runs on the stream and the scratch of
 * `ctx` (which must outlive it; one object at a time per context call, like every context call) and
 * owns two raw frame slots that swap roles (n + 1 after amhip_stereo_set_pairs_in_flight(n)), the rectified pair + mask, the disparity map, the cloud,
 * the running point count and the PointCloud2 payload, plus a second stream on which host frames are
 * uploaded from pinned staging while the previous pair is still being matched.
 * cam: camera 0 of the NCamera; K = [fu 0 cu; 0 fv cv; 0 0 1] (:37-40) also when undistorting (the
 * reference does not switch to the undistorter's output intrinsics).  T_C_B7: get_T_C_B(0).
 * The parameters of the selected matcher are checked here, by the matcher's own rules
 * (amhip_sgbm_disparity_dev / amhip_bm_disparity_dev).  Argument errors are reported before the
 * context is looked at. */
int amhip_stereo_create(amhip_ctx* ctx, const amhip_camera* cam, const double* T_C_B7,
                        const amhip_stereo_settings* settings, amhip_stereo** out);
int amhip_stereo_destroy(amhip_stereo* stereo);
/* A newly constructed object: first_frame_ = true, the cloud emptied, the payload zeroed. */
int amhip_stereo_reset(amhip_stereo* stereo);
/* How many pairs amhip_stereo_add_frames / _dev keep in flight: n in [1, AMHIP_STEREO_MAX_BATCH],
 * 1 by default (an extension beside the reference's class; not part of amhip_stereo_settings).  For
 * every n the used frames are taken in groups of up to n consecutive pairs, by one piece of code
 * (n = 1: groups of one, which is also how amhip_stereo_add_frame runs its pair): each frame is
 * staged and undistorted once (n + 1 frame slots), the pairs of a group are rectified into stacks,
 * ONE matcher call serves the group, and the append-mode densify then runs pair by pair in order.
 * The cloud, the intensities, the point count, `pairs`, the PointCloud2 payload and every status
 * are bit for bit the same for every n: a pair with a zero baseline cuts its group (the pairs
 * before it are kept, then the call fails), and a zero w found on the device silences that pair and
 * every later one, never an earlier one (each pair of a group of more than one has its own copy of
 * the error word, taken in stream order behind its rectifier).  This call allocates the slots and stacks (AMHIP_ERR_NOMEM if they
 * cannot be had; the object then keeps its previous n) and waits for the object's work; a frame
 * carried over from earlier calls is kept.  add_frames settles the matcher's scratch for a whole
 * group before its first pair.  amhip_stereo_add_frame (one frame at a time) is unaffected. */
int amhip_stereo_set_pairs_in_flight(amhip_stereo* stereo, int n);

/* stereo::Stereo::addFrame (stereo.cpp:113-147).  T_G_B7: the body pose.  The camera pose is
 *   T_G_C = T_G_B * T_C_B^-1 (:43,129-137), amhip_compose_T_G_C's arithmetic, FP64 on the host;
 *   t_G_C its position, R_G_C the rotation matrix of its quaternion (w, x, y, z) as Eigen's
 *   toRotationMatrix spells it:  tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w,
 *   txx = tx x, txy = ty x, txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z,
 *   R = [1 - (tyy + tzz), txy - twz, txz + twy;  txy + twz, 1 - (txx + tzz), tyz - twx;
 *        txz - twy, tyz + twx, 1 - (txx + tyy)].
 * The image is 8UC1, camera width x height, rows `step` bytes apart (step >= width).  channels == 3:
 * the reference converts a gray copy only to pass its own type check and then hands the RAW colour
 * image to OpenCV's matchers, which refuse it: AMHIP_ERR_ARG.  Any other channel count:
 * AMHIP_ERR_ARG (LOG(FATAL), :123).  (Value checks come before the object is looked at.)
 * The first call after creation / reset only stores the frame as "left" and leaves the cloud as it
 * is; every later call makes one pair with its predecessor and REPLACES the cloud with that pair's
 * (:178), `pairs` = 1.  With images_need_undistortion the frame goes through the camera's mapped
 * undistorter (bilinear; the forward mosaic's remap, see amhip_mosaic_*) once, before it is used; a
 * camera without a distortion model has the identity map and the step is skipped.
 * The host form copies the image into pinned staging before it returns (the caller may free it);
 * the _dev form reads dev_image in stream order on the context's stream.  Asynchronous: no
 * synchronisation of the context's stream, no read-back.  A pair whose baseline is 0
 * (densifier.cpp:39) is AMHIP_ERR_ARG at once; a zero w of the rectification (rectifier.cpp:93,99) is
 * found on the device: that pair and every later one add nothing and amhip_stereo_cloud reports
 * AMHIP_ERR_ARG with the pairs before it.  After a failing call: amhip_stereo_reset. */
int amhip_stereo_add_frame(amhip_stereo* stereo, const double* T_G_B7, const uint8_t* host_image,
                           size_t step, int channels);
int amhip_stereo_add_frame_dev(amhip_stereo* stereo, const double* T_G_B7, const uint8_t* dev_image,
                               size_t step, int channels);

/* stereo::Stereo::addFrames (stereo.cpp:82-111): the cloud is emptied, frame i is used iff
 * (i + 1) % use_every_nth_image == 0 (:91-93), every used frame goes through addFrame and the
 * pairs' clouds are CONCATENATED in order, each in raster order (what amhip_densify_dev emits).
 * Like the reference this does not touch first_frame_: on a fresh / reset object the first used frame
 * only becomes "left"; after earlier calls it pairs with the frame left over from them.
 * Capacity is settled before the first pair (pairs x width x height points worst case, grown once;
 * AMHIP_ERR_NOMEM if that cannot be had); between the first and the last pair there is no
 * allocation, no synchronisation of the context's stream and no copy of a count (the block matcher's
 * scratch is the context's and is sized by the first pair).  The host form waits only for the upload
 * that last used a staging buffer (two frames back).  The sequence stops at the first failing pair
 * and keeps the pairs before it.
 * host_images[i]: frame i, rows steps[i] bytes apart.  _dev: one stack on the GPU, frame i at
 * dev_frames + i * frame_stride, rows row_step bytes apart. */
int amhip_stereo_add_frames(amhip_stereo* stereo, const double* T_G_B7xF,
                            const uint8_t* const* host_images, const size_t* steps, int channels,
                            size_t F);
int amhip_stereo_add_frames_dev(amhip_stereo* stereo, const double* T_G_B7xF,
                                const uint8_t* dev_frames, size_t frame_stride, size_t row_step,
                                int channels, size_t F);

/* The cloud: the last add_frame's pair, or the last add_frames' sequence.  Synchronises the context
 * (the ONE read-back of the point count) and returns its sticky status.  dev_xyz (3 n doubles, AoS) /
 * dev_intensities (n int32): the layout amhip_dsm_process_dev / amhip_ortho_from_pcl_process_dev
 * take; they stay valid until the next add_frame / add_frames / destroy on the object.  Any output
 * pointer may be NULL. */
int amhip_stereo_cloud(amhip_stereo* stereo, const double** dev_xyz, const int32_t** dev_intensities,
                       size_t* n, size_t* pairs);

/* The sensor_msgs::PointCloud2 payload (point_cloud_ros_msg_.data) of the LAST pair, filled in the
 * emit pass of that pair (densifier.cpp:53-106, stereo.cpp:46-76): point_step 16, row_step 16 width,
 * width x height slots of x, y, z as float32 ((float)point_G) and rgb = gray << 16 | gray << 8 | gray
 * as uint32; invalid pixels hold the quiet-NaN pattern 0x7FC00000 in all four fields.  The reference
 * advances point_offset BEFORE it writes (:58): pixel k lands in slot k + 1, slot 0 keeps the zeros
 * of data.resize() and the last pixel's write falls 16 bytes behind the buffer (undefined behaviour
 * there).  Reproduced: the shift, the zero slot 0; the last pixel is dropped.  All zero before the
 * first pair.  Overwritten by the next pair like point_cloud_ros_msg_.  In stream order on the
 * context's stream (amhip_ctx_synchronize before reading it from elsewhere). */
int amhip_stereo_point_cloud2_dev(amhip_stereo* stereo, const void** dev_data, size_t* bytes);

/* ---- session: one map served through HOST matrices by one or several GPUs ---------------
 *
 * What the drop-in classes share per grid_map::GridMap (the .cc files under aerial_mapper_amd/cpp): the map
 * is cut into tiles_i x tiles_j windows, window k = (k % tiles_i, k / tiles_i) lives on
 * devices[k] (NULL = all on device 0; a device may serve several windows), everything inside ONE
 * host process like the reference's demos (main-dsm.cc:103-107, main-ortho-backward-grid.cc:
 * 128-141).  A DSM call uploads one slice of the cloud per window, every device selects what
 * every window needs of its slice (cells + halo margin) and the selections travel device to
 * device (hipMemcpyPeerAsync over xGMI); frames and poses are replicated.
 * The layers stay resident between calls: whether a host matrix still holds what the devices
 * hold is decided by a 64-bit content sum (host threads on the way in, a kernel on the way out)
 * -- equal: no transfer; the layer's initial constant: a lazy device-side reset; anything
 * else: uploaded.  Outputs the kernels left unchanged are not downloaded; of a layer that a call
 * changed only inside a rectangle it knows (a small cloud's bounding box on a large map, the
 * tiles a small batch of frames can see: the incremental use case) only that rectangle is
 * (tuning knob session_no_partial: whole windows).  Results are those of the single-context calls
 * (same kernels; windows reproduce the full map).
 * tuning knob session_always_copy / amhip_session_set_always_copy: every matrix up and down.
 * amhip_session_transfer_stats: bytes of layer data uploaded / downloaded since the session was
 * created (clouds and frames not counted). */
typedef struct amhip_session amhip_session;
int amhip_session_create(const amhip_grid_desc* grid, int tiles_i, int tiles_j,
                         const int32_t* devices, amhip_session** out);
void amhip_session_destroy(amhip_session* s);
int amhip_session_num_windows(const amhip_session* s);
amhip_ctx* amhip_session_context(amhip_session* s, int window);
int amhip_session_window(const amhip_session* s, int window, int32_t* i0_j0_rows_cols);
int amhip_session_set_always_copy(amhip_session* s, int on);
int amhip_session_set_dsm_precision(amhip_session* s, int mode);  /* AMHIP_DSM_FAST / _EXACT */
int amhip_session_transfer_stats(const amhip_session* s, uint64_t* uploaded_bytes,
                                 uint64_t* downloaded_bytes);
/* Where the LAST host-buffer call on this session (DSM / backward mosaic / OrthoFromPcl) spent its
 * time, window 0's view: out8 = { total_ms, h2d_ms (wall clock until the call's inputs -- cloud or
 * frames -- were handed to the copy engine; pageable sources block that long), host_sum_ms (host
 * content sums, running beside the upload), kernel_ms (HIP events around the call's kernels),
 * dev_sum_wait_ms (wall clock spent waiting for device content sums that could not run beside a
 * download), d2h_ms (HIP events around the downloads), bytes uploaded as inputs, layer bytes
 * downloaded }. */
int amhip_session_last_profile(const amhip_session* s, double* out8);
/* dsm::Dsm::process (dsm.cc:186-201): `elevation` = the GridMap's matrix (map rows x cols,
 * column-major), read and written like the reference does. */
int amhip_session_dsm_process(amhip_session* s, const double* host_xyz, size_t n, int radius_sq,
                              double center_easting, double center_northing, float* elevation);
/* ortho::OrthoFromPcl::process (ortho-from-pcl.cc:20-113): `ortho` = the GridMap's matrix. */
int amhip_session_ortho_from_pcl_process(amhip_session* s, const double* host_xyz,
                                         const int32_t* host_intensities, size_t n, int radius_sq,
                                         int adaptive, float* ortho);
/* ortho::OrthoBackwardGrid::process (ortho-backward-grid.cc:223-239): the six matrices of the
 * map (all required except the one of ortho / colored_ortho the mode does not write). */
int amhip_session_ortho_backward_process(
    amhip_session* s, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho);
/* ... with the occlusion test of amhip_ortho_backward_process_occl.  A session of one window runs
 * it; a session of several windows is refused (AMHIP_ERR_ARG: the ray leaves the window). */
int amhip_session_ortho_backward_process_occl(
    amhip_session* s, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho, double margin_m);
/* ... blended (amhip_ortho_backward_process_blend): every window's context holds its own cells'
 * sums, and a map whose matrices were set back to their initial constants restarts them (its
 * observation_index is NaN).  Without the occlusion test a session of several windows runs it and
 * gives the one-window layers; with it only a session of one window (AMHIP_ERR_ARG otherwise). */
int amhip_session_ortho_backward_process_blend(
    amhip_session* s, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho,
    const amhip_ortho_blend_opts* opts);

/* With timing enabled every launch is bracketed by hipEvents on the
 * context's stream.  amhip_ctx_kernel_time() synchronises, then reports the
 * accumulated milliseconds and launch count of one slot since the last
 * amhip_ctx_timing_reset(). */
int amhip_ctx_enable_timing(amhip_ctx* ctx, int on);
int amhip_ctx_timing_reset(amhip_ctx* ctx);
int amhip_ctx_kernel_time(amhip_ctx* ctx, int kernel, double* total_ms,
                          int64_t* launches);
const char* amhip_kernel_name(int kernel);

/* Counters of the last amhip_dsm_process*: points kept after the bin-range
 * filter, number of bins, bin edge in cells. */
int amhip_ctx_dsm_stats(amhip_ctx* ctx, int64_t* points_binned,
                        int64_t* num_bins, int32_t* bin_cells);
/* Which binning sort the last amhip_dsm_process* / amhip_ortho_from_pcl_process* of the context took
 * (host bookkeeping, no synchronisation): -1 none yet, 0 the one-level counting sort, 1 the
 * three-pass sort with its count pass, 2 the three-pass sort on runs (tuning key sort_runs). */
#define AMHIP_SORT_ONE_LEVEL 0
#define AMHIP_SORT_COUNT 1
#define AMHIP_SORT_RUNS 2
int amhip_ctx_dsm_sort_pipeline(amhip_ctx* ctx, int32_t* pipeline);

/* Where the gather tiles of the last amhip_dsm_process* went (synchronises): out8[0..6] = tiles
 * on the lists of the tiled gather -- [0] occupied class-0 tiles (sparse calls only), [1] / [2]
 * capacity classes 1 / 2 (denser than the main launch's LDS image), [3] beyond any LDS image
 * (wave-per-block kernel), [4] / [5] tiles the single-precision gather handed to the FP64 kernel
 * (height range leaves no room under the 1e-4 m error bound: rough terrain), [6] those beyond
 * its largest image -- and out8[7] = tiles of the map.  All zero when the LDS-tiled gather was
 * not used. */
int amhip_ctx_dsm_gather_stats(amhip_ctx* ctx, int64_t* out8);

/* Order `other_stream` (hipStream_t as void*) behind everything the context has enqueued so far: an
 * event recorded on the context's stream, waited for by the other stream -- no host wait.  For
 * callers that feed asynchronous calls (`*_dev` entry points) from buffers another stream refills. */
int amhip_ctx_order_after(amhip_ctx* ctx, void* other_stream);

/* The session's map as a grid_map_msgs/GridMap message (ROS 1 wire format): the resident layers
 * travel from the devices straight into `out`.  layer_ids[l] = the amhip layer behind message
 * layer l, or -1: host_layers[l] (rows x cols floats, column-major) is copied, NaN-filled when
 * null.  cap >= amhip_grid_map_msg_bytes(..); *written = the message size. */
int amhip_session_grid_map_msg(amhip_session* s, uint64_t stamp_ns, const char* frame_id,
                               int num_layers, const char* const* layer_names,
                               const int32_t* layer_ids, const float* const* host_layers,
                               uint8_t* out, size_t cap, size_t* written);
/* amhip_layer_to_image for the whole map of a session (every window on its own device). */
int amhip_session_layer_to_image(amhip_session* s, int layer, int bgr, float lower, float upper,
                                 uint8_t* host_image, size_t step);
/* amhip_layer_write_jpeg for the whole map of a session, from the assembled image. */
int amhip_session_layer_write_jpeg(amhip_session* s, int layer, int bgr, float lower, float upper,
                                   int quality, const char* filename);
/* amhip_layer_write_png for the whole map of a session, the same way. */
int amhip_session_layer_write_png(amhip_session* s, int layer, int bgr, float lower, float upper,
                                  const char* filename);
/* amhip_layer_write_geotiff for the whole map of a session: the north-up raster assembled through
 * the host, encoded on the first window's device; the bytes of a single context's file. */
int amhip_session_layer_write_geotiff(amhip_session* s, int layer, int kind, float lower, float upper, int tile,
                                      int utm_zone, int northern, const char* filename);

/* amhip_layer_read_geotiff for every window of a session (each decodes the chunks under its own cells),
 * then into `matrix`, the GridMap's host matrix of the layer (rows x cols, column-major): cells the file
 * does not reach keep the matrix's values.  The session's content sums agree with the matrix
 * afterwards: the next call that is handed the same matrix uploads no byte of it.  On any error no
 * window's layer and no cell of the matrix has changed. */
int amhip_session_layer_read_geotiff(amhip_session* s, int layer, const char* filename, float* matrix);
/* ... with overviews (amhip_geotiff_write_ovr of the assembled raster: the single context's pyramid),
 * and from a level of the file (-1: the automatic choice, the same for every window). */
int amhip_session_layer_write_geotiff_ovr(amhip_session* s, int layer, int kind, float lower, float upper,
                                          int tile, int overviews, int utm_zone, int northern,
                                          const char* filename);
int amhip_session_layer_read_geotiff_level(amhip_session* s, int layer, const char* filename, int level,
                                           float* matrix);

/* ---- tuning knobs: the ONE door for switches that select among correct implementations ----------
 * (tests force every path through them, A-B timing flips them; none is needed in normal use).
 * amhip_set_tuning(key, value) -- value NaN clears the key -- or, for hosts that cannot be
 * recompiled, AMHIP_TUNING="key=value,key,..." in the environment (read once; a bare key = 1).
 * Unknown keys are an error (AMHIP_ERR_ARG) / a warning on stderr.  Process-wide; looked up when a
 * call is made.  Keys:
 *   sort_one_level            clouds of any size take the one-level counting sort
 *   p3_min_points (2^20)      cloud size from which the three-pass partition sort is used
 *   p3_target (1536)          points per sub-partition the sort's plan aims for
 *   p3_cap (2048)             points a placement workgroup sorts in its registers / LDS
 *   p3_rounds_cap, p3_rounds_reread   placement in rounds (sub-partitions beyond one LDS image)
 *                             forced at test size: image of n points / re-reading instead of registers
 *   no_launch_skips           launch every capacity-class / big-list kernel whatever the previous
 *                             call's counters say
 *   sort_runs (1)             the three-pass sort without its count pass (local sorts, runs gathered)
 *                             where the call is eligible: FP64 point pipeline, whole untiled context,
 *                             at most 2^27 points; 0: the counting pipeline everywhere
 *   dsm_canon_all             every FP64 quotient goes through the order-independent double-double sums
 *   knn_global_bins           the optional k-cap mode on the plain global-bins kernel (default: LDS-tiled)
 *   dsm_no_rough_switch       the single-precision mode stays in its own pipeline on rough scenes
 *   dsm_no_subwindow          small clouds onto large maps are binned over the whole window
 *   eager_reset               amhip_layers_reset fills the layers at once (default: fused into producers)
 *   ortho_exact_fold, ortho_no_prune, no_coarse_cull, ortho_no_tile_list
 *                             mosaic: every pair in the reference's arithmetic / keep dominated frames /
 *                             no small-batch pre-cull / dispatch every tile of a large map instead of a
 *                             list of visible ones
 *   no_distorted_cull, no_distorted_prune, distorted_square_cull   cameras with a distortion model
 *   jpegd_coef_budget_mb (4096)  amhip_io_decode_jpeg_frames: MB of coefficient scratch per group of frames;
 *                             groups run one after another (a small value forces several groups)
 *   pnge_scratch_budget_mb (4096)  amhip_io_encode_png_frames / amhip_io_write_png_frames: MB of encoder
 *                             scratch per group of frames
 *   tiffe_scratch_budget_mb (4096)  amhip_geotiff_encode_dev and its kin: MB of encoder scratch per group of
 *                             tiles; groups run one after another, at least one tile each
 *   tiffd_scratch_budget_mb (4096)  amhip_geotiff_decode_dev and its kin: MB of inflated chunks per group of
 *                             chunks; groups run one after another, at least one chunk each
 *   jpege_scratch_budget_mb (4096)  amhip_io_encode_jpeg_frames / amhip_io_write_jpeg_frames: MB of encoder
 *                             scratch (340 B per scan block) per group of frames; groups run one after
 *                             another, at least one frame each
 *   pngd_raw_budget_mb (4096)  amhip_io_decode_png_frames: MB of raw scanlines per group of frames; groups run
 *                             one after another, at least one frame each
 *   session_always_copy, session_threads, session_scalar_sums, session_no_partial,
 *   session_serial_sums       device content sums always before the downloads (round 5's order)
 *   session_verify_partial, session_trace          amhip_session: every matrix both ways on every
 *                             call / host threads of the content sums / scalar sums / whole-window
 *                             downloads / re-sum partial downloads / phase timings on stderr
 *   (lab builds, -DAMHIP_TIMING_PROBES: gather_tj, gather_nt, gather_class_cap0..2, f32_variant, fx_theta)
 * Environment variables the library itself reads, all of them: AMHIP_TUNING (above), AMHIP_DSM_FAST /
 * AMHIP_DSM_EXACT (amhip_default_dsm_precision); the C++ drop-in classes add AERIAL_MAPPER_HIP_DEVICE
 * and AERIAL_MAPPER_HIP_DEVICES (aerial_mapper_amd/cpp/shim_common.*). */
int amhip_set_tuning(const char* key, double value);
double amhip_get_tuning(const char* key, double dflt);
/* AMHIP_DSM_EXACT unless the environment says AMHIP_DSM_FAST=1 (and not AMHIP_DSM_EXACT): what new
 * contexts, sessions and dsm::Dsm objects start with. */
int amhip_default_dsm_precision(void);

/* The library's build id: 16 hex digits of the SHA-256 over its sources, headers and compiler flags
 * (aerial_mapper_amd/build.py).  Profiles collected from one build are refused as evidence for
 * another (bench.py). */
const char* amhip_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* AERIAL_MAPPER_HIP_H_ */
