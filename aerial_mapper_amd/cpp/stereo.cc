// stereo::Stereo over the C ABI (see include/aerial-mapper-dense-pcl/stereo.h).
#include "aerial-mapper-dense-pcl/stereo.h"

#include <cstring>
#include <vector>

#include "shim_common.h"

namespace stereo {

using amhip_shim::check_status;
using amhip_shim::fatal;
using amhip_shim::pose_to7;

Stereo::Stereo(const std::shared_ptr<aslam::NCamera> ncameras, const Settings& settings,
               const BlockMatchingParameters& block_matching_params)
    : ncameras_(ncameras), settings_(settings), ctx_(nullptr), stereo_(nullptr) {
  if (!ncameras_) fatal("Stereo", "CHECK(ncameras_)");
  // The object needs a context (stream, matcher scratch) but no map: a one-cell grid.
  amhip_grid_desc grid;
  amhip_make_grid(1.0, 1.0, 1.0, 0.0, 0.0, &grid);
  check_status(amhip_ctx_create(&grid, amhip_shim::default_device(), &ctx_), "Stereo");
  const amhip_camera cam = amhip_shim::describe_camera(ncameras_->getCamera(kFrameIdx));
  double tcb[7];
  pose_to7(ncameras_->get_T_C_B(kFrameIdx), tcb);
  amhip_stereo_settings s;
  amhip_stereo_default_settings(&s);
  s.use_every_nth_image = settings_.use_every_nth_image;
  s.images_need_undistortion = settings_.images_need_undistortion ? 1 : 0;
  s.use_bm = block_matching_params.use_BM ? 1 : 0;
  const BlockMatchingParameters::SGBM& g = block_matching_params.sgbm;
  const amhip_sgbm_params sgbm = {g.min_disparity, g.num_disparities, g.pre_filter_cap,
                                  g.uniqueness_ratio, g.speckle_window_size, g.speckle_range,
                                  g.disp_12_max_diff, g.p1, g.p2, g.block_size};
  const BlockMatchingParameters::BM& b = block_matching_params.bm;
  const amhip_bm_params bm = {b.min_disparity, b.num_disparities, b.pre_filter_cap,
                              b.pre_filter_size, b.uniqueness_ratio, b.texture_threshold,
                              b.speckle_window_size, b.speckle_range, b.disp_12_max_diff,
                              b.block_size};
  s.sgbm = sgbm;
  s.bm = bm;
  check_status(amhip_stereo_create(ctx_, &cam, tcb, &s, &stereo_), "Stereo");
}

Stereo::~Stereo() {
  if (stereo_) amhip_stereo_destroy(stereo_);
  if (ctx_) amhip_ctx_destroy(ctx_);
}

void Stereo::setPairsInFlight(int n) {
  check_status(amhip_stereo_set_pairs_in_flight(stereo_, n), "Stereo::setPairsInFlight");
}

static void check_image(const Image& image, const aslam::Camera& camera, const char* where) {
  if (image.channels() != 1 && image.channels() != 3) fatal(where, "Image type not supported");
  if (image.cols != static_cast<int>(camera.imageWidth()) ||
      image.rows != static_cast<int>(camera.imageHeight()))
    fatal(where, "image size differs from the camera's");
}

void Stereo::download(AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                      std::vector<int>* point_cloud_intensities, const char* where) {
  const double* dev_xyz = nullptr;
  const int32_t* dev_intensities = nullptr;
  size_t n = 0, pairs = 0;
  check_status(amhip_stereo_cloud(stereo_, &dev_xyz, &dev_intensities, &n, &pairs), where);
  static_assert(sizeof(Eigen::Vector3d) == 3 * sizeof(double), "points are AoS x, y, z doubles");
  static_assert(sizeof(int) == sizeof(int32_t), "intensities are 32-bit");
  point_cloud->resize(n);
  if (point_cloud_intensities) point_cloud_intensities->resize(n);
  if (n == 0) return;
  check_status(amhip_io_download_point_cloud(
                   dev_xyz, point_cloud_intensities ? dev_intensities : nullptr, n,
                   reinterpret_cast<double*>(point_cloud->data()),
                   point_cloud_intensities ? reinterpret_cast<int32_t*>(point_cloud_intensities->data())
                                           : nullptr),
               where);
}

void Stereo::addFrames(const Poses& T_G_Bs, const Images& images,
                       AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                       std::vector<int>* point_cloud_intensities) {
  if (!point_cloud) fatal("Stereo::addFrames", "CHECK(point_cloud)");
  // the reference loops over images.size() and indexes T_G_Bs with it (stereo.cpp:92-97)
  if (T_G_Bs.size() < images.size()) fatal("Stereo::addFrames", "fewer poses than images");
  const size_t F = images.size();
  std::vector<double> tgb(7 * F + 7);
  std::vector<const uint8_t*> data(F + 1);
  std::vector<size_t> steps(F + 1);
  int channels = 1;
  for (size_t f = 0; f < F; ++f) {
    check_image(images[f], ncameras_->getCamera(kFrameIdx), "Stereo::addFrames");
    pose_to7(T_G_Bs[f], &tgb[7 * f]);
    data[f] = images[f].data;
    steps[f] = static_cast<size_t>(images[f].step);
    if (images[f].channels() != 1) channels = images[f].channels();
  }
  check_status(amhip_stereo_add_frames(stereo_, tgb.data(), data.data(), steps.data(), channels, F),
               "Stereo::addFrames");
  download(point_cloud, point_cloud_intensities, "Stereo::addFrames");
}

void Stereo::addFrame(const Pose& T_G_B, const Image& image,
                      AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                      std::vector<int>* point_cloud_intensities) {
  if (!point_cloud) fatal("Stereo::addFrame", "CHECK(point_cloud)");
  check_image(image, ncameras_->getCamera(kFrameIdx), "Stereo::addFrame");
  double tgb[7];
  pose_to7(T_G_B, tgb);
  check_status(amhip_stereo_add_frame(stereo_, tgb, image.data, static_cast<size_t>(image.step),
                                      image.channels()),
               "Stereo::addFrame");
  size_t n = 0, pairs = 0;
  check_status(amhip_stereo_cloud(stereo_, nullptr, nullptr, &n, &pairs), "Stereo::addFrame");
  // the first frame has no partner yet: the caller's cloud stays as it is (stereo.cpp:127-134)
  if (pairs == 0) return;
  download(point_cloud, point_cloud_intensities, "Stereo::addFrame");
}

std::vector<uint8_t> Stereo::pointCloud2Payload() const {
  const void* dev = nullptr;
  size_t bytes = 0;
  check_status(amhip_stereo_point_cloud2_dev(stereo_, &dev, &bytes), "Stereo::pointCloud2Payload");
  check_status(amhip_ctx_synchronize(ctx_), "Stereo::pointCloud2Payload");
  std::vector<uint8_t> out(bytes);
  // (a plain device -> host copy through the point-cloud download: bytes / 4 32-bit words, no xyz)
  check_status(amhip_io_download_point_cloud(static_cast<const double*>(dev),
                                             static_cast<const int32_t*>(dev), bytes / 4, nullptr,
                                             reinterpret_cast<int32_t*>(out.data())),
               "Stereo::pointCloud2Payload");
  return out;
}

}  // namespace stereo
