// The public surface of stereo::Stereo and its parameter structs, as statements that hold for the
// reference's headers (aerial_mapper_dense_pcl/include/aerial-mapper-dense-pcl/{stereo,common}.h)
// and must hold for include/aerial-mapper-dense-pcl/ of this repository: compiled with
// -fsyntax-only (tests/test_api_conformance_stereo.py; tests/cpp/api_conformance.cc is the model).
#include <memory>
#include <type_traits>
#include <vector>

#include <aerial-mapper-dense-pcl/stereo.h>

typedef AlignedType<std::vector, Eigen::Vector3d>::type Cloud;

// stereo.h:45-47
static_assert(std::is_constructible<stereo::Stereo, const std::shared_ptr<aslam::NCamera>,
                                    const stereo::Settings&,
                                    const stereo::BlockMatchingParameters&>::value,
              "Stereo(ncameras, settings, block_matching_params)");
// stereo.h:49-51, :53-55 (the intensities default to nullptr: checked by the calls below)
static_assert(std::is_same<decltype(static_cast<void (stereo::Stereo::*)(
                               const stereo::Poses&, const stereo::Images&, Cloud*, std::vector<int>*)>(
                               &stereo::Stereo::addFrames)),
                           void (stereo::Stereo::*)(const stereo::Poses&, const stereo::Images&, Cloud*,
                                                    std::vector<int>*)>::value,
              "addFrames(T_G_Bs, images, point_cloud, point_cloud_intensities)");
static_assert(std::is_same<decltype(static_cast<void (stereo::Stereo::*)(
                               const stereo::Pose&, const stereo::Image&, Cloud*, std::vector<int>*)>(
                               &stereo::Stereo::addFrame)),
                           void (stereo::Stereo::*)(const stereo::Pose&, const stereo::Image&, Cloud*,
                                                    std::vector<int>*)>::value,
              "addFrame(T_G_B, image, point_cloud, point_cloud_intensities)");
static_assert(stereo::Stereo::kFrameIdx == 0u, "kFrameIdx");

// common.h:31-35
static_assert(std::is_same<decltype(stereo::Settings::use_every_nth_image), size_t>::value, "size_t");
static_assert(std::is_same<decltype(stereo::Settings::images_need_undistortion), bool>::value, "bool");
static_assert(std::is_same<decltype(stereo::Settings::show_rectification), bool>::value, "bool");
// common.h:81-110
static_assert(std::is_same<decltype(stereo::BlockMatchingParameters::use_BM), bool>::value, "bool");
static_assert(std::is_same<decltype(stereo::BlockMatchingParameters::sgbm),
                           stereo::BlockMatchingParameters::SGBM>::value, "sgbm");
static_assert(std::is_same<decltype(stereo::BlockMatchingParameters::bm),
                           stereo::BlockMatchingParameters::BM>::value, "bm");
static_assert(std::is_same<decltype(stereo::BlockMatchingParameters::SGBM::p2), int>::value, "int");
static_assert(std::is_same<decltype(stereo::BlockMatchingParameters::BM::texture_threshold), int>::value, "int");
// common.h:112-115
static_assert(std::is_same<stereo::Pose, kindr::minimal::QuatTransformation>::value, "Pose");
static_assert(std::is_same<stereo::Poses, std::vector<stereo::Pose> >::value, "Poses");
static_assert(std::is_same<stereo::Image, cv::Mat>::value, "Image");
static_assert(std::is_same<stereo::Images, std::vector<cv::Mat> >::value, "Images");

// the defaults (member initialisers are not constant expressions: checked when this is run, and
// read by the compiler either way)
inline bool defaults_are_the_references() {
  const stereo::Settings s;
  const stereo::BlockMatchingParameters p;
  const stereo::BlockMatchingParameters::SGBM& g = p.sgbm;
  const stereo::BlockMatchingParameters::BM& b = p.bm;
  return s.use_every_nth_image == 1 && !s.images_need_undistortion && s.show_rectification &&
         !p.use_BM && g.min_disparity == 1 && g.num_disparities == 80 && g.pre_filter_cap == 35 &&
         g.uniqueness_ratio == 10 && g.speckle_window_size == 100 && g.speckle_range == 20 &&
         g.disp_12_max_diff == 0 && g.p1 == 120 && g.p2 == 250 && g.block_size == 9 &&
         b.min_disparity == 1 && b.num_disparities == 80 && b.pre_filter_cap == 31 &&
         b.pre_filter_size == 9 && b.uniqueness_ratio == 80 && b.texture_threshold == 20 &&
         b.speckle_window_size == 100 && b.speckle_range == 5 && b.disp_12_max_diff == 0 &&
         b.block_size == 15;
}

// the calls of main-dense-pcl.cc and main-ortho-backward-grid-incremental.cc:149, with and without
// the optional intensities
inline void calls(stereo::Stereo& stereo, const stereo::Poses& T_G_Bs, const stereo::Images& images) {
  Cloud point_cloud;
  std::vector<int> point_cloud_intensities;
  stereo.addFrames(T_G_Bs, images, &point_cloud, &point_cloud_intensities);
  stereo.addFrames(T_G_Bs, images, &point_cloud);
  stereo.addFrame(T_G_Bs[0], images[0], &point_cloud, &point_cloud_intensities);
  stereo.addFrame(T_G_Bs[0], images[0], &point_cloud);
}

#ifdef API_STEREO_MAIN
int main() { return defaults_are_the_references() ? 0 : 1; }
#endif
