// stereo::Settings, stereo::BlockMatchingParameters and the container typedefs of the dense
// point-cloud package -- drop-in for the reference's
// aerial_mapper_dense_pcl/include/aerial-mapper-dense-pcl/common.h:29-117 (same names, members and
// defaults).  The structs that only travel between the reference's own Rectifier / Densifier
// (StereoRigParameters, RectifiedStereoPair, DensifiedStereoPair) have no counterpart: those steps
// run on the GPU behind stereo::Stereo.
#ifndef AERIAL_MAPPER_HIP_DENSE_PCL_COMMON_H_
#define AERIAL_MAPPER_HIP_DENSE_PCL_COMMON_H_

#include <cstddef>
#include <vector>

#include "aerial-mapper-deps.h"
#include "aerial-mapper-utils/utils-nearest-neighbor.h"

namespace stereo {

struct Settings {
  size_t use_every_nth_image = 1;
  bool images_need_undistortion = false;
  bool show_rectification = true;  // accepted, not used: there is no GUI on this path
};

struct BlockMatchingParameters {
  // Uses SGBM if "use_BM" is false.
  bool use_BM = false;

  struct SGBM {
    int min_disparity = 1;
    int num_disparities = 80;
    int pre_filter_cap = 35;
    int uniqueness_ratio = 10;
    int speckle_window_size = 100;
    int speckle_range = 20;
    int disp_12_max_diff = 0;
    int p1 = 120;
    int p2 = 250;
    int block_size = 9;
  } sgbm;

  struct BM {
    int min_disparity = 1;
    int num_disparities = 80;
    int pre_filter_cap = 31;
    int pre_filter_size = 9;
    int uniqueness_ratio = 80;
    int texture_threshold = 20;
    int speckle_window_size = 100;
    int speckle_range = 5;
    int disp_12_max_diff = 0;
    int block_size = 15;
  } bm;
};

typedef kindr::minimal::QuatTransformation Pose;
typedef std::vector<Pose> Poses;
typedef cv::Mat Image;
typedef std::vector<Image> Images;

}  // namespace stereo

#endif  // AERIAL_MAPPER_HIP_DENSE_PCL_COMMON_H_
