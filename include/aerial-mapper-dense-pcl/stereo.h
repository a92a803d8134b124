// stereo::Stereo on MI355X -- drop-in for the reference class
// (aerial_mapper_dense_pcl/include/aerial-mapper-dense-pcl/stereo.h:42-94): same namespace,
// constructor, addFrames and addFrame signatures, so main-dense-pcl.cc and
// main-ortho-backward-grid-incremental.cc:149 compile against it unchanged.  Undistortion,
// rectification, block matching and the reprojection run on the GPU (amhip_stereo_*,
// include/aerial_mapper_hip.h); the result comes back with one download per call.
// Left out: the ROS members (node handle, publishers, point_cloud_ros_msg_ -- its payload is
// available on the device, see pointCloud2Payload) and visualizeRectification.
#ifndef AERIAL_MAPPER_HIP_DENSE_PCL_STEREO_H_
#define AERIAL_MAPPER_HIP_DENSE_PCL_STEREO_H_

#include <cstdint>
#include <memory>
#include <vector>

#include "aerial-mapper-dense-pcl/common.h"

struct amhip_ctx;
struct amhip_stereo;

namespace stereo {

class Stereo {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  Stereo(const std::shared_ptr<aslam::NCamera> ncameras, const Settings& settings,
         const BlockMatchingParameters& block_matching_params);
  ~Stereo();
  Stereo(const Stereo&) = delete;
  Stereo& operator=(const Stereo&) = delete;

  void addFrames(const Poses& T_G_Bs, const Images& images,
                 AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                 std::vector<int>* point_cloud_intensities = nullptr);

  void addFrame(const Pose& T_G_B, const Image& image,
                AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                std::vector<int>* point_cloud_intensities = nullptr);

  // --- extension ------------------------------------------------------------------------------
  // point_cloud_ros_msg_.data of the last stereo pair (height x width slots of 16 bytes, see
  // amhip_stereo_point_cloud2_dev), downloaded.
  std::vector<uint8_t> pointCloud2Payload() const;
  // How many stereo pairs addFrames keeps in flight (1 .. 16, default 1): with n > 1 the block
  // matcher serves up to n consecutive pairs per launch (amhip_stereo_set_pairs_in_flight).  The
  // cloud is bit for bit that of n = 1.  addFrame is unaffected.
  void setPairsInFlight(int n);

  static constexpr size_t kFrameIdx = 0u;

 private:
  void download(AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud,
                std::vector<int>* point_cloud_intensities, const char* where);

  std::shared_ptr<aslam::NCamera> ncameras_;
  Settings settings_;
  amhip_ctx* ctx_;
  amhip_stereo* stereo_;
};

}  // namespace stereo

#endif  // AERIAL_MAPPER_HIP_DENSE_PCL_STEREO_H_
