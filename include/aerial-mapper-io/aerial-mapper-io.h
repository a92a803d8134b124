// The four typedefs of aerial-mapper-io.h:17-20 that appear in the mosaic
// classes' signatures, and the text-format loaders of io::AerialMapperIO that
// sit directly in front of the hot path:
//   loadPointCloudFromFile (both overloads, aerial-mapper-io.cc:309-347) --
//     tokenised and parsed on the GPU (amhip_io_parse_point_cloud_text);
//   loadPosesFromFileStandard (:103-121) -- a few KB, read on the host;
//   subtractOriginFromPoses.
//   toGeoTiff / writeDataToDEMGeoTiffColor (:349-509) -- the same files without
//     GDAL (amhip_geotiff_write_u8: baseline TIFF + GeoTIFF tags).
//   loadImagesFromFile (:207-227) -- the cv::imread("<prefix><i>.jpg") per pose as one
//     batched baseline JPEG decoder on the GPU (amhip_io_decode_jpeg_frames): the pixels
//     libjpeg gives at its defaults; EXIF orientation is not applied; no imshow.
//   loadImagesFromFile(directory, image_names, ..) (:229-249) -- the
//     cv::imread("<directory><name>.png") per name as one batched PNG decoder on the GPU
//     (amhip_io_decode_png_frames): inflate as zlib defines it, the pixels Pillow gives; 8 bit,
//     not interlaced; gray from a colour file by libpng's rgb_to_gray rule (adopted, unpinned);
//     no imshow.
// The camera-rig loader (aslam YAML) and the format converters stay the reference's.
#ifndef AERIAL_MAPPER_HIP_IO_TYPES_H_
#define AERIAL_MAPPER_HIP_IO_TYPES_H_

#include <string>
#include <vector>

#include "aerial-mapper-deps.h"
#include "aerial-mapper-utils/utils-nearest-neighbor.h"

typedef kindr::minimal::QuatTransformation Pose;
typedef std::vector<Pose> Poses;
typedef cv::Mat Image;
typedef std::vector<Image> Images;

namespace io {

enum PoseFormat { Standard, COLMAP, PIX4D, ROS };

class AerialMapperIO {
 public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW
  AerialMapperIO() {}

  void loadPosesFromFileStandard(const std::string& filename, Poses* T_G_Bs);

  void loadPointCloudFromFile(const std::string& filename_point_cloud,
                              AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud_xyz,
                              std::vector<int>* point_cloud_intensities);

  void loadPointCloudFromFile(const std::string& filename_point_cloud,
                              AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud_xyz);

  void subtractOriginFromPoses(const Eigen::Vector3d& origin, Poses* T_G_Bs);

  // <filename_base><i>.jpg, i = 0 .. num_poses - 1, decoded on the GPU and appended to *images
  // (8UC1, or 8UC3 B, G, R).  A missing or undecodable file is fatal.
  void loadImagesFromFile(const std::string& filename_base, size_t num_poses, Images* images,
                          bool load_colored_images = false);

  // <directory><name>.png for every name, decoded on the GPU and appended to *images (8UC1, or
  // 8UC3 B, G, R).  A missing or refused file is fatal and named.
  void loadImagesFromFile(const std::string& directory, std::vector<std::string> image_names,
                          Images* images, bool load_colored_images = false);

  void writeDataToDEMGeoTiffColor(const cv::Mat& ortho_image, const Eigen::Vector2d& xy,
                                  const std::string& geotiff_filename);

  void toGeoTiff(const cv::Mat& orthomosaic, const Eigen::Vector2d& xy,
                 const std::string& geotiff_filename);

  // --- extension: keep the parsed cloud in HBM (3 * n doubles AoS + n int32,
  // the layout of amhip_dsm_process_dev / amhip_ortho_from_pcl_process_dev);
  // release both with amhip_io_free().
  void loadPointCloudFromFileToDevice(const std::string& filename_point_cloud, double** dev_xyz,
                                      int32_t** dev_intensities, size_t* num_points);

  // --- extension: keep the decoded frames in HBM as one stack (frame f at *dev_frames + f *
  // *frame_stride, rows *row_step bytes apart: the layout amhip_ortho_backward_process_dev,
  // amhip_mosaic_batch_dev and amhip_stereo_add_frames_dev take); release with amhip_io_free().
  void loadImagesFromFileToDevice(const std::string& filename_base, size_t num_poses,
                                  bool load_colored_images, uint8_t** dev_frames, int* width, int* height,
                                  size_t* row_step, size_t* frame_stride);

  // --- extension: the same for the .png overload.
  void loadImagesFromFileToDevice(const std::string& directory,
                                  const std::vector<std::string>& image_names,
                                  bool load_colored_images, uint8_t** dev_frames, int* width, int* height,
                                  size_t* row_step, size_t* frame_stride);

  // --- extension: the same cloud as a binary file (amhip_io_write_point_cloud_binary) and its
  // loader, staged through pinned buffers straight into HBM.
  void savePointCloudToBinaryFile(const std::string& filename,
                                  const AlignedType<std::vector, Eigen::Vector3d>::type& point_cloud_xyz,
                                  const std::vector<int>& point_cloud_intensities);
  void loadPointCloudFromBinaryFileToDevice(const std::string& filename, double** dev_xyz,
                                            int32_t** dev_intensities, size_t* num_points);
};

}  // namespace io

#endif  // AERIAL_MAPPER_HIP_IO_TYPES_H_
