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
//   loadPosesFromFile (:35-56), loadPosesFromFileRos (:58-101) -- read on the host.
//   toStandardFormat / convertFromSimulation (:123-205) and exportPix4dGeofile (:272-307) -- their
//     loops of cv::imwrite as ONE batched baseline JPEG encode on the GPU
//     (amhip_io_write_jpeg_frames): the files libjpeg writes at cv::imwrite's quality 95;
//     toStandardFormat's frames go from the PNG decoder's stack in HBM straight into the encoder;
//     no imshow / waitKey.
// The camera-rig loader (aslam YAML) stays the reference's.
#ifndef AERIAL_MAPPER_HIP_IO_TYPES_H_
#define AERIAL_MAPPER_HIP_IO_TYPES_H_

#include <cstdint>
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

  // Standard: loadPosesFromFileStandard; COLMAP and PIX4D are fatal ("Not yet implemented!")
  void loadPosesFromFile(const PoseFormat& format, const std::string& filename, Poses* T_G_Bs);

  void loadPosesFromFileStandard(const std::string& filename, Poses* T_G_Bs);

  // records `time x y z qx qy qz qw`; the time is read as a double and stored as int64_t
  void loadPosesFromFileRos(const std::string& filename, Poses* T_G_Bs,
                            std::vector<int64_t>* timestamps_ns);

  // toStandardFormat("/tmp/to_convert/", "vi_imu_poses.csv", "blender_id_time.csv", "/tmp/simulation2/")
  void convertFromSimulation();

  // <directory><filename_vi_imu_poses> (loadPosesFromFileRos) and <directory><filename_blender_id_time>
  // (`id name` pairs, the image's timestamp is name - 1) -> <new_directory>opt_poses.txt (the pose of
  // every image, `x y z qw qx qy qz`) and <new_directory>image_<i>.jpg, <directory>cam0/<name>.png
  // decoded and encoded again on the GPU.  An image without a pose is fatal.
  void toStandardFormat(const std::string& directory, const std::string& filename_vi_imu_poses,
                        const std::string& filename_blender_id_time, const std::string& new_directory);

  // /tmp/pix4d/image_%010d.jpeg, numbered from 1, and /tmp/pix4d/geofile.txt (`image_<n>.jpeg x y z`).
  // The images go to the device once, as one stack, and are encoded in one batch; they must agree in
  // size and type (fatal, naming the image).  The directory is not created.
  void exportPix4dGeofile(const Poses& T_G_Cs, const Images& images);
  // --- extension: the same into another directory
  void exportPix4dGeofile(const Poses& T_G_Cs, const Images& images, const std::string& output_directory);

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

  // --- extension: the twin of loadImagesFromFileToDevice: F frames of a stack in HBM (8UC1 or 8UC3
  // B, G, R) -> filenames[f], one batched JPEG encode (amhip_io_write_jpeg_frames).  A file that
  // cannot be written is fatal and named; the files before it stay.
  void writeImagesToFileFromDevice(const uint8_t* dev_frames, size_t F, int width, int height, int channels,
                                   size_t row_step, size_t frame_stride,
                                   const std::vector<std::string>& filenames, int quality = 95);

  // --- extension: its PNG twin (amhip_io_write_png_frames): the files cv::imwrite writes for names
  // that end in .png, without loss.  A twin and not a dispatch on each name: a call is one batched
  // encode with one codec, and writeImagesToFileFromDevice keeps writing JPEG whatever the names say.
  void writePngImagesToFileFromDevice(const uint8_t* dev_frames, size_t F, int width, int height, int channels,
                                      size_t row_step, size_t frame_stride,
                                      const std::vector<std::string>& filenames);

  // --- extension: a layer of the map as a GeoTIFF GIS tools read as it is: north-up (x easting, y
  // northing), georeferenced from the map's own geometry in UTM zone `utm_zone`, tiled and
  // Deflate-compressed on the GPU (amhip_session_layer_write_geotiff).  "colored_ortho" goes as
  // three byte bands R, G, B; every other layer of the GPU path ("elevation", "ortho",
  // "elevation_angle", "num_observations", "observation_index") as 32-bit floats with nodata NaN.
  // The map's matrices are what is written: they are uploaded to the map's session first.  The
  // reference has no such writer (its two GDAL calls write uncompressed bytes); any other layer name
  // and a file that cannot be written are fatal.
  void writeLayerToGeoTiff(const grid_map::GridMap& map, const std::string& layer, const std::string& filename,
                           int utm_zone, bool northern);
  // ... with overviews (amhip_session_layer_write_geotiff_ovr): `overviews` levels behind the raster, each
  // half the one before it, reduced on the GPU; -1: until a level fits one tile; 0: the file above.
  void writeLayerToGeoTiff(const grid_map::GridMap& map, const std::string& layer, const std::string& filename,
                           int utm_zone, bool northern, int overviews);

  // --- extension: the other way.  A Deflate GeoTIFF -- what writeLayerToGeoTiff wrote, or a terrain model
  // from elsewhere -- under a layer of the map, decoded on the GPU (amhip_session_layer_read_geotiff): a
  // cell takes the pixel its centre lies in; a cell outside the raster, on a nodata pixel or on a NaN keeps
  // the map's value.  Nothing is resampled or reprojected: the file has to be in the map's coordinates.
  // One band goes to any layer of the GPU path, three bands of bytes to "colored_ortho" only.  A file
  // the reader refuses, or one that fails to decode, is fatal with the library's text; the map is then
  // as it was.
  void loadLayerFromGeoTiff(grid_map::GridMap* map, const std::string& layer, const std::string& filename);
  // ... from a level of the file's pyramid (amhip_session_layer_read_geotiff_level): 0 the raster itself,
  // k its k-th overview, -1 the coarsest level whose pixels are no larger than the map's cells.
  void loadLayerFromGeoTiff(grid_map::GridMap* map, const std::string& layer, const std::string& filename, int level);

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
