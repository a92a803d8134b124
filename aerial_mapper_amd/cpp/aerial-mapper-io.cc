// io::AerialMapperIO's text and image loaders, format converters and image writers over the C ABI
// (see include/aerial-mapper-io/aerial-mapper-io.h).
#include "aerial-mapper-io/aerial-mapper-io.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <memory>
#include <string>
#include <vector>

#include "shim_common.h"

namespace io {

namespace {

// read-only mapping of a whole file (the parser wants the bytes, not a stream)
struct MappedFile {
  const char* data;
  size_t size;
  int fd;
  explicit MappedFile(const std::string& name) : data(nullptr), size(0), fd(-1) {
    fd = ::open(name.c_str(), O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (::fstat(fd, &st) != 0 || st.st_size <= 0) return;
    void* p = ::mmap(nullptr, static_cast<size_t>(st.st_size), PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) return;
    data = static_cast<const char*>(p);
    size = static_cast<size_t>(st.st_size);
    ::close(fd);   // (the mapping stays: loadImagesFromFile maps one file per pose, any number of them)
    fd = -1;
  }
  ~MappedFile() {
    if (data) ::munmap(const_cast<char*>(data), size);
    if (fd >= 0) ::close(fd);
  }
};

int device_index() {
  return amhip_shim::default_device();
}

}  // namespace

void AerialMapperIO::loadPointCloudFromFileToDevice(const std::string& filename_point_cloud,
                                                    double** dev_xyz, int32_t** dev_intensities,
                                                    size_t* num_points) {
  if (filename_point_cloud.empty())
    amhip_shim::fatal("loadPointCloudFromFile", "CHECK(filename_point_cloud != \"\")");
  if (!dev_xyz || !dev_intensities || !num_points)
    amhip_shim::fatal("loadPointCloudFromFile", "CHECK(point_cloud_xyz)");
  std::fprintf(stderr, "[aerial_mapper_hip] Loading pointcloud from: %s\n",
               filename_point_cloud.c_str());
  MappedFile file(filename_point_cloud);
  size_t slow = 0;
  amhip_shim::check_status(
      amhip_io_parse_point_cloud_text(device_index(), file.data, file.size, dev_xyz,
                                      dev_intensities, num_points, &slow),
      "loadPointCloudFromFile");
  if (*num_points == 0)
    amhip_shim::fatal("loadPointCloudFromFile", "CHECK(point_cloud_xyz->size() > 0)");
}

void AerialMapperIO::loadPointCloudFromFile(
    const std::string& filename_point_cloud,
    AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud_xyz,
    std::vector<int>* point_cloud_intensities) {
  if (!point_cloud_xyz) amhip_shim::fatal("loadPointCloudFromFile", "CHECK(point_cloud_xyz)");
  if (!point_cloud_intensities)
    amhip_shim::fatal("loadPointCloudFromFile", "CHECK(point_cloud_intensities)");
  double* dxyz = nullptr;
  int32_t* dint = nullptr;
  size_t n = 0;
  loadPointCloudFromFileToDevice(filename_point_cloud, &dxyz, &dint, &n);
  // the reference push_back()s: append to whatever the vectors hold
  static_assert(sizeof(Eigen::Vector3d) == 3 * sizeof(double), "Vector3d must be 3 packed doubles");
  static_assert(sizeof(int) == sizeof(int32_t), "int must be 32 bits");
  const size_t at = point_cloud_xyz->size(), at_i = point_cloud_intensities->size();
  point_cloud_xyz->resize(at + n);
  point_cloud_intensities->resize(at_i + n);
  amhip_shim::check_status(
      amhip_io_download_point_cloud(dxyz, dint, n,
                                    reinterpret_cast<double*>(point_cloud_xyz->data() + at),
                                    reinterpret_cast<int32_t*>(point_cloud_intensities->data() + at_i)),
      "loadPointCloudFromFile");
  amhip_io_free(dxyz);
  amhip_io_free(dint);
}

void AerialMapperIO::loadPointCloudFromFile(
    const std::string& filename_point_cloud,
    AlignedType<std::vector, Eigen::Vector3d>::type* point_cloud_xyz) {
  std::vector<int> intensities;
  loadPointCloudFromFile(filename_point_cloud, point_cloud_xyz, &intensities);
}

namespace {

typedef int (*DecodeFrames)(int, const uint8_t* const*, const size_t*, size_t, int, uint8_t**, int*, int*,
                            size_t*, size_t*);

// aerial-mapper-io.cc:207-227: cv::imread(filename_base + std::to_string(i) + ".jpg") per pose
std::vector<std::string> jpg_names(const std::string& filename_base, size_t num_poses) {
  std::vector<std::string> names;
  for (size_t i = 0; i < num_poses; ++i) names.push_back(filename_base + std::to_string(i) + ".jpg");
  return names;
}

// aerial-mapper-io.cc:229-249: cv::imread(directory + image_names[i] + ".png") per name
std::vector<std::string> png_names(const std::string& directory, const std::vector<std::string>& image_names) {
  std::vector<std::string> names;
  for (const std::string& name : image_names) names.push_back(directory + name + ".png");
  return names;
}

// every file mapped and handed to the decoder: one stack in HBM
void decode_files(const std::vector<std::string>& names, const char* none, DecodeFrames decode,
                  bool load_colored_images, uint8_t** dev_frames, int* width, int* height, size_t* row_step,
                  size_t* frame_stride) {
  if (!dev_frames || !width || !height || !row_step || !frame_stride)
    amhip_shim::fatal("loadImagesFromFile", "CHECK(images)");
  if (names.empty()) amhip_shim::fatal("loadImagesFromFile", none);
  std::vector<std::unique_ptr<MappedFile> > mapped;
  std::vector<const uint8_t*> files;
  std::vector<size_t> lens;
  for (const std::string& name : names) {
    mapped.emplace_back(new MappedFile(name));
    if (!mapped.back()->data)
      amhip_shim::fatal("loadImagesFromFile", ("cannot read " + name).c_str());
    files.push_back(reinterpret_cast<const uint8_t*>(mapped.back()->data));
    lens.push_back(mapped.back()->size);
  }
  const int rc = decode(device_index(), files.data(), lens.data(), files.size(), load_colored_images ? 1 : 0,
                        dev_frames, width, height, row_step, frame_stride);
  if (rc != AMHIP_OK) {
    // the library names the frame; the caller knows files: name the file as well
    const std::string text = amhip_last_error();
    const size_t at = text.find("frame ");
    std::string file;
    if (at != std::string::npos) {
      const size_t k = static_cast<size_t>(std::strtoul(text.c_str() + at + 6, nullptr, 10));
      if (k < names.size()) file = " (" + names[k] + ")";
    }
    amhip_shim::fatal("loadImagesFromFile", (text + file).c_str());
  }
}

// ... downloaded and appended to *images as cv::Mats
void load_files(const std::vector<std::string>& names, const char* none, DecodeFrames decode,
                bool load_colored_images, Images* images) {
  if (!images) amhip_shim::fatal("loadImagesFromFile", "CHECK(images)");
  uint8_t* dev = nullptr;
  int w = 0, h = 0;
  size_t row_step = 0, frame_stride = 0;
  decode_files(names, none, decode, load_colored_images, &dev, &w, &h, &row_step, &frame_stride);
  const int ch = load_colored_images ? 3 : 1;
  std::vector<uint8_t> host(names.size() * frame_stride);
  amhip_shim::check_status(amhip_io_download_frames(dev, host.size(), host.data()), "loadImagesFromFile");
  amhip_io_free(dev);
  for (size_t i = 0; i < names.size(); ++i) {
#if AERIAL_MAPPER_REAL_DEPS
    cv::Mat image(h, w, load_colored_images ? CV_8UC3 : CV_8UC1);
#else
    cv::Mat image(h, w, ch);
#endif
    for (int y = 0; y < h; ++y)
      std::memcpy(image.data + static_cast<size_t>(y) * image.step,
                  host.data() + i * frame_stride + static_cast<size_t>(y) * row_step,
                  static_cast<size_t>(w) * ch);
    images->push_back(image);   // (the reference push_back()s: append)
  }
}

const char kNoPoses[] = "no poses: no images to load";
const char kNoNames[] = "no image names: no images to load";

}  // namespace

void AerialMapperIO::loadImagesFromFileToDevice(const std::string& filename_base, size_t num_poses,
                                                bool load_colored_images, uint8_t** dev_frames,
                                                int* width, int* height, size_t* row_step,
                                                size_t* frame_stride) {
  decode_files(jpg_names(filename_base, num_poses), kNoPoses, amhip_io_decode_jpeg_frames, load_colored_images,
               dev_frames, width, height, row_step, frame_stride);
}

void AerialMapperIO::loadImagesFromFileToDevice(const std::string& directory,
                                                const std::vector<std::string>& image_names,
                                                bool load_colored_images, uint8_t** dev_frames,
                                                int* width, int* height, size_t* row_step,
                                                size_t* frame_stride) {
  decode_files(png_names(directory, image_names), kNoNames, amhip_io_decode_png_frames, load_colored_images,
               dev_frames, width, height, row_step, frame_stride);
}

void AerialMapperIO::loadImagesFromFile(const std::string& directory, std::vector<std::string> image_names,
                                        Images* images, bool load_colored_images) {
  load_files(png_names(directory, image_names), kNoNames, amhip_io_decode_png_frames, load_colored_images, images);
}

void AerialMapperIO::loadImagesFromFile(const std::string& filename_base, size_t num_poses,
                                        Images* images, bool load_colored_images) {
  load_files(jpg_names(filename_base, num_poses), kNoPoses, amhip_io_decode_jpeg_frames, load_colored_images,
             images);
}

void AerialMapperIO::loadPosesFromFileStandard(const std::string& filename, Poses* T_G_Bs) {
  if (!T_G_Bs) amhip_shim::fatal("loadPosesFromFileStandard", "CHECK(T_G_Bs)");
  if (filename.empty()) amhip_shim::fatal("loadPosesFromFileStandard", "Empty filename");
  std::fprintf(stderr, "[aerial_mapper_hip] Loading body poses from: %s\n", filename.c_str());
  std::ifstream infile(filename);
  double x, y, z, qw, qx, qy, qz;
  while (infile >> x >> y >> z >> qw >> qx >> qy >> qz) {
    T_G_Bs->push_back(Pose(kindr::minimal::RotationQuaternion(qw, qx, qy, qz),
                           Eigen::Vector3d(x, y, z)));
    if (infile.eof()) break;
  }
  if (T_G_Bs->empty()) amhip_shim::fatal("loadPosesFromFileStandard", "No poses loaded.");
}

void AerialMapperIO::loadPosesFromFile(const PoseFormat& format, const std::string& filename, Poses* T_G_Bs) {
  if (!T_G_Bs) amhip_shim::fatal("loadPosesFromFile", "CHECK(T_G_Bs)");
  if (filename.empty()) amhip_shim::fatal("loadPosesFromFile", "Empty filename");
  switch (format) {
    case PoseFormat::Standard:
      loadPosesFromFileStandard(filename, T_G_Bs);
      break;
    case PoseFormat::COLMAP:
    case PoseFormat::PIX4D:
      amhip_shim::fatal("loadPosesFromFile", "Not yet implemented!");
    case PoseFormat::ROS:   // (commented out in the reference's switch as well)
      break;
  }
}

void AerialMapperIO::loadPosesFromFileRos(const std::string& filename, Poses* T_G_Bs,
                                          std::vector<int64_t>* timestamps_ns) {
  if (!T_G_Bs) amhip_shim::fatal("loadPosesFromFileRos", "CHECK(T_G_Bs)");
  if (filename.empty()) amhip_shim::fatal("loadPosesFromFileRos", "Empty filename");
  if (!timestamps_ns) amhip_shim::fatal("loadPosesFromFileRos", "CHECK(timestamps_ns)");
  std::fprintf(stderr, "[aerial_mapper_hip] Loading body poses from: %s\n", filename.c_str());
  std::ifstream infile(filename);
  double x, y, z, qw, qx, qy, qz;
  double timestamp_ns;
  while (infile >> timestamp_ns >> x >> y >> z >> qx >> qy >> qz >> qw) {
    timestamps_ns->push_back(static_cast<int64_t>(timestamp_ns));
    T_G_Bs->push_back(Pose(kindr::minimal::RotationQuaternion(qw, qx, qy, qz), Eigen::Vector3d(x, y, z)));
    if (infile.eof()) break;
  }
  if (T_G_Bs->empty()) amhip_shim::fatal("loadPosesFromFileRos", "No poses loaded.");
  if (T_G_Bs->size() != timestamps_ns->size())
    amhip_shim::fatal("loadPosesFromFileRos", "CHECK(T_G_Bs->size() == timestamps_ns->size())");
}

void AerialMapperIO::writeImagesToFileFromDevice(const uint8_t* dev_frames, size_t F, int width, int height,
                                                 int channels, size_t row_step, size_t frame_stride,
                                                 const std::vector<std::string>& filenames, int quality) {
  if (filenames.size() != F) amhip_shim::fatal("writeImagesToFileFromDevice", "CHECK(filenames.size() == F)");
  std::vector<const char*> names;
  for (const std::string& name : filenames) names.push_back(name.c_str());
  amhip_shim::check_status(
      amhip_io_write_jpeg_frames(device_index(), dev_frames, 1, F, width, height, channels, row_step,
                                 frame_stride, quality, names.data()),
      "writeImagesToFileFromDevice");
}

void AerialMapperIO::writePngImagesToFileFromDevice(const uint8_t* dev_frames, size_t F, int width, int height,
                                                    int channels, size_t row_step, size_t frame_stride,
                                                    const std::vector<std::string>& filenames) {
  if (filenames.size() != F) amhip_shim::fatal("writePngImagesToFileFromDevice", "CHECK(filenames.size() == F)");
  std::vector<const char*> names;
  for (const std::string& name : filenames) names.push_back(name.c_str());
  amhip_shim::check_status(
      amhip_io_write_png_frames(device_index(), dev_frames, 1, F, width, height, channels, row_step,
                                frame_stride, names.data()),
      "writePngImagesToFileFromDevice");
}

void AerialMapperIO::convertFromSimulation() {
  toStandardFormat("/tmp/to_convert/", "vi_imu_poses.csv", "blender_id_time.csv", "/tmp/simulation2/");
}

void AerialMapperIO::toStandardFormat(const std::string& directory, const std::string& filename_vi_imu_poses,
                                      const std::string& filename_blender_id_time,
                                      const std::string& new_directory) {
  // all body poses with their timestamps
  Poses T_G_Bs;
  std::vector<int64_t> timestamps_ns;
  loadPosesFromFileRos(directory + filename_vi_imu_poses, &T_G_Bs, &timestamps_ns);
  // the images' names and timestamps
  std::ifstream infile(directory + filename_blender_id_time);
  double id, image_name;
  std::vector<std::string> image_names;
  std::vector<int64_t> image_timestamps;
  while (infile >> id >> image_name) {
    image_names.push_back(std::to_string(static_cast<int64_t>(image_name)));
    image_timestamps.push_back(static_cast<int64_t>(image_name) - 1);
    if (infile.eof()) break;
  }
  // every image's pose: the last one whose timestamp matches (the reference's loop has no break)
  Poses T_G_Bs_associated;
  for (size_t i = 0u; i < image_timestamps.size(); ++i) {
    bool found_pose_for_image = false;
    Pose T_G_B;
    for (size_t j = 0u; j < timestamps_ns.size(); ++j) {
      if (timestamps_ns[j] == image_timestamps[i]) {
        found_pose_for_image = true;
        T_G_B = T_G_Bs[j];
      }
    }
    if (!found_pose_for_image)
      amhip_shim::fatal("toStandardFormat", ("CHECK(found_pose_for_image): no pose at timestamp " +
                                             std::to_string(image_timestamps[i]) + " for image " +
                                             image_names[i] + ".png").c_str());
    T_G_Bs_associated.push_back(T_G_B);
  }
  std::ofstream fs;
  fs.open((new_directory + "opt_poses.txt").c_str());
  for (const Pose& T_G_B : T_G_Bs_associated) {
    double p[7];
    amhip_shim::pose_to7(T_G_B, p);
    fs << p[0] << " " << p[1] << " " << p[2] << " " << p[3] << " " << p[4] << " " << p[5] << " " << p[6]
       << std::endl;
  }
  fs.close();
  // cam0/<name>.png -> one stack in HBM -> image_<i>.jpg, no cv::Mat in between
  uint8_t* dev = nullptr;
  int w = 0, h = 0;
  size_t row_step = 0, frame_stride = 0;
  loadImagesFromFileToDevice(directory + "cam0/", image_names, false, &dev, &w, &h, &row_step, &frame_stride);
  std::vector<std::string> filenames;
  for (size_t i = 0u; i < image_names.size(); ++i)
    filenames.push_back(new_directory + "image_" + std::to_string(i) + ".jpg");
  writeImagesToFileFromDevice(dev, image_names.size(), w, h, 1, row_step, frame_stride, filenames);
  amhip_io_free(dev);
}

void AerialMapperIO::exportPix4dGeofile(const Poses& T_G_Cs, const Images& images) {
  exportPix4dGeofile(T_G_Cs, images, "/tmp/pix4d");
}

void AerialMapperIO::exportPix4dGeofile(const Poses& T_G_Cs, const Images& images,
                                        const std::string& output_directory) {
  if (images.size() != T_G_Cs.size())
    amhip_shim::fatal("exportPix4dGeofile", "CHECK(images.size() == T_G_Cs.size())");
  if (images.empty()) return;   // (the reference's loop does not run; geofile.txt is left empty)
  const int w = images[0].cols, h = images[0].rows, ch = images[0].channels();
  const size_t row = static_cast<size_t>(w) * ch, frame = row * h;
  // one tight stack, uploaded once
  std::vector<uint8_t> stack(images.size() * frame);
  std::vector<std::string> stems, filenames;
  for (size_t i = 0u; i < images.size(); ++i) {
    const Image& image = images[i];
    bool same = image.cols == w && image.rows == h && image.channels() == ch && image.data;
#if AERIAL_MAPPER_REAL_DEPS
    same = same && image.depth() == CV_8U;
#endif
    if (!same)
      amhip_shim::fatal("exportPix4dGeofile",
                        ("image " + std::to_string(i) + " differs from image 0 in size or type (" +
                         std::to_string(w) + " x " + std::to_string(h) + ", " + std::to_string(ch) +
                         " channels of 8 bits are expected)").c_str());
    for (int y = 0; y < h; ++y)
      std::memcpy(stack.data() + i * frame + static_cast<size_t>(y) * row,
                  image.data + static_cast<size_t>(y) * image.step, row);
    char number[32];
    std::snprintf(number, sizeof(number), "%010zu", i + 1);
    stems.push_back(std::string("image_") + number + ".jpeg");
    filenames.push_back(output_directory + "/" + stems.back());
  }
  std::vector<const char*> names;
  for (const std::string& name : filenames) names.push_back(name.c_str());
  amhip_shim::check_status(
      amhip_io_write_jpeg_frames(device_index(), stack.data(), 0, images.size(), w, h, ch, row, frame, 95,
                                 names.data()),
      "exportPix4dGeofile");
  std::ofstream fs;
  fs.open((output_directory + "/geofile.txt").c_str());
  for (size_t i = 0u; i < images.size(); ++i) {
    const Eigen::Vector3d& xyz = T_G_Cs[i].getPosition();
    fs << stems[i] << " " << std::setprecision(15) << xyz(0) << " " << std::setprecision(15) << xyz(1) << " "
       << std::setprecision(15) << xyz(2) << std::endl;
  }
  fs.close();
}

void AerialMapperIO::subtractOriginFromPoses(const Eigen::Vector3d& origin, Poses* T_G_Bs) {
  if (!T_G_Bs) amhip_shim::fatal("subtractOriginFromPoses", "CHECK(T_G_Bs)");
  if (T_G_Bs->empty()) amhip_shim::fatal("subtractOriginFromPoses", "CHECK(T_G_Bs->size() > 0u)");
  for (Pose& T : *T_G_Bs) {
    const Eigen::Vector3d& t = T.getPosition();
    T = Pose(T.getRotation(), Eigen::Vector3d(t(0) - origin(0), t(1) - origin(1), t(2) - origin(2)));
  }
}

// aerial-mapper-io.cc:349-431: one byte band; the geotransform is the constant the reference
// hard-codes (`xy` is not used there either), UTM 32 north on WGS 84.
void AerialMapperIO::toGeoTiff(const cv::Mat& orthomosaic, const Eigen::Vector2d& /*xy*/,
                               const std::string& geotiff_filename) {
  if (orthomosaic.empty() || orthomosaic.channels() != 1)
    amhip_shim::fatal("toGeoTiff", "an 8UC1 image is expected (orthomosaic.at<uchar>)");
  const double gt[6] = {464499.00, 1.0, 0.0, 5.2727e+06, 0.0, -1.0};
  amhip_shim::check_status(
      amhip_geotiff_write_u8(geotiff_filename.c_str(), orthomosaic.data, orthomosaic.cols,
                             orthomosaic.rows, orthomosaic.step, 1, gt, 32, 1),
      "toGeoTiff");
}

// aerial-mapper-io.cc:433-509: three byte bands, band 1 / 2 / 3 = channel 2 / 0 / 1 of the
// cv::Vec3b pixel (the reference's "TODO: Fix color bands"), unit pixels anchored at xy.
void AerialMapperIO::writeDataToDEMGeoTiffColor(const cv::Mat& ortho_image,
                                                const Eigen::Vector2d& xy,
                                                const std::string& geotiff_filename) {
  if (ortho_image.empty() || ortho_image.channels() != 3)
    amhip_shim::fatal("writeDataToDEMGeoTiffColor", "an 8UC3 image is expected (at<cv::Vec3b>)");
  const int w = ortho_image.cols, h = ortho_image.rows;
  std::vector<uint8_t> bands(static_cast<size_t>(w) * h * 3);
  for (int y = 0; y < h; ++y) {
    const uint8_t* src = ortho_image.data + static_cast<size_t>(y) * ortho_image.step;
    uint8_t* dst = bands.data() + static_cast<size_t>(y) * w * 3;
    for (int x = 0; x < w; ++x) {
      dst[3 * x + 0] = src[3 * x + 2];
      dst[3 * x + 1] = src[3 * x + 0];
      dst[3 * x + 2] = src[3 * x + 1];
    }
  }
  const double gt[6] = {xy(0), 1.0, 0.0, xy(1), 0.0, -1.0};
  amhip_shim::check_status(
      amhip_geotiff_write_u8(geotiff_filename.c_str(), bands.data(), w, h,
                             static_cast<size_t>(w) * 3, 3, gt, 32, 1),
      "writeDataToDEMGeoTiffColor");
}

// extension: see the header.  The session's windows get the map's own matrix first (a session that was
// made for this call knows nothing of it yet), then the whole map is written from them.
void AerialMapperIO::writeLayerToGeoTiff(const grid_map::GridMap& map, const std::string& layer,
                                         const std::string& filename, int utm_zone, bool northern) {
  writeLayerToGeoTiff(map, layer, filename, utm_zone, northern, 0);
}

void AerialMapperIO::writeLayerToGeoTiff(const grid_map::GridMap& map, const std::string& layer,
                                         const std::string& filename, int utm_zone, bool northern, int overviews) {
  static const char* const kLayers[AMHIP_NUM_LAYERS] = {"ortho", "elevation", "elevation_angle", "num_observations",
                                                        "observation_index", "colored_ortho"};
  int id = -1;
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l)
    if (layer == kLayers[l]) id = l;
  if (id < 0 || !map.exists(layer))
    amhip_shim::fatal("writeLayerToGeoTiff", ("no layer '" + layer + "' the GPU path holds").c_str());
  const grid_map::Matrix& m = map[layer];
  const size_t rows = static_cast<size_t>(m.rows());
  amhip_session* session = amhip_shim::acquire_session(map, nullptr, "writeLayerToGeoTiff");
  std::vector<float> block;
  for (int k = 0; k < amhip_session_num_windows(session); ++k) {
    int32_t w[4];   // i0, j0, rows, cols
    amhip_shim::check_status(amhip_session_window(session, k, w), "writeLayerToGeoTiff");
    block.resize(static_cast<size_t>(w[2]) * w[3]);
    for (int j = 0; j < w[3]; ++j)
      std::memcpy(block.data() + static_cast<size_t>(j) * w[2], m.data() + w[0] + (static_cast<size_t>(w[1]) + j) * rows,
                  sizeof(float) * w[2]);
    amhip_shim::check_status(amhip_layer_upload(amhip_session_context(session, k), id, block.data()),
                             "writeLayerToGeoTiff");
  }
  const int kind = id == AMHIP_LAYER_COLORED_ORTHO ? AMHIP_GEOTIFF_RGB8 : AMHIP_GEOTIFF_F32;
  const int status =
      overviews == 0 ? amhip_session_layer_write_geotiff(session, id, kind, 0.0f, 255.0f, 0, utm_zone, northern ? 1 : 0,
                                                         filename.c_str())
                     : amhip_session_layer_write_geotiff_ovr(session, id, kind, 0.0f, 255.0f, 0, overviews, utm_zone,
                                                             northern ? 1 : 0, filename.c_str());
  amhip_shim::release_session(session);
  amhip_shim::check_status(status, "writeLayerToGeoTiff");
}

// extension: see the header.  The session takes the map's own matrix in as the layer's state (cells the
// file does not reach keep it), places the file's pixels on the GPU and hands the matrix back.
void AerialMapperIO::loadLayerFromGeoTiff(grid_map::GridMap* map, const std::string& layer,
                                          const std::string& filename) {
  loadLayerFromGeoTiff(map, layer, filename, 0);
}

void AerialMapperIO::loadLayerFromGeoTiff(grid_map::GridMap* map, const std::string& layer,
                                          const std::string& filename, int level) {
  static const char* const kLayers[AMHIP_NUM_LAYERS] = {"ortho", "elevation", "elevation_angle", "num_observations",
                                                        "observation_index", "colored_ortho"};
  int id = -1;
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l)
    if (layer == kLayers[l]) id = l;
  if (!map || id < 0 || !map->exists(layer))
    amhip_shim::fatal("loadLayerFromGeoTiff", ("no layer '" + layer + "' the GPU path holds").c_str());
  grid_map::Matrix& m = (*map)[layer];
  amhip_session* session = amhip_shim::acquire_session(*map, nullptr, "loadLayerFromGeoTiff");
  const int status = level == 0 ? amhip_session_layer_read_geotiff(session, id, filename.c_str(), m.data())
                                : amhip_session_layer_read_geotiff_level(session, id, filename.c_str(), level, m.data());
  amhip_shim::release_session(session);
  amhip_shim::check_status(status, "loadLayerFromGeoTiff");
}

void AerialMapperIO::savePointCloudToBinaryFile(
    const std::string& filename,
    const AlignedType<std::vector, Eigen::Vector3d>::type& point_cloud_xyz,
    const std::vector<int>& point_cloud_intensities) {
  static_assert(sizeof(Eigen::Vector3d) == 3 * sizeof(double), "Vector3d must be 3 packed doubles");
  if (!point_cloud_intensities.empty() && point_cloud_intensities.size() != point_cloud_xyz.size())
    amhip_shim::fatal("savePointCloudToBinaryFile", "CHECK(xyz.size() == intensities.size())");
  amhip_shim::check_status(
      amhip_io_write_point_cloud_binary(
          filename.c_str(), reinterpret_cast<const double*>(point_cloud_xyz.data()),
          point_cloud_intensities.empty()
              ? nullptr
              : reinterpret_cast<const int32_t*>(point_cloud_intensities.data()),
          point_cloud_xyz.size()),
      "savePointCloudToBinaryFile");
}

void AerialMapperIO::loadPointCloudFromBinaryFileToDevice(const std::string& filename,
                                                          double** dev_xyz,
                                                          int32_t** dev_intensities,
                                                          size_t* num_points) {
  amhip_shim::check_status(
      amhip_io_load_point_cloud_binary(device_index(), filename.c_str(), dev_xyz, dev_intensities,
                                       num_points),
      "loadPointCloudFromBinaryFileToDevice");
  if (*num_points == 0)
    amhip_shim::fatal("loadPointCloudFromBinaryFileToDevice", "CHECK(point_cloud_xyz->size() > 0)");
}

}  // namespace io
