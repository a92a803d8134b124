// shim_write_images.cc -- the drop-in io::AerialMapperIO members that write frames as JPEG files, one
// batched encode on the GPU behind the reference's signatures:
//   shim_write_images <src/> <dst/> <pix4d> <again/>
// runs toStandardFormat on the simulated dataset in <src/> (-> <dst/>opt_poses.txt, <dst/>image_<i>.jpg),
// loadPosesFromFile on the poses it wrote, exportPix4dGeofile(poses, the images loaded back, <pix4d>), and
// loadImagesFromFileToDevice + writeImagesToFileFromDevice (-> <again/>again_<i>.jpg).
// tests/test_gpu_cpp_write_images.py compares every file with what the Python mirrors wrote.  A pose
// missing in <src/> or a <pix4d> that does not exist ends the program through the shim's fatal path.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "aerial-mapper-io/aerial-mapper-io.h"
#include "aerial_mapper_hip.h"

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: shim_write_images <src/> <dst/> <pix4d> <again/>\n");
    return 2;
  }
  const std::string src = argv[1], dst = argv[2], pix4d = argv[3], again = argv[4];
  io::AerialMapperIO io_handler;
  io_handler.toStandardFormat(src, "vi_imu_poses.csv", "blender_id_time.csv", dst);

  Poses poses;
  io_handler.loadPosesFromFile(io::PoseFormat::Standard, dst + "opt_poses.txt", &poses);
  if (poses.empty()) return 1;
  const size_t n = poses.size();

  Images images;
  io_handler.loadImagesFromFile(dst + "image_", n, &images);
  if (images.size() != n) return 1;
  io_handler.exportPix4dGeofile(poses, images, pix4d);

  uint8_t* dev = nullptr;
  int w = 0, h = 0;
  size_t row_step = 0, frame_stride = 0;
  io_handler.loadImagesFromFileToDevice(dst + "image_", n, false, &dev, &w, &h, &row_step, &frame_stride);
  std::vector<std::string> names;
  for (size_t i = 0; i < n; ++i) names.push_back(again + "again_" + std::to_string(i) + ".jpg");
  io_handler.writeImagesToFileFromDevice(dev, n, w, h, 1, row_step, frame_stride, names, 50);
  if (amhip_io_free(dev) != AMHIP_OK) return 1;

  std::vector<int64_t> stamps;
  Poses ros;
  io_handler.loadPosesFromFileRos(src + "vi_imu_poses.csv", &ros, &stamps);
  std::printf("wrote %zu images of %d x %d; %zu ros poses, first timestamp %lld\n", n, w, h, ros.size(),
              static_cast<long long>(stamps[0]));
  return 0;
}
