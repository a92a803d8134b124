// shim_write_images_png.cc -- the drop-in io::AerialMapperIO::writePngImagesToFileFromDevice, the PNG
// twin of writeImagesToFileFromDevice:
//   shim_write_images_png <base> <n> <colored> <out/>
// loads <base><i>.jpg for i < n with loadImagesFromFileToDevice and writes the stack, without its
// pixels leaving HBM, to <out/>frame_<i>.png.  tests/test_gpu_cpp_write_images_png.py compares the
// files with tests/png_encode_reference.py.  A file that cannot be written ends the program through
// the shim's fatal path.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "aerial-mapper-io/aerial-mapper-io.h"
#include "aerial_mapper_hip.h"

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: shim_write_images_png <base> <n> <colored> <out/>\n");
    return 2;
  }
  const std::string base = argv[1], out = argv[4];
  const size_t n = static_cast<size_t>(std::atoi(argv[2]));
  const bool colored = std::atoi(argv[3]) != 0;
  io::AerialMapperIO io_handler;
  uint8_t* dev = nullptr;
  int w = 0, h = 0;
  size_t row_step = 0, frame_stride = 0;
  io_handler.loadImagesFromFileToDevice(base, n, colored, &dev, &w, &h, &row_step, &frame_stride);
  std::vector<std::string> names;
  for (size_t i = 0; i < n; ++i) names.push_back(out + "frame_" + std::to_string(i) + ".png");
  io_handler.writePngImagesToFileFromDevice(dev, n, w, h, colored ? 3 : 1, row_step, frame_stride, names);
  if (amhip_io_free(dev) != AMHIP_OK) return 1;
  std::printf("wrote %zu images of %d x %d\n", n, w, h);
  return 0;
}
