// shim_load_images_png.cc -- the drop-in io::AerialMapperIO::loadImagesFromFile(directory,
// image_names, ..) (PNG frames decoded on the GPU behind the reference's signature) and its ToDevice
// extension.
//   shim_load_images_png <directory> <gray|colored> <out> <name>...
// reads <directory><name>.png, writes "<width> <height> <channels> <count>\n" and the images' bytes
// row by row to <out>; tests/test_gpu_cpp_load_images_png.py compares them with
// tests/png_decode_reference.py.  The stack loadImagesFromFileToDevice leaves in HBM must hold the
// same bytes (checked here after a download).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aerial-mapper-io/aerial-mapper-io.h"
#include "aerial_mapper_hip.h"

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: shim_load_images_png <directory> <gray|colored> <out> <name>...\n");
    return 2;
  }
  const std::string directory = argv[1];
  const bool colored = std::string(argv[2]) == "colored";
  std::vector<std::string> names(argv + 4, argv + argc);
  const size_t n = names.size();
  io::AerialMapperIO loader;
  Images images;
  images.push_back(Image(2, 2, 1));   // the reference push_back()s: what is there stays in front
  loader.loadImagesFromFile(directory, names, &images, colored);
  if (images.size() != n + 1 || images[0].rows != 2) return 1;
  images.erase(images.begin());
  const int ch = colored ? 3 : 1;
  const int w = images[0].cols, h = images[0].rows;
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 1;
  std::fprintf(f, "%d %d %d %zu\n", w, h, ch, images.size());
  for (const Image& im : images) {
    if (im.cols != w || im.rows != h || im.channels() != ch) return 1;
    for (int y = 0; y < h; ++y)
      std::fwrite(im.data + static_cast<size_t>(y) * im.step, 1, static_cast<size_t>(w) * ch, f);
  }
  std::fclose(f);

  uint8_t* dev = nullptr;
  int dw = 0, dh = 0;
  size_t row_step = 0, frame_stride = 0;
  loader.loadImagesFromFileToDevice(directory, names, colored, &dev, &dw, &dh, &row_step, &frame_stride);
  if (!dev || dw != w || dh != h || row_step != static_cast<size_t>(w) * ch || frame_stride != row_step * h) return 1;
  std::vector<uint8_t> host(n * frame_stride);
  if (amhip_io_download_frames(dev, host.size(), host.data()) != AMHIP_OK) return 1;
  if (amhip_io_free(dev) != AMHIP_OK) return 1;
  for (size_t i = 0; i < n; ++i)
    for (int y = 0; y < h; ++y)
      if (std::memcmp(host.data() + i * frame_stride + static_cast<size_t>(y) * row_step,
                      images[i].data + static_cast<size_t>(y) * images[i].step, static_cast<size_t>(w) * ch) != 0) {
        std::fprintf(stderr, "device stack differs from the images: frame %zu row %d\n", i, y);
        return 1;
      }
  std::printf("loaded %zu images of %d x %d x %d\n", n, w, h, ch);
  return 0;
}
