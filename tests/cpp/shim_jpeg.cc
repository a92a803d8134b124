// shim_jpeg.cc -- the drop-in ortho::OrthoForwardHomography writes the file its settings name:
// batch() with filename_mosaic_output = argv[1] must leave a JPEG file there (encoded on the GPU
// from the device-resident result_) and the 8-bit mosaic as <name>.ppm beside it, as before.
// tests/test_gpu_cpp_jpeg.py compares the two through tests/jpeg_reference.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "aerial-mapper-ortho/ortho-forward-homography.h"

static uint64_t g_state = 0x2545F4914F6CDD1DULL;
static double urand() {  // splitmix64 -> [0,1)
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return (z >> 11) * (1.0 / 9007199254740992.0);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: shim_jpeg <filename_mosaic_output> [colored]\n");
    return 2;
  }
  const bool colored = argc > 2 && std::string(argv[2]) == "colored";
  const int W = 160, H = 120, F = 6;
  aslam::Camera cam(120.0, 120.0, (W - 1) / 2.0, (H - 1) / 2.0, W, H);
  std::shared_ptr<aslam::NCamera> ncameras(new aslam::NCamera(
      cam, aslam::Transformation(kindr::minimal::RotationQuaternion(1, 0, 0, 0),
                                 Eigen::Vector3d(0.02, -0.01, 0.03))));
  ortho::Settings settings;
  settings.batch = true;
  settings.ground_plane_elevation_m = 402.0;
  settings.width_mosaic_pixels = 250;   // (neither a multiple of 16)
  settings.height_mosaic_pixels = 203;
  settings.origin = Eigen::Vector3d(5.0, -3.0, 0.0);
  settings.filename_mosaic_output = argv[1];
  const double s45 = std::sqrt(0.5);
  Poses T_G_Bs;
  Images images;
  for (int f = 0; f < F; ++f) {
    const double px = 5.0 - 40.0 + 14.0 * f;
    const double py = -3.0 + ((f % 3) - 1) * 20.0;
    double q[4] = {0.01 * (f - 3), s45, s45 + 0.004 * f, 0.003 * (3 - f)};
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    T_G_Bs.push_back(Pose(kindr::minimal::RotationQuaternion(q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq),
                          Eigen::Vector3d(px, py, 500.0)));
    Image img(H, W, colored ? 3 : 1);
    for (size_t b = 0; b < static_cast<size_t>(H) * img.step; ++b) {
      const int v = static_cast<int>(urand() * 256.0);
      img.data[b] = static_cast<uint8_t>(v < 5 ? 0 : v);
    }
    images.push_back(img);
  }
  ortho::OrthoForwardHomography mosaic(ncameras, settings);
  mosaic.batch(T_G_Bs, images);
  size_t covered = 0;
  for (uint8_t m : mosaic.result_mask()) covered += m != 0;
  std::printf("covered %zu of %d\n", covered, 250 * 203);
  return covered > 0 ? 0 : 1;
}
