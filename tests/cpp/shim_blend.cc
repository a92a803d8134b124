// shim_blend.cc -- ortho::OrthoBackwardGrid::setBlend through the drop-in class
// (tests/test_gpu_cpp_ortho_blend.py).  The scene comes in files, the layers go out in files:
//   shim_blend <dir> on|off <sharpness>
//   on: setBlend(true, sharpness); off: setBlend(true, sharpness), then setBlend(false)
//   reads  <dir>/elevation.f32 (cols x rows floats, the GridMap's column-major matrix),
//          <dir>/poses.f64 (F x 7: tx ty tz qw qx qy qz), <dir>/frames.u8 (F x 54 x 96 gray)
//   writes <dir>/<layer>.<on|off>.f32 for the five layers of the mosaic
// The map and the camera are those of tests/ortho_occlusion_scenes.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "aerial-mapper-grid-map/aerial-mapper-grid-map.h"
#include "aerial-mapper-ortho/ortho-backward-grid.h"

template <typename T>
static std::vector<T> read_all(const std::string& path) {
  std::vector<T> out;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::perror(path.c_str());
    std::exit(2);
  }
  T buf[4096];
  size_t n;
  while ((n = std::fread(buf, sizeof(T), 4096, f)) > 0) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

static void write_all(const std::string& path, const float* data, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(data, sizeof(float), n, f) != n) {
    std::perror(path.c_str());
    std::exit(2);
  }
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <dir> on|off <sharpness>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1], mode = argv[2];
  const bool on = mode == "on";
  const int sharpness = std::atoi(argv[3]);

  grid_map::Settings gs;
  gs.center_easting = 0.0;
  gs.center_northing = 0.0;
  gs.delta_easting = 40.0;
  gs.delta_northing = 36.0;
  gs.resolution = 0.5;
  grid_map::AerialGridMap map(gs);
  grid_map::GridMap* m = map.getMutable();
  const int rows = m->getSize()(0), cols = m->getSize()(1);
  const size_t cells = static_cast<size_t>(rows) * cols;
  const std::vector<float> elevation = read_all<float>(dir + "/elevation.f32");
  if (rows != 80 || cols != 72 || elevation.size() != cells) return 3;
  std::memcpy((*m)["elevation"].data(), elevation.data(), cells * sizeof(float));

  const int W = 96, H = 54;
  aslam::Camera cam(70.0, 70.0, 47.5, 26.5, W, H);
  std::shared_ptr<aslam::NCamera> ncameras(new aslam::NCamera(
      cam, aslam::Transformation(kindr::minimal::RotationQuaternion(1, 0, 0, 0), Eigen::Vector3d(0.0, 0.0, 0.0))));
  const std::vector<double> poses = read_all<double>(dir + "/poses.f64");
  const std::vector<uint8_t> pixels = read_all<uint8_t>(dir + "/frames.u8");
  const size_t F = poses.size() / 7;
  if (F == 0 || poses.size() != 7 * F || pixels.size() != F * W * H) return 4;
  Poses T_G_Bs;
  Images images;
  for (size_t f = 0; f < F; ++f) {
    const double* p = &poses[7 * f];
    T_G_Bs.push_back(Pose(kindr::minimal::RotationQuaternion(p[3], p[4], p[5], p[6]), Eigen::Vector3d(p[0], p[1], p[2])));
    Image img(H, W, 1);
    for (int v = 0; v < H; ++v) std::memcpy(img.data + v * img.step, &pixels[(f * H + v) * W], W);
    images.push_back(img);
  }
  ortho::Settings so;
  ortho::OrthoBackwardGrid mosaic(ncameras, so, m);
  mosaic.setBlend(true, sharpness);
  if (!on) mosaic.setBlend(false);   // (the plain mosaic again)
  mosaic.process(T_G_Bs, images, m);

  const char* layers[5] = {"elevation_angle", "observation_index", "num_observations", "ortho", "colored_ortho"};
  for (int l = 0; l < 5; ++l) write_all(dir + "/" + layers[l] + "." + mode + ".f32", (*m)[layers[l]].data(), cells);
  return 0;
}
