// The drop-in io::AerialMapperIO::writeLayerToGeoTiff with overviews and loadLayerFromGeoTiff with a
// level, on a 66 x 94-cell map: writes <dir>/elevation.tif with two overviews, reads it back at level
// 1 and at the automatic level into maps of the same geometry whose heights are all NaN, and leaves
// the three matrices (<dir>/layers.bin: rows, cols as int32, then written, level 1, automatic) for
// tests/test_gpu_geotiff_pyramid.py to repeat through the Python calls.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>

#include "aerial-mapper-grid-map/aerial-mapper-grid-map.h"
#include "aerial-mapper-io/aerial-mapper-io.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  grid_map::Settings st;
  st.center_easting = 464980.0;
  st.center_northing = 5272690.0;
  st.delta_easting = 16.5;
  st.delta_northing = 23.5;
  st.resolution = 0.25;
  grid_map::AerialGridMap map(st), at_one(st), by_choice(st);
  grid_map::GridMap* m = map.getMutable();
  grid_map::Matrix& elevation = (*m)["elevation"];
  const int rows = (int)elevation.rows(), cols = (int)elevation.cols();
  unsigned s = 2025u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i)
      elevation(i, j) = next() % 5 == 0 ? nan : 400.0f + 10.0f * std::sin(0.3f * i) * std::cos(0.2f * j);
  io::AerialMapperIO io_handler;
  io_handler.writeLayerToGeoTiff(*m, "elevation", dir + "/elevation.tif", 32, true, 2);
  grid_map::Matrix& one = (*at_one.getMutable())["elevation"];
  grid_map::Matrix& choice = (*by_choice.getMutable())["elevation"];
  one.setConstant(nan);
  choice.setConstant(nan);
  io_handler.loadLayerFromGeoTiff(at_one.getMutable(), "elevation", dir + "/elevation.tif", 1);
  io_handler.loadLayerFromGeoTiff(by_choice.getMutable(), "elevation", dir + "/elevation.tif", -1);
  std::ofstream out(dir + "/layers.bin", std::ios::binary);
  const int32_t size[2] = {rows, cols};
  out.write((const char*)size, 8);
  out.write((const char*)elevation.data(), sizeof(float) * rows * cols);
  out.write((const char*)one.data(), sizeof(float) * rows * cols);
  out.write((const char*)choice.data(), sizeof(float) * rows * cols);
  std::printf("ok %d %d\n", rows, cols);
  return 0;
}
