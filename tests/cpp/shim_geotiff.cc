// The drop-in io::AerialMapperIO::writeLayerToGeoTiff on a 33 x 47-cell map: writes
// <dir>/elevation.tif, <dir>/colored_ortho.tif and the two layers they were made from
// (<dir>/layers.bin: rows, cols as int32, then the matrices as they lie in memory) for
// tests/test_gpu_geotiff.py to encode again through the Python call.
#include <cmath>
#include <cstdio>
#include <cstring>
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
  st.resolution = 0.5;
  grid_map::AerialGridMap map(st);
  grid_map::GridMap* m = map.getMutable();
  grid_map::Matrix& elevation = (*m)["elevation"];
  grid_map::Matrix& colour = (*m)["colored_ortho"];
  const int rows = (int)elevation.rows(), cols = (int)elevation.cols();
  unsigned s = 2024u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const bool hole = next() % 5 == 0;
      elevation(i, j) = hole ? std::numeric_limits<float>::quiet_NaN()
                             : 400.0f + 10.0f * std::sin(0.3f * i) * std::cos(0.2f * j);
      const unsigned rgb = next() & 0xFFFFFFu;
      float packed;
      std::memcpy(&packed, &rgb, 4);
      colour(i, j) = next() % 7 == 0 ? std::numeric_limits<float>::quiet_NaN() : packed;
    }
  io::AerialMapperIO io_handler;
  io_handler.writeLayerToGeoTiff(*m, "elevation", dir + "/elevation.tif", 32, true);
  io_handler.writeLayerToGeoTiff(*m, "colored_ortho", dir + "/colored_ortho.tif", 19, false);
  std::ofstream out(dir + "/layers.bin", std::ios::binary);
  const int32_t size[2] = {rows, cols};
  out.write((const char*)size, 8);
  out.write((const char*)elevation.data(), sizeof(float) * rows * cols);
  out.write((const char*)colour.data(), sizeof(float) * rows * cols);
  std::printf("ok %d %d\n", rows, cols);
  return 0;
}
