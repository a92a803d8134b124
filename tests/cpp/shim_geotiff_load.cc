// The drop-in io::AerialMapperIO::loadLayerFromGeoTiff on a 33 x 47-cell map: writeLayerToGeoTiff of
// "elevation" and "colored_ortho", then loadLayerFromGeoTiff into a second map of the same geometry,
// then the matrices are compared bit for bit; a third map, shifted by three cells, keeps its own values
// where the file does not reach.  Prints "ok <rows> <cols> <cells the shifted map took>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "aerial-mapper-grid-map/aerial-mapper-grid-map.h"
#include "aerial-mapper-io/aerial-mapper-io.h"

static bool same_bits(const grid_map::Matrix& a, const grid_map::Matrix& b) {
  return a.rows() == b.rows() && a.cols() == b.cols() &&
         std::memcmp(a.data(), b.data(), sizeof(float) * a.rows() * a.cols()) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  grid_map::Settings st;
  st.center_easting = 464980.0;
  st.center_northing = 5272690.0;
  st.delta_easting = 16.5;
  st.delta_northing = 23.5;
  st.resolution = 0.5;
  grid_map::AerialGridMap source(st), target(st);
  grid_map::GridMap* m = source.getMutable();
  grid_map::Matrix& elevation = (*m)["elevation"];
  grid_map::Matrix& colour = (*m)["colored_ortho"];
  const int rows = (int)elevation.rows(), cols = (int)elevation.cols();
  unsigned s = 2025u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const bool hole = next() % 5 == 0;
      elevation(i, j) = hole ? std::numeric_limits<float>::quiet_NaN()
                             : 400.0f + 10.0f * std::sin(0.3f * i) * std::cos(0.2f * j);
      const unsigned rgb = next() & 0xFFFFFFu;
      float packed;
      std::memcpy(&packed, &rgb, 4);
      colour(i, j) = packed;
    }
  io::AerialMapperIO io_handler;
  io_handler.writeLayerToGeoTiff(*m, "elevation", dir + "/elevation.tif", 32, true);
  io_handler.writeLayerToGeoTiff(*m, "colored_ortho", dir + "/colored_ortho.tif", 32, true);
  grid_map::GridMap* t = target.getMutable();
  io_handler.loadLayerFromGeoTiff(t, "elevation", dir + "/elevation.tif");
  io_handler.loadLayerFromGeoTiff(t, "colored_ortho", dir + "/colored_ortho.tif");
  // (the holes: the fresh map's own NaN, the same bits as the source's quiet NaN)
  if (!same_bits((*t)["elevation"], elevation)) return std::printf("elevation differs\n"), 1;
  if (!same_bits((*t)["colored_ortho"], colour)) return std::printf("colored_ortho differs\n"), 1;
  // three cells to the east: map rows 0..2 lie outside the file and keep the sentinel
  st.center_easting += 1.5;
  grid_map::AerialGridMap shifted(st);
  grid_map::GridMap* q = shifted.getMutable();
  (*q)["elevation"].setConstant(-5.0f);
  io_handler.loadLayerFromGeoTiff(q, "elevation", dir + "/elevation.tif");
  int took = 0;
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const float got = (*q)["elevation"](i, j);
      // cell i of the shifted map is cell i - 3 of the source (x falls with i)
      const float want = i >= 3 && elevation(i - 3, j) == elevation(i - 3, j) ? elevation(i - 3, j) : -5.0f;
      if (std::memcmp(&got, &want, 4) != 0) return std::printf("shifted map differs at %d %d\n", i, j), 1;
      took += got != -5.0f;
    }
  std::printf("ok %d %d %d\n", rows, cols, took);
  return 0;
}
