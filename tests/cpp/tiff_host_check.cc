// tiff_host_check.cc -- the host-only part of the GeoTIFF encoder (amhip_tiff_host.h) as a
// stand-alone program: tests/test_geotiff_reference.py compiles it under the address and
// undefined-behaviour sanitizers and compares what it prints with tests/geotiff_reference.py.
//   head WIDTH HEIGHT KIND TILE ZONE NORTHERN GT0 .. GT5 COUNT...   the file in front of the tiles, in
//        hex, then the file's size; "refused" when the file would exceed 2^32 - 1 bytes
//   bound WIDTH HEIGHT KIND TILE                                     tiles, bytes in front, bound
//   args                                                             the argument checks, a line each
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_tiff_host.h"

using namespace amhip;

static int head(int argc, char** argv) {
  if (argc < 15) return 2;
  const int width = std::atoi(argv[2]), height = std::atoi(argv[3]), kind = std::atoi(argv[4]);
  const int tile = std::atoi(argv[5]), zone = std::atoi(argv[6]), northern = std::atoi(argv[7]);
  double gt[6];
  for (int k = 0; k < 6; ++k) gt[k] = std::strtod(argv[8 + k], nullptr);
  std::vector<uint64_t> counts;
  for (int k = 14; k < argc; ++k) counts.push_back(std::strtoull(argv[k], nullptr, 10));
  if (counts.size() != tiff::tile_count(width, height, tile)) return 3;
  const tiff::GeoTags geo = tiff::make_geo_tags(gt, zone, northern);
  tiff::Container c;
  if (!tiff::build_container(width, height, kind, tile, geo, counts.data(), counts.size(), &c)) {
    std::printf("refused\n");
    return c.head.empty() ? 0 : 4;   // (nothing built)
  }
  if (c.head.size() > tiff::head_bytes(kind, counts.size())) return 5;
  for (uint8_t b : c.head) std::printf("%02x", b);
  std::printf("\n%" PRIu64 "\n", c.file_bytes);
  return 0;
}

static void line(const char* why) { std::printf("%s\n", why ? why : "ok"); }

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "head")) return head(argc, argv);
  if (argc == 6 && !std::strcmp(argv[1], "bound")) {
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), kind = std::atoi(argv[4]), tile = std::atoi(argv[5]);
    const uint64_t n = tiff::tile_count(w, h, tile);
    std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, tiff::head_bytes(kind, n), tiff::file_bound(w, h, kind, tile));
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "args")) {
    const double up[6] = {1.0, 0.5, 0.0, 2.0, 0.0, -0.5}, rot[6] = {1.0, 0.5, 0.1, 2.0, 0.0, -0.5};
    const double flip[6] = {1.0, 0.5, 0.0, 2.0, 0.0, 0.5};
    line(tiff::check_raster(1, 1, 0, 0));
    line(tiff::check_raster(65535, 65535, 2, 1024));
    line(tiff::check_raster(0, 5, 0, 16));
    line(tiff::check_raster(5, 65536, 0, 16));
    line(tiff::check_raster(5, 5, 3, 16));
    line(tiff::check_raster(5, 5, -1, 16));
    line(tiff::check_raster(5, 5, 1, 8));
    line(tiff::check_raster(5, 5, 1, 24));
    line(tiff::check_raster(5, 5, 1, 1040));
    line(tiff::check_geo(up, 32));
    line(tiff::check_geo(rot, 32));
    line(tiff::check_geo(flip, 32));
    line(tiff::check_geo(up, 0));
    line(tiff::check_geo(up, 61));
    return 0;
  }
  return 2;
}
