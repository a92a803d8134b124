// amhip_tiff_host.h -- the part of the GeoTIFF writers that needs no device: the geo tags of a
// north-up UTM raster (shared by amhip_geotiff_write_u8, amhip_export.hip, and the tiled Deflate
// writer, amhip_tiff_encode.hip), the argument checks, and the container of the tiled file: header,
// IFD, out-of-line values and tile tables from the tiles' byte counts.  No HIP in here:
// tests/cpp/tiff_host_check.cc compiles it alone under the address and undefined-behaviour
// sanitizers.  The file is defined in DESIGN 4.16.
#ifndef AMHIP_TIFF_HOST_H_
#define AMHIP_TIFF_HOST_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_png_encode_host.h"

namespace amhip {
namespace tiff {

enum { kShort = 3, kLong = 4, kAscii = 2, kDouble = 12 };
enum Kind { kF32 = 0, kU8 = 1, kRgb8 = 2 };

struct Tag {
  uint16_t tag, type;
  uint32_t count;
  uint32_t value;  // the value, or the file offset of the values
};

// ---- geo tags -----------------------------------------------------------------------------------
// ModelPixelScale, ModelTiepoint, GeoKeyDirectory and GeoAsciiParams: what SetProjCS(..) +
// SetWellKnownGeogCS("WGS84") + SetUTM(zone, north) describe (aerial-mapper-io.cc:390-394,
// :467-474): EPSG 326zz / 327zz, PixelIsArea.
struct GeoTags {
  double scale[3], tie[6];
  uint16_t keys[32];
  std::string ascii;   // (written with its terminating zero)
};

inline GeoTags make_geo_tags(const double* geotransform, int utm_zone, int northern) {
  GeoTags g;
  char citation[96];
  std::snprintf(citation, sizeof(citation), "UTM %d (WGS84) in %s hemisphere.|", utm_zone,
                northern ? "northern" : "southern");
  g.ascii = std::string(citation) + "WGS 84|";
  const uint16_t cit_len = (uint16_t)std::strlen(citation);
  const uint16_t geokeys[32] = {
      1, 1, 0, 7,                                          // version, revision, minor, keys
      1024, 0, 1, 1,                                       // GTModelType = projected
      1025, 0, 1, 1,                                       // GTRasterType = PixelIsArea
      1026, 34737, cit_len, 0,                             // GTCitation
      2048, 0, 1, 4326,                                    // GeographicType = WGS 84
      2049, 34737, 7, cit_len,                             // GeogCitation "WGS 84|"
      3072, 0, 1, (uint16_t)((northern ? 32600 : 32700) + utm_zone),  // ProjectedCSType
      3076, 0, 1, 9001,                                    // ProjLinearUnits = metre
  };
  for (int k = 0; k < 32; ++k) g.keys[k] = geokeys[k];
  g.scale[0] = geotransform[1];
  g.scale[1] = -geotransform[5];
  g.scale[2] = 0.0;
  const double tie[6] = {0.0, 0.0, 0.0, geotransform[0], geotransform[3], 0.0};
  for (int k = 0; k < 6; ++k) g.tie[k] = tie[k];
  return g;
}

inline bool north_up(const double* gt) {
  return gt[2] == 0.0 && gt[4] == 0.0 && gt[1] > 0.0 && gt[5] < 0.0;
}

// ---- the tiled Deflate file ---------------------------------------------------------------------
inline int bands_of(int kind) { return kind == kRgb8 ? 3 : 1; }
inline int pixel_bytes(int kind) { return kind == kF32 ? 4 : kind == kRgb8 ? 3 : 1; }
inline uint32_t tile_side(int tile) { return tile == 0 ? 256u : (uint32_t)tile; }
inline bool tile_ok(int tile) { return tile == 0 || (tile >= 16 && tile <= 1024 && tile % 16 == 0); }
inline uint64_t tiles_across(int width, int tile) { return ((uint64_t)width + tile_side(tile) - 1) / tile_side(tile); }
inline uint64_t tile_count(int width, int height, int tile) { return tiles_across(width, tile) * tiles_across(height, tile); }
// the predictor bytes of one tile: every tile is full size
inline uint64_t tile_raw(int kind, int tile) {
  return (uint64_t)tile_side(tile) * tile_side(tile) * (uint64_t)pixel_bytes(kind);
}

// null: fine; else which field is wrong
inline const char* check_kind(int kind) {
  return kind != kF32 && kind != kU8 && kind != kRgb8 ? "kind must be 0 (f32), 1 (u8) or 2 (rgb8)" : nullptr;
}
inline const char* check_tile(int tile) {
  return tile_ok(tile) ? nullptr : "tile must be a multiple of 16 in 16..1024, or 0 (256)";
}
inline const char* check_raster(int width, int height, int kind, int tile) {
  if (width < 1 || width > 65535) return "width must be 1..65535";
  if (height < 1 || height > 65535) return "height must be 1..65535";
  if (const char* why = check_kind(kind)) return why;
  return check_tile(tile);
}
inline const char* check_geo(const double* geotransform, int utm_zone) {
  if (!north_up(geotransform))
    return "geotransform: only north-up geotransforms (GT2 = GT4 = 0, GT1 > 0, GT5 < 0)";
  if (utm_zone < 1 || utm_zone > 60) return "utm_zone must be 1..60";
  return nullptr;
}

// where the tile data start: behind the IFD and the out-of-line values, on a multiple of 16
struct Container {
  std::vector<uint8_t> head;   // the file up to the first tile, `data_at` bytes
  uint64_t file_bytes;         // ... and with the tiles
};

// The file in front of the tile data for tiles of `counts[t]` bytes (row-major tile order), tightly
// packed from the next multiple of 16 behind the values.  The IFD at offset 8, tags ascending;
// out-of-line values behind it in tag order, word aligned; tile tables as LONG, inline when there is
// one tile.  false (nothing built): the file would exceed 2^32 - 1 bytes.
inline bool build_container(int width, int height, int kind, int tile, const GeoTags& geo,
                            const uint64_t* counts, uint64_t ntiles, Container* out) {
  const uint32_t side = tile_side(tile);
  const int bands = bands_of(kind);
  const bool f32 = kind == kF32;
  const int ntags = f32 ? 18 : 17;
  const uint32_t ifd_at = 8;
  const uint64_t extra_at = ifd_at + 2 + (uint64_t)ntags * 12 + 4;
  // sizes first: nothing is allocated for a file that is refused
  auto even = [](uint64_t n) { return n + (n & 1u); };
  uint64_t at = extra_at;
  auto place = [&](uint64_t n) {
    const uint64_t a = at;
    at += even(n);
    return a;
  };
  const uint64_t bits_at = bands == 3 ? place(6) : 0;
  const uint64_t offs_at = ntiles > 1 ? place(4 * ntiles) : 0;
  const uint64_t cnts_at = ntiles > 1 ? place(4 * ntiles) : 0;
  const uint64_t fmt_at = bands == 3 ? place(6) : 0;
  const uint64_t scale_at = place(sizeof(geo.scale));
  const uint64_t tie_at = place(sizeof(geo.tie));
  const uint64_t keys_at = place(sizeof(geo.keys));
  const uint64_t ascii_at = place(geo.ascii.size() + 1);
  const uint64_t data_at = (at + 15u) & ~(uint64_t)15u;
  uint64_t total = data_at;
  for (uint64_t t = 0; t < ntiles; ++t) {
    if (counts[t] > 0xFFFFFFFFull || total + counts[t] > 0xFFFFFFFFull) return false;
    total += counts[t];
  }
  std::vector<uint8_t>& head = out->head;
  head.assign((size_t)data_at, 0);
  auto put16 = [&](uint64_t where, uint16_t v) { std::memcpy(head.data() + where, &v, 2); };
  auto put32 = [&](uint64_t where, uint32_t v) { std::memcpy(head.data() + where, &v, 4); };
  uint64_t run = data_at;
  for (uint64_t t = 0; t < ntiles && ntiles > 1; ++t) {
    put32(offs_at + 4 * t, (uint32_t)run);
    put32(cnts_at + 4 * t, (uint32_t)counts[t]);
    run += counts[t];
  }
  if (bands == 3) {
    for (int k = 0; k < 3; ++k) {
      put16(bits_at + 2 * k, 8);
      put16(fmt_at + 2 * k, 1);
    }
  }
  std::memcpy(head.data() + scale_at, geo.scale, sizeof(geo.scale));
  std::memcpy(head.data() + tie_at, geo.tie, sizeof(geo.tie));
  std::memcpy(head.data() + keys_at, geo.keys, sizeof(geo.keys));
  std::memcpy(head.data() + ascii_at, geo.ascii.c_str(), geo.ascii.size() + 1);
  const Tag tags[18] = {
      {256, kLong, 1, (uint32_t)width},
      {257, kLong, 1, (uint32_t)height},
      {258, kShort, (uint32_t)bands, bands == 3 ? (uint32_t)bits_at : f32 ? 32u : 8u},
      {259, kShort, 1, 8},                          // Adobe Deflate
      {262, kShort, 1, bands == 3 ? 2u : 1u},       // RGB / BlackIsZero
      {277, kShort, 1, (uint32_t)bands},
      {284, kShort, 1, 1},                          // pixel interleaved
      {317, kShort, 1, f32 ? 3u : 2u},              // floating point / horizontal differencing
      {322, kLong, 1, side},
      {323, kLong, 1, side},
      {324, kLong, (uint32_t)ntiles, ntiles > 1 ? (uint32_t)offs_at : (uint32_t)data_at},
      {325, kLong, (uint32_t)ntiles, ntiles > 1 ? (uint32_t)cnts_at : (uint32_t)counts[0]},
      {339, kShort, (uint32_t)bands, bands == 3 ? (uint32_t)fmt_at : f32 ? 3u : 1u},
      {33550, kDouble, 3, (uint32_t)scale_at},
      {33922, kDouble, 6, (uint32_t)tie_at},
      {34735, kShort, 32, (uint32_t)keys_at},
      {34737, kAscii, (uint32_t)geo.ascii.size() + 1, (uint32_t)ascii_at},
      {42113, kAscii, 4, 0x006E616Eu},              // GDAL_NODATA "nan", inline
  };
  head[0] = 'I';
  head[1] = 'I';
  put16(2, 42);
  put32(4, ifd_at);
  put16(ifd_at, (uint16_t)ntags);
  for (int k = 0; k < ntags; ++k) {
    const uint64_t e = ifd_at + 2 + 12 * (uint64_t)k;
    put16(e, tags[k].tag);
    put16(e + 2, tags[k].type);
    put32(e + 4, tags[k].count);
    put32(e + 8, tags[k].value);
  }
  // (the four bytes behind the entries stay zero: no further IFD)
  out->file_bytes = total;
  return true;
}

// the bytes of the file in front of its tiles
inline uint64_t head_bytes(int kind, uint64_t ntiles) {
  const uint64_t ntags = kind == kF32 ? 18 : 17;
  uint64_t at = 8 + 2 + ntags * 12 + 4;
  if (kind == kRgb8) at += 12;
  if (ntiles > 1) at += 8 * ntiles;
  at += 24 + 48 + 64;
  at += 48;   // GeoAsciiParams: at most "UTM 60 (WGS84) in northern hemisphere.|WGS 84|" and its zero, even
  return (at + 15u) & ~(uint64_t)15u;
}

// worst-case size of the file: every tile's zlib bound behind the largest head
inline uint64_t file_bound(int width, int height, int kind, int tile) {
  const uint64_t n = tile_count(width, height, tile);
  return head_bytes(kind, n) + n * pnge::zlib_bound(tile_raw(kind, tile));
}

}  // namespace tiff
}  // namespace amhip

#endif  // AMHIP_TIFF_HOST_H_
