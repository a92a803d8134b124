// amhip_tiff_host.h -- the part of the GeoTIFF writers that needs no device: the geo tags of a
// north-up UTM raster (shared by amhip_geotiff_write_u8, amhip_export.hip, and the tiled Deflate
// writer, amhip_tiff_encode.hip), the argument checks, and the container of the tiled file: header,
// IFDs (level 0 and its overviews), out-of-line values and tile tables from the tiles'
// byte counts.  No HIP in here:
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

// ---- the pyramid -------------------------------------------------------------------
// Level k >= 1 is ceil(w / 2) x ceil(h / 2) of level k - 1.  The tiles of a call are one list: level
// 0's in row-major order, then level 1's, and so on.
constexpr int kMaxOverviews = 16;

struct Level {
  int width, height;
  uint64_t first, ntiles;   // its tiles in the call's list
};

// The number of overview levels `overviews` asks for: n >= 0 as given, -1: until both sides of the
// last level are at most the tile's.  null: fine, *n set; else what is wrong with the field.
inline const char* check_overviews(int width, int height, int tile, int overviews, int* n) {
  if (overviews < -1 || overviews > kMaxOverviews) return "overviews must be -1 (automatic) or 0..16";
  const int side = (int)tile_side(tile);
  int w = width, h = height, k = 0;
  while (overviews < 0 ? (w > side || h > side) : k < overviews) {
    if (w == 1 && h == 1) return "overviews: more levels than the raster has (a 1 x 1 level is not reduced)";
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    ++k;
  }
  *n = k;
  return nullptr;
}

inline std::vector<Level> make_levels(int width, int height, int tile, int overviews) {
  std::vector<Level> levels;
  uint64_t first = 0;
  for (int k = 0; k <= overviews; ++k) {
    const Level l = {width, height, first, tile_count(width, height, tile)};
    levels.push_back(l);
    first += l.ntiles;
    width = (width + 1) / 2;
    height = (height + 1) / 2;
  }
  return levels;
}

struct Container {
  std::vector<uint8_t> head;        // the file up to the first tile
  uint64_t file_bytes;              // ... and with the tiles
  std::vector<uint64_t> level_at;   // where every level's tiles start
};

// The file in front of the tile data for tiles of `counts[t]` bytes (the call's list).  The header,
// then IFD 0 at offset 8, IFD 1, ..: tags ascending, each IFD's out-of-line values behind it in tag
// order, word aligned; tile tables as LONG, inline when a level has one tile; the IFDs chained, the
// last one's next-IFD offset 0.  IFD 0 carries the geo tags; an overview IFD carries NewSubfileType
// = 1 and none.  Tile data from the next multiple of 16 behind the last values: the coarsest level
// first, level 0 last, each level's tiles in row-major order, tightly packed.  With one level this is
// the file of DESIGN 4.16.  false (nothing built): the file would exceed 2^32 - 1 bytes.
inline bool build_pyramid(const std::vector<Level>& levels, int kind, int tile, const GeoTags& geo,
                          const uint64_t* counts, Container* out) {
  const uint32_t side = tile_side(tile);
  const int bands = bands_of(kind);
  const bool f32 = kind == kF32;
  const size_t L = levels.size();
  struct Where {
    uint64_t ifd_at, bits_at, offs_at, cnts_at, fmt_at, scale_at, tie_at, keys_at, ascii_at;
    int ntags;
  };
  std::vector<Where> where(L);
  // sizes first: nothing is allocated for a file that is refused
  auto even = [](uint64_t n) { return n + (n & 1u); };
  uint64_t at = 8;
  auto place = [&](uint64_t n) {
    const uint64_t a = at;
    at += even(n);
    return a;
  };
  for (size_t k = 0; k < L; ++k) {
    Where& w = where[k];
    const uint64_t ntiles = levels[k].ntiles;
    w.ntags = k == 0 ? (f32 ? 18 : 17) : (f32 ? 15 : 14);
    w.ifd_at = place(2 + (uint64_t)w.ntags * 12 + 4);
    w.bits_at = bands == 3 ? place(6) : 0;
    w.offs_at = ntiles > 1 ? place(4 * ntiles) : 0;
    w.cnts_at = ntiles > 1 ? place(4 * ntiles) : 0;
    w.fmt_at = bands == 3 ? place(6) : 0;
    w.scale_at = w.tie_at = w.keys_at = w.ascii_at = 0;
    if (k == 0) {
      w.scale_at = place(sizeof(geo.scale));
      w.tie_at = place(sizeof(geo.tie));
      w.keys_at = place(sizeof(geo.keys));
      w.ascii_at = place(geo.ascii.size() + 1);
    }
    if (at > 0xFFFFFFFFull) return false;
  }
  const uint64_t data_at = (at + 15u) & ~(uint64_t)15u;
  uint64_t total = data_at;
  std::vector<uint64_t> level_at(L);
  for (size_t k = L; k-- > 0;) {
    level_at[k] = total;
    for (uint64_t t = 0; t < levels[k].ntiles; ++t) {
      const uint64_t n = counts[levels[k].first + t];
      if (n > 0xFFFFFFFFull || total + n > 0xFFFFFFFFull) return false;
      total += n;
    }
  }
  std::vector<uint8_t>& head = out->head;
  head.assign((size_t)data_at, 0);
  auto put16 = [&](uint64_t where_, uint16_t v) { std::memcpy(head.data() + where_, &v, 2); };
  auto put32 = [&](uint64_t where_, uint32_t v) { std::memcpy(head.data() + where_, &v, 4); };
  head[0] = 'I';
  head[1] = 'I';
  put16(2, 42);
  put32(4, (uint32_t)where[0].ifd_at);
  for (size_t k = 0; k < L; ++k) {
    const Where& w = where[k];
    const uint64_t ntiles = levels[k].ntiles;
    const uint64_t* cnt = counts + levels[k].first;
    uint64_t run = level_at[k];
    for (uint64_t t = 0; t < ntiles && ntiles > 1; ++t) {
      put32(w.offs_at + 4 * t, (uint32_t)run);
      put32(w.cnts_at + 4 * t, (uint32_t)cnt[t]);
      run += cnt[t];
    }
    if (bands == 3) {
      for (int b = 0; b < 3; ++b) {
        put16(w.bits_at + 2 * b, 8);
        put16(w.fmt_at + 2 * b, 1);
      }
    }
    if (k == 0) {
      std::memcpy(head.data() + w.scale_at, geo.scale, sizeof(geo.scale));
      std::memcpy(head.data() + w.tie_at, geo.tie, sizeof(geo.tie));
      std::memcpy(head.data() + w.keys_at, geo.keys, sizeof(geo.keys));
      std::memcpy(head.data() + w.ascii_at, geo.ascii.c_str(), geo.ascii.size() + 1);
    }
    const Tag tags[19] = {
        {254, kLong, 1, 1},                           // NewSubfileType: a reduced-resolution image (overviews only)
        {256, kLong, 1, (uint32_t)levels[k].width},
        {257, kLong, 1, (uint32_t)levels[k].height},
        {258, kShort, (uint32_t)bands, bands == 3 ? (uint32_t)w.bits_at : f32 ? 32u : 8u},
        {259, kShort, 1, 8},                          // Adobe Deflate
        {262, kShort, 1, bands == 3 ? 2u : 1u},       // RGB / BlackIsZero
        {277, kShort, 1, (uint32_t)bands},
        {284, kShort, 1, 1},                          // pixel interleaved
        {317, kShort, 1, f32 ? 3u : 2u},              // floating point / horizontal differencing
        {322, kLong, 1, side},
        {323, kLong, 1, side},
        {324, kLong, (uint32_t)ntiles, ntiles > 1 ? (uint32_t)w.offs_at : (uint32_t)level_at[k]},
        {325, kLong, (uint32_t)ntiles, ntiles > 1 ? (uint32_t)w.cnts_at : (uint32_t)cnt[0]},
        {339, kShort, (uint32_t)bands, bands == 3 ? (uint32_t)w.fmt_at : f32 ? 3u : 1u},
        {33550, kDouble, 3, (uint32_t)w.scale_at},    // (IFD 0 only, as the three behind it)
        {33922, kDouble, 6, (uint32_t)w.tie_at},
        {34735, kShort, 32, (uint32_t)w.keys_at},
        {34737, kAscii, (uint32_t)geo.ascii.size() + 1, (uint32_t)w.ascii_at},
        {42113, kAscii, 4, 0x006E616Eu},              // GDAL_NODATA "nan", inline (f32 only)
    };
    put16(w.ifd_at, (uint16_t)w.ntags);
    uint64_t e = w.ifd_at + 2;
    for (int t = 0; t < 19; ++t) {
      const bool geo_tag = tags[t].tag >= 33550 && tags[t].tag <= 34737;
      if ((tags[t].tag == 254 && k == 0) || (geo_tag && k != 0) || (tags[t].tag == 42113 && !f32)) continue;
      put16(e, tags[t].tag);
      put16(e + 2, tags[t].type);
      put32(e + 4, tags[t].count);
      put32(e + 8, tags[t].value);
      e += 12;
    }
    // (the last IFD's four bytes behind the entries stay zero: no further IFD)
    if (k + 1 < L) put32(e, (uint32_t)where[k + 1].ifd_at);
  }
  out->file_bytes = total;
  out->level_at = level_at;
  return true;
}

// ... of a file without overviews
inline bool build_container(int width, int height, int kind, int tile, const GeoTags& geo,
                            const uint64_t* counts, uint64_t ntiles, Container* out) {
  (void)ntiles;
  return build_pyramid(make_levels(width, height, tile, 0), kind, tile, geo, counts, out);
}

// the bytes of the file in front of its tiles, at the most
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

// ... with `overviews` (>= 0, checked) levels behind level 0: an overview's IFD and values take no
// more than IFD 0's
inline uint64_t file_bound_ovr(int width, int height, int kind, int tile, int overviews) {
  uint64_t sum = 0;
  for (const Level& l : make_levels(width, height, tile, overviews))
    sum += head_bytes(kind, l.ntiles) + l.ntiles * pnge::zlib_bound(tile_raw(kind, tile));
  return sum;
}

}  // namespace tiff
}  // namespace amhip

#endif  // AMHIP_TIFF_HOST_H_
