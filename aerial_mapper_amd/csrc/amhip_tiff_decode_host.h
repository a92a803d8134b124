// amhip_tiff_decode_host.h -- the host-only part of the GeoTIFF reader (amhip_tiff_decode.hip): the
// parser of one IFD of a classic little-endian TIFF -- the first, or a level's (the chain walk and the
// level rules of DESIGN 4.18 stand at the end) --, the descriptor of the raster and one entry per
// chunk (a tile or a strip).  No HIP in here: tests/cpp/tiff_decode_host_main.cc compiles it alone
// under the address and undefined-behaviour sanitizers, tests/cpp/tiff_pyramid_host_main.cc the levels.
// The accepted set is DESIGN 4.17:
//
//   layout        tiles (322 / 323 / 324 / 325; width and length multiples of 16) or strips (273 / 278 /
//                 279; RowsPerStrip absent or larger than the height: one strip)
//   Compression   1 (none), 8 (Adobe Deflate), 32946 (the old Deflate code)
//   samples       f32 (1 band, 32 bit, SampleFormat 3), u8 / u16 (1 band, SampleFormat 1 or absent),
//                 i16 (1 band, 16 bit, SampleFormat 2), rgb8 (3 bands of 8 bit, PlanarConfiguration 1)
//   Predictor     1, 2 (differences of whole samples, stride = bands), 3 (f32 only: libtiff's fpDiff);
//                 with Compression 1 the tag is checked and then ignored, as libtiff ignores it
//   geo tags      ModelPixelScale + one ModelTiepoint, or a ModelTransformation without rotation;
//                 north-up only; GeoKey 1025 = 2 (PixelIsPoint) moves the origin by half a pixel, so
//                 the geotransform always describes pixel areas; GeoKey 3072 is the EPSG code
//   GDAL_NODATA   as strtod reads it
// Everything else is refused with a text that names the tag and the value.  Every count and offset
// is checked against the file's length before it is used, and every chunk handed on lies inside
// the file.
#ifndef AMHIP_TIFF_DECODE_HOST_H_
#define AMHIP_TIFF_DECODE_HOST_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace amhip {
namespace tiffd {

enum Kind { kF32 = 0, kU8 = 1, kRgb8 = 2, kU16 = 3, kI16 = 4 };   // (0..2 as the writer's, amhip_tiff_host.h)

inline int pixel_bytes(int kind) {
  return kind == kF32 ? 4 : kind == kU8 ? 1 : kind == kRgb8 ? 3 : 2;
}

struct Chunk {
  uint64_t offset, count;   // its bytes in the file
  uint64_t raw_len;         // its bytes behind the decompressor
  uint32_t rows;            // image rows it holds (a tile: the tile's length, padding included)
};

struct Parsed {
  int32_t width, height, bands, kind;
  int32_t tiled;                    // 1: tiles, 0: strips
  uint32_t chunk_w, chunk_h;        // tile width and length; strips: the image's width, rows per strip
  uint32_t across, down;            // chunks per row of chunks (strips: 1), rows of chunks
  int32_t compression, predictor;
  int32_t has_geo, epsg, raster_type;
  double gt[6];
  int32_t has_nodata;
  double nodata;
  std::vector<Chunk> chunks;        // row-major
};

inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline double le_f64(const uint8_t* p) {
  uint64_t v = 0;
  for (int k = 7; k >= 0; --k) v = (v << 8) | p[k];
  double d;
  std::memcpy(&d, &v, 8);
  return d;
}

// one IFD entry whose values have been checked to lie inside the file
struct Entry {
  bool have = false;
  uint16_t type = 0;
  uint32_t count = 0;
  const uint8_t* at = nullptr;   // the first value
};

inline int type_bytes(int type) {
  switch (type) {
    case 1: case 2: case 6: case 7: return 1;
    case 3: case 8: return 2;
    case 4: case 9: case 11: case 13: return 4;
    case 5: case 10: case 12: case 16: case 17: case 18: return 8;
  }
  return 0;
}

// The header -> the offset of the first IFD, or false with a text in err.
inline bool first_ifd(const uint8_t* file, size_t len, uint64_t* at, char* err, size_t errcap) {
  auto fail = [&](const char* fmt, long long a, long long b) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
    return false;
  };
  if (!file || len < 8) return fail("no TIFF header (%lld bytes)", (long long)len, 0);
  if (file[0] == 'M' && file[1] == 'M') return fail("big-endian TIFF (byte order MM) is not read", 0, 0);
  if (file[0] != 'I' || file[1] != 'I') return fail("no TIFF header (byte order mark)", 0, 0);
  const int version = le16(file + 2);
  if (version == 43) return fail("BigTIFF (version 43) is not read", 0, 0);
  if (version != 42) return fail("no TIFF header (version %lld)", version, 0);
  *at = le32(file + 4);
  return true;
}

// The IFD at byte `ifd` of the file -> *out, or false with a text in err.
inline bool parse_ifd(const uint8_t* file, size_t len, uint64_t ifd, Parsed* out, char* err, size_t errcap) {
  auto fail = [&](const char* fmt, long long a, long long b) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
    return false;
  };
  auto fail3 = [&](const char* fmt, unsigned long long a, unsigned long long b, unsigned long long c) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b, c);
    return false;
  };
  auto fail_text = [&](const char* text) {
    if (err && errcap) std::snprintf(err, errcap, "%s", text);
    return false;
  };
  Parsed& P = *out;
  P = Parsed();
  if (ifd < 8 || ifd + 2 > len) return fail("the IFD at byte %lld lies outside the file", (long long)ifd, 0);
  const uint64_t n = le16(file + ifd);
  if (ifd + 2 + 12 * n + 4 > len) return fail("the IFD at byte %lld (%lld entries) runs past the file", (long long)ifd, (long long)n);

  // the tags this reader looks at
  enum { kNumTags = 24 };
  static const uint16_t kTags[kNumTags] = {256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284,
                                           317, 320, 322, 323, 324, 325, 338, 339, 33550, 33922, 34264, 34735};
  Entry e[kNumTags + 1];   // (+ GDAL_NODATA)
  auto slot = [&](int tag) -> Entry& {
    if (tag == 42113) return e[kNumTags];
    for (int k = 0; k < kNumTags; ++k)
      if (kTags[k] == tag) return e[k];
    return e[0];   // (not reached: only called with tags of the list)
  };
  for (uint64_t k = 0; k < n; ++k) {
    const uint8_t* p = file + ifd + 2 + 12 * k;
    const int tag = le16(p), type = le16(p + 2);
    const uint32_t count = le32(p + 4);
    bool wanted = tag == 42113;
    for (int q = 0; q < kNumTags; ++q) wanted = wanted || kTags[q] == tag;
    if (!wanted) continue;   // (any other tag: not looked at, whatever it says)
    const int tb = type_bytes(type);
    if (!tb) return fail("tag %lld: field type %lld", tag, type);
    const uint64_t size = (uint64_t)tb * count;
    const uint8_t* at = p + 8;
    if (size > 4) {
      const uint64_t off = le32(p + 8);
      if (off > len || size > len - off) return fail("tag %lld: its values at byte %lld run past the file", tag, (long long)off);
      at = file + off;
    }
    Entry& s = slot(tag);
    if (s.have) return fail("tag %lld appears twice", tag, 0);
    s.have = true;
    s.type = (uint16_t)type;
    s.count = count;
    s.at = at;
  }
  // value k of an entry of SHORTs or LONGs
  auto uint_at = [](const Entry& s, uint32_t k) -> uint32_t { return s.type == 3 ? le16(s.at + 2 * k) : le32(s.at + 4 * k); };
  bool bad = false;
  char bad_text[96] = {0};
  // a scalar tag of type SHORT or LONG; absent: dflt
  auto scalar = [&](int tag, uint32_t dflt) -> uint32_t {
    const Entry& s = slot(tag);
    if (!s.have) return dflt;
    if ((s.type != 3 && s.type != 4) || s.count < 1) {
      if (!bad) std::snprintf(bad_text, sizeof(bad_text), "tag %d: field type %d, count %u (a SHORT or LONG is expected)", tag, (int)s.type, s.count);
      bad = true;
      return dflt;
    }
    return uint_at(s, 0);
  };
  const uint32_t width = scalar(256, 0), height = scalar(257, 0);
  const uint32_t compression = scalar(259, 1), photometric = scalar(262, 1), fill_order = scalar(266, 1);
  const uint32_t orientation = scalar(274, 1), bands = scalar(277, 1), planar = scalar(284, 1);
  const uint32_t predictor = scalar(317, 1);
  if (bad) return fail_text(bad_text);
  if (!slot(256).have || width < 1 || width > (1u << 20)) return fail("tag 256 (ImageWidth): %lld is outside 1..2^20", width, 0);
  if (!slot(257).have || height < 1 || height > (1u << 20)) return fail("tag 257 (ImageLength): %lld is outside 1..2^20", height, 0);
  if (compression != 1 && compression != 8 && compression != 32946)
    return fail("tag 259 (Compression): %lld (1, 8 and 32946 are read; no LZW, PackBits, JPEG, ZSTD, LERC)", compression, 0);
  if (photometric == 3 || slot(320).have) return fail("tag 262 (PhotometricInterpretation): %lld, a palette image", photometric, 0);
  if (fill_order != 1) return fail("tag 266 (FillOrder): %lld", fill_order, 0);
  if (orientation != 1) return fail("tag 274 (Orientation): %lld", orientation, 0);
  if (bands != 1 && bands != 3) return fail("tag 277 (SamplesPerPixel): %lld (1 or 3 bands are read)", bands, 0);
  if (slot(338).have && slot(338).count > 0) return fail("tag 338 (ExtraSamples): %lld extra samples", slot(338).count, 0);
  // BitsPerSample and SampleFormat: one value, or one per band, all equal
  uint32_t bits = 1, fmt = 1;
  {
    const Entry& b = slot(258);
    if (b.have) {
      if ((b.type != 3 && b.type != 4) || (b.count != 1 && b.count != bands)) return fail("tag 258 (BitsPerSample): %lld values for %lld bands", b.count, bands);
      bits = uint_at(b, 0);
      for (uint32_t k = 1; k < b.count; ++k)
        if (uint_at(b, k) != bits) return fail("tag 258 (BitsPerSample): %lld and %lld in one pixel", bits, uint_at(b, k));
    }
    const Entry& f = slot(339);
    if (f.have) {
      if ((f.type != 3 && f.type != 4) || (f.count != 1 && f.count != bands)) return fail("tag 339 (SampleFormat): %lld values for %lld bands", f.count, bands);
      fmt = uint_at(f, 0);
      for (uint32_t k = 1; k < f.count; ++k)
        if (uint_at(f, k) != fmt) return fail("tag 339 (SampleFormat): %lld and %lld in one pixel", fmt, uint_at(f, k));
    }
  }
  int kind = -1;
  if (bands == 3) {
    if (bits != 8) return fail("tag 258 (BitsPerSample): %lld with three bands (8 is read)", bits, 0);
    if (fmt != 1) return fail("tag 339 (SampleFormat): %lld with three bands", fmt, 0);
    if (planar != 1) return fail("tag 284 (PlanarConfiguration): %lld with three bands", planar, 0);
    kind = kRgb8;
  } else if (bits == 32 && fmt == 3) {
    kind = kF32;
  } else if (bits == 8 && fmt == 1) {
    kind = kU8;
  } else if (bits == 16 && fmt == 1) {
    kind = kU16;
  } else if (bits == 16 && fmt == 2) {
    kind = kI16;
  } else if (bits != 8 && bits != 16 && bits != 32) {
    return fail("tag 258 (BitsPerSample): %lld (8, 16 and 32 are read)", bits, 0);
  } else {
    return fail("tag 339 (SampleFormat): %lld with %lld bits", fmt, bits);
  }
  if (predictor < 1 || predictor > 3) return fail("tag 317 (Predictor): %lld", predictor, 0);
  if (predictor == 3 && kind != kF32) return fail("tag 317 (Predictor): 3 with samples that are no 32-bit floats (%lld bits)", bits, 0);
  P.width = (int32_t)width;
  P.height = (int32_t)height;
  P.bands = (int32_t)bands;
  P.kind = kind;
  P.compression = (int32_t)compression;
  // (libtiff's predictor is a part of its LZW and Deflate codecs: an uncompressed file's tag is not acted on)
  P.predictor = compression == 1 ? 1 : (int32_t)predictor;
  const uint64_t bpp = (uint64_t)pixel_bytes(kind);

  // ---- layout ------------------------------------------------------------------------------------
  int off_tag, cnt_tag;
  if (slot(322).have || slot(323).have || slot(324).have) {
    const uint32_t tw = scalar(322, 0), th = scalar(323, 0);
    if (bad) return fail_text(bad_text);
    if (tw < 16 || tw % 16 || tw > (1u << 20)) return fail("tag 322 (TileWidth): %lld is no multiple of 16 in 16..2^20", tw, 0);
    if (th < 16 || th % 16 || th > (1u << 20)) return fail("tag 323 (TileLength): %lld is no multiple of 16 in 16..2^20", th, 0);
    P.tiled = 1;
    P.chunk_w = tw;
    P.chunk_h = th;
    P.across = (width + tw - 1) / tw;
    P.down = (height + th - 1) / th;
    off_tag = 324;
    cnt_tag = 325;
  } else {
    uint32_t rps = scalar(278, 0xFFFFFFFFu);
    if (bad) return fail_text(bad_text);
    if (rps < 1) return fail("tag 278 (RowsPerStrip): %lld", rps, 0);
    if (rps > height) rps = height;
    P.tiled = 0;
    P.chunk_w = width;
    P.chunk_h = rps;
    P.across = 1;
    P.down = (height + rps - 1) / rps;
    off_tag = 273;
    cnt_tag = 279;
  }
  const Entry& offs = slot(off_tag);
  const Entry& cnts = slot(cnt_tag);
  if (!offs.have) return fail("tag %lld (the chunks' offsets) is missing", off_tag, 0);
  if (!cnts.have) return fail("tag %lld (the chunks' byte counts) is missing", cnt_tag, 0);
  if (offs.type != 3 && offs.type != 4) return fail("tag %lld: field type %lld (SHORT or LONG is read)", off_tag, offs.type);
  if (cnts.type != 3 && cnts.type != 4) return fail("tag %lld: field type %lld (SHORT or LONG is read)", cnt_tag, cnts.type);
  const uint64_t nchunks = (uint64_t)P.across * P.down;
  if (offs.count != nchunks) return fail3("tag %llu: %llu entries, the layout has %llu chunks", off_tag, offs.count, nchunks);
  if (cnts.count != nchunks) return fail3("tag %llu: %llu entries, the layout has %llu chunks", cnt_tag, cnts.count, nchunks);
  P.chunks.resize((size_t)nchunks);
  for (uint64_t t = 0; t < nchunks; ++t) {
    Chunk& c = P.chunks[(size_t)t];
    c.offset = uint_at(offs, (uint32_t)t);
    c.count = uint_at(cnts, (uint32_t)t);
    if (P.tiled) {
      c.rows = P.chunk_h;
    } else {
      const uint64_t r0 = t * P.chunk_h;
      c.rows = (uint32_t)(height - r0 < P.chunk_h ? height - r0 : P.chunk_h);
    }
    c.raw_len = (uint64_t)c.rows * P.chunk_w * bpp;
    if (c.offset > len || c.count > len - c.offset)
      return fail("chunk %lld: its bytes at %lld run past the file", (long long)t, (long long)c.offset);
    const uint8_t* z = file + c.offset;
    if (compression == 1) {
      if (c.count != c.raw_len) return fail3("chunk %llu: %llu bytes uncompressed, its rows take %llu", t, c.count, c.raw_len);
    } else {
      if (c.count < 6) return fail("chunk %lld: %lld bytes are no zlib stream", (long long)t, (long long)c.count);
      const int cmf = z[0], flg = z[1];
      if ((cmf & 15) != 8) return fail("chunk %lld: zlib header: compression method %lld", (long long)t, cmf & 15);
      if ((cmf >> 4) > 7) return fail("chunk %lld: zlib header: CINFO %lld", (long long)t, cmf >> 4);
      if ((cmf * 256 + flg) % 31 != 0) return fail("chunk %lld: zlib header: FCHECK", (long long)t, 0);
      if (flg & 0x20) return fail("chunk %lld: zlib header: FDICT set", (long long)t, 0);
    }
  }

  // ---- geo tags ----------------------------------------------------------------------------------
  const Entry& scale = slot(33550);
  const Entry& tie = slot(33922);
  const Entry& xform = slot(34264);
  double gt[6] = {0, 1, 0, 0, 0, 1};
  bool geo = false;
  if (scale.have || tie.have) {
    if (!scale.have) return fail("tag 33922 (ModelTiepoint) without tag 33550 (ModelPixelScale)", 0, 0);
    if (!tie.have) return fail("tag 33550 (ModelPixelScale) without tag 33922 (ModelTiepoint)", 0, 0);
    if (scale.type != 12 || scale.count < 2) return fail("tag 33550 (ModelPixelScale): field type %lld, count %lld", scale.type, scale.count);
    if (tie.type != 12 || tie.count != 6) return fail("tag 33922 (ModelTiepoint): field type %lld, %lld values (one tiepoint is read)", tie.type, tie.count);
    const double sx = le_f64(scale.at), sy = le_f64(scale.at + 8);
    double t[6];
    for (int k = 0; k < 6; ++k) t[k] = le_f64(tie.at + 8 * k);
    gt[0] = t[3] - t[0] * sx;
    gt[1] = sx;
    gt[2] = 0.0;
    gt[3] = t[4] + t[1] * sy;
    gt[4] = 0.0;
    gt[5] = -sy;
    geo = true;
  } else if (xform.have) {
    if (xform.type != 12 || xform.count != 16) return fail("tag 34264 (ModelTransformation): field type %lld, count %lld", xform.type, xform.count);
    double m[16];
    for (int k = 0; k < 16; ++k) m[k] = le_f64(xform.at + 8 * k);
    if (m[1] != 0.0 || m[4] != 0.0) return fail("tag 34264 (ModelTransformation): rotation terms are not zero", 0, 0);
    gt[0] = m[3];
    gt[1] = m[0];
    gt[2] = 0.0;
    gt[3] = m[7];
    gt[4] = 0.0;
    gt[5] = m[5];
    geo = true;
  }
  P.raster_type = 1;
  const Entry& keys = slot(34735);
  if (keys.have) {
    if (keys.type != 3 || keys.count < 4) return fail("tag 34735 (GeoKeyDirectory): field type %lld, count %lld", keys.type, keys.count);
    const uint64_t nkeys = le16(keys.at + 6);
    if (4 + 4 * nkeys > keys.count) return fail("tag 34735 (GeoKeyDirectory): %lld keys in %lld values", (long long)nkeys, keys.count);
    for (uint64_t k = 1; k <= nkeys; ++k) {
      const uint8_t* q = keys.at + 8 * k;
      const int id = le16(q), loc = le16(q + 2), value = le16(q + 6);
      if (loc != 0) continue;
      if (id == 1025) {
        if (value != 1 && value != 2) return fail("tag 34735 (GeoKeyDirectory): key 1025 (RasterType) %lld", value, 0);
        P.raster_type = value;
      } else if (id == 3072) {
        P.epsg = value;
      }
    }
  }
  if (geo) {
    if (!(gt[1] > 0.0) || !(gt[5] < 0.0) || !(gt[1] < 1e300) || !(gt[5] > -1e300))
      return fail("geo tags: only north-up rasters are read (pixel width > 0, pixel height < 0)", 0, 0);
    if (P.raster_type == 2) {   // the tiepoint is a pixel's centre: the area's corner lies half a pixel before it
      gt[0] = gt[0] - 0.5 * gt[1];
      gt[3] = gt[3] - 0.5 * gt[5];
    }
  }
  P.has_geo = geo ? 1 : 0;
  for (int k = 0; k < 6; ++k) P.gt[k] = gt[k];

  const Entry& nd = slot(42113);
  if (nd.have) {
    if (nd.type != 2) return fail("tag 42113 (GDAL_NODATA): field type %lld", nd.type, 0);
    char text[64];
    const size_t m = nd.count < sizeof(text) - 1 ? nd.count : sizeof(text) - 1;
    std::memcpy(text, nd.at, m);
    text[m] = 0;
    char* end = nullptr;
    const double v = std::strtod(text, &end);
    if (end == text) return fail("tag 42113 (GDAL_NODATA): no number in its %lld characters", nd.count, 0);
    P.has_nodata = 1;
    P.nodata = v;
  }
  return true;
}

// The whole file's first IFD -> *out, or false with a text in err.
inline bool parse(const uint8_t* file, size_t len, Parsed* out, char* err, size_t errcap) {
  uint64_t ifd = 0;
  if (!first_ifd(file, len, &ifd, err, errcap)) return false;
  return parse_ifd(file, len, ifd, out, err, errcap);
}

// ---- levels ------------------------------------------------------------------------
// Level 0 is IFD 0; level k >= 1 is the k-th later IFD of the chain whose NewSubfileType (254) has
// bit 0 (reduced resolution) set and bit 2 (mask) clear.  Masks and pages (254 absent, or bit 0
// clear) are passed over.  At most kMaxIfds IFDs; an offset that comes twice is refused.
constexpr size_t kMaxIfds = 64;

struct Ifd {
  uint64_t at;               // its offset
  uint32_t width, height;    // 256 / 257 where they are one SHORT or LONG, else 0
  bool overview;             // 254: bit 0 set, bit 2 clear
};

inline bool walk_chain(const uint8_t* file, size_t len, std::vector<Ifd>* ifds, char* err, size_t errcap) {
  auto fail = [&](const char* fmt, long long a, long long b) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
    return false;
  };
  ifds->clear();
  uint64_t at = 0;
  if (!first_ifd(file, len, &at, err, errcap)) return false;
  do {
    if (ifds->size() == kMaxIfds) return fail("the IFD chain has more than %lld IFDs", (long long)kMaxIfds, 0);
    for (const Ifd& seen : *ifds)
      if (seen.at == at) return fail("the IFD chain returns to the IFD at byte %lld", (long long)at, 0);
    if (at < 8 || at + 2 > len) return fail("the IFD at byte %lld lies outside the file", (long long)at, 0);
    const uint64_t n = le16(file + at);
    if (at + 2 + 12 * n + 4 > len) return fail("the IFD at byte %lld (%lld entries) runs past the file", (long long)at, (long long)n);
    Ifd d = {at, 0, 0, false};
    for (uint64_t k = 0; k < n; ++k) {
      const uint8_t* p = file + at + 2 + 12 * k;
      const int tag = le16(p), type = le16(p + 2);
      if ((tag != 254 && tag != 256 && tag != 257) || (type != 3 && type != 4) || le32(p + 4) != 1) continue;
      const uint32_t v = type == 3 ? le16(p + 8) : le32(p + 8);   // (one SHORT or LONG lies in the entry)
      if (tag == 254) d.overview = (v & 1u) && !(v & 4u);
      else if (tag == 256) d.width = v;
      else d.height = v;
    }
    ifds->push_back(d);
    at = le32(file + at + 2 + 12 * n);
  } while (at != 0);
  return true;
}

// the chain's levels: indices into ifds
inline std::vector<size_t> levels_of(const std::vector<Ifd>& ifds) {
  std::vector<size_t> lv(1, 0);
  for (size_t k = 1; k < ifds.size(); ++k)
    if (ifds[k].overview) lv.push_back(k);
  return lv;
}

// Level `level` of the file -> *out, *nlevels (may be null), or false with a text in err.  A level
// k >= 1 passes the checks of IFD 0 (the text names the level and the IFD), has IFD 0's kind, and
// no level up to it is larger than the one before it in either dimension, or as large in both.  Its
// geotransform is the base's with GT1 * W0 / Wk and GT5 * H0 / Hk (GDAL's rule); geo keys and nodata
// are the base's.
inline bool parse_level(const uint8_t* file, size_t len, int level, Parsed* out, int* nlevels, char* err, size_t errcap) {
  std::vector<Ifd> ifds;
  if (!walk_chain(file, len, &ifds, err, errcap)) return false;
  const std::vector<size_t> lv = levels_of(ifds);
  if (nlevels) *nlevels = (int)lv.size();
  if (level < 0 || (size_t)level >= lv.size()) {
    if (err && errcap) std::snprintf(err, errcap, "level %d: the file has %zu level%s", level, lv.size(), lv.size() == 1 ? "" : "s");
    return false;
  }
  Parsed base;
  if (!parse_ifd(file, len, ifds[0].at, &base, err, errcap)) return false;
  if (level == 0) {
    *out = base;
    return true;
  }
  for (int j = 1; j <= level; ++j) {
    const Ifd& a = ifds[lv[(size_t)j - 1]];
    const Ifd& b = ifds[lv[(size_t)j]];
    if (!a.width || !a.height || !b.width || !b.height) continue;   // (the level's own parse names the tag)
    if (b.width > a.width || b.height > a.height || (b.width == a.width && b.height == a.height)) {
      if (err && errcap)
        std::snprintf(err, errcap, "level %d (IFD %zu): %u x %u is not smaller than level %d, %u x %u", j, lv[(size_t)j],
                      b.width, b.height, j - 1, a.width, a.height);
      return false;
    }
  }
  const size_t m = lv[(size_t)level];
  char text[200];
  if (!parse_ifd(file, len, ifds[m].at, out, text, sizeof(text))) {
    if (err && errcap) std::snprintf(err, errcap, "level %d (IFD %zu at byte %llu): %s", level, m, (unsigned long long)ifds[m].at, text);
    return false;
  }
  if (out->kind != base.kind) {
    if (err && errcap)
      std::snprintf(err, errcap, "level %d (IFD %zu at byte %llu): its samples are of kind %d, level 0's of kind %d", level, m,
                    (unsigned long long)ifds[m].at, (int)out->kind, (int)base.kind);
    return false;
  }
  out->has_geo = base.has_geo;
  out->epsg = base.epsg;
  out->raster_type = base.raster_type;
  for (int k = 0; k < 6; ++k) out->gt[k] = base.gt[k];
  out->gt[1] = base.gt[1] * (double)base.width / (double)out->width;
  out->gt[5] = base.gt[5] * (double)base.height / (double)out->height;
  out->has_nodata = base.has_nodata;
  out->nodata = base.nodata;
  return true;
}

// The automatic choice for a map of resolution `res`: the coarsest level whose pixels are no larger
// than a cell in either direction (GT1_k <= res and -GT5_k <= res, compared as doubles); none: 0.
// base: level 0, parsed.
inline int auto_level(const Parsed& base, const std::vector<Ifd>& ifds, double res) {
  const std::vector<size_t> lv = levels_of(ifds);
  for (size_t k = lv.size(); k-- > 1;) {
    const Ifd& d = ifds[lv[k]];
    if (!d.width || !d.height) continue;
    const double gt1 = base.gt[1] * (double)base.width / (double)d.width;
    const double gt5 = base.gt[5] * (double)base.height / (double)d.height;
    if (gt1 <= res && -gt5 <= res) return (int)k;
  }
  return 0;
}

// the chunk's place in the layout, for error texts: "tile row 1, column 2" / "strip 3"
inline void chunk_name(const Parsed& p, size_t t, char* out, size_t cap) {
  if (p.tiled) std::snprintf(out, cap, "chunk %zu (tile row %zu, column %zu)", t, t / p.across, t % p.across);
  else std::snprintf(out, cap, "chunk %zu (strip %zu)", t, t);
}

}  // namespace tiffd
}  // namespace amhip

#endif  // AMHIP_TIFF_DECODE_HOST_H_
