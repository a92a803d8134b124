// amhip_png_decode_host.h -- the host-only part of the PNG decoder (amhip_png_decode.hip): the
// chunk parser, the per-frame descriptor the kernels read and the list of IDAT payloads that make
// one zlib stream.  No HIP in here: tests/cpp/png_decode_host_main.cc compiles it alone under the
// address and undefined-behaviour sanitizers.
//
// Accepted: the signature; IHDR first, 13 bytes, width and height 1..65535, bit depth 8, colour
// types 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha), 6 (RGBA), compression 0, filter 0, no
// interlace; PLTE (a multiple of 3, at most 768 bytes; needed and non-empty for colour type 3);
// one run of consecutive IDAT chunks (an empty one among them is fine); IEND.  The CRC of IHDR,
// PLTE, IDAT and IEND is checked; every other chunk is skipped as it is, CRC and all (tRNS and gAMA
// included); bytes behind IEND are ignored.  The zlib header (CM 8, CINFO <= 7, FCHECK, FDICT 0)
// and the four Adler-32 bytes are taken from the concatenated payloads: they may straddle chunks.
// Everything else is refused with a text that names the field or chunk.  Every read is checked
// against the file's length, and every span handed on lies inside the file.
#ifndef AMHIP_PNG_DECODE_HOST_H_
#define AMHIP_PNG_DECODE_HOST_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace amhip {
namespace pngd {

// what the kernels need of one file.  Offsets are into the buffer that holds the call's streams.
struct Frame {
  int32_t width, height;
  int32_t colour_type;      // 0, 2, 3, 4, 6
  int32_t bpp;              // bytes per pixel in the scanlines: 1, 3, 1, 2, 4
  int32_t plte_entries;     // 0: no PLTE
  uint32_t adler;           // the stream's trailer
  uint64_t stream_begin;    // first deflate byte (behind the two bytes of the zlib header)
  uint64_t stream_end;      // the Adler-32 trailer: no byte at or behind it is read
  uint64_t raw_len;         // height * (1 + width * bpp): the filtered scanlines
  uint64_t raw_base;        // the frame's first byte in the raw scratch (a multiple of 16)
  uint8_t plte[768];        // R, G, B per entry
};

struct Span {
  size_t begin, len;        // one IDAT payload in the file
};

struct Parsed {
  Frame f;
  std::vector<Span> idat;   // in file order; their bytes, concatenated, are the zlib stream
  size_t zlen;              // its length: header, deflate data, trailer
};

inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0) {
  static uint32_t table[256];
  static bool made = false;
  if (!made) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      table[i] = c;
    }
    made = true;
  }
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
  return ~crc;
}

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

inline int bytes_per_pixel(int colour_type) {
  switch (colour_type) {
    case 0: return 1;
    case 2: return 3;
    case 3: return 1;
    case 4: return 2;
    case 6: return 4;
  }
  return 0;
}

// byte k of the concatenated IDAT payloads (k < zlen)
inline uint8_t stream_byte(const uint8_t* file, const std::vector<Span>& idat, size_t k) {
  for (const Span& s : idat) {
    if (k < s.len) return file[s.begin + k];
    k -= s.len;
  }
  return 0;
}

// The whole file.  Returns true and fills *out (stream_begin / stream_end relative to the
// concatenated stream; raw_base left 0), or false with a text in err.
inline bool parse(const uint8_t* file, size_t len, Parsed* out, char* err, size_t errcap) {
  auto fail = [&](const char* fmt, int a, int b) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
    return false;
  };
  auto fail_chunk = [&](const char* fmt, const uint8_t* type) {
    char name[5];
    for (int i = 0; i < 4; ++i) name[i] = (type[i] >= 'A' && type[i] <= 'z') ? (char)type[i] : '?';
    name[4] = 0;
    if (err && errcap) std::snprintf(err, errcap, fmt, name);
    return false;
  };
  Frame* f = &out->f;
  std::memset(f, 0, sizeof(*f));
  out->idat.clear();
  out->zlen = 0;
  static const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (!file || len < 8 || std::memcmp(file, kSignature, 8) != 0) return fail("no PNG signature", 0, 0);
  size_t p = 8;
  bool have_ihdr = false, have_plte = false, have_iend = false, idat_open = false, idat_closed = false;
  while (!have_iend) {
    if (p == len) return fail(out->idat.empty() && !idat_open ? "no IDAT chunk" : "no IEND chunk", 0, 0);
    if (len - p < 8) return fail("truncated chunk header at byte %d", (int)p, 0);
    const uint32_t L = be32(file + p);
    const uint8_t* type = file + p + 4;
    // (length, type, payload, CRC: 12 + L bytes)
    if ((uint64_t)L + 12 > (uint64_t)(len - p)) {
      if (L > 0x7FFFFFFFu || (uint64_t)L > (uint64_t)len) return fail_chunk("chunk %s: its length runs past the file", type);
      return fail_chunk("chunk %s: truncated", type);
    }
    const uint8_t* pl = file + p + 8;
    const bool is_ihdr = std::memcmp(type, "IHDR", 4) == 0, is_plte = std::memcmp(type, "PLTE", 4) == 0;
    const bool is_idat = std::memcmp(type, "IDAT", 4) == 0, is_iend = std::memcmp(type, "IEND", 4) == 0;
    if (!have_ihdr && !is_ihdr) return fail("IHDR is not the first chunk", 0, 0);
    if (is_ihdr || is_plte || is_idat || is_iend) {
      if (crc32(type, (size_t)L + 4) != be32(pl + L)) return fail_chunk("chunk %s: bad CRC", type);
    } else if (!(type[0] & 0x20)) {
      return fail_chunk("unknown critical chunk %s", type);
    }
    if (idat_open && !is_idat) {
      idat_open = false;
      idat_closed = true;
    }
    if (is_ihdr) {
      if (have_ihdr) return fail("second IHDR", 0, 0);
      if (L != 13) return fail("IHDR: length %d", (int)L, 0);
      const uint32_t w = be32(pl), h = be32(pl + 4);
      if (w < 1 || w > 65535u || h < 1 || h > 65535u) return fail("IHDR: width or height outside 1..65535", 0, 0);
      const int depth = pl[8], ct = pl[9];
      if (!(ct == 0 || ct == 2 || ct == 3 || ct == 4 || ct == 6)) return fail("IHDR: colour type %d", ct, 0);
      if (depth != 8) return fail("IHDR: bit depth %d", depth, 0);
      if (pl[10] != 0) return fail("IHDR: compression method %d", pl[10], 0);
      if (pl[11] != 0) return fail("IHDR: filter method %d", pl[11], 0);
      if (pl[12] != 0) return fail("IHDR: interlace method %d (Adam7)", pl[12], 0);
      f->width = (int32_t)w;
      f->height = (int32_t)h;
      f->colour_type = ct;
      f->bpp = bytes_per_pixel(ct);
      f->raw_len = (uint64_t)h * (1u + (uint64_t)w * (uint64_t)f->bpp);
      have_ihdr = true;
    } else if (is_plte) {
      if (have_plte) return fail("second PLTE", 0, 0);
      if (!out->idat.empty() || idat_closed) return fail("PLTE behind IDAT", 0, 0);
      if (L == 0 || L % 3 != 0 || L > 768) return fail("PLTE: length %d", (int)L, 0);
      std::memcpy(f->plte, pl, L);
      f->plte_entries = (int32_t)(L / 3);
      have_plte = true;
    } else if (is_idat) {
      if (idat_closed) return fail("IDAT behind another chunk: the run of IDAT chunks is interrupted", 0, 0);
      idat_open = true;
      Span s;
      s.begin = p + 8;
      s.len = L;
      out->idat.push_back(s);
      out->zlen += L;
    } else if (is_iend) {
      have_iend = true;
    }
    p += 12 + (size_t)L;
  }
  if (out->idat.empty()) return fail("no IDAT chunk", 0, 0);
  if (f->colour_type == 3 && !have_plte) return fail("colour type 3 without a PLTE chunk", 0, 0);
  if (out->zlen < 6) return fail("IDAT: %d bytes are no zlib stream", (int)out->zlen, 0);
  const int cmf = stream_byte(file, out->idat, 0), flg = stream_byte(file, out->idat, 1);
  if ((cmf & 15) != 8) return fail("zlib header: compression method %d", cmf & 15, 0);
  if ((cmf >> 4) > 7) return fail("zlib header: CINFO %d", cmf >> 4, 0);
  if ((cmf * 256 + flg) % 31 != 0) return fail("zlib header: FCHECK", 0, 0);
  if (flg & 0x20) return fail("zlib header: FDICT set", 0, 0);
  f->adler = 0;
  for (size_t k = 0; k < 4; ++k) f->adler = (f->adler << 8) | stream_byte(file, out->idat, out->zlen - 4 + k);
  f->stream_begin = 2;
  f->stream_end = out->zlen - 4;
  return true;
}

// the concatenated payloads, zlen bytes, to dst
inline void concat(const uint8_t* file, const Parsed& p, uint8_t* dst) {
  for (const Span& s : p.idat) {
    if (s.len) std::memcpy(dst, file + s.begin, s.len);
    dst += s.len;
  }
}

// status words the kernels leave per frame
enum Status : uint32_t {
  kOk = 0,
  kBadCode = 1,          // a bit pattern no code has, or a symbol outside the alphabet
  kOverSubscribed = 2,
  kIncomplete = 3,
  kBadDynHeader = 4,     // HLIT > 286, HDIST > 30, a repeat without a previous length or past HLIT + HDIST,
                         // or no end-of-block code
  kBadBlockType = 5,
  kBadStoredLen = 6,
  kDistTooFar = 7,
  kEndsEarly = 8,
  kTooShort = 9,
  kTooLong = 10,
  kBadFilter = 11,
  kBadAdler = 12,
  kBadIndex = 13,
};

inline const char* status_text(uint32_t s) {
  switch (s) {
    case kOk: return "ok";
    case kBadCode: return "an undefined Huffman code";
    case kOverSubscribed: return "an over-subscribed set of code lengths";
    case kIncomplete: return "an incomplete set of code lengths";
    case kBadDynHeader: return "a dynamic block's header is out of range (HLIT, HDIST, a repeat, or no end-of-block code)";
    case kBadBlockType: return "block type 3";
    case kBadStoredLen: return "a stored block's LEN is not ~NLEN";
    case kDistTooFar: return "a distance that reaches behind the first output byte";
    case kEndsEarly: return "the stream ends before its final block does";
    case kTooShort: return "the stream holds fewer bytes than the image's scanlines";
    case kTooLong: return "the stream holds more bytes than the image's scanlines";
    case kBadFilter: return "a filter type above 4";
    case kBadAdler: return "an Adler-32 mismatch";
    case kBadIndex: return "a palette index outside PLTE";
  }
  return "unknown status";
}

}  // namespace pngd
}  // namespace amhip

#endif  // AMHIP_PNG_DECODE_HOST_H_
