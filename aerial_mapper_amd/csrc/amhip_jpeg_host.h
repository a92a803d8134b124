// amhip_jpeg_host.h -- the host-only part of the JPEG encoder (amhip_jpeg.hip): libjpeg's
// standard tables, jpeg_set_quality's table scaling, the canonical Huffman codes and the header
// segments of a baseline file.  No HIP in here: tests/cpp/jpeg_host_main.cc compiles it alone
// under the address and undefined-behaviour sanitizers.
#ifndef AMHIP_JPEG_HOST_H_
#define AMHIP_JPEG_HOST_H_

#include <cstddef>
#include <cstdint>

namespace amhip {
namespace jpeg {

// jpeg_natural_order (jutils.c): zigzag position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// std_luminance_quant_tbl / std_chrominance_quant_tbl (jcparam.c), natural order
constexpr uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
     14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// std_huff_tables (jcparam.c): codes per length 1..16, then the symbols
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// What the entropy kernels look up: per table (0 luminance, 1 chrominance) the DC categories
// 0..11 and the 256 run/size symbols, each entry = code | length << 16 (0: no such symbol).
struct HuffTables {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};

// jpeg_make_c_derived_tbl (jchuff.c): canonical codes, counted up within a length
constexpr HuffTables make_huff_tables() {
  HuffTables t = {};
  for (int tbl = 0; tbl < 2; ++tbl) {
    for (int kind = 0; kind < 2; ++kind) {
      const uint8_t* bits = kind ? kAcBits[tbl] : kDcBits[tbl];
      const uint8_t* vals = kind ? kAcVals[tbl] : kDcVals;
      uint32_t code = 0;
      int k = 0;
      for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) {
          const uint32_t e = code | ((uint32_t)len << 16);
          if (kind) t.ac[tbl][vals[k]] = e;
          else t.dc[tbl][vals[k]] = e;
          ++code;
          ++k;
        }
        code <<= 1;
      }
    }
  }
  return t;
}

// quality 1..100 -> both tables in natural order (jpeg_quality_scaling, jpeg_add_quant_table with
// force_baseline: (base * scale + 50) / 100 clamped to 1..255)
inline void quant_tables(int quality, uint8_t out[2][64]) {
  if (quality < 1) quality = 1;
  if (quality > 100) quality = 100;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      int v = ((int)kStdQuant[t][i] * scale + 50) / 100;
      out[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// the longest code one block can take, in bytes: the DC code (<= 11 bits) and its value (<= 11),
// 63 coefficients of a 16-bit code and a 10-bit value each
constexpr size_t kMaxBlockBytes = (11 + 11 + 63 * (16 + 10) + 7) / 8;
// SOI, APP0, two DQT, SOF0 with three components, four DHT, SOS with three components
constexpr size_t kMaxHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14;

// blocks the scan codes: gray block by block; colour in MCUs of 16 x 16 pixels, 4 + 1 + 1 blocks
inline size_t scan_blocks(int width, int height, int channels) {
  if (channels == 1) return (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
  return (size_t)((width + 15) / 16) * (size_t)((height + 15) / 16) * 6u;
}

// worst-case file size: headers, every block at its longest, every byte stuffed, EOI
inline size_t file_bound(int width, int height, int channels) {
  return kMaxHeaderBytes + 2 * (scan_blocks(width, height, channels) * kMaxBlockBytes + 1) + 2;
}

// write_file_header, write_frame_header, write_scan_header (jcmarker.c): SOI, APP0 (JFIF 1.01, no
// units, density 1 x 1), one DQT per table, SOF0, one DHT per table (DC, AC per component), SOS.
// Gray files declare their one component 2 x 2 as Pillow's subsampling=2 does (a one-component
// scan is not interleaved, so nothing else changes).  Returns the bytes written, 0 when `cap` is
// too small.
inline size_t write_header(uint8_t* out, size_t cap, int width, int height, int channels, int quality) {
  if (cap < kMaxHeaderBytes) return 0;
  uint8_t* p = out;
  auto marker = [&](uint8_t m, size_t payload) {
    *p++ = 0xFF;
    *p++ = m;
    *p++ = (uint8_t)((payload + 2) >> 8);
    *p++ = (uint8_t)((payload + 2) & 255);
  };
  *p++ = 0xFF;
  *p++ = 0xD8;
  marker(0xE0, 14);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (uint8_t b : jfif) *p++ = b;
  uint8_t q[2][64];
  quant_tables(quality, q);
  const int ntab = channels == 1 ? 1 : 2;
  for (int t = 0; t < ntab; ++t) {
    marker(0xDB, 65);
    *p++ = (uint8_t)t;
    for (int z = 0; z < 64; ++z) *p++ = q[t][kZigzag[z]];
  }
  marker(0xC0, 6 + 3 * (size_t)channels);
  *p++ = 8;
  *p++ = (uint8_t)(height >> 8);
  *p++ = (uint8_t)(height & 255);
  *p++ = (uint8_t)(width >> 8);
  *p++ = (uint8_t)(width & 255);
  *p++ = (uint8_t)channels;
  for (int c = 0; c < channels; ++c) {
    *p++ = (uint8_t)(c + 1);
    *p++ = c == 0 ? 0x22 : 0x11;
    *p++ = c == 0 ? 0 : 1;
  }
  for (int t = 0; t < ntab; ++t)
    for (int kind = 0; kind < 2; ++kind) {
      const size_t nvals = kind ? 162 : 12;
      marker(0xC4, 1 + 16 + nvals);
      *p++ = (uint8_t)((kind << 4) | t);
      const uint8_t* bits = kind ? kAcBits[t] : kDcBits[t];
      const uint8_t* vals = kind ? kAcVals[t] : kDcVals;
      for (int i = 0; i < 16; ++i) *p++ = bits[i];
      for (size_t i = 0; i < nvals; ++i) *p++ = vals[i];
    }
  marker(0xDA, 1 + 2 * (size_t)channels + 3);
  *p++ = (uint8_t)channels;
  for (int c = 0; c < channels; ++c) {
    *p++ = (uint8_t)(c + 1);
    *p++ = c == 0 ? 0x00 : 0x11;
  }
  *p++ = 0;
  *p++ = 63;
  *p++ = 0;
  return (size_t)(p - out);
}

// the argument rules every encoder entry point shares; nullptr when they hold
inline const char* check_image_args(size_t step, int width, int height, int channels, int quality) {
  if (channels != 1 && channels != 3) return "channels must be 1 (8UC1) or 3 (8UC3, B G R)";
  if (quality < 0 || quality > 100) return "quality must be 1..100 (0: 95)";
  if (width < 1 || width > 65535 || height < 1 || height > 65535) return "width and height must be 1..65535";
  if (step < (size_t)width * (size_t)channels) return "step smaller than an image row";
  return nullptr;
}

}  // namespace jpeg
}  // namespace amhip

#endif  // AMHIP_JPEG_HOST_H_
