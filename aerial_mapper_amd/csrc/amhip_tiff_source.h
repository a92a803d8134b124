// amhip_tiff_source.h -- where a GeoTIFF call's samples come from and how a pixel is read: what the
// tile producer (amhip_tiff_encode.hip) and the overview reduction (amhip_tiff_overview.hip) share,
// so that level 1 of a layer call reduces exactly the pixels level 0 holds.  DESIGN 4.16, 4.18.
#ifndef AMHIP_TIFF_SOURCE_H_
#define AMHIP_TIFF_SOURCE_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amhip_layer_image.h"
#include "amhip_tiff_host.h"

namespace amhip {

// where a call's samples come from
struct TileSrc {
  const void* base;          // layer: the window's floats, column-major; raster: row-major pixels
  unsigned long long step;   // layer: floats per column (the window's rows); raster: bytes per row
  int width, height;         // of the raster
  uint32_t side, across;     // tile side, tiles per row of tiles
  uint32_t row_bytes;        // side * bytes per pixel
  uint32_t first;            // the launch's first tile of this raster
  uint32_t frame0;           // ... and the frame of the group's buffers it goes to
  float lower, upper;        // u8 from a layer
};

// Pixel (r, c) of the raster as it lies in the file before the predictor, lowest byte first: the
// float's bits, the byte, or R | G << 8 | B << 16.  Outside the raster: zero.
// A layer: raster pixel (r, c) is cell (i, j) = (width - 1 - c, r) of the window, so
// along a raster row the reads walk a layer column backwards, one float after the other.
template <int kKind, bool kLayer>
__device__ __forceinline__ uint32_t fetch(const TileSrc& src, uint32_t r, uint32_t c) {
  if (r >= (uint32_t)src.height || c >= (uint32_t)src.width) return 0;
  if (kLayer) {
    const float v = static_cast<const float*>(src.base)[(size_t)((uint32_t)src.width - 1u - c) + (size_t)r * src.step];
    if (kKind == tiff::kF32) return __float_as_uint(v);
    if (kKind == tiff::kU8) return to_image_u8(v, src.lower, src.upper);
    const uint32_t bits = (v == v) ? __float_as_uint(v) : 0u;   // packed R << 16 | G << 8 | B
    return ((bits >> 16) & 255u) | (bits & 0xFF00u) | ((bits & 255u) << 16);
  }
  const uint8_t* p = static_cast<const uint8_t*>(src.base) + (size_t)r * src.step;
  if (kKind == tiff::kF32) {
    p += (size_t)c * 4u;
    if ((reinterpret_cast<size_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
  if (kKind == tiff::kU8) return p[c];
  p += (size_t)c * 3u;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// amhip_tiff_overview.hip: the raster `src` describes (from a layer or row-major) -> its reduction by
// two, ceil(width / 2) x ceil(height / 2) pixels, row-major and tightly packed at
// `dst`.  Asynchronous on `stream`.
int tovr_reduce(hipStream_t stream, int kind, bool from_layer, const TileSrc& src, void* dst);

}  // namespace amhip

#endif  // AMHIP_TIFF_SOURCE_H_
