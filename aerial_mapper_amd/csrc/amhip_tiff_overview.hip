// amhip_tiff_overview.hip -- the overview levels of the GeoTIFF writer: level k from
// level k - 1 by the average of the 2 x 2 block, clipped at an odd edge.
//   k_tovr_reduce   a lane per output pixel, a row of the output per blockIdx.y.  It reads its (at
//                   most) four source pixels through fetch<> of the tile producer -- so level 1 of a
//                   layer call reduces the pixels level 0 holds, without a level-0 raster -- and
//                   writes a row-major, tightly packed raster in the sample type.
// f32: NaN is nodata; the others are added as doubles in the fixed order (2r, 2c), (2r, 2c + 1),
// (2r + 1, 2c), (2r + 1, 2c + 1) and the sum divided by their number, one IEEE operation each
// (-ffp-contract=off, no fast-math); none: the quiet NaN 0x7FC00000.  u8 / rgb8: (sum + n / 2) / n per
// band over the n pixels of the clipped block.  rgb8 reads and writes single bytes (a pixel has
// three; neighbouring lanes' bytes share cache lines); no LDS in any form.
#include "amhip_common.h"
#include "amhip_tiff_source.h"

namespace amhip {

namespace {

// Stores: pixel (r, c) of the output at dst + (r * w + c) * bytes per pixel, r < h, c < w: inside the
// w * h pixels the caller allocated.  Loads: fetch<> is called for pixels inside the source only.
template <int kKind, bool kLayer>
__global__ void __launch_bounds__(256) k_tovr_reduce(TileSrc src, uint8_t* dst, uint32_t w, uint32_t h) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x, r = blockIdx.y;
  if (c >= w || r >= h) return;
  const uint32_t sw = (uint32_t)src.width, sh = (uint32_t)src.height;
  const size_t at = (size_t)r * w + c;
  if (kKind == tiff::kF32) {
    double s = 0.0;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t sr = 2u * r + (k >> 1), sc = 2u * c + (k & 1u);
      if (sr < sh && sc < sw) {
        const float v = __uint_as_float(fetch<kKind, kLayer>(src, sr, sc));
        if (v == v) {
          s = s + (double)v;
          ++n;
        }
      }
    }
    // (+inf with -inf gives a NaN whose sign is the processor's choice: every NaN is written as the
    // one nodata value, so that the file does not depend on where it was computed)
    float out = n ? (float)(s / (double)n) : 0.0f;
    if (!n || out != out) out = __uint_as_float(0x7FC00000u);
    reinterpret_cast<float*>(dst)[at] = out;   // (dst comes from hipMalloc: aligned)
  } else {
    uint32_t sum[3] = {0, 0, 0}, n = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t sr = 2u * r + (k >> 1), sc = 2u * c + (k & 1u);
      if (sr < sh && sc < sw) {
        const uint32_t v = fetch<kKind, kLayer>(src, sr, sc);
        sum[0] += v & 255u;
        sum[1] += (v >> 8) & 255u;
        sum[2] += (v >> 16) & 255u;
        ++n;
      }
    }
    // (n is 1, 2 or 4: r < h = ceil(sh / 2) and c < w = ceil(sw / 2) put (2r, 2c) inside the source)
    const uint32_t half = n >> 1, sh_n = n == 4 ? 2u : n == 2 ? 1u : 0u;
    if (kKind == tiff::kU8) {
      dst[at] = (uint8_t)((sum[0] + half) >> sh_n);
    } else {
      dst[3u * at] = (uint8_t)((sum[0] + half) >> sh_n);
      dst[3u * at + 1u] = (uint8_t)((sum[1] + half) >> sh_n);
      dst[3u * at + 2u] = (uint8_t)((sum[2] + half) >> sh_n);
    }
  }
}

template <int kKind>
void launch(hipStream_t stream, bool from_layer, const TileSrc& src, uint8_t* dst, uint32_t w, uint32_t h) {
  const dim3 grid((w + 255u) / 256u, h);
  if (from_layer) hipLaunchKernelGGL((k_tovr_reduce<kKind, true>), grid, dim3(256), 0, stream, src, dst, w, h);
  else hipLaunchKernelGGL((k_tovr_reduce<kKind, false>), grid, dim3(256), 0, stream, src, dst, w, h);
}

}  // namespace

int tovr_reduce(hipStream_t stream, int kind, bool from_layer, const TileSrc& src, void* dst) {
  const uint32_t w = ((uint32_t)src.width + 1u) / 2u, h = ((uint32_t)src.height + 1u) / 2u;   // (h <= 32768: a grid.y)
  uint8_t* out = static_cast<uint8_t*>(dst);
  if (kind == tiff::kF32) launch<tiff::kF32>(stream, from_layer, src, out, w, h);
  else if (kind == tiff::kU8) launch<tiff::kU8>(stream, from_layer, src, out, w, h);
  else launch<tiff::kRgb8>(stream, from_layer, src, out, w, h);
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

}  // namespace amhip
