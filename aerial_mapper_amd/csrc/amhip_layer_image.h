// amhip_layer_image.h -- a layer's cell as a pixel: what the layer-to-image kernels
// (amhip_export.hip) and the GeoTIFF tile producer (amhip_tiff_encode.hip) both apply.
#ifndef AMHIP_LAYER_IMAGE_H_
#define AMHIP_LAYER_IMAGE_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace amhip {

// toImage(): image = zeros(size(0), size(1)); the layer is clamped to [lower, upper]; every cell
// with a finite value becomes (uchar)(((v - lower) / (upper - lower)) * (float)255) -- float
// arithmetic, truncating cast; the others stay 0.
__device__ __forceinline__ uint8_t to_image_u8(float v, float lower, float upper) {
  if (!isfinite(v)) return 0;
  v = fminf(fmaxf(v, lower), upper);
  const float t = ((v - lower) / (upper - lower)) * 255.0f;
  return (uint8_t)(int)t;
}

}  // namespace amhip

#endif  // AMHIP_LAYER_IMAGE_H_
