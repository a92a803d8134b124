// amhip_ortho_blend.h -- the arithmetic of the blended backward-grid mosaic (DESIGN.md section
// 4.20): the weight of one contributing (cell, frame) pair and the value a cell's sums end in.
// Host + device: the kernel (amhip_ortho_blend.hip) and the stand-alone program of the unit tests
// (tests/cpp/ortho_blend_host_main.cc) compile the same functions.
//
// The rule.  All arithmetic FP64, every operation rounded on its own (the library is built with
// -ffp-contract=off; no fma here), in the order written.  (cx, cy, cz): the cell's landmark in the
// camera frame (transform_point); I: the pair's nearest pixel, the plain mosaic's keypoint.
//   zz = cz * cz; n2 = (cx * cx + cy * cy) + zz; s2 = zz / n2        sin^2 of the view angle
//   w = s2; `sharpness` times: w = w * w                              sin^2 .. sin^32
//   acc = acc + w * (double)I  (per channel);  wsum = wsum + w        frames ascending
//   at the end of a call, wsum > 0:  value = rint(acc / wsum)         round half to even
#ifndef AMHIP_ORTHO_BLEND_H_
#define AMHIP_ORTHO_BLEND_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AMHIP_BLEND_HD __host__ __device__ __forceinline__
#else
#define AMHIP_BLEND_HD inline
#endif

namespace amhip {

constexpr int kBlendMaxSharpness = 4;

// zz = cz * cz and n2 = (cx * cx + cy * cy) + zz are the fold's own terms: the caller has them
AMHIP_BLEND_HD double blend_weight(double zz, double n2, int sharpness) {
  double w = zz / n2;
  for (int s = 0; s < sharpness; ++s) w = w * w;
  return w;
}

// one channel of a cell with wsum > 0: a weighted mean of bytes, so 0 .. 255 after the rounding
AMHIP_BLEND_HD double blend_value(double acc, double wsum) { return std::rint(acc / wsum); }

// the three channels as colorVectorToValue packs them (R << 16 | G << 8 | B, the bits as a float)
AMHIP_BLEND_HD uint32_t blend_pack_bgr(double b, double g, double r) {
  return ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
}

}  // namespace amhip

#endif  // AMHIP_ORTHO_BLEND_H_
