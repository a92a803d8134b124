// amhip_ortho_dev.h -- device functions the backward-grid mosaic kernels share (amhip_ortho.hip,
// amhip_ortho_occl.hip): one pair in the reference's arithmetic (distortion, projection and
// visibility test, view angle), the conservative frame cull against a bounding sphere, and a
// cell's write-back.
#ifndef AMHIP_ORTHO_DEV_H_
#define AMHIP_ORTHO_DEV_H_

#include "amhip_common.h"
#include "amhip_atan_cr.h"
#include "amhip_device.h"

namespace amhip {

// V3, cross3, transform_point, exact_view_inline, fold_init / fold_pair / fold_finish: amhip_ortho_fold.h

__device__ __forceinline__ void distort_point(const OrthoParams& p, double* px,
                                              double* py) {
  double x = *px, y = *py;
  if (p.distortion == AMHIP_DIST_RADTAN) {
    const double k1 = p.dist[0], k2 = p.dist[1], p1 = p.dist[2], p2 = p.dist[3];
    const double mx2 = x * x;
    const double my2 = y * y;
    const double mxy = x * y;
    const double rho2 = mx2 + my2;
    const double rad = k1 * rho2 + k2 * rho2 * rho2;
    const double nx = x + (x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2));
    const double ny = y + (y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2));
    x = nx;
    y = ny;
  } else if (p.distortion == AMHIP_DIST_EQUIDISTANT) {
    const double r = sqrt(x * x + y * y);
    // atan to 76 bits, rounded once (amhip_atan_cr.h: the correctly rounded value in all but one
    // call in ~8 million) -- what a host libm returns in 99.9 % of its calls (glibc 2.35),
    // whichever libm that is; the device library's own differs from the host's by an ulp far
    // more often, and an ulp here can move a keypoint across a pixel boundary
    const double theta = atan_device(r);
    const double th2 = theta * theta;
    const double th4 = th2 * th2;
    const double th6 = th4 * th2;
    const double th8 = th4 * th4;
    const double thetad =
        theta * (1.0 + p.dist[0] * th2 + p.dist[1] * th4 + p.dist[2] * th6 +
                 p.dist[3] * th8);
    const double scaling = (r > 1e-8) ? thetad / r : 1.0;
    x = x * scaling;
    y = y * scaling;
  }
  *px = x;
  *py = y;
}

// aslam::PinholeCamera::project3 + the visibility test of
// ortho-backward-grid.cc:164-171.
__device__ __forceinline__ bool project_visible(const OrthoParams& p,
                                                const V3& c, double* u,
                                                double* v) {
  const double rz = 1.0 / c.z;
  double kx = c.x * rz;
  double ky = c.y * rz;
  if (p.distortion != AMHIP_DIST_NONE) distort_point(p, &kx, &ky);
  *u = p.fu * kx + p.cu;
  *v = p.fv * ky + p.cv;
  const bool in_box = (*u >= 0.0) && (*v >= 0.0) && (*u < (double)p.width) &&
                      (*v < (double)p.height);
  // status not in {POINT_BEHIND_CAMERA, PROJECTION_INVALID} <=> z > 1e-10
  return in_box && (c.z > 1e-10);
}

// asin(|z| / ||p||) exactly as the reference evaluates it
// (ortho-backward-grid.cc:173-176).  Deliberately NOT inlined: it is needed
// once per cell and in rare near ties, and inlining libm's asin three times per
// unrolled cell costs ~25 VGPRs (one wave per SIMD of occupancy).
__device__ __noinline__ double view_angle(double abs_z, double n2) {
  const double norm = sqrt(n2);
  return asin(abs_z / norm);
}

__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

// Can the frame with pose T (= T_C_G) see any point of the sphere?  Conservative:
// false only if the sphere lies entirely behind the camera or outside one of
// the four side planes of the view pyramid.
__device__ __forceinline__ bool frame_may_see(const OrthoParams& p, const FramePose& T,
                                              const V3& centre, double radius) {
  const V3 cc = transform_point(T, centre);
  bool keep = !(cc.z < -radius);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = p.pl[k][0] * cc.x + p.pl[k][1] * cc.y + p.pl[k][2] * cc.z;
    if (d < -radius) keep = false;
  }
  return keep;
}

// aerial-mapper-grid-map.cc:40-48: elevation_angle 0, observation_index NaN,
// ortho 255 / colored_ortho NaN
__device__ __forceinline__ void write_initial(const OrthoParams& p, float* __restrict__ angle,
                                              float* __restrict__ index, float* __restrict__ out,
                                              int i, int j) {
  const size_t at = (size_t)i + (size_t)j * (size_t)p.rows;
  angle[at] = 0.0f;
  index[at] = __builtin_nanf("");
  out[at] = p.colored ? __builtin_nanf("") : 255.0f;
}

// a wave-uniform double, moved to scalar registers
__device__ __forceinline__ double uniform_d(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// The sampled pixel of a cell's winning view as the output layer stores it
// (ortho-backward-grid.cc:186-208).
__device__ __forceinline__ float read_pixel(const OrthoParams& p, const uint8_t* __restrict__ frames,
                                            int frame, int kp_x, int kp_y) {
  const uint8_t* px = frames + (size_t)frame * p.frame_stride + (size_t)kp_y * p.row_step;
  if (p.colored) {
    // cv::Vec3b = (B, G, R); colorVectorToValue packs R<<16 | G<<8 | B
    px += (size_t)kp_x * 3u;
    const unsigned bits = ((unsigned)px[2] << 16) | ((unsigned)px[1] << 8) | (unsigned)px[0];
    return __uint_as_float(bits);
  }
  return (float)px[kp_x];
}

// One cell's results (ortho-backward-grid.cc:181-208): angle, frame index, the
// `num_observations += itself` updates and the sampled pixel.
__device__ __forceinline__ void store_cell(const OrthoParams& p, float* __restrict__ elevation_angle,
                                           float* __restrict__ observation_index,
                                           float* __restrict__ num_observations,
                                           float* __restrict__ out_layer, int i, int j, float angle,
                                           int frame, int accepted, float pixel) {
  const size_t at = (size_t)i + (size_t)j * (size_t)p.rows;
  elevation_angle[at] = angle;
  observation_index[at] = (float)frame;
  // layer_num_observations(x, y) += layer_num_observations(x, y), once per
  // accepted update (ortho-backward-grid.cc:183): doubles the stored value.
  if (!p.virt_nobs) {
    float nobs = num_observations[at];
    if (nobs != 0.0f) {
      for (int n = 0; n < accepted; ++n) nobs += nobs;
      num_observations[at] = nobs;
    }
  }
  out_layer[at] = pixel;
}

__device__ __forceinline__ void write_cell(const OrthoParams& p, const uint8_t* __restrict__ frames,
                                           float* __restrict__ elevation_angle,
                                           float* __restrict__ observation_index,
                                           float* __restrict__ num_observations,
                                           float* __restrict__ out_layer, int i, int j, float angle,
                                           int frame, int accepted, int kp_x, int kp_y) {
  store_cell(p, elevation_angle, observation_index, num_observations, out_layer, i, j, angle, frame,
             accepted, read_pixel(p, frames, frame, kp_x, kp_y));
}

}  // namespace amhip

#endif  // AMHIP_ORTHO_DEV_H_
