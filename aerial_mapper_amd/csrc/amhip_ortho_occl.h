// amhip_ortho_occl.h -- the occlusion test of the true-ortho mosaic:
// is the surface between a cell and a camera in the way?  One function, host + device: the kernel
// (amhip_ortho_occl.hip) and the stand-alone program of the unit tests
// (tests/cpp/ortho_occl_host_main.cc) compile the same march.
//
// The rule.  All arithmetic FP64, every operation rounded on its own (the library is built with
// -ffp-contract=off; no fma here), in the order written:
//   h = (double)elevation(i, j); NaN: not occluded (the pair is invisible anyway)
//   di = (x_c - tx) / res, dj = (y_c - ty) / res    the ray in index space: a step towards the
//                                                   camera is a step of (di, dj) / m cells
//   m = max(|di|, |dj|), dz = tz - h; !(dz > 0): not occluded
//   for k = 1, 2, ... while (double)k < m:
//     s = (double)k / m
//     ii = i + (int)rint(s * di), jj = j + (int)rint(s * dj)     rint: round half to even
//     (ii, jj) outside the map: stop, not occluded
//     z = h + s * dz
//     (double)elevation(ii, jj) > z + margin: occluded          strict; a NaN sample is false
//   not occluded
// One cell per step along the ray's major axis, so k = 1 is never the cell itself, and a camera
// within one cell of the cell (m <= 1) makes no step.
#ifndef AMHIP_ORTHO_OCCL_H_
#define AMHIP_ORTHO_OCCL_H_

#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define AMHIP_OCCL_HD __host__ __device__ __forceinline__
#else
#define AMHIP_OCCL_HD inline
#endif

namespace amhip {

constexpr int kOcclBatch = 4;

// elevation: rows x cols, column-major (cell (i, j) at i + j * rows), the whole map.
// (x_c, y_c): the centre of cell (i, j) (amhip_cell_position); h: (double)elevation(i, j);
// (tx, ty, tz): the camera centre in the map frame; margin >= 0 (+inf: nothing occludes).
// zcut: the march stops (not occluded) as soon as z exceeds it.  Exact for any zcut >= the
// largest finite elevation of the map: z only grows along the ray (dz > 0), and no sample above
// z + margin >= z can exist beyond that point.  +inf: no cut-off.
// A camera centre that is not finite makes no step (its pairs are invisible: the projection of
// the cell is NaN), so the index arithmetic below never sees a NaN.
AMHIP_OCCL_HD bool occl_march(const float* elevation, int rows, int cols, int i, int j, double x_c,
                              double y_c, double h, double tx, double ty, double tz, double res,
                              double margin, double zcut) {
  if (h != h) return false;
  const double di = (x_c - tx) / res;
  const double dj = (y_c - ty) / res;
  const double adi = std::fabs(di), adj = std::fabs(dj);
  const double m = adi > adj ? adi : adj;
  const double dz = tz - h;
  if (!(dz > 0.0)) return false;
  if (!(m <= 1.7976931348623157e308)) return false;  // (inf or NaN)
  // kOcclBatch steps at a time: first the samples of the batch (independent loads, in flight
  // together -- a step at a time the march is a chain of dependent memory round trips), then
  // their outcomes in the order of k, so that the first event along the ray decides as in the
  // rule.  A sample behind that event was read for nothing; it is read only if it lies in the map.
  for (int k0 = 1; (double)k0 < m; k0 += kOcclBatch) {
    double z[kOcclBatch];
    float e[kOcclBatch];
    int state[kOcclBatch];  // 0: a sample, 1: outside the map, 2: beyond the camera (k >= m)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int b = 0; b < kOcclBatch; ++b) {
      const int k = k0 + b;
      z[b] = 0.0;
      e[b] = 0.0f;
      state[b] = 2;
      if (!((double)k < m)) continue;
      const double s = (double)k / m;
      const double oi = std::rint(s * di), oj = std::rint(s * dj);
      // (|oi|, |oj| <= k + 1, but a cell index plus that may still leave int: compare as doubles)
      const double fi = (double)i + oi, fj = (double)j + oj;
      state[b] = 1;
      if (!(fi >= 0.0 && fi < (double)rows && fj >= 0.0 && fj < (double)cols)) continue;
      state[b] = 0;
      z[b] = h + s * dz;
      e[b] = elevation[(size_t)(int)fi + (size_t)(int)fj * (size_t)rows];
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int b = 0; b < kOcclBatch; ++b) {
      if (state[b] != 0) return false;
      if (z[b] > zcut) return false;
      if ((double)e[b] > z[b] + margin) return true;
    }
  }
  return false;
}

}  // namespace amhip

#endif  // AMHIP_ORTHO_OCCL_H_
