// amhip_stereo.hip -- semi-global block matching (OpenCV's StereoSGBM, MODE_SGBM, 8UC1) on MI355X.
//
// Replaces stereo::BlockMatchingSGBM::computeDisparityMap
//   aerial_mapper_dense_pcl/src/block-matching-sgbm.cpp (cv::StereoSGBM::compute, then / 16 and the
//   rectification mask), the step between amhip_rectify_stereo_pair_dev and amhip_densify_dev.
// The rules are those of tests/sgbm_reference.py (a NumPy restatement of OpenCV's stereosgbm.cpp);
// this file reproduces it bit for bit (tests/test_gpu_sgbm.py).  Every step is integer arithmetic.
//
//   k_sgbm_hsum     per (row, 64-column tile): the two prefiltered channels of both images in LDS,
//                   the Birchfield-Tomasi pixel cost (8 bits) of the tile + halo in LDS, its
//                   horizontal box sum (columns replicated) -> hsum (uint16, in the S buffer)
//   k_sgbm_vsum     per (column, disparity) and 32-row chunk: the vertical running sum -> C (uint16)
//   k_sgbm_path     one wave walks one chain of one direction (row, column or diagonal), the
//                   disparities across the lanes (d = 64 j + lane), d +- 1 by lane shuffles, minLr
//                   by a wave reduction; the first direction writes S, the next three add to it, the
//                   last (right -> left) adds its Lr and picks the winner: uniqueness, subpixel,
//                   disp1 and the right-image map disp2 (64-bit atomicMin on (minS, 0xFFFF - x))
//   k_sgbm_lrcheck  the left-right check against disp2
//   k_sgbm_median   3x3 median, borders replicated
//   k_sgbm_uf_*     filterSpeckles: union-find over the 4-connected relation (halving only while
//                   uniting), then each pixel's root read without writes, region sizes by atomics
//   k_sgbm_final    small regions -> invalid, CV_16S out, float / 16 with the mask
// C + S + hsum and the maps live in the context's scratch (amhip::Ctx::stereo_ws), grown on demand;
// block matching (below) carves its own layout out of the same block.
//
// Batches (amhip_*_disparity_batch_dev): blockIdx.z is the pair.  Pair b reads its images and mask
// and writes its outputs at base + b * batch stride; its scratch is the single-pair layout at
// b * (scratch bytes of one pair).  Every index a kernel forms (rows, columns, chains, union-find
// labels, the disp2 keys) is an index into the pair's own arrays, so nothing crosses from one pair
// into the next, and a batch of one is the single-pair call.
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>

#include "amhip_common.h"

namespace amhip {

constexpr int kSgbmTX = 64;        // output columns per k_sgbm_hsum workgroup
constexpr int kSgbmMaxSW2 = 5;     // block_size <= 11
constexpr int kSgbmMaxD = 256;
constexpr int kSgbmVRows = 32;     // rows per k_sgbm_vsum chunk
constexpr int kSgbmInf = 1 << 28;  // Lr at d = -1 / d >= D ("MAX_COST")

struct SgbmDims {
  int W, H, minD, maxD, D, minX1, maxX1, w1, SW2, SH2;
  int ftzero, P1, P2, uniq, disp12, invalid, speckle_win, speckle_diff;
};

// pair blockIdx.z of a batch: `stride` bytes from one pair's array to the next pair's
template <typename T>
__device__ __forceinline__ T* pair_at(T* p, size_t stride) {
  using B = typename std::conditional<std::is_const<T>::value, const uint8_t, uint8_t>::type;
  return reinterpret_cast<T*>(reinterpret_cast<B*>(p) + (size_t)blockIdx.z * stride);
}

// calcPixelCostBT's channel c (0: x-Sobel through clipTab, 1: raw) of column r of row y, packed
// with the min / max over it and its half-pixel neighbours: v | v0 << 8 | v1 << 16
__device__ __forceinline__ int sgbm_chan(const uint8_t* __restrict__ img, size_t step, int W, int H,
                                         int y, int r, int c, int ftz) {
  if (r <= 0 || r >= W - 1) return ftz;
  const uint8_t* row = img + (size_t)y * step;
  if (c == 1) return row[r];
  const uint8_t* up = img + (size_t)(y > 0 ? y - 1 : y) * step;
  const uint8_t* dn = img + (size_t)(y < H - 1 ? y + 1 : y) * step;
  const int s = ((int)row[r + 1] - (int)row[r - 1]) * 2 + ((int)up[r + 1] - (int)up[r - 1]) +
                ((int)dn[r + 1] - (int)dn[r - 1]);
  return min(max(s, -ftz), ftz) + ftz;
}

__device__ __forceinline__ unsigned sgbm_packed(const uint8_t* __restrict__ img, size_t step, int W,
                                                int H, int y, int r, int c, int ftz) {
  const int v = sgbm_chan(img, step, W, H, y, r, c, ftz);
  const int vl = r > 0 ? (v + sgbm_chan(img, step, W, H, y, r - 1, c, ftz)) / 2 : v;
  const int vr = r < W - 1 ? (v + sgbm_chan(img, step, W, H, y, r + 1, c, ftz)) / 2 : v;
  const int v0 = min(min(vl, vr), v), v1 = max(max(vl, vr), v);
  return (unsigned)v | ((unsigned)v0 << 8) | ((unsigned)v1 << 16);
}

__device__ __forceinline__ int sgbm_bt(unsigned a, unsigned b) {
  const int u = a & 255, u0 = (a >> 8) & 255, u1 = (a >> 16) & 255;
  const int v = b & 255, v0 = (b >> 8) & 255, v1 = (b >> 16) & 255;
  const int c0 = max(max(0, u - v1), v0 - u);
  const int c1 = max(max(0, v - u1), u0 - v);
  return min(c0, c1);
}

__global__ void __launch_bounds__(256)
k_sgbm_hsum(SgbmDims p, const uint8_t* __restrict__ left, size_t lstep,
            const uint8_t* __restrict__ right, size_t rstep, uint16_t* __restrict__ hsum,
            size_t lbs, size_t rbs, size_t ws) {
  left = pair_at(left, lbs);
  right = pair_at(right, rbs);
  hsum = pair_at(hsum, ws);
  constexpr int kNL = kSgbmTX + 2 * kSgbmMaxSW2;
  __shared__ unsigned sl[2][kNL];
  __shared__ unsigned sr[2][kNL + kSgbmMaxD];
  __shared__ uint8_t pc[kNL * kSgbmMaxD];
  const int y = blockIdx.y;
  const int x0 = blockIdx.x * kSgbmTX;
  const int xa = max(x0 - p.SW2, 0), xb = min(x0 + kSgbmTX + p.SW2, p.w1);
  const int NL = xb - xa, NR = NL + p.D - 1;
  const int rbase = xa + p.minX1 - p.maxD + 1;  // right column of (left xa, d = D - 1)
  for (int i = threadIdx.x; i < 2 * NL; i += blockDim.x) {
    const int c = i / NL, k = i - c * NL;
    sl[c][k] = sgbm_packed(left, lstep, p.W, p.H, y, xa + p.minX1 + k, c, p.ftzero);
  }
  for (int i = threadIdx.x; i < 2 * NR; i += blockDim.x) {
    const int c = i / NR, k = i - c * NR;
    sr[c][k] = sgbm_packed(right, rstep, p.W, p.H, y, rbase + k, c, p.ftzero);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NL * p.D; i += blockDim.x) {
    const int k = i / p.D, d = i - k * p.D;
    const int kr = k + p.D - 1 - d;  // right column X - (d + minD)
    pc[i] = (uint8_t)(sgbm_bt(sl[0][k], sr[0][kr]) + (sgbm_bt(sl[1][k], sr[1][kr]) >> 2));
  }
  __syncthreads();
  const int nout = min(kSgbmTX, p.w1 - x0);
  for (int i = threadIdx.x; i < nout * p.D; i += blockDim.x) {
    const int xo = i / p.D, d = i - xo * p.D;
    const int x1 = x0 + xo;
    int s = 0;
    for (int dx = -p.SW2; dx <= p.SW2; ++dx) {
      const int xx = min(max(x1 + dx, 0), p.w1 - 1);
      s += pc[(xx - xa) * p.D + d];
    }
    hsum[((size_t)y * p.w1 + x1) * p.D + d] = (uint16_t)s;
  }
}

__global__ void __launch_bounds__(256)
k_sgbm_vsum(SgbmDims p, const uint16_t* __restrict__ hsum, uint16_t* __restrict__ C, size_t ws) {
  hsum = pair_at(hsum, ws);
  C = pair_at(C, ws);
  const size_t plane = (size_t)p.w1 * p.D;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const int y0 = blockIdx.y * kSgbmVRows, y1 = min(y0 + kSgbmVRows, p.H);
  const int hold = max(p.H - 1 - p.SH2, 0);  // the last row whose block cost is updated
  auto ye = [&](int y) { return y == 0 ? 0 : min(y, hold); };
  int r = ye(y0), c = 0;
  for (int k = -p.SH2; k <= p.SH2; ++k) c += hsum[(size_t)min(max(r + k, 0), p.H - 1) * plane + i];
  C[(size_t)y0 * plane + i] = (uint16_t)c;
  for (int y = y0 + 1; y < y1; ++y) {
    const int rn = ye(y);
    if (rn != r) {
      c += (int)hsum[(size_t)min(rn + p.SH2, p.H - 1) * plane + i] -
           (int)hsum[(size_t)max(rn - p.SH2 - 1, 0) * plane + i];
      r = rn;
    }
    C[(size_t)y * plane + i] = (uint16_t)c;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// directions: 0 left->right, 1 top, 2 top-left, 3 top-right, 4 right->left
// MODE 0: S = Lr; 1: S += Lr; 2: Lr + S -> winner (disp1, disp2 keys)
template <int NJ, int MODE>
__global__ void __launch_bounds__(256)
k_sgbm_path(SgbmDims p, int dir, const uint16_t* __restrict__ C, int32_t* __restrict__ S,
            int16_t* __restrict__ disp1, unsigned long long* __restrict__ key2, size_t ws) {
  C = pair_at(C, ws);
  S = pair_at(S, ws);
  disp1 = pair_at(disp1, ws);
  key2 = pair_at(key2, ws);
  const int lane = threadIdx.x & 63;
  const int chain = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int w1 = p.w1, H = p.H, D = p.D;
  int x, y, sx, sy, len;
  if (dir == 0 || dir == 4) {
    if (chain >= H) return;
    y = chain, sy = 0, len = w1;
    x = dir == 0 ? 0 : w1 - 1, sx = dir == 0 ? 1 : -1;
  } else if (dir == 1) {
    if (chain >= w1) return;
    x = chain, y = 0, sx = 0, sy = 1, len = H;
  } else {
    if (chain >= H + w1 - 1) return;
    sy = 1;
    sx = dir == 2 ? 1 : -1;
    if (chain < H) {
      y = chain, x = dir == 2 ? 0 : w1 - 1;
    } else {
      y = 0, x = dir == 2 ? chain - H + 1 : chain - H;  // (top-right: columns 0 .. w1-2)
    }
    len = min(dir == 2 ? w1 - x : x + 1, H - y);
  }
  int Lp[NJ];
  bool val[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    val[j] = j * 64 + lane < D;
    Lp[j] = val[j] ? 0 : kSgbmInf;
  }
  int mL = 0;
  const int P1 = p.P1, P2 = p.P2;
  int cn[NJ], sn[NJ];
  auto load = [&](int xx, int yy, int* cv, int* sv) {
    const size_t o = ((size_t)yy * w1 + xx) * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      cv[j] = val[j] ? (int)C[o + j * 64 + lane] : 0;
      if (MODE != 0) sv[j] = val[j] ? S[o + j * 64 + lane] : 0;
    }
  };
  load(x, y, cn, sn);
  for (int t = 0; t < len; ++t) {
    int cc[NJ], sc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) cc[j] = cn[j], sc[j] = sn[j];
    if (t + 1 < len) load(x + sx, y + sy, cn, sn);  // (independent of the chain: in flight meanwhile)
    // d - 1 and d + 1 of the previous Lr: rotate by one lane, carry across the 64-blocks
    int up[NJ], dn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      up[j] = __shfl(Lp[j], (lane + 63) & 63, 64);
      dn[j] = __shfl(Lp[j], (lane + 1) & 63, 64);
    }
    int L[NJ];
    int m = kSgbmInf;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int lm = lane == 0 ? (j == 0 ? kSgbmInf : up[j - 1]) : up[j];
      const int lq = lane == 63 ? (j == NJ - 1 ? kSgbmInf : dn[j + 1]) : dn[j];
      // OpenCV: (C + P2) + min(Lr_p[d], Lr_p[d-1] + P1, Lr_p[d+1] + P1, minLr_p + P2) - (minLr_p + P2)
      const int best = min(min(Lp[j], lm + P1), min(lq + P1, mL + P2));
      L[j] = val[j] ? cc[j] + best - mL : kSgbmInf;
      m = min(m, L[j]);
    }
    m = wave_min(m);
    const size_t o = ((size_t)y * w1 + x) * D;
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (val[j]) S[o + j * 64 + lane] = L[j];
    } else if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (val[j]) S[o + j * 64 + lane] = sc[j] + L[j];
    } else {
      int s[NJ];
      int key = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        s[j] = min(sc[j] + L[j], 32767);  // OpenCV's int16 S: saturate_cast, every Lr >= 0
        if (val[j]) key = min(key, s[j] * 256 + j * 64 + lane);  // lowest d of the minimum
      }
      key = wave_min(key);
      const int minS = key >> 8, bd = key & 255;
      bool bad = false;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int d = j * 64 + lane;
        bad = bad || (val[j] && s[j] * (100 - p.uniq) < minS * 100 && abs(bd - d) > 1);
      }
      // (every S saturated: OpenCV's bestDisp stays -1 and the pixel ends invalid, no disp2 write)
      bad = __any(bad) || minS >= 32767;
      auto at = [&](int d) {  // S[d] of this pixel, d wave-uniform
        int v = s[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j)
          if ((d >> 6) == j) v = s[j];
        return __shfl(v, d & 63, 64);
      };
      int d16 = bd * 16;
      if (bd > 0 && bd < D - 1) {
        const int sm = at(bd - 1), sp = at(bd + 1), s0 = minS;
        const int den = max(sm + sp - 2 * s0, 1);
        d16 = bd * 16 + ((sm - sp) * 16 + den) / (den * 2);  // C division: truncates
      }
      if (lane == 0) {
        const int X = x + p.minX1;
        const size_t row = (size_t)y * p.W;
        if (bad) {
          disp1[row + X] = (int16_t)p.invalid;
        } else {
          disp1[row + X] = (int16_t)(d16 + p.minD * 16);
          const int x2 = X - bd - p.minD;
          atomicMin(&key2[row + x2], ((unsigned long long)minS << 16) | (unsigned long long)(0xFFFF - X));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) Lp[j] = L[j];
    mL = m;
    x += sx;
    y += sy;
  }
}

__device__ __forceinline__ int sgbm_disp2(const unsigned long long* __restrict__ key2, size_t row,
                                          int xx, int invalid) {
  const unsigned long long k = key2[row + xx];
  return k == ~0ull ? invalid : (0xFFFF - (int)(k & 0xFFFF)) - xx;
}

__global__ void __launch_bounds__(256)
k_sgbm_lrcheck(SgbmDims p, const int16_t* __restrict__ disp1,
               const unsigned long long* __restrict__ key2, int16_t* __restrict__ out, size_t ws) {
  disp1 = pair_at(disp1, ws);
  key2 = pair_at(key2, ws);
  out = pair_at(out, ws);
  const int X = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (X >= p.W) return;
  const size_t row = (size_t)y * p.W;
  int d1 = (X >= p.minX1 && X < p.maxX1) ? (int)disp1[row + X] : p.invalid;
  if (d1 != p.invalid) {
    const int lo = d1 >> 4, hi = (d1 + 15) >> 4;
    const int xl = X - lo, xh = X - hi;
    bool fl = false, fh = false;
    if (xl >= 0 && xl < p.W) {
      const int v = sgbm_disp2(key2, row, xl, p.invalid);
      fl = v >= p.minD && abs(v - lo) > p.disp12;
    }
    if (xh >= 0 && xh < p.W) {
      const int v = sgbm_disp2(key2, row, xh, p.invalid);
      fh = v >= p.minD && abs(v - hi) > p.disp12;
    }
    if (fl && fh) d1 = p.invalid;
  }
  out[row + X] = (int16_t)d1;
}

__global__ void __launch_bounds__(256)
k_sgbm_median(int W, int H, const int16_t* __restrict__ in, int16_t* __restrict__ out, size_t ws) {
  in = pair_at(in, ws);
  out = pair_at(out, ws);
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  int v[9];
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = min(max(y + dy, 0), H - 1), xx = min(max(x + dx, 0), W - 1);
      v[(dy + 1) * 3 + dx + 1] = in[(size_t)yy * W + xx];
    }
#pragma unroll
  for (int i = 1; i < 9; ++i)
#pragma unroll
    for (int j = i; j > 0; --j) {
      const int a = v[j - 1], b = v[j];
      v[j - 1] = min(a, b);
      v[j] = max(a, b);
    }
  out[(size_t)y * W + x] = (int16_t)v[4];
}

// ---- filterSpeckles: union-find (parents only ever point to smaller indices) ----------------
__device__ __forceinline__ int uf_load(int* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int* par, int x) {
  int p = uf_load(&par[x]);
  while (p != x) {
    const int g = uf_load(&par[p]);
    if (g != p) __hip_atomic_store(&par[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // halving
    x = p;
    p = g;
  }
  return x;
}

// the root without writes: once the unions are done, par no longer changes under it (a halving
// store here could put back a stale, non-root ancestor over a label another thread has written)
__device__ __forceinline__ int uf_root(const int* __restrict__ par, int x) {
  int p = par[x];
  while (p != x) {
    x = p;
    p = par[x];
  }
  return x;
}

__device__ __forceinline__ void uf_unite(int* par, int a, int b) {
  while (true) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&par[a], a, b) == a) return;
  }
}

__global__ void __launch_bounds__(256)
k_sgbm_uf_init(int n, int* __restrict__ par, int* __restrict__ cnt, size_t ws) {
  par = pair_at(par, ws);
  cnt = pair_at(cnt, ws);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  par[i] = i;
  cnt[i] = 0;
}

__global__ void __launch_bounds__(256)
k_sgbm_uf_union(SgbmDims p, const int16_t* __restrict__ a, int* par, size_t ws) {
  a = pair_at(a, ws);
  par = pair_at(par, ws);  // (labels are pixel indices of this pair's image alone)
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  const int i = y * p.W + x;
  const int v = a[i];
  if (v == p.invalid) return;
  if (x + 1 < p.W) {
    const int w = a[i + 1];
    if (w != p.invalid && abs(v - w) <= p.speckle_diff) uf_unite(par, i, i + 1);
  }
  if (y + 1 < p.H) {
    const int w = a[i + p.W];
    if (w != p.invalid && abs(v - w) <= p.speckle_diff) uf_unite(par, i, i + p.W);
  }
}

__global__ void __launch_bounds__(256)
k_sgbm_uf_count(SgbmDims p, const int16_t* __restrict__ a, const int* __restrict__ par,
                int* __restrict__ lab, int* __restrict__ cnt, size_t ws) {
  a = pair_at(a, ws);
  par = pair_at(par, ws);
  lab = pair_at(lab, ws);
  cnt = pair_at(cnt, ws);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.W * p.H || a[i] == p.invalid) return;
  const int r = uf_root(par, i);
  lab[i] = r;
  atomicAdd(&cnt[r], 1);
}

__global__ void __launch_bounds__(256)
k_sgbm_final(SgbmDims p, const int16_t* __restrict__ med, const int* __restrict__ lab,
             const int* __restrict__ cnt, const uint8_t* __restrict__ mask, size_t mask_step,
             float* __restrict__ disp, size_t disp_step, int16_t* __restrict__ raw, size_t raw_step,
             size_t ws, size_t mbs, size_t dbs, size_t wbs) {
  med = pair_at(med, ws);
  cnt = pair_at(cnt, ws);
  if (lab) lab = pair_at(lab, ws);
  if (mask) mask = pair_at(mask, mbs);
  if (raw) raw = pair_at(raw, wbs);
  disp = pair_at(disp, dbs);
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  const int i = y * p.W + x;
  int v = med[i];
  if (lab && v != p.invalid && cnt[lab[i]] <= p.speckle_win) v = p.invalid;
  if (raw) reinterpret_cast<int16_t*>(reinterpret_cast<uint8_t*>(raw) + (size_t)y * raw_step)[x] = (int16_t)v;
  float f = (float)v / 16.0f;
  if (mask && mask[(size_t)y * mask_step + x] == 0) f = 1.0f;  // kMaxInvalidDisparity
  reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(disp) + (size_t)y * disp_step)[x] = f;
}

template <int NJ>
static void launch_paths(Ctx* c, const SgbmDims& p, unsigned B, size_t ws, const uint16_t* C, int32_t* S,
                         int16_t* disp1, unsigned long long* key2) {
  // (the chains of all B pairs in one launch: chains x B waves)
  const unsigned rows = (unsigned)((p.H + 3) / 4), cols = (unsigned)((p.w1 + 3) / 4),
                 diag = (unsigned)((p.H + p.w1 - 1 + 3) / 4);
  hipLaunchKernelGGL((k_sgbm_path<NJ, 0>), dim3(rows, 1, B), dim3(256), 0, c->stream, p, 0, C, S, disp1, key2, ws);
  hipLaunchKernelGGL((k_sgbm_path<NJ, 1>), dim3(cols, 1, B), dim3(256), 0, c->stream, p, 1, C, S, disp1, key2, ws);
  hipLaunchKernelGGL((k_sgbm_path<NJ, 1>), dim3(diag, 1, B), dim3(256), 0, c->stream, p, 2, C, S, disp1, key2, ws);
  hipLaunchKernelGGL((k_sgbm_path<NJ, 1>), dim3(diag, 1, B), dim3(256), 0, c->stream, p, 3, C, S, disp1, key2, ws);
  hipLaunchKernelGGL((k_sgbm_path<NJ, 2>), dim3(rows, 1, B), dim3(256), 0, c->stream, p, 4, C, S, disp1, key2, ws);
}

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The CV_16S map stores 16 * d: the invalid marker (min_disparity - 1) * 16 and the largest value
// (below (min_disparity + num_disparities) * 16, the subpixel term included) must fit an int16.
static bool cv16s_holds(int min_disparity, int num_disparities) {
  return (min_disparity - 1) * 16 >= -32768 && (min_disparity + num_disparities) * 16 <= 32767;
}

// ---- block matching (OpenCV's StereoBM, PREFILTER_XSOBEL, 8UC1): tests/bm_reference.py -------
//   k_bm_prefilter  per pixel: prefilterXSobel of both images (rows in pairs, an odd last row and
//                   the border columns = cap) -> scratch; FILTERED outside the matched region
//   k_bm_match      per (32-column tile, 64-row band): the band's prefiltered rows (+ the window's
//                   rows above / below, the left strip + SW2 halo, the right strip + D - 1) in LDS;
//                   8 lanes per column, lane g holding d = 8 j + g (j < D / 8); the vertical window sums run
//                   down the band in registers (entering row added, leaving row subtracted, each
//                   row's horizontal SAD summed from LDS); texture, winner, uniqueness and subpixel
//                   by shuffles over the 8 lanes of a column
// then the SGBM tail: k_sgbm_uf_* (filterSpeckles, speckle_range unscaled) and k_sgbm_final.
constexpr int kBmTX = 32;        // output columns per k_bm_match workgroup (8 lanes each)
constexpr int kBmTY = 64;        // output rows per k_bm_match workgroup
constexpr int kBmMaxSW2 = 15;    // block_size <= 31
constexpr int kBmRows = kBmTY + 2 * kBmMaxSW2;
constexpr int kBmLW = kBmTX + 2 * kBmMaxSW2;               // left strip, bytes per row
constexpr int kBmRW = kBmTX + 2 * kBmMaxSW2 + kSgbmMaxD;   // right strip (>= LW + D - 1)

struct BmDims {
  int W, H, minD, D, cap, SW2, uniq, texture, lofs, rofs, filtered;
  int xa, xb, ya, yb;  // the matched region: getValidDisparityROI within [lofs, lofs + width1)
};

__global__ void __launch_bounds__(256)
k_bm_prefilter(BmDims p, const uint8_t* __restrict__ left, size_t lstep,
               const uint8_t* __restrict__ right, size_t rstep, uint8_t* __restrict__ fl,
               uint8_t* __restrict__ fr, int16_t* __restrict__ raw, size_t lbs, size_t rbs, size_t ws) {
  left = pair_at(left, lbs);
  right = pair_at(right, rbs);
  fl = pair_at(fl, ws);
  fr = pair_at(fr, ws);
  raw = pair_at(raw, ws);
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  const size_t i = (size_t)y * p.W + x;
  uint8_t a = (uint8_t)p.cap, b = (uint8_t)p.cap;
  // the row pairs stop one row short of an odd H (that row, and columns 0 / W-1, stay cap)
  if (x > 0 && x < p.W - 1 && y < (p.H & ~1)) {
    const int yu = y > 0 ? y - 1 : 1, yd = y < p.H - 1 ? y + 1 : p.H - 2;
    const uint8_t* im[2] = {left, right};
    const size_t st[2] = {lstep, rstep};
    uint8_t out[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint8_t* r0 = im[k] + (size_t)yu * st[k];
      const uint8_t* r1 = im[k] + (size_t)y * st[k];
      const uint8_t* r2 = im[k] + (size_t)yd * st[k];
      const int s = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) +
                    ((int)r2[x + 1] - (int)r2[x - 1]);
      out[k] = (uint8_t)(min(max(s, -p.cap), p.cap) + p.cap);
    }
    a = out[0];
    b = out[1];
  }
  fl[i] = a;
  fr[i] = b;
  if (x < p.xa || x >= p.xb || y < p.ya || y >= p.yb) raw[i] = (int16_t)p.filtered;
}

// NJ = D / 8: d values per lane
template <int NJ>
__global__ void __launch_bounds__(256)
k_bm_match(BmDims p, const uint8_t* __restrict__ fl, const uint8_t* __restrict__ fr,
           int16_t* __restrict__ raw, size_t ws) {
  __shared__ uint8_t sL[kBmRows][kBmLW];
  __shared__ uint8_t sR[kBmRows][kBmRW];
  fl = pair_at(fl, ws);
  fr = pair_at(fr, ws);
  raw = pair_at(raw, ws);
  const int SW2 = p.SW2, D = 8 * NJ;
  const int X0 = p.xa + blockIdx.x * kBmTX;
  const int y0 = p.ya + blockIdx.y * kBmTY, y1 = min(y0 + kBmTY, p.yb);
  const int r0 = y0 - SW2, nrows = y1 - y0 + 2 * SW2;  // rows r0 .. r0 + nrows - 1, all inside
  const int nL = kBmTX + 2 * SW2;
  const int rmax = p.W - D;                            // the right base column's clamp
  const int lo = min(max(X0 - SW2 - p.lofs + p.rofs, 0), rmax);
  const int nR = min(max(X0 + kBmTX - 1 + SW2 - p.lofs + p.rofs, 0), rmax) + D - lo;
  for (int i = threadIdx.x; i < nrows * nL; i += 256) {
    const int r = i / nL, k = i - r * nL;
    sL[r][k] = fl[(size_t)(r0 + r) * p.W + min(max(X0 - SW2 + k, 0), p.W - 1)];
  }
  for (int i = threadIdx.x; i < nrows * nR; i += 256) {
    const int r = i / nR, k = i - r * nR;
    sR[r][k] = fr[(size_t)(r0 + r) * p.W + lo + k];
  }
  __syncthreads();
  const int xl = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int X = X0 + xl;
  const int base = X - p.lofs + p.rofs - lo;  // (right base column of dx) = clamp(base + lo + dx) - lo
  // one row's contribution (sign +1) and another's (sign -1) to the window sums
  auto rows = [&](int ra, int rb, bool two, int* v, int& t) {
    for (int dx = -SW2; dx <= SW2; ++dx) {
      const int kl = xl + dx + SW2;
      const int kr = min(max(base + lo + dx, 0), rmax) - lo + g;
      const int la = sL[ra][kl];
      t += abs(la - p.cap);
      if (two) t -= abs((int)sL[rb][kl] - p.cap);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        int s = abs(la - (int)sR[ra][kr + 8 * j]);
        if (two) s -= abs((int)sL[rb][kl] - (int)sR[rb][kr + 8 * j]);
        v[j] += s;
      }
    }
  };
  int vs[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) vs[j] = 0;
  int tsum = 0;
  for (int r = 0; r < 2 * SW2; ++r) rows(r, 0, false, vs, tsum);
  for (int y = y0; y < y1; ++y) {
    const int rin = y - y0 + 2 * SW2;
    if (y == y0)
      rows(rin, 0, false, vs, tsum);
    else
      rows(rin, rin - 2 * SW2 - 1, true, vs, tsum);
    // winner: the first d of the minimum (key = sad << 9 | d)
    int key = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NJ; ++j) key = min(key, (vs[j] << 9) | (8 * j + g));
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) key = min(key, __shfl_xor(key, o, 64));
    const int minsad = key >> 9, mind = key & 511;
    const int thresh = minsad + (int)((long long)minsad * p.uniq / 100);
    const int pi = mind + 1 < D ? mind + 1 : D - 2;  // sad[D] := sad[D-2]
    const int ni = mind > 0 ? mind - 1 : 1;          // sad[-1] := sad[1]
    int bad = 0, pv = 0, nv = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = 8 * j + g;
      bad |= (abs(d - mind) > 1 && vs[j] <= thresh) ? 1 : 0;
      pv += d == pi ? vs[j] : 0;
      nv += d == ni ? vs[j] : 0;
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      bad |= __shfl_xor(bad, o, 64);
      pv += __shfl_xor(pv, o, 64);
      nv += __shfl_xor(nv, o, 64);
    }
    if (g == 0 && X < p.xb) {
      int out;
      if (tsum < p.texture || (p.uniq > 0 && bad)) {
        out = p.filtered;
      } else {
        const int den = pv + nv - 2 * minsad + abs(pv - nv);
        out = ((D - mind - 1 + p.minD) * 256 + (den != 0 ? (pv - nv) * 256 / den : 0) + 15) >> 4;
      }
      raw[(size_t)y * p.W + X] = (int16_t)out;
    }
  }
}

// one instantiation per num_disparities (16 .. 256 in steps of 16)
template <int NJ = 2>
static void launch_bm_match(Ctx* c, const BmDims& p, dim3 grid, const uint8_t* fl, const uint8_t* fr,
                            int16_t* raw, size_t ws) {
  if constexpr (NJ < 32) {
    if (p.D != 8 * NJ) return launch_bm_match<NJ + 2>(c, p, grid, fl, fr, raw, ws);
  }
  hipLaunchKernelGGL(k_bm_match<NJ>, grid, dim3(256), 0, c->stream, p, fl, fr, raw, ws);
}

static int stereo_fail(const char* fn, const char* msg) {
  return arg_failure((std::string(fn) + ": " + msg).c_str());
}

// the context's stereo scratch holds `total` bytes (kept between calls; grown, never shrunk)
static int stereo_scratch(Ctx* c, size_t total) {
  if (c->stereo_ws && c->stereo_ws_cap >= total) return AMHIP_OK;
  if (c->stereo_ws) {
    AMHIP_TRY(hipFree(c->stereo_ws));  // (waits for the kernels that still use it)
    c->stereo_ws = nullptr;
    c->stereo_ws_cap = 0;
  }
  // grow by 1/8 so that slightly larger follow-up images do not reallocate
  size_t want = total + total / 8 + 256;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->stereo_ws), want);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    want = total;
    e = hipMalloc(reinterpret_cast<void**>(&c->stereo_ws), want);
  }
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    c->stereo_ws = nullptr;
    set_last_error("stereo matcher: out of device memory for the scratch of the batch");
    return AMHIP_ERR_NOMEM;
  }
  AMHIP_TRY(e);
  c->stereo_ws_cap = want;
  return AMHIP_OK;
}

// ---- the argument rules: each once; stereo_check holds the order in which they are reported ----
static int params_check(const char* fn, const amhip_sgbm_params& q, int width, int height) {
  if (width < 3 || height < 1 || width > 32767 || height > 32767)
    return stereo_fail(fn, "width must be in [3, 32767], height in [1, 32767]");
  if (q.num_disparities <= 0 || q.num_disparities % 16 != 0 || q.num_disparities > kSgbmMaxD)
    return stereo_fail(fn, "num_disparities must be a positive multiple of 16, <= 256");
  if (q.block_size > 11 || (q.block_size > 0 && q.block_size % 2 == 0))
    return stereo_fail(fn, "block_size must be odd and <= 11 (0: OpenCV's 5)");
  if (q.min_disparity < -4096 || q.min_disparity > 4096 || q.pre_filter_cap > 63 ||
      q.uniqueness_ratio > 100 || q.p1 > 4096 || q.p2 > 4096)
    return stereo_fail(fn, "parameter out of range");
  if (!cv16s_holds(q.min_disparity, q.num_disparities))
    return stereo_fail(fn, "the CV_16S map cannot hold this disparity range: "
                           "min_disparity must be >= -2047 and min_disparity + num_disparities <= 2047");
  // (the map's values span less than 2^16, so every range >= 4096 acts alike; 16 * range must fit an int)
  if (q.speckle_range < -4096 || q.speckle_range > 4096)
    return stereo_fail(fn, "speckle_range must be in [-4096, 4096]");
  return AMHIP_OK;
}

// (the one parameter rule that is reported behind the image rules; BM has none)
static int columns_check(const char* fn, const amhip_sgbm_params& q, int width) {
  const int maxD = q.min_disparity + q.num_disparities;
  const int w1 = width + std::min(q.min_disparity, 0) - std::max(maxD, 0);
  if (w1 > 0 && w1 <= (q.block_size > 0 ? q.block_size : 5) / 2)
    return stereo_fail(fn, "fewer matchable columns than half the block");
  return AMHIP_OK;
}
static int columns_check(const char*, const amhip_bm_params&, int) { return AMHIP_OK; }

// StereoBM::compute's CV_Asserts on the wrapper's effective parameters, then this implementation's
// limits
static int params_check(const char* fn, const amhip_bm_params& q, int width, int height) {
  if (width < 1 || height < 1 || width > 32767 || height > 32767)
    return stereo_fail(fn, "width and height must be in [1, 32767]");
  if (q.num_disparities <= 0 || q.num_disparities % 16 != 0 || q.num_disparities > kSgbmMaxD)
    return stereo_fail(fn, "num_disparities must be a positive multiple of 16, <= 256");
  if (q.block_size % 2 == 0 || q.block_size < 5 || q.block_size > 2 * kBmMaxSW2 + 1 ||
      q.block_size > std::min(width, height))
    return stereo_fail(fn, "block_size must be odd, in [5, 31] and <= min(width, height)");
  if (q.pre_filter_size < 1 || q.pre_filter_size > 63)
    return stereo_fail(fn, "pre_filter_size (the effective preFilterCap) must be in [1, 63]");
  if (q.texture_threshold < 0) return stereo_fail(fn, "texture_threshold must be >= 0");
  if (q.uniqueness_ratio < 0) return stereo_fail(fn, "uniqueness_ratio must be >= 0");
  if (q.min_disparity < -4096 || q.min_disparity > 4096)
    return stereo_fail(fn, "min_disparity must be in [-4096, 4096]");
  if (!cv16s_holds(q.min_disparity, q.num_disparities))
    return stereo_fail(fn, "the CV_16S map cannot hold this disparity range: "
                           "min_disparity must be >= -2047 and min_disparity + num_disparities <= 2047");
  return AMHIP_OK;
}

static int image_check(const char* fn, int width, const StereoImages& im) {
  const size_t W = (size_t)width;
  if (im.left_step < W || im.right_step < W || (im.mask && im.mask_step < W) ||
      im.disp_step < W * sizeof(float) || (im.raw && im.raw_step < W * sizeof(int16_t)))
    return stereo_fail(fn, "a row step is smaller than the width");
  if (im.disp_step % sizeof(float) != 0 || (im.raw && im.raw_step % sizeof(int16_t) != 0))
    return stereo_fail(fn, "output steps must be multiples of the element size");
  return AMHIP_OK;
}

static int batch_check(const char* fn, int height, const StereoImages& im) {
  if (im.batch < 1 || im.batch > AMHIP_STEREO_MAX_BATCH) return stereo_fail(fn, "batch must be in [1, 16]");
  const size_t H = (size_t)height;
  const BatchStrides& bs = im.bs;
  if (bs.left < H * im.left_step || bs.right < H * im.right_step || (im.mask && bs.mask < H * im.mask_step) ||
      bs.disp < H * im.disp_step || (im.raw && bs.raw < H * im.raw_step))
    return stereo_fail(fn, "a batch stride is smaller than height * row step");
  if (bs.disp % sizeof(float) != 0 || (im.raw && bs.raw % sizeof(int16_t) != 0))
    return stereo_fail(fn, "output batch strides must be multiples of the element size");
  return AMHIP_OK;
}

// Every argument error of a matcher call, without a device.  A call with several faults reports the
// first of: null argument, width / height, the matcher's parameters, row steps, element sizes,
// SGBM's matchable columns, the batch.
template <typename Params>
static int stereo_check(const char* fn, const Params* q, int width, int height, const StereoImages& im) {
  if (!q || !im.left || !im.right || !im.disp) return stereo_fail(fn, "null argument");
  int rc;
  if ((rc = params_check(fn, *q, width, height))) return rc;
  if ((rc = image_check(fn, width, im))) return rc;
  if ((rc = columns_check(fn, *q, width))) return rc;
  return batch_check(fn, height, im);
}

// ---- SGBM: the scratch of one pair, the launches ----------------------------------------------
// computeDisparitySGBM's preamble (tests/sgbm_reference.py: derived)
static SgbmDims sgbm_dims(const amhip_sgbm_params* q, int width, int height) {
  SgbmDims p;
  std::memset(&p, 0, sizeof(p));
  p.W = width;
  p.H = height;
  p.minD = q->min_disparity;
  p.maxD = p.minD + q->num_disparities;
  p.D = q->num_disparities;
  p.P1 = q->p1 > 0 ? q->p1 : 2;
  p.P2 = std::max(q->p2 > 0 ? q->p2 : 5, p.P1 + 1);
  p.ftzero = std::max(q->pre_filter_cap, 15) | 1;
  p.uniq = q->uniqueness_ratio >= 0 ? q->uniqueness_ratio : 10;
  p.disp12 = q->disp_12_max_diff > 0 ? q->disp_12_max_diff : 1;
  const int win = q->block_size > 0 ? q->block_size : 5;
  p.SW2 = p.SH2 = win / 2;
  p.minX1 = std::max(p.maxD, 0);
  p.maxX1 = width + std::min(p.minD, 0);
  p.w1 = p.maxX1 - p.minX1;
  p.invalid = (p.minD - 1) * 16;
  p.speckle_win = q->speckle_window_size;
  p.speckle_diff = 16 * q->speckle_range;
  return p;
}

struct SgbmScratch {
  size_t oC, oS, o1, oK, oL, oM, oP, oN, oB, total;  // total: one pair's bytes, a multiple of 256
};

static SgbmScratch sgbm_scratch(const SgbmDims& p) {
  const size_t npix = (size_t)p.W * p.H;
  const size_t vol = p.w1 > 0 ? (size_t)p.H * p.w1 * p.D : 0;
  SgbmScratch o;
  o.oC = 0;
  o.oS = o.oC + align256(vol * 2);
  o.o1 = o.oS + align256(vol * 4);
  o.oK = o.o1 + align256(npix * 2);
  o.oL = o.oK + align256(npix * 8);
  o.oM = o.oL + align256(npix * 2);
  o.oP = o.oM + align256(npix * 2);
  o.oN = o.oP + align256(npix * 4);
  o.oB = o.oN + align256(npix * 4);
  o.total = o.oB + align256(npix * 4);
  return o;
}

// the union-find arrays of the speckle filter in one pair's scratch
struct SpeckleScratch {
  int *par, *cnt, *lab;
};

// The tail of both matchers: filterSpeckles (if `speckle`) over the CV_16S map `map` of every pair,
// then the final pass into the caller's arrays.  Of s it reads W, H, invalid and the speckle fields.
static void speckle_and_final(Ctx* c, const SgbmDims& s, bool speckle, const int16_t* map,
                              const SpeckleScratch& u, size_t wsb, const StereoImages& im) {
  const unsigned B = (unsigned)im.batch;
  const size_t npix = (size_t)s.W * s.H;
  const dim3 rowgrid((unsigned)((s.W + 255) / 256), (unsigned)s.H, B);
  if (speckle) {
    const dim3 nb((unsigned)((npix + 255) / 256), 1, B);
    hipLaunchKernelGGL(k_sgbm_uf_init, nb, dim3(256), 0, c->stream, (int)npix, u.par, u.cnt, wsb);
    hipLaunchKernelGGL(k_sgbm_uf_union, rowgrid, dim3(256), 0, c->stream, s, map, u.par, wsb);
    hipLaunchKernelGGL(k_sgbm_uf_count, nb, dim3(256), 0, c->stream, s, map, u.par, u.lab, u.cnt, wsb);
  }
  hipLaunchKernelGGL(k_sgbm_final, rowgrid, dim3(256), 0, c->stream, s, map, speckle ? u.lab : nullptr,
                     u.cnt, im.mask, im.mask_step, im.disp, im.disp_step, im.raw, im.raw_step, wsb,
                     im.bs.mask, im.bs.disp, im.bs.raw);
}

static int stereo_run(Ctx* c, const amhip_sgbm_params* q, int width, int height, const StereoImages& im) {
  const SgbmDims p = sgbm_dims(q, width, height);
  const bool matched = p.w1 > 0;
  const size_t npix = (size_t)width * height;
  const SgbmScratch o = sgbm_scratch(p);
  const unsigned B = (unsigned)im.batch;
  const size_t wsb = o.total;  // pair b's scratch: the single-pair layout at b * wsb
  int rc;
  if ((rc = stereo_scratch(c, wsb * B))) return rc;
  uint8_t* ws = c->stereo_ws;
  uint16_t* C = reinterpret_cast<uint16_t*>(ws + o.oC);
  int32_t* S = reinterpret_cast<int32_t*>(ws + o.oS);
  uint16_t* hsum = reinterpret_cast<uint16_t*>(ws + o.oS);  // (dead once C is built)
  int16_t* disp1 = reinterpret_cast<int16_t*>(ws + o.o1);
  unsigned long long* key2 = reinterpret_cast<unsigned long long*>(ws + o.oK);
  int16_t* lr = reinterpret_cast<int16_t*>(ws + o.oL);
  int16_t* med = reinterpret_cast<int16_t*>(ws + o.oM);
  const SpeckleScratch u = {reinterpret_cast<int*>(ws + o.oP), reinterpret_cast<int*>(ws + o.oN),
                            reinterpret_cast<int*>(ws + o.oB)};

  ScopedTimer t(c, AMHIP_K_STEREO);
  const dim3 rowgrid((unsigned)((width + 255) / 256), (unsigned)height, B);
  if (matched) {
    if (B == 1)
      AMHIP_TRY(hipMemsetAsync(key2, 0xFF, npix * 8, c->stream));
    else  // (one row of npix keys per pair, wsb bytes apart)
      AMHIP_TRY(hipMemset2DAsync(key2, wsb, 0xFF, npix * 8, B, c->stream));
    hipLaunchKernelGGL(k_sgbm_hsum, dim3((unsigned)((p.w1 + kSgbmTX - 1) / kSgbmTX), (unsigned)height, B),
                       dim3(256), 0, c->stream, p, im.left, im.left_step, im.right, im.right_step, hsum,
                       im.bs.left, im.bs.right, wsb);
    hipLaunchKernelGGL(k_sgbm_vsum, dim3((unsigned)(((size_t)p.w1 * p.D + 255) / 256),
                                         (unsigned)((height + kSgbmVRows - 1) / kSgbmVRows), B),
                       dim3(256), 0, c->stream, p, hsum, C, wsb);
    if (p.D <= 64)
      launch_paths<1>(c, p, B, wsb, C, S, disp1, key2);
    else if (p.D <= 128)
      launch_paths<2>(c, p, B, wsb, C, S, disp1, key2);
    else if (p.D <= 192)
      launch_paths<3>(c, p, B, wsb, C, S, disp1, key2);
    else
      launch_paths<4>(c, p, B, wsb, C, S, disp1, key2);
  }
  // (no match possible: every pixel INVALID_DISP_SCALED; disp1 / key2 are not read)
  hipLaunchKernelGGL(k_sgbm_lrcheck, rowgrid, dim3(256), 0, c->stream, p, disp1, key2, lr, wsb);
  hipLaunchKernelGGL(k_sgbm_median, rowgrid, dim3(256), 0, c->stream, width, height, lr, med, wsb);
  speckle_and_final(c, p, q->speckle_window_size > 0, med, u, wsb, im);
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

// ---- BM ---------------------------------------------------------------------------------------
struct BmScratch {
  size_t oL, oR, oD, oP, oN, oB, total;  // total: one pair's bytes, a multiple of 256
};

static BmScratch bm_scratch(int width, int height) {
  const size_t npix = (size_t)width * height;
  BmScratch o;
  o.oL = 0;
  o.oR = o.oL + align256(npix);
  o.oD = o.oR + align256(npix);
  o.oP = o.oD + align256(npix * 2);
  o.oN = o.oP + align256(npix * 4);
  o.oB = o.oN + align256(npix * 4);
  o.total = o.oB + align256(npix * 4);
  return o;
}

static int stereo_run(Ctx* c, const amhip_bm_params* q, int width, int height, const StereoImages& im) {
  // the wrapper's setters (block-matching-bm.h): preFilterCap = pre_filter_size (the second
  // setPreFilterCap wins), disp12MaxDiff stays -1; findStereoCorrespondenceBM's preamble and
  // getValidDisparityROI (tests/bm_reference.py: effective, region)
  BmDims p;
  std::memset(&p, 0, sizeof(p));
  p.W = width;
  p.H = height;
  p.minD = q->min_disparity;
  p.D = q->num_disparities;
  p.cap = q->pre_filter_size;
  p.SW2 = q->block_size / 2;
  p.uniq = q->uniqueness_ratio;
  p.texture = q->texture_threshold;
  p.lofs = std::max(p.D - 1 + p.minD, 0);
  p.rofs = -std::min(p.D - 1 + p.minD, 0);
  p.filtered = (int)(int16_t)((p.minD - 1) * 16);
  const int width1 = width - p.rofs - p.D + 1;
  const int maxD = p.minD + p.D - 1;
  p.xa = std::max(maxD, 0) + p.SW2;
  p.xb = std::min(width - p.SW2, p.lofs + width1);
  p.ya = p.SW2;
  p.yb = height - p.SW2;
  if (p.lofs >= width || p.rofs >= width || width1 < 1 || p.xb <= p.xa || p.yb <= p.ya)
    p.xa = p.xb = p.ya = p.yb = 0;  // nothing matched: FILTERED everywhere
  const bool matched = p.xb > p.xa;

  const BmScratch o = bm_scratch(width, height);
  const unsigned B = (unsigned)im.batch;
  const size_t wsb = o.total;  // pair b's scratch: the single-pair layout at b * wsb
  int rc;
  if ((rc = stereo_scratch(c, wsb * B))) return rc;
  uint8_t* ws = c->stereo_ws;
  uint8_t* fl = ws + o.oL;
  uint8_t* fr = ws + o.oR;
  int16_t* disp = reinterpret_cast<int16_t*>(ws + o.oD);
  const SpeckleScratch u = {reinterpret_cast<int*>(ws + o.oP), reinterpret_cast<int*>(ws + o.oN),
                            reinterpret_cast<int*>(ws + o.oB)};

  // the speckle filter and the final pass are SGBM's, on these fields
  SgbmDims s;
  std::memset(&s, 0, sizeof(s));
  s.W = width;
  s.H = height;
  s.invalid = p.filtered;
  s.speckle_win = q->speckle_window_size;
  s.speckle_diff = q->speckle_range;  // (StereoBM: unscaled, in 1/16 pixel)

  ScopedTimer t(c, AMHIP_K_STEREO);
  const dim3 rowgrid((unsigned)((width + 255) / 256), (unsigned)height, B);
  hipLaunchKernelGGL(k_bm_prefilter, rowgrid, dim3(256), 0, c->stream, p, im.left, im.left_step, im.right,
                     im.right_step, fl, fr, disp, im.bs.left, im.bs.right, wsb);
  if (matched) {
    const dim3 grid((unsigned)((p.xb - p.xa + kBmTX - 1) / kBmTX),
                    (unsigned)((p.yb - p.ya + kBmTY - 1) / kBmTY), B);
    launch_bm_match(c, p, grid, fl, fr, disp, wsb);
  }
  speckle_and_final(c, s, q->speckle_range >= 0 && q->speckle_window_size > 0, disp, u, wsb, im);
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

int stereo_scratch_reserve(Ctx* c, const amhip_stereo_settings& s, int width, int height, int batch) {
  const size_t one = s.use_bm ? bm_scratch(width, height).total
                              : sgbm_scratch(sgbm_dims(&s.sgbm, width, height)).total;
  return stereo_scratch(c, one * (size_t)batch);
}

template <typename Params>
static int params_only_check(const char* fn, const Params& q, int width, int height) {
  const int rc = params_check(fn, q, width, height);
  return rc ? rc : columns_check(fn, q, width);
}

// (under the names of the one-pair exports, whose texts amhip_stereo_create has always reported)
int stereo_params_check(const amhip_stereo_settings& s, int width, int height) {
  return s.use_bm ? params_only_check("amhip_bm_disparity_dev", s.bm, width, height)
                  : params_only_check("amhip_sgbm_disparity_dev", s.sgbm, width, height);
}

int stereo_match(Ctx* c, const amhip_stereo_settings& s, int width, int height, const StereoImages& im) {
  return s.use_bm ? stereo_run(c, &s.bm, width, height, im) : stereo_run(c, &s.sgbm, width, height, im);
}

// what the exports share: every check, the context, its device, the launches
template <typename Params>
static int stereo_entry(const char* fn, amhip_ctx* h, const Params* q, int width, int height,
                        const StereoImages& im) {
  int rc = stereo_check(fn, q, width, height, im);
  if (rc) return rc;
  if (!h) return arg_failure("null context");
  Ctx* c = &h->impl;
  if ((rc = ctx_use_device(c))) return rc;
  return stereo_run(c, q, width, height, im);
}

// the strides of a one-pair call: one image each (nothing is read at them)
static BatchStrides one_pair(const StereoImages& im, int height) {
  const size_t H = (size_t)height;
  return {H * im.left_step, H * im.right_step, H * im.mask_step, H * im.disp_step, H * im.raw_step};
}

}  // namespace amhip

using namespace amhip;

extern "C" {

void amhip_sgbm_default_params(amhip_sgbm_params* out) {
  if (!out) return;
  // BlockMatchingParameters::SGBM (aerial_mapper_dense_pcl common.h)
  out->min_disparity = 1;
  out->num_disparities = 80;
  out->pre_filter_cap = 35;
  out->uniqueness_ratio = 10;
  out->speckle_window_size = 100;
  out->speckle_range = 20;
  out->disp_12_max_diff = 0;
  out->p1 = 120;
  out->p2 = 250;
  out->block_size = 9;
}

int amhip_sgbm_disparity_dev(amhip_ctx* h, const amhip_sgbm_params* q, int width, int height,
                             const uint8_t* dev_left, size_t left_step, const uint8_t* dev_right,
                             size_t right_step, const uint8_t* dev_mask, size_t mask_step,
                             float* dev_disparity, size_t disp_step, int16_t* dev_raw,
                             size_t raw_step) {
  StereoImages im = {dev_left, left_step, dev_right, right_step, dev_mask, mask_step, dev_disparity,
                     disp_step, dev_raw, raw_step, 1, {}};
  im.bs = one_pair(im, height);
  return stereo_entry("amhip_sgbm_disparity_dev", h, q, width, height, im);
}

int amhip_sgbm_disparity_batch_dev(amhip_ctx* h, const amhip_sgbm_params* q, int width, int height,
                                   int batch, const uint8_t* dev_left, size_t left_step,
                                   size_t left_batch_stride, const uint8_t* dev_right, size_t right_step,
                                   size_t right_batch_stride, const uint8_t* dev_mask, size_t mask_step,
                                   size_t mask_batch_stride, float* dev_disparity, size_t disp_step,
                                   size_t disp_batch_stride, int16_t* dev_raw, size_t raw_step,
                                   size_t raw_batch_stride) {
  const StereoImages im = {dev_left, left_step, dev_right, right_step, dev_mask, mask_step, dev_disparity,
                           disp_step, dev_raw, raw_step, batch,
                           {left_batch_stride, right_batch_stride, mask_batch_stride, disp_batch_stride,
                            raw_batch_stride}};
  return stereo_entry("amhip_sgbm_disparity_batch_dev", h, q, width, height, im);
}

void amhip_bm_default_params(amhip_bm_params* out) {
  if (!out) return;
  // BlockMatchingParameters::BM (aerial_mapper_dense_pcl common.h)
  out->min_disparity = 1;
  out->num_disparities = 80;
  out->pre_filter_cap = 31;
  out->pre_filter_size = 9;
  out->uniqueness_ratio = 80;
  out->texture_threshold = 20;
  out->speckle_window_size = 100;
  out->speckle_range = 5;
  out->disp_12_max_diff = 0;
  out->block_size = 15;
}

int amhip_bm_disparity_dev(amhip_ctx* h, const amhip_bm_params* q, int width, int height,
                           const uint8_t* dev_left, size_t left_step, const uint8_t* dev_right,
                           size_t right_step, const uint8_t* dev_mask, size_t mask_step,
                           float* dev_disparity, size_t disp_step, int16_t* dev_raw,
                           size_t raw_step) {
  StereoImages im = {dev_left, left_step, dev_right, right_step, dev_mask, mask_step, dev_disparity,
                     disp_step, dev_raw, raw_step, 1, {}};
  im.bs = one_pair(im, height);
  return stereo_entry("amhip_bm_disparity_dev", h, q, width, height, im);
}

int amhip_bm_disparity_batch_dev(amhip_ctx* h, const amhip_bm_params* q, int width, int height,
                                 int batch, const uint8_t* dev_left, size_t left_step,
                                 size_t left_batch_stride, const uint8_t* dev_right, size_t right_step,
                                 size_t right_batch_stride, const uint8_t* dev_mask, size_t mask_step,
                                 size_t mask_batch_stride, float* dev_disparity, size_t disp_step,
                                 size_t disp_batch_stride, int16_t* dev_raw, size_t raw_step,
                                 size_t raw_batch_stride) {
  const StereoImages im = {dev_left, left_step, dev_right, right_step, dev_mask, mask_step, dev_disparity,
                           disp_step, dev_raw, raw_step, batch,
                           {left_batch_stride, right_batch_stride, mask_batch_stride, disp_batch_stride,
                            raw_batch_stride}};
  return stereo_entry("amhip_bm_disparity_batch_dev", h, q, width, height, im);
}

}  // extern "C"
