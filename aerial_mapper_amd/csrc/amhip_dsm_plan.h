// amhip_dsm_plan.h -- what the host decides about one DSM call before anything is launched: the
// radius ladder, the bins, the sort plan, the gather's tile shape and LDS image (plan_dsm), the
// capacity classes of the gather launches (plan_gather_classes) and the rough-terrain switch of the
// single-precision mode (rough_policy_step).  Pure functions of their arguments: no HIP, no context,
// no tuning store -- tests/cpp/dsm_plan_host_main.cc compiles this header alone.
#ifndef AMHIP_DSM_PLAN_H_
#define AMHIP_DSM_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "aerial_mapper_hip.h"

namespace amhip {

constexpr int kMaxLevels = 24;  // radius ladder: R, then lambda_k * R (<= 22 for R = 1)
constexpr int kMaxW0 = 16;      // largest first-level window (cells) the LDS gather handles
constexpr int kTileI = 64;      // cells of a gather tile along i: one per lane
constexpr int kMaxRegionRows = 96;  // bin rows of a region

// Geometry + search parameters of one DSM call, passed by value to kernels.
struct DsmParams {
  // grid_map_core getPosition: x_i = base_x + res * (-(double)i)
  double base_x, base_y, res;
  int rows, cols;    // size of the window this context owns
  int i_off, j_off;  // its position inside the (global) map
  // dsm.cc:42-43: px = p.x - center_northing, py = p.y - center_easting
  double sub_x, sub_y;
  // 0: dsm::Dsm (exact hit = CHECK failure); 1: ortho::OrthoFromPcl (exact hit
  // = that point's value, ortho-from-pcl.cc:91-96)
  int pcl_mode;
  // adaptive OrthoFromPcl passes: touch only cells no earlier pass has filled
  int only_unfilled;
  // binning: bins of B x B cells, grid extended by M cells on every side
  double inv_res;
  int B, M, nbx, nby;
  // radius ladder (squared radii, exactly the doubles dsm.cc:127-144 uses)
  int nlevels;
  double T[kMaxLevels];
  int w[kMaxLevels];  // conservative window half-width in cells for T[k]
  // LDS-tiled gather (first level only): per window row dj in [-w0, w0] the
  // half-width in cells of the disc of squared radius T[0]
  int lds_ok;                 // 0 -> every tile takes the global-memory path
  // three-pass partition sort plan (p3_n1 == 0: not used)
  int p3_r1;                  // bin rows per first-pass partition
  int p3_c, p3_w;             // column blocks per bin row, bins per column block
  int p3_n1, p3_n2;           // partitions of pass 1; sub-partitions of each (= p3_r1 * p3_c)
  int p3_cap;                 // points a pass-3 workgroup can sort in LDS
  // Every sort pass turns every point into its keys again: four integer divisions by
  // B / p3_r1 / p3_w per point and pass were ~half of the passes' VALU time.  Multipliers
  // m = floor(2^32 / d) + 1: n / d == umulhi(n, m) for n * d < 2^32 (0: d == 1; ~0: n * d may
  // reach 2^32 on this grid -> the real division); div_by() in amhip_sort.hip
  unsigned mul_B, mul_r1, mul_w;
  int wr[2 * kMaxW0 + 1];
  int wr2[2 * kMaxW0 + 2];    // the same for a pair of cells (j, j+1): max of both
  int wrp[kMaxW0 + 1];        // per trip (window rows 2k, 2k+1 of the pair): max of wr2
  int lds_cap;                // points the tile's LDS image can hold
  int lds_cells;              // cell-offset table entries reserved (+1 sentinel)
  int tile_j;                 // tile height in cells: 32, or 16 for dense clouds
  int tiles_i, tiles_j;
  unsigned lds_bytes;
  // single-precision gather with exact guards (k_dsm_gather_f32): point
  // positions as 32-bit fixed point in units of 2^-fx_S cells (wrapping: only differences of
  // at most w0 + 2 cells are ever formed), squared distances in f32 in (2^-fx_S cells)^2
  // OPTIONAL capped mode (not a reference code path): only the knn_k nearest points of a
  // cell's search result take part (0 = off = the reference's behaviour)
  int knn_k;
  int fx_ok;                  // 0 -> the FP64 gather only; 1 -> the sort leaves 16-byte records
                              // (amhip_sort.hip, "the record pipeline") and the single-precision
                              // gather runs on them
  int fx_S;
  float fx_thi, fx_tlo;       // T[0] in those units, widened / narrowed by the decision margin
  float fx_denmax;            // a hit nearer than fx_theta cells makes the weight sum exceed this
  float fx_epsw;              // bound on the relative error of one weight
  unsigned lds_bytes_f32;
  int canon_all;              // tests: every FP64 quotient goes through canonical_search (amhip_dsm.hip)
  // Where cell (i, j) of THIS call's window lives in the layer it writes: out_i0 + i + (out_j0 + j)
  // * out_pitch.  A call on the context's whole window: 0, 0, rows.  A small cloud onto a large map
  // runs on a SUB-window around the cloud's bounding box (amhip_api.hip: dsm_subwindow) and
  // writes into the full layer.
  int out_i0, out_j0, out_pitch;
};
static_assert(sizeof(DsmParams) == 832, "DsmParams is passed by value to every DSM and sort kernel");

// ---------------------------------------------------------------------------
// the tile lists of one call (amhip_dsm.hip: TileLists)
// ---------------------------------------------------------------------------
constexpr int kListHdr = 8;         // counters in front of the tile lists
constexpr int kNumLists = 7;
// [kListHdr counters] then kNumLists arrays of ntiles tile ids (the device side indexes them by
// these numbers: wave_append_tile, tile_occupancy_block).  Who writes, who walks:
enum TileList : int {
  kListMain = 0,           // occupied class-0 tiles, filled by the pre-pass on sparse calls only; walked by
                           // the main launch of a sparse call (FP64 or single-precision list kernel)
  kListClass1 = 1,         // class-1 / class-2 tiles (pre-pass); walked by the list launches with the
  kListClass2 = 2,         // larger LDS images, FP64 or single precision
  kListWaveBlock = 3,      // class 3: more points than any LDS image holds (pre-pass); k_dsm_gather_dense
  kListRedoOwn = 4,        // FP64 redo with an image of cap0 points: class-0 tiles the single-precision main
                           // launch hands back, or the pre-pass files for it (bin_z, rej_own); FP64 list launch
  kListRedoBig = 5,        // FP64 redo with the largest image (cap2): tiles the single-precision class launches
                           // (or a main launch whose own FP64 image fits no CU) hand back, or the pre-pass files
  kListRedoWaveBlock = 6,  // redo beyond the largest image; k_dsm_gather_dense<false>
};
constexpr int kStatRedoUnlisted = 7;  // counter only: pre-classified tiles on NO list (a dense launch takes them)

// tiles of the previous call that went to the FP64 kernel for their height spread
inline double rejected_tiles(const volatile unsigned* stats) {
  return (double)stats[kListRedoOwn] + (double)stats[kListRedoBig] + (double)stats[kListRedoWaveBlock] +
         (double)stats[kStatRedoUnlisted];
}

// ---------------------------------------------------------------------------
// the LDS image of a gather tile
// ---------------------------------------------------------------------------
// What gather_tile / gather_tile_f32 (amhip_dsm.hip) carve out of the launch's dynamic LDS, in this order:
//   points      lds_cap + kLdsSpareSlots slots.  FP64: an array of double2 (x, y) and one of double (z),
//               lds_cap + 1 entries each; single precision: one uint4 record per slot
//   s_off       lds_cells + 1 words: the cell-offset table
//   s_rowg      kLdsRowStartWords:  global start of a region bin-row
//   s_rowp      kLdsRowPrefixWords: prefix of the row lengths
//   s_scan      kLdsScanWords:      block-scan scratch
//   s_ctl       kLdsCtlWords64 / kLdsCtlWords32: np, nflag, ... (single precision: + the height range's keys)
//   s_flag      kTileI * tile_j half-words: the cells left for the fallback path
// and behind them three terms that no kernel addresses: padding.  They stay, because removing them changes
// the LDS bytes per workgroup, hence how many workgroups a CU holds.
constexpr int kLdsPointBytes64 = 24;
constexpr int kLdsPointBytes32 = 16;
constexpr int kLdsSpareSlots = 2;
constexpr int kLdsRowStartWords = kMaxRegionRows;
constexpr int kLdsRowPrefixWords = kMaxRegionRows + 1;
constexpr int kLdsScanWords = 24;
constexpr int kLdsCtlWords64 = 4;
constexpr int kLdsCtlWords32 = 8;
constexpr int kLdsPadWords = 4 * kMaxW0 + 4;  // padding
constexpr int kLdsPadBytesF32 = 64;           // padding, single-precision image only
constexpr int kLdsPadBytesTail = 64;          // padding
constexpr long kLdsBudgetTwoPerCU = 80 * 1024;   // of a CU's 160 KB: an image that leaves two workgroups per CU
constexpr long kLdsBudgetOnePerCU = 150 * 1024;  // the largest image a launch asks for: one workgroup per CU

constexpr int lds_point_bytes(bool f32) { return f32 ? kLdsPointBytes32 : kLdsPointBytes64; }
// bytes from the cell table to the end of the flags: what the kernels address behind the points
constexpr size_t lds_table_bytes(bool f32, int lds_cells, int tile_j) {
  return ((size_t)lds_cells + 1 + kLdsRowStartWords + kLdsRowPrefixWords + kLdsScanWords +
          (f32 ? kLdsCtlWords32 : kLdsCtlWords64)) * sizeof(uint32_t) +
         (size_t)kTileI * tile_j * sizeof(uint16_t);
}
// everything but the points, in whole 16-byte quads
constexpr size_t lds_fixed_bytes(bool f32, int lds_cells, int tile_j) {
  return (lds_table_bytes(f32, lds_cells, tile_j) + kLdsPadWords * sizeof(uint32_t) + (f32 ? kLdsPadBytesF32 : 0) +
          kLdsPadBytesTail + 15) & ~size_t(15);
}
// the image with room for `cap` points (cap even: the points are then whole quads too)
constexpr unsigned lds_image_bytes(bool f32, int cap, int lds_cells, int tile_j) {
  return (unsigned)(((size_t)cap + kLdsSpareSlots) * lds_point_bytes(f32) + lds_fixed_bytes(f32, lds_cells, tile_j));
}
// the largest (even: the cell table behind the points is read and written in 16-byte quads) cap whose
// image stays within `limit` bytes
inline int lds_cap_fit(bool f32, long limit, int lds_cells, int tile_j) {
  return (int)((limit - (long)lds_fixed_bytes(f32, lds_cells, tile_j)) / lds_point_bytes(f32) - kLdsSpareSlots) & ~1;
}

// ---------------------------------------------------------------------------
// plan_dsm
// ---------------------------------------------------------------------------
// Everything the plan of a call depends on.  The tuning values are a snapshot taken by the caller.
struct DsmPlanInput {
  amhip_grid_desc grid;                    // the (global) map
  int win_i0, win_j0, win_rows, win_cols;  // the window of it this call works on
  int radius_sq;
  double center_easting, center_northing;
  int mode, pcl_lambda;  // mode 0: dsm::Dsm ladder.  mode 1: ortho::OrthoFromPcl, one search with the
                         // squared radius `radius_sq * pcl_lambda` (pcl_lambda = 1 for the first search,
                         // 10, 100, ... for the adaptive retries, ortho-from-pcl.cc:63-71)
  size_t num_points;
  int dsm_exact, dsm_exact_now, dsm_knn;   // precision state of the context
  // tuning knobs
  int canon_all;
  size_t p3_min_points;
  double p3_target;
  int p3_cap;
  int knn_global_bins;
#ifdef AMHIP_TIMING_PROBES
  double gather_tj, fx_theta;              // (0: not set)
#endif
};

inline void grid_bases(const amhip_grid_desc& g, double* bx, double* by) {
  // getPosition: (mapPosition + (0.5*length - 0.5*resolution)) + resolution*(-i)
  const double off_x = 0.5 * g.length_x - 0.5 * g.resolution;
  const double off_y = 0.5 * g.length_y - 0.5 * g.resolution;
  *bx = g.pos_x + off_x;
  *by = g.pos_y + off_y;
}

// Squared search radii in the order dsm.cc:127-144 tries them: the initial
// search with T = R, then lambda*R for lambda = 1, 1.1, 1.1^2, ... where
// lambda is updated by `lambda *= 1.1` and the loop stops once lambda*R > 7.
// false: more than kMaxLevels radii (radius_sq < 1 only)
inline bool plan_ladder(const DsmPlanInput& in, DsmParams* p) {
  int n = 0;
  if (in.mode == 0) {
    p->T[n++] = static_cast<double>(in.radius_sq);
    double lambda = 1.0;
    for (;;) {
      if (n >= kMaxLevels) return false;
      p->T[n++] = lambda * in.radius_sq;
      lambda *= 1.1;
      if (lambda * in.radius_sq > 7.0) break;
    }
  } else {
    p->T[n++] = static_cast<double>(in.pcl_lambda * in.radius_sq);  // int product, like the reference
  }
  p->nlevels = n;
  // a point within sqrt(T) of the centre of cell i lies in a cell whose index
  // differs from i by at most floor(sqrt(T)/res + 0.5) (+ slack for rounding)
  for (int k = 0; k < n; ++k)
    p->w[k] = static_cast<int>(std::floor(std::sqrt(p->T[k]) / in.grid.resolution + 0.5 + 1e-6));
  return true;
}

// Bins of B x B cells over the window grown by M cells on every side.  Bin edge = the first search
// radius in cells: the LDS gather then needs exactly one ring of bins around a tile.
// false: more bins than 32-bit bin ids
inline bool plan_bins(const DsmPlanInput& in, DsmParams* p) {
  int B = std::min(std::max(p->w[0], 1), 8);
  // adaptive retries: huge radii -> coarse bins, global gather only
  if (in.mode == 1 && in.pcl_lambda > 1) B = std::max(p->w[0] / 4, 1);
  const int wmax = std::max(0, *std::max_element(p->w, p->w + p->nlevels));
  p->B = B;
  p->M = ((wmax + B - 1) / B) * B;
  const long long ex = (long long)p->rows + 2LL * p->M;
  const long long ey = (long long)p->cols + 2LL * p->M;
  p->nbx = static_cast<int>((ex + B - 1) / B);
  p->nby = static_cast<int>((ey + B - 1) / B);
  const unsigned long long nbins = (unsigned long long)p->nbx * (unsigned long long)p->nby;
  return nbins + 1 < 0xFFFFFFFFull;
}

constexpr int kP3PlaceMaxCap = 2048;  // LDS capacity (points) the sort's register-resident placement handles

// Three-pass partition sort plan (amhip_sort.hip; p3_n1 == 0: not used).  Worth it once the cloud is
// large enough that the sort is bandwidth bound; sub-partitions are sized for ~1.5 K points (a pass-3
// workgroup sorts up to p3_cap of them in LDS, more through a direct-placement fallback).
inline void plan_sort(const DsmPlanInput& in, DsmParams* p) {
  p->p3_n1 = 0;
  const int r1 = (p->nby + 127) / 128;
  const int n1 = (p->nby + r1 - 1) / r1;
  const int cmax = 256 / r1;
  if (r1 > 256 || cmax < 1 || in.num_points < in.p3_min_points) return;
  int cc = static_cast<int>((double)in.num_points / ((double)p->nby * in.p3_target) + 0.5);
  cc = std::min(std::min(std::max(cc, 1), cmax), p->nbx);
  const int w = (p->nbx + cc - 1) / cc;
  if (w > 4096 || (long long)n1 * r1 * cc > 32768) return;
  p->p3_r1 = r1;
  p->p3_c = cc;
  p->p3_w = w;
  p->p3_n1 = n1;
  p->p3_n2 = r1 * cc;
  p->p3_cap = std::max(std::min(in.p3_cap, kP3PlaceMaxCap), 64);
}

// Division-free keys for the sort passes (DsmParams::mul_*): the multiplier of n / d for n <= n_max
inline unsigned division_multiplier(unsigned long long n_max, int d) {
  if (d <= 1) return 0u;
  if (n_max * (unsigned long long)d >= (1ull << 32)) return 0xFFFFFFFFu;
  return (unsigned)((1ull << 32) / (unsigned long long)d) + 1u;
}
inline void plan_multipliers(DsmParams* p) {
  const unsigned long long cells_max =
      (unsigned long long)std::max(p->rows, p->cols) + 2ull * (unsigned long long)p->M + 1ull;
  p->mul_B = division_multiplier(cells_max, p->B);
  p->mul_r1 = p->p3_n1 ? division_multiplier((unsigned long long)p->nby + 1ull, p->p3_r1) : 0xFFFFFFFFu;
  p->mul_w = p->p3_n1 ? division_multiplier((unsigned long long)p->nbx + 1ull, p->p3_w) : 0xFFFFFFFFu;
}

// This call runs in single precision (given an LDS image: fx_ok): dsm::Dsm only -- OrthoFromPcl
// interpolates int32 values (8-bit intensities in the pipeline, any int32 through the ABI: the FP64
// pipeline holds the whole range, tests/test_gpu_ortho_from_pcl_edges.py) whose spread leaves no room
// under the error bound --, not in the exact mode or under its rough-terrain hold, not in the capped mode
// (always the FP64 pipeline: sorted doubles, no records), and only while the sort's records hold the call:
// a cell in 16 + 16 bits, a row of the cloud in 32 -- larger maps / clouds stay in FP64.
inline bool runs_single_precision(const DsmPlanInput& in, const DsmParams& p) {
  const bool rec_fits = (long long)p.rows + 2LL * p.M <= 65535 && (long long)p.cols + 2LL * p.M <= 65535 &&
                        in.num_points < 0xFFFFFFFFull;
  return in.mode == 0 && !in.dsm_exact && !in.dsm_exact_now && !in.dsm_knn && rec_fits;
}

// points the region of an interior tile of height tj must hold: E + 5 sqrt(E) for the cloud's MEAN
// density (p: rows, cols, w[0], B, M set)
inline double region_need(const DsmParams& p, int tj, size_t num_points) {
  const int w0h = p.w[0], B = p.B;
  const double rho = (double)num_points / ((double)p.rows * (double)p.cols);
  // bins an interior tile's region spans (same integer arithmetic as the kernel)
  const int bi = (kTileI + kTileI - 1 + w0h + p.M) / B - (kTileI - w0h + p.M) / B + 1;
  const int bj = (tj + tj - 1 + w0h + p.M) / B - (tj - w0h + p.M) / B + 1;
  const double e = rho * (double)(bi * B) * (double)(bj * B);
  return e + 5.0 * std::sqrt(e);
}

// Tile height and LDS point capacity of the main launch from the cloud's MEAN density (points per
// cell).  64x16 tiles with 1024 slots need ~37 KB of LDS -> 4 workgroups per CU; denser clouds take
// 64x32 / 2048 (2 per CU), then 64x16 / 2048.  A tile that still overflows (clustered cloud) takes the
// global-memory path on its own.  Single-precision mode: 16-byte records, so 4096 points still leave two
// workgroups per CU -- clouds of ~1.2 .. 2.2 points per cell keep the one-workgroup-per-tile launch --,
// and 7680 one.  Returns the capacity.
inline int plan_tile_shape(const DsmPlanInput& in, DsmParams* p) {
  auto need = [&](int tj) { return region_need(*p, tj, in.num_points); };
  int tile_j = 16, cap = 2048;
  if (need(16) <= 1024.0) {
    cap = 1024;
  } else if (need(32) <= 2048.0) {
    tile_j = 32;
  } else if (need(16) > 2048.0 && runs_single_precision(in, *p) && need(16) <= 7680.0) {
    cap = need(16) <= 4096.0 ? 4096 : 7680;
  }
#ifdef AMHIP_TIMING_PROBES
  if (in.gather_tj != 0.0) {  // tuning knob
    tile_j = (int)in.gather_tj == 16 ? 16 : 32;
    cap = (tile_j == 16 && need(16) <= 1024.0) ? 1024 : 2048;  // (the density still picks the capacity)
  }
#endif
  p->tile_j = tile_j;
  p->tiles_i = (p->rows + kTileI - 1) / kTileI;
  p->tiles_j = (p->cols + tile_j - 1) / tile_j;
  return cap;
}

// Disc-shaped window of the first search: a point whose cell row differs by dj from the query's is at
// least (|dj| - 0.5) * res away in y; what is left of the radius bounds its column distance.
inline void plan_disc_tables(const DsmPlanInput& in, DsmParams* p) {
  const int w0 = p->w[0];
  const double r2 = p->T[0] / (in.grid.resolution * in.grid.resolution);  // in cells^2
  for (int dj = -w0; dj <= w0; ++dj) {
    const double dy = std::fabs((double)dj) - 0.5 - 1e-6;
    const double rem = dy > 0.0 ? r2 - dy * dy : r2;
    const int wr = rem > 0.0 ? static_cast<int>(std::floor(std::sqrt(rem) + 0.5 + 1e-6)) : 0;
    p->wr[dj + w0] = std::min(wr, w0);
  }
  for (int r = 0; r <= 2 * w0 + 1; ++r) {
    const int a = r <= 2 * w0 ? p->wr[r] : 0;
    const int b = r >= 1 ? p->wr[r - 1] : 0;
    p->wr2[r] = std::max(a, b);
  }
  for (int k = 0; k <= w0; ++k) p->wrp[k] = std::max(p->wr2[2 * k], p->wr2[2 * k + 1]);
}

// The FP64 image of the main launch.  false: it fits no CU.
inline bool plan_lds_image(int cap, DsmParams* p) {
  const int w0 = p->w[0];
  const int rw = kTileI + 2 * w0 + 2 * (p->B - 1);
  const int rh = p->tile_j + 2 * w0 + 2 * (p->B - 1);
  // row pairs, +1 pair for the parity shift, +1 spill; (lds_cells + 1) entries, a multiple of
  // four with three to spare: the single-precision gather clears / scans the table in quads
  p->lds_cells = ((rw * (rh + 4) + 4 + 3) & ~3) - 1;
  p->lds_cap = cap;  // == kCap of the kernel instance
  p->lds_bytes = lds_image_bytes(false, cap, p->lds_cells, p->tile_j);
  // (a 4096- / 7680-point main launch exists in single precision only; the FP64 kernels then
  // run on lists with images of their own size: plan_gather_classes)
  return !(p->lds_bytes > kLdsBudgetOnePerCU && cap <= 2048);
}

// Single-precision gather with exact guards (amhip_dsm.hip: k_dsm_gather_f32): the fixed-point scale,
// the decision margins and the image of 16-byte records
inline void plan_f32_guards(const DsmPlanInput& in, DsmParams* p) {
  int S = 28;
  while (((long long)(p->w[0] + 2) << S) >= (1LL << 31)) --S;
  const double scale2 = std::ldexp(1.0, 2 * S);
  const double tc = p->T[0] / (in.grid.resolution * in.grid.resolution) * scale2;
  // |d2_f32 - d2_reference| <= 3e-7 relative at the search radius; anything
  // inside +-2e-6 is decided by the FP64 routine
  const double margin = 2e-6;
  // (cells within theta of a point go to the FP64 routine: 0.02 -> 0.005 takes 0.07 ms of
  // redo tails off the 50 M-point gather and costs the error budget a factor 2.2 in eps_w --
  // a tile's height half-range limit goes from 7.6 to 6.2 m; measured)
  double theta = 0.005;  // cells
#ifdef AMHIP_TIMING_PROBES
  if (in.fx_theta != 0.0) theta = in.fx_theta;
#endif
  const double q = std::ldexp(1.0, -(S + 1));
  p->fx_S = S;
  p->fx_thi = static_cast<float>(tc * (1.0 + margin));
  p->fx_tlo = static_cast<float>(tc * (1.0 - margin));
  p->fx_denmax = static_cast<float>(1.0 / (theta * theta * scale2));
  p->fx_epsw = static_cast<float>(2.0 * std::sqrt(2.0) * q / theta + 4e-7);
  p->lds_bytes_f32 = lds_image_bytes(true, p->lds_cap, p->lds_cells, p->tile_j);
  p->fx_ok = 1;
}

// AMHIP_OK, or AMHIP_ERR_ARG with *why naming the reason.
inline int plan_dsm(const DsmPlanInput& in, DsmParams* out, const char** why) {
  DsmParams p;
  std::memset(&p, 0, sizeof(p));
  grid_bases(in.grid, &p.base_x, &p.base_y);
  p.res = in.grid.resolution;
  p.inv_res = 1.0 / in.grid.resolution;
  p.rows = in.win_rows;
  p.cols = in.win_cols;
  p.i_off = in.win_i0;
  p.j_off = in.win_j0;
  p.sub_x = in.center_northing;  // dsm.cc:42
  p.sub_y = in.center_easting;   // dsm.cc:43
  p.canon_all = in.canon_all ? 1 : 0;
  p.pcl_mode = in.mode;
  if (!plan_ladder(in, &p)) {
    *why = "radius ladder too long";
    return AMHIP_ERR_ARG;
  }
  if (!plan_bins(in, &p)) {
    *why = "grid too large for 32-bit bin ids";
    return AMHIP_ERR_ARG;
  }
  plan_sort(in, &p);
  plan_multipliers(&p);
  // ---- LDS-tiled gather (amhip_dsm.hip: k_dsm_gather_tiled), first level only ----
  const int cap = plan_tile_shape(in, &p);
  const int w0 = p.w[0];
  p.lds_ok = (w0 >= 1 && w0 <= kMaxW0 && !(in.mode == 1 && in.pcl_lambda > 1)) ? 1 : 0;
  if (p.lds_ok) {
    plan_disc_tables(in, &p);
    if (!plan_lds_image(cap, &p)) p.lds_ok = 0;
  }
  // (capped mode: the LDS-tiled gather's own build, k_dsm_gather_tiled_knn; tuning knob knn_global_bins:
  // one lane per cell on the global bins, the round-1 kernel)
  p.knn_k = in.mode == 0 ? in.dsm_knn : 0;
  if (p.knn_k && in.knn_global_bins) p.lds_ok = 0;
  if (p.lds_ok && runs_single_precision(in, p)) plan_f32_guards(in, &p);
  p.out_i0 = p.out_j0 = 0;
  p.out_pitch = p.rows;
  *out = p;
  return AMHIP_OK;
}

// ---------------------------------------------------------------------------
// plan_gather_classes
// ---------------------------------------------------------------------------
// Capacity classes (k_dsm_tile_occupancy): tiles whose first-level region holds more points than the
// main launch's LDS image go to list launches with larger images (fewer workgroups per CU, still
// LDS-resident); beyond that gather_tile() takes the global-memory path.  Capacities follow the
// workgroups a CU's 160 KB of LDS can hold: class 1 = the most that still leaves two per CU; class 2 =
// everything one workgroup can take -- up to the register instances the library holds (launch_gathers):
constexpr int kClass1CeilingTj16 = 2752, kClass1CeilingTj32 = 2432;  // FP64 instances of class 1
constexpr int kClass2CeilingTj16 = 5600, kClass2CeilingTj32 = 5200;  // ... of class 2
constexpr int kClass1CeilingF32 = 4096, kClass2CeilingF32 = 7680;    // single-precision instances
constexpr int kMainCapMaxFp64 = 2048;   // (a main launch above it is a single-precision one)
constexpr int class1_ceiling(int tile_j) { return tile_j == 16 ? kClass1CeilingTj16 : kClass1CeilingTj32; }
constexpr int class2_ceiling(int tile_j) { return tile_j == 16 ? kClass2CeilingTj16 : kClass2CeilingTj32; }

struct GatherCallFlags {
  bool fill_untouched;   // the gather writes the initial value into cells it leaves
  bool mask, unfilled;   // the call has a fill mask / an unfilled-cell counter
  bool bin_z_valid;      // the sort left per-bin height ranges
};
struct GatherClasses {
  bool f32;           // single-precision mode
  bool sparse;        // only the occupied tiles are visited, by a fixed grid walking kListMain
  bool use_bin_z;     // the pre-pass files tiles without room under the error bound by their bins' height ranges
  bool rej_own;       // the FP64 kernel's image of cap0 points fits a CU: redo tiles go to kListRedoOwn
  bool rej_dense;     // ... and are taken by a dense launch filtering on occ instead of the list
  bool skip_classes;  // no class launches: the main launch takes every class
  int cap0;           // points of the main launch's LDS image
  int cap1, cap2;     // FP64 images of classes 1, 2
  int capf1, capf2;   // single-precision images of classes 1, 2
  int ccap0, ccap1, ccap2;  // what the occupancy pre-pass classifies by
  unsigned long long sig;   // the geometry this call's tile counters will describe
};

// p: a plan with lds_ok.  prev_stats: the previous call's tile counters (kListHdr words of a pinned
// mirror that is never waited for -- a value one call late is as good --, or null), prev_ntiles its tile
// count (0: not the LDS-tiled gather), prev_sig the signature it left.
inline GatherClasses plan_gather_classes(const DsmParams& p, size_t n, const GatherCallFlags& fl,
                                         const volatile unsigned* prev_stats, int64_t prev_ntiles,
                                         unsigned long long prev_sig, bool no_launch_skips) {
  GatherClasses g;
  const unsigned ntiles = (unsigned)p.tiles_i * (unsigned)p.tiles_j;
  // Sparse call (few points per map cell, the layer already materialized)
  g.sparse = !fl.fill_untouched && ntiles > 8192 && (double)n * 16.0 < (double)p.rows * (double)p.cols;
  g.f32 = p.fx_ok && !p.pcl_mode && !p.only_unfilled && !fl.mask && !fl.unfilled;
  g.cap0 = p.lds_cap;
  // (the rest of the LDS image -- cell table, row tables, flags -- grows with the search window: wide
  // radii / coarse grids leave less room for points; a class that cannot hold more than the one below
  // it stays empty.  cap0 > 2048: a single-precision main launch -- the FP64 images keep their own sizes)
  auto fit = [&](bool f32, long limit) { return lds_cap_fit(f32, limit, p.lds_cells, p.tile_j); };
  g.cap1 = std::max(std::min(g.cap0, kMainCapMaxFp64), std::min(class1_ceiling(p.tile_j), fit(false, kLdsBudgetTwoPerCU)));
  g.cap2 = std::max(g.cap1, std::min(class2_ceiling(p.tile_j), fit(false, kLdsBudgetOnePerCU)));
  // Single-precision mode: its records take 16 bytes against the FP64 kernel's 24, so the same two LDS
  // budgets hold more points: classes 1 and 2 are cut at capf1 / capf2 and walked by list launches of
  // the single-precision kernel; what those hand back goes to the FP64 kernel's largest image
  // (kListRedoBig) or, beyond it, to the wave-per-block kernel (kListRedoWaveBlock).
  g.capf1 = std::max(g.cap0, std::min(kClass1CeilingF32, fit(true, kLdsBudgetTwoPerCU)));
  g.capf2 = std::max(g.capf1, std::min(kClass2CeilingF32, fit(true, kLdsBudgetOnePerCU)));
  g.ccap0 = g.cap0;
  g.ccap1 = g.f32 ? g.capf1 : g.cap1;
  g.ccap2 = g.f32 ? g.capf2 : g.cap2;
  // single-precision mode after the three-pass sort: tiles whose height range leaves no room under the
  // error bound go straight onto the FP64 list the kernel would hand them to -- kListRedoOwn while the
  // FP64 kernel's image of cap0 points fits a CU (rej_own), else kListRedoBig, or kListRedoWaveBlock
  // beyond its largest image
  g.rej_own = g.cap0 <= kMainCapMaxFp64 || (long)p.lds_bytes <= kLdsBudgetOnePerCU;
  g.use_bin_z = g.f32 && fl.bin_z_valid;
  // Rough scenes: when the PREVIOUS call pre-classified more than a tenth of its tiles for the FP64
  // kernel, that kernel is launched densely over the tiles (one workgroup each, filtering on occ) instead
  // of walking a list of tens of thousands with a fixed grid; a tenth or less: the list (an empty dense
  // launch would cost 0.18 ms of idle workgroups on smooth terrain).  Either is correct for any count.
  g.rej_dense = g.use_bin_z && g.cap0 <= kMainCapMaxFp64 && !g.sparse && prev_stats && prev_ntiles > 0 &&
                rejected_tiles(prev_stats) * 10.0 > (double)prev_ntiles;
  // The capacity-class launches behind the main one (classes 1, 2, the wave-per-block kernel) are SKIPPED
  // when the previous call of this geometry left all three lists empty: the main launch then takes every
  // class -- a stray denser tile walks the global bins (gather_tile: use_lds false), slower, same result
  // -- and the counters this call leaves bring the class launches back for the next one.
  g.sig = 1469598103934665603ull;
  for (const int v : {p.rows, p.cols, p.i_off, p.j_off, p.tile_j, p.lds_cap, p.B, p.M, p.w[0], p.pcl_mode, g.cap1, g.cap2})
    g.sig = (g.sig ^ (unsigned long long)(unsigned)v) * 1099511628211ull;
  g.skip_classes = !g.f32 && !g.sparse && prev_stats && prev_sig == g.sig && prev_stats[kListClass1] == 0u &&
                   prev_stats[kListClass2] == 0u && prev_stats[kListWaveBlock] == 0u && !no_launch_skips;
  return g;
}

// ---------------------------------------------------------------------------
// rough_policy_step
// ---------------------------------------------------------------------------
// The single-precision mode on rough terrain (amhip_api.hip: dsm_rough_policy): after a call that filed
// more than half of its tiles for the FP64 kernel, that call's successor and the next kRoughHoldCalls
// run the FP64 pipeline outright.
constexpr int kRoughHoldCalls = 15;
struct RoughState {
  int hold;             // calls left before the single-precision pipeline is tried again
  bool last_call_f32;   // the last DSM call ran the record pipeline with bin ranges
  int64_t last_ntiles;  // gather tiles of the last call
};
// enabled: the context is in the single-precision mode and the switch is not turned off.  stats: the last
// call's tile counters (may be null).  Returns 1 when this call runs the FP64 pipeline outright.
inline int rough_policy_step(RoughState* s, bool enabled, const volatile unsigned* stats) {
  if (!enabled) return 0;
  if (s->hold > 0) {
    --s->hold;
    return 1;
  }
  if (s->last_call_f32 && s->last_ntiles > 0 && stats && rejected_tiles(stats) * 2.0 > (double)s->last_ntiles) {
    s->hold = kRoughHoldCalls;
    return 1;
  }
  return 0;
}

}  // namespace amhip

#endif  // AMHIP_DSM_PLAN_H_
