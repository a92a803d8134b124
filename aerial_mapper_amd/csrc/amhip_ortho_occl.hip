// amhip_ortho_occl.hip -- the backward-grid mosaic with an occlusion test ("true ortho";
// DESIGN.md section 4.19).
//
// The reference's visibility rule (ortho-backward-grid.cc:164-171) asks whether a cell's landmark
// projects into the frame in front of the camera, not whether the surface in between is in the
// way: on a DSM with buildings the ground behind a roof is painted with the roof.  This kernel
// folds with one more term, visible = in_box && z > 1e-10 && !occluded(cell, frame), where
// occluded() marches the elevation layer from the cell towards the camera (amhip_ortho_occl.h).
// Everything else is k_ortho_backward's (amhip_ortho.hip): one workgroup per tile of 64 x 64
// cells, the tile's frame list from the conservative sphere cull, every pair in the reference's
// arithmetic, ascending, strict `>` against the float-rounded running maximum.
//
// What it does NOT take over is the dominance pruning of the frame list: dominated() drops a
// frame because a frame fully visible over the tile beats it at every landmark -- which says
// nothing once the dominator can be occluded at some of them.
//
// The march is evaluated lazily: only for a pair that is otherwise visible AND whose angle would
// be accepted.  An occluded pair and a losing pair leave the fold in the same state, so the
// layers are the same bits as with the march in front of every pair; a cell marches about once
// per accepted update instead of once per frame of the list.
#include "amhip_ortho_dev.h"
#include "amhip_ortho_occl.h"

namespace amhip {

namespace {

constexpr int kOcclTileJ = kOrthoTileJ;
constexpr int kOcclThreads = 256;
constexpr int kOcclWaves = kOcclThreads / 64;
constexpr int kOcclSlab = 16;                       // cell columns folded at a time ...
constexpr int kOcclCells = kOcclSlab / kOcclWaves;  // ... = cells per lane
constexpr int kOcclChunk = 1024;                    // frames culled per pass

// (out of line: one copy of the loop for the four cells of a lane, nothing of it live in the fold)
__device__ __noinline__ bool occluded(const float* __restrict__ elevation, int rows, int cols, int i,
                                      int j, double x_c, double y_c, double h,
                                      const double* __restrict__ centre, double res, double margin,
                                      double zcut) {
  return occl_march(elevation, rows, cols, i, j, x_c, y_c, h, centre[0], centre[1], centre[2], res,
                    margin, zcut);
}

// The frames of [chunk0, chunk0 + chunk_n), chunk_n <= kOcclChunk, that may see the sphere:
// ascending in s_cand.  Returns their number (the same in every thread); ends with a barrier.
__device__ __forceinline__ int occl_cull_chunk(const OrthoParams& p, const FramePose* __restrict__ poses,
                                               const V3& centre, double radius, int chunk0,
                                               int chunk_n, int* s_cand, int* s_wave_cnt) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  int ncand = 0;
  for (int r = 0; r < chunk_n; r += kOcclThreads) {
    const int f = chunk0 + r + (int)threadIdx.x;
    bool keep = false;
    if (f < chunk0 + chunk_n) keep = !p.cull || frame_may_see(p, poses[f], centre, radius);
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();  // previous round's readers of s_wave_cnt are done
    if (lane == 0) s_wave_cnt[wid] = __popcll(m);
    __syncthreads();
    int base = ncand, tot = 0;
#pragma unroll
    for (int w = 0; w < kOcclWaves; ++w) {
      const int cw = s_wave_cnt[w];
      if (w < wid) base += cw;
      tot += cw;
    }
    if (keep) s_cand[base + before] = f;  // (base + before < chunk_n <= kOcclChunk)
    ncand += tot;
  }
  __syncthreads();  // s_cand complete
  return ncand;
}

}  // namespace

// One workgroup per tile (blockIdx = tile).  The layers' memory is real (the caller materialized
// a lazily reset layer): untouched cells are simply not written.
__global__ void __launch_bounds__(kOcclThreads)
k_ortho_occl_backward(OrthoParams p, OcclParams q, const FramePose* __restrict__ poses,
                      const uint8_t* __restrict__ frames, const float* __restrict__ elevation,
                      float* __restrict__ elevation_angle, float* __restrict__ observation_index,
                      float* __restrict__ num_observations, float* __restrict__ out_layer,
                      unsigned* __restrict__ dev_err) {
  __shared__ float s_red[2 * kOcclWaves];
  __shared__ int s_cand[kOcclChunk];
  __shared__ int s_wave_cnt[kOcclWaves];
  __shared__ float s_elev[kTileI * kOcclTileJ];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int tile_x = (int)blockIdx.x, tile_y = (int)blockIdx.y;
  const int i = tile_x * kTileI + lane;
  const int j0 = tile_y * kOcclTileJ;
  const bool i_ok = i < p.rows;

  // tile extents (cell centres)
  const int i_hi = min(tile_x * kTileI + kTileI, p.rows) - 1;
  const int j_hi = min(j0 + kOcclTileJ, p.cols) - 1;
  const double xa = p.base_x + p.res * (-(double)(tile_x * kTileI + p.i_off));
  const double xb = p.base_x + p.res * (-(double)(i_hi + p.i_off));
  const double ya = p.base_y + p.res * (-(double)(j0 + p.j_off));
  const double yb = p.base_y + p.res * (-(double)(j_hi + p.j_off));
  const double hx = 0.5 * fabs(xa - xb), hy = 0.5 * fabs(ya - yb);

  // ---- the tile's elevation range (and its elevations, parked in LDS for the slabs) ----------
  float zmin = __builtin_huge_valf(), zmax = -__builtin_huge_valf();
  if (i_ok) {
    for (int j = j0 + wid; j <= j_hi; j += kOcclWaves) {
      const float e = elevation[(size_t)i + (size_t)j * (size_t)p.rows];
      s_elev[(j - j0) * kTileI + lane] = e;  // (the slab that folds column j is this wave's)
      if (e == e) {  // NaN elevation can never be visible
        zmin = fminf(zmin, e);
        zmax = fmaxf(zmax, e);
      }
    }
  }
  zmin = wave_min_f(zmin);
  zmax = wave_max_f(zmax);
  if (lane == 0) {
    s_red[wid] = zmin;
    s_red[kOcclWaves + wid] = zmax;
  }
  __syncthreads();
  zmin = s_red[0];
  zmax = s_red[kOcclWaves];
#pragma unroll
  for (int w = 1; w < kOcclWaves; ++w) {
    zmin = fminf(zmin, s_red[w]);
    zmax = fmaxf(zmax, s_red[kOcclWaves + w]);
  }
  if (!(zmin <= zmax)) return;  // no finite elevation in the tile: every cell keeps its values

  // bounding sphere of the tile's landmarks (cell centres x elevation range); generous slack:
  // the cull only has to be conservative
  const V3 centre = {uniform_d(0.5 * (xa + xb)), uniform_d(0.5 * (ya + yb)),
                     uniform_d(0.5 * ((double)zmin + (double)zmax))};
  const double hz = 0.5 * ((double)zmax - (double)zmin);
  const double radius =
      uniform_d((sqrt(hx * hx + hy * hy + hz * hz) * (1.0 + 1e-9) + 1e-6) * p.radius_scale);
  // the march's height cut-off: the largest elevation of the whole map (ordered key)
  const double zcut = uniform_d(from_ordered_key(*q.zmax_key));

  // up to kOcclChunk frames: one list for the whole tile; more: culled per slab, chunk by chunk
  const bool single = p.num_frames <= kOcclChunk;
  int ncand0 = 0;
  if (single) ncand0 = occl_cull_chunk(p, poses, centre, radius, 0, p.num_frames, s_cand, s_wave_cnt);

  const double lx = p.base_x + p.res * (-(double)(i + p.i_off));
#pragma unroll 1
  for (int js = j0; js <= j_hi; js += kOcclSlab) {
    // ---- per-lane fold state: k_ortho_backward's (amhip_ortho.hip).  The reference keeps
    // (float)asin(|z| / ||p||) and accepts a view iff its asin exceeds that float; unless the two
    // squared sines are within 2.5e-6 (relative) of each other their order decides, and only a
    // near tie evaluates the angles.  The winner's angle is evaluated once, at the end.
    float elev[kOcclCells];
    float best[kOcclCells];  // stored angle (valid iff have_f)
    bool have_f[kOcclCells];
    double zb[kOcclCells];   // |z| and ||p||^2 of the current best view
    double n2b[kOcclCells];
    int best_f[kOcclCells], best_u[kOcclCells], best_v[kOcclCells], accepted[kOcclCells];
    bool bad_alpha = false;
#pragma unroll
    for (int c = 0; c < kOcclCells; ++c) {
      const int j = js + wid + c * kOcclWaves;
      const bool cell = i_ok && j < p.cols;
      elev[c] = cell ? s_elev[(j - j0) * kTileI + lane] : __builtin_nanf("");
      best[c] = cell ? elevation_angle[(size_t)i + (size_t)j * (size_t)p.rows] : 0.0f;
      have_f[c] = true;
      n2b[c] = 1.0;
      if (best[c] >= 1.5707964f)
        zb[c] = __builtin_huge_val();  // no asin exceeds (float)(pi/2)
      else if (best[c] > 0.0f)
        zb[c] = sin((double)best[c]);  // incremental mode: angle left by earlier batches
      else if (best[c] == best[c])
        zb[c] = 0.0;                   // fresh layer: every visible view wins (alpha > 0)
      else
        zb[c] = __builtin_huge_val();  // NaN in the layer: `alpha > NaN` never holds
      best_f[c] = -1;
      best_u[c] = best_v[c] = 0;
      accepted[c] = 0;
    }

    for (int chunk0 = 0; chunk0 < p.num_frames; chunk0 += kOcclChunk) {
      int ncand = ncand0;
      if (!single)
        ncand = occl_cull_chunk(p, poses, centre, radius, chunk0, min(kOcclChunk, p.num_frames - chunk0),
                                s_cand, s_wave_cnt);
      if (i_ok) {
        for (int k = 0; k < ncand; ++k) {
          const int f = __builtin_amdgcn_readfirstlane(s_cand[k]);
          const FramePose T = poses[f];
#pragma unroll
          for (int c = 0; c < kOcclCells; ++c) {
            const int j = js + wid + c * kOcclWaves;
            const double ly = p.base_y + p.res * (-(double)(j + p.j_off));
            const V3 landmark = {lx, ly, (double)elev[c]};
            const V3 cp = transform_point(T, landmark);
            double u, v;
            if (!project_visible(p, cp, &u, &v)) continue;
            const double zz = cp.z * cp.z;
            const double n2 = cp.x * cp.x + cp.y * cp.y + zz;
            const double lhs = zz * n2b[c];
            const double rhs = (zb[c] * zb[c]) * n2;
            bool accept = lhs > rhs * (1.0 + 2.5e-6);
            const bool reject = lhs < rhs * (1.0 - 2.5e-6);
            bool exact = false;
            float exact_angle = 0.0f;
            if (!accept && !reject) {
              // near tie: the reference's own arithmetic decides
              asm volatile("" ::: "memory");
              if (!have_f[c]) {
                best[c] = (float)view_angle(zb[c], n2b[c]);
                have_f[c] = true;
              }
              const double alpha = view_angle(fabs(cp.z), n2);
              if (!(alpha > 0.0)) bad_alpha = true;  // CHECK(alpha > 0.0)
              if (alpha > (double)best[c]) {
                exact_angle = (float)alpha;
                accept = true;
                exact = true;
              }
            }
            // the one term this kernel adds, asked last: a pair that loses needs no march
            if (accept && occluded(elevation, p.rows, p.cols, i, j, lx, ly, (double)elev[c],
                                   q.centres + 3 * (size_t)f, p.res, q.margin, zcut))
              accept = false;
            if (accept) {
              if (exact) best[c] = exact_angle;
              have_f[c] = exact;
              zb[c] = fabs(cp.z);
              n2b[c] = n2;
              best_f[c] = f;
              accepted[c]++;
              best_v[c] = min((int)round(v), p.height - 1);
              best_u[c] = min((int)round(u), p.width - 1);
            }
          }
        }
      }
      if (single) break;
      __syncthreads();  // everyone is done with s_cand before the next chunk
    }

    if (bad_alpha) atomicOr(dev_err, kDevErrAlphaNonPos);

    // ---- write back: a cell no view was accepted for keeps what the layers held -------------
#pragma unroll
    for (int c = 0; c < kOcclCells; ++c) {
      const int j = js + wid + c * kOcclWaves;
      if (!(i_ok && j < p.cols) || accepted[c] == 0) continue;
      if (!have_f[c]) {
        // the winning view's angle, evaluated exactly like the reference does
        const double alpha = view_angle(zb[c], n2b[c]);
        if (!(alpha > 0.0)) atomicOr(dev_err, kDevErrAlphaNonPos);  // CHECK(alpha > 0.0)
        best[c] = (float)alpha;
      }
      write_cell(p, frames, elevation_angle, observation_index, num_observations, out_layer, i, j,
                 best[c], best_f[c], accepted[c], best_u[c], best_v[c]);
    }
  }
}

// The largest elevation of the map (NaN never enters; +inf does, and switches the cut-off off)
// when the context does not know the range of its heights: an ordered key, atomicMax per wave.
__global__ void __launch_bounds__(256)
k_ortho_occl_zmax(const float* __restrict__ elevation, size_t cells,
                  unsigned long long* __restrict__ zmax_key) {
  float hi = -__builtin_huge_valf();
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (size_t)gridDim.x * 256) {
    const float e = elevation[k];
    if (e == e) hi = fmaxf(hi, e);
  }
  hi = wave_max_f(hi);
  if ((threadIdx.x & 63) == 0) atomicMax(zmax_key, ordered_key((double)hi));
}

int ortho_occl_run(Ctx* c, const OrthoPlan& plan, const OcclParams& q, const FramePose* dev_poses,
                   const uint8_t* dev_frames, unsigned long long* own_zmax_key) {
  ScopedTimer t(c, AMHIP_K_ORTHO);
  const OrthoParams& p = plan.p;
  float* out = p.colored ? c->layers[AMHIP_LAYER_COLORED_ORTHO] : c->layers[AMHIP_LAYER_ORTHO];
  c->dirty_on_device = false;  // (a dense launch can write anywhere in the map)
  c->dirty[0] = c->dirty[1] = 0;
  c->dirty[2] = c->win_rows;
  c->dirty[3] = c->win_cols;
  if (own_zmax_key) {  // (holds key(-inf): uploaded with the frame table)
    const unsigned grid = (unsigned)std::min<size_t>((c->cells + 255) / 256, 1024);
    hipLaunchKernelGGL(k_ortho_occl_zmax, dim3(grid), dim3(256), 0, c->stream,
                       c->layers[AMHIP_LAYER_ELEVATION], c->cells, own_zmax_key);
  }
  hipLaunchKernelGGL(k_ortho_occl_backward, dim3(plan.launch.grid_x, plan.launch.grid_y),
                     dim3(kOcclThreads), 0, c->stream, p, q, dev_poses, dev_frames,
                     c->layers[AMHIP_LAYER_ELEVATION], c->layers[AMHIP_LAYER_ELEVATION_ANGLE],
                     c->layers[AMHIP_LAYER_OBSERVATION_INDEX],
                     c->layers[AMHIP_LAYER_NUM_OBSERVATIONS], out, c->dev_err);
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

}  // namespace amhip
