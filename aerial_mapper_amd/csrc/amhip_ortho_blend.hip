// amhip_ortho_blend.hip -- the blended backward-grid mosaic.
//
// The reference paints a cell with one nearest pixel of the single most-nadir view: wherever the
// winning frame changes from one cell to the next, exposure differences show as a seam, and a
// cell ten frames see carries the noise of one.  This kernel gives the cell the weighted mean of
// the nearest pixels of EVERY view that is visible from it (and, with the occlusion test of
// section 4.19 on, unoccluded), weighted by a power of the sine of the view angle
// (amhip_ortho_blend.h).  The sums live in per-cell FP64 accumulators of the context, so frames
// 0..k in one call and k+1..F in the next give the bits of one call with all of them.
//
// Everything else is k_ortho_occl_backward's (amhip_ortho_occl.hip): one workgroup per tile of
// 64 x 64 cells, the tile's frame list from the conservative sphere cull (no dominance pruning: a
// dominated view still contributes), every pair in the reference's arithmetic, ascending; the
// fold for elevation_angle / observation_index / num_observations is that kernel's, beside the
// sums.  The march can no longer be lazy: a losing but visible view has to be tested, because it
// contributes.
//
// One lane owns a cell: the accumulators are read once and written once per cell and call,
// coalesced along i like the layers; no atomics.
#include "amhip_ortho_dev.h"
#include "amhip_ortho_blend.h"
#include "amhip_ortho_occl.h"

namespace amhip {

namespace {

constexpr int kBlendTileJ = kOrthoTileJ;
constexpr int kBlendThreads = 256;
constexpr int kBlendWaves = kBlendThreads / 64;
constexpr int kBlendSlab = 16;                         // cell columns folded at a time ...
constexpr int kBlendCells = kBlendSlab / kBlendWaves;  // ... = cells per lane
constexpr int kBlendChunk = 1024;                      // frames culled per pass

// (out of line: one copy of the loop for the four cells of a lane)
__device__ __noinline__ bool blend_occluded(const float* __restrict__ elevation, int rows, int cols,
                                            int i, int j, double x_c, double y_c, double h,
                                            const double* __restrict__ centre, double res,
                                            double margin, double zcut) {
  return occl_march(elevation, rows, cols, i, j, x_c, y_c, h, centre[0], centre[1], centre[2], res,
                    margin, zcut);
}

// The frames of [chunk0, chunk0 + chunk_n), chunk_n <= kBlendChunk, that may see the sphere:
// ascending in s_cand.  Returns their number (the same in every thread); ends with a barrier.
__device__ __forceinline__ int blend_cull_chunk(const OrthoParams& p, const FramePose* __restrict__ poses,
                                                const V3& centre, double radius, int chunk0,
                                                int chunk_n, int* s_cand, int* s_wave_cnt) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  int ncand = 0;
  for (int r = 0; r < chunk_n; r += kBlendThreads) {
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
    for (int w = 0; w < kBlendWaves; ++w) {
      const int cw = s_wave_cnt[w];
      if (w < wid) base += cw;
      tot += cw;
    }
    if (keep) s_cand[base + before] = f;  // (base + before < chunk_n <= kBlendChunk)
    ncand += tot;
  }
  __syncthreads();  // s_cand complete
  return ncand;
}

}  // namespace

// One workgroup per tile (blockIdx = tile).  The layers' memory is real (the caller materialized
// a lazily reset layer): untouched cells are simply not written.  NCH: 1 gray, 3 colour (B, G, R).
template <int NCH, bool OCCL>
__global__ void __launch_bounds__(kBlendThreads)
k_ortho_blend_backward(OrthoParams p, OcclParams q, BlendParams b, const FramePose* __restrict__ poses,
                       const uint8_t* __restrict__ frames, const float* __restrict__ elevation,
                       float* __restrict__ elevation_angle, float* __restrict__ observation_index,
                       float* __restrict__ num_observations, float* __restrict__ out_layer,
                       unsigned* __restrict__ dev_err) {
  __shared__ float s_red[2 * kBlendWaves];
  __shared__ int s_cand[kBlendChunk];
  __shared__ int s_wave_cnt[kBlendWaves];
  __shared__ float s_elev[kTileI * kBlendTileJ];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int tile_x = (int)blockIdx.x, tile_y = (int)blockIdx.y;
  const int i = tile_x * kTileI + lane;
  const int j0 = tile_y * kBlendTileJ;
  const bool i_ok = i < p.rows;

  // tile extents (cell centres)
  const int i_hi = min(tile_x * kTileI + kTileI, p.rows) - 1;
  const int j_hi = min(j0 + kBlendTileJ, p.cols) - 1;
  const double xa = p.base_x + p.res * (-(double)(tile_x * kTileI + p.i_off));
  const double xb = p.base_x + p.res * (-(double)(i_hi + p.i_off));
  const double ya = p.base_y + p.res * (-(double)(j0 + p.j_off));
  const double yb = p.base_y + p.res * (-(double)(j_hi + p.j_off));
  const double hx = 0.5 * fabs(xa - xb), hy = 0.5 * fabs(ya - yb);

  // ---- the tile's elevation range (and its elevations, parked in LDS for the slabs) ----------
  float zmin = __builtin_huge_valf(), zmax = -__builtin_huge_valf();
  if (i_ok) {
    for (int j = j0 + wid; j <= j_hi; j += kBlendWaves) {
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
    s_red[kBlendWaves + wid] = zmax;
  }
  __syncthreads();
  zmin = s_red[0];
  zmax = s_red[kBlendWaves];
#pragma unroll
  for (int w = 1; w < kBlendWaves; ++w) {
    zmin = fminf(zmin, s_red[w]);
    zmax = fmaxf(zmax, s_red[kBlendWaves + w]);
  }
  // no finite elevation in the tile: no pair contributes, every cell keeps its values -- but the
  // loop below still runs (over an empty frame list), because a cell of a reset map restarts its
  // sums whether anything sees it or not
  const bool blind = !(zmin <= zmax);

  // bounding sphere of the tile's landmarks (cell centres x elevation range); generous slack:
  // the cull only has to be conservative
  const V3 centre = {uniform_d(0.5 * (xa + xb)), uniform_d(0.5 * (ya + yb)),
                     uniform_d(blind ? 0.0 : 0.5 * ((double)zmin + (double)zmax))};
  const double hz = blind ? 0.0 : 0.5 * ((double)zmax - (double)zmin);
  const double radius =
      uniform_d((sqrt(hx * hx + hy * hy + hz * hz) * (1.0 + 1e-9) + 1e-6) * p.radius_scale);
  // the march's height cut-off: the largest elevation of the whole map (ordered key)
  double zcut = 0.0;
  if (OCCL) zcut = uniform_d(from_ordered_key(*q.zmax_key));

  // up to kBlendChunk frames: one list for the whole tile; more: culled per slab, chunk by chunk
  const int num_frames = blind ? 0 : p.num_frames;
  const bool single = num_frames <= kBlendChunk;
  int ncand0 = 0;
  if (single && !blind) ncand0 = blend_cull_chunk(p, poses, centre, radius, 0, num_frames, s_cand, s_wave_cnt);

  const double lx = p.base_x + p.res * (-(double)(i + p.i_off));
#pragma unroll 1
  for (int js = j0; js <= j_hi; js += kBlendSlab) {
    // ---- per-lane fold state: k_ortho_occl_backward's (amhip_ortho_occl.hip) ------------------
    float elev[kBlendCells];
    float best[kBlendCells];  // stored angle (valid iff have_f)
    bool have_f[kBlendCells];
    double zb[kBlendCells];   // |z| and ||p||^2 of the current best view
    double n2b[kBlendCells];
    int best_f[kBlendCells], accepted[kBlendCells];
    // ---- and the sums (amhip_ortho_blend.h) ---------------------------------------------------
    double wsum[kBlendCells], acc[kBlendCells][NCH];
    bool restart[kBlendCells], contributed[kBlendCells];
    bool bad_alpha = false;
#pragma unroll
    for (int c = 0; c < kBlendCells; ++c) {
      const int j = js + wid + c * kBlendWaves;
      const bool cell = i_ok && j < p.cols;
      const size_t at = (size_t)i + (size_t)j * (size_t)p.rows;
      elev[c] = cell ? s_elev[(j - j0) * kTileI + lane] : __builtin_nanf("");
      best[c] = cell ? elevation_angle[at] : 0.0f;
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
      accepted[c] = 0;
      // a cell no view was ever accepted for (observation_index NaN: a fresh or a reset map)
      // starts its sums from zero; any other continues from what the buffers hold
      const float index = cell ? observation_index[at] : 0.0f;
      restart[c] = cell && index != index;
      contributed[c] = false;
      const bool load = cell && !restart[c];
      wsum[c] = load ? b.wsum[at] : 0.0;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) acc[c][ch] = load ? b.acc[(size_t)ch * b.plane + at] : 0.0;
    }

    for (int chunk0 = 0; chunk0 < num_frames; chunk0 += kBlendChunk) {
      int ncand = ncand0;
      if (!single)
        ncand = blend_cull_chunk(p, poses, centre, radius, chunk0, min(kBlendChunk, num_frames - chunk0),
                                 s_cand, s_wave_cnt);
      if (i_ok) {
        for (int k = 0; k < ncand; ++k) {
          const int f = __builtin_amdgcn_readfirstlane(s_cand[k]);
          const FramePose T = poses[f];
#pragma unroll
          for (int c = 0; c < kBlendCells; ++c) {
            const int j = js + wid + c * kBlendWaves;
            const double ly = p.base_y + p.res * (-(double)(j + p.j_off));
            const V3 landmark = {lx, ly, (double)elev[c]};
            const V3 cp = transform_point(T, landmark);
            double u, v;
            if (!project_visible(p, cp, &u, &v)) continue;
            // the occlusion term, asked of every visible pair: a losing view contributes too
            if (OCCL && blend_occluded(elevation, p.rows, p.cols, i, j, lx, ly, (double)elev[c],
                                       q.centres + 3 * (size_t)f, p.res, q.margin, zcut))
              continue;
            const double zz = cp.z * cp.z;
            const double n2 = cp.x * cp.x + cp.y * cp.y + zz;
            // ---- the pair contributes its nearest pixel --------------------------------------
            {
              const double w = blend_weight(zz, n2, b.sharpness);
              const int kp_y = min((int)round(v), p.height - 1);
              const int kp_x = min((int)round(u), p.width - 1);
              const uint8_t* px = frames + (size_t)f * p.frame_stride + (size_t)kp_y * p.row_step +
                                  (size_t)kp_x * (size_t)NCH;
#pragma unroll
              for (int ch = 0; ch < NCH; ++ch) acc[c][ch] = acc[c][ch] + w * (double)px[ch];
              wsum[c] = wsum[c] + w;
              contributed[c] = true;
            }
            // ---- the fold ---------------------------------------------------------------------
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
            if (accept) {
              if (exact) best[c] = exact_angle;
              have_f[c] = exact;
              zb[c] = fabs(cp.z);
              n2b[c] = n2;
              best_f[c] = f;
              accepted[c]++;
            }
          }
        }
      }
      if (single) break;
      __syncthreads();  // everyone is done with s_cand before the next chunk
    }

    if (bad_alpha) atomicOr(dev_err, kDevErrAlphaNonPos);

    // ---- write back ---------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < kBlendCells; ++c) {
      const int j = js + wid + c * kBlendWaves;
      if (!(i_ok && j < p.cols)) continue;
      const size_t at = (size_t)i + (size_t)j * (size_t)p.rows;
      // the sums: what the next call continues from (a restarted cell's zeros included)
      if (restart[c] || contributed[c]) {
        b.wsum[at] = wsum[c];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) b.acc[(size_t)ch * b.plane + at] = acc[c][ch];
      }
      // the cell's value; every weight underflowed or nothing contributed: it keeps what it held
      const bool paint = contributed[c] && wsum[c] > 0.0;
      float pixel = 0.0f;
      if (paint) {
        if constexpr (NCH == 3)
          pixel = __uint_as_float(blend_pack_bgr(blend_value(acc[c][0], wsum[c]), blend_value(acc[c][1], wsum[c]),
                                                 blend_value(acc[c][2], wsum[c])));
        else
          pixel = (float)blend_value(acc[c][0], wsum[c]);
      }
      if (accepted[c] == 0) {  // a cell no view was accepted for keeps what the other layers held
        if (paint) out_layer[at] = pixel;
        continue;
      }
      if (!have_f[c]) {
        // the winning view's angle, evaluated exactly like the reference does
        const double alpha = view_angle(zb[c], n2b[c]);
        if (!(alpha > 0.0)) atomicOr(dev_err, kDevErrAlphaNonPos);  // CHECK(alpha > 0.0)
        best[c] = (float)alpha;
      }
      store_cell(p, elevation_angle, observation_index, num_observations, out_layer, i, j, best[c],
                 best_f[c], accepted[c], paint ? pixel : out_layer[at]);
    }
  }
}

// The largest elevation of the map when the context does not know the range of its heights:
// k_ortho_occl_zmax's reduction (amhip_ortho_occl.hip, which stays a translation unit of its own).
__global__ void __launch_bounds__(256)
k_ortho_blend_zmax(const float* __restrict__ elevation, size_t cells,
                   unsigned long long* __restrict__ zmax_key) {
  float hi = -__builtin_huge_valf();
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (size_t)gridDim.x * 256) {
    const float e = elevation[k];
    if (e == e) hi = fmaxf(hi, e);
  }
  hi = wave_max_f(hi);
  if ((threadIdx.x & 63) == 0) atomicMax(zmax_key, ordered_key((double)hi));
}

template <int NCH, bool OCCL>
static void blend_launch(Ctx* c, const OrthoPlan& plan, const OcclParams& q, const BlendParams& b,
                         const FramePose* dev_poses, const uint8_t* dev_frames, float* out) {
  hipLaunchKernelGGL((k_ortho_blend_backward<NCH, OCCL>), dim3(plan.launch.grid_x, plan.launch.grid_y),
                     dim3(kBlendThreads), 0, c->stream, plan.p, q, b, dev_poses, dev_frames,
                     c->layers[AMHIP_LAYER_ELEVATION], c->layers[AMHIP_LAYER_ELEVATION_ANGLE],
                     c->layers[AMHIP_LAYER_OBSERVATION_INDEX],
                     c->layers[AMHIP_LAYER_NUM_OBSERVATIONS], out, c->dev_err);
}

int ortho_blend_run(Ctx* c, const OrthoPlan& plan, const OcclParams* q, const BlendParams& b,
                    const FramePose* dev_poses, const uint8_t* dev_frames,
                    unsigned long long* own_zmax_key) {
  ScopedTimer t(c, AMHIP_K_ORTHO);
  const OrthoParams& p = plan.p;
  float* out = p.colored ? c->layers[AMHIP_LAYER_COLORED_ORTHO] : c->layers[AMHIP_LAYER_ORTHO];
  c->dirty_on_device = false;  // (a dense launch can write anywhere in the map)
  c->dirty[0] = c->dirty[1] = 0;
  c->dirty[2] = c->win_rows;
  c->dirty[3] = c->win_cols;
  if (q && own_zmax_key) {  // (holds key(-inf): uploaded with the frame table)
    const unsigned grid = (unsigned)std::min<size_t>((c->cells + 255) / 256, 1024);
    hipLaunchKernelGGL(k_ortho_blend_zmax, dim3(grid), dim3(256), 0, c->stream,
                       c->layers[AMHIP_LAYER_ELEVATION], c->cells, own_zmax_key);
  }
  const OcclParams none = {0.0, nullptr, nullptr};
  if (p.colored) {
    if (q) blend_launch<3, true>(c, plan, *q, b, dev_poses, dev_frames, out);
    else blend_launch<3, false>(c, plan, none, b, dev_poses, dev_frames, out);
  } else {
    if (q) blend_launch<1, true>(c, plan, *q, b, dev_poses, dev_frames, out);
    else blend_launch<1, false>(c, plan, none, b, dev_poses, dev_frames, out);
  }
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

}  // namespace amhip
