// amhip_ortho_plan.h -- what the host decides about one backward-grid mosaic call before anything is
// launched: the poses (hpose_*), the view bounds of a camera with a distortion model
// (camera_view_bounds), the side planes of the frame cull (side_planes), the frame table the kernels
// read (build_frame_table) and the parameter set and launch shape of the call (plan_ortho_call).
// Pure functions of their arguments: no HIP, no context, no tuning store --
// tests/cpp/ortho_plan_host_main.cc compiles this header alone.
#ifndef AMHIP_ORTHO_PLAN_H_
#define AMHIP_ORTHO_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "aerial_mapper_hip.h"
#include "amhip_dsm_plan.h"  // grid_bases, kTileI
#include "amhip_ortho_fold.h"
#include "amhip_session_plan.h"  // LayerState

namespace amhip {

constexpr int kOrthoTileJ = 64;  // a mosaic workgroup's tile: kTileI x kOrthoTileJ cells

// Geometry, camera and switches of one mosaic call, passed by value to kernels.
struct OrthoParams {
  double base_x, base_y, res;
  int rows, cols;
  int i_off, j_off;
  // camera
  double fu, fv, cu, cv;
  double dist[4];
  int width, height, distortion;
  // frames
  int num_frames;
  int channels, colored;
  size_t frame_stride, row_step;
  // side planes of the frame cull in the camera frame (unit normals, inside = n.p >= 0): the
  // view pyramid of an undistorted camera, the outer rectangle of one with a distortion model
  double pl[4][3];
  int cull;
  // lazy reset: elevation_angle / observation_index / the output layer are
  // logically in their initial state but their memory is not filled -- do not
  // read them, and write the initial values into every cell no view is
  // accepted for; same for num_observations (initial 0: `+= itself` keeps it)
  int virt_out, virt_nobs;
  // the global elevation range is available: pre-cull the frames with it and
  // leave the tile before touching its elevation when nothing can see it
  int coarse;
  // margin-guarded fold (amhip_ortho_fold.h): undistorted pinhole, unit
  // quaternions; the frame table follows the poses in the same buffer
  int fast;
  FoldCam fold;
  // dominance pruning of a tile's frame list (frame_bounds / dominated):
  // undistorted pinhole, num_observations logically zero
  int prune;
  // the bounding spheres assume rigid poses; |q|^2 = 1 + dev scales distances
  // by that much: radii are multiplied by 1 + 2 max|dev|
  double radius_scale;
  // cameras with a distortion model: |p| <= r_in z  =>  visible by a clear
  // margin (0: unknown); lets frame_bounds() call a frame fully visible
  double r_in;
};
static_assert(sizeof(OrthoParams) == 360, "OrthoParams is passed by value to every mosaic kernel");

// ---------------------------------------------------------------------------
// pose arithmetic
// ---------------------------------------------------------------------------
// THE one place in the product that holds the external pose formulas (minkindr's QuatTransformation
// over Eigen's quaternion; mirrored by oracle/amo_compat.h), used to build T_G_C = T_G_B * T_C_B^-1
// and T_C_G = T_G_C^-1 on the host.  The rotation is amhip_ortho_fold.h's transform_point without its
// translation, so the composition and the per-cell transform agree operation for operation.
// Two upstream variants are known and NOT implemented here ("Parity first", 1 and 2; a
// switchable profile for them changes results and is a pull request of its own):
//   * hpose_compose's quaternion product is Eigen's generic quat_product; with SSE2 an x86-64 build
//     of Eigen takes the specialisation of Geometry/arch/Geometry_SSE.h, which associates the same
//     sixteen products differently (last-ulp differences whenever T_C_B is not the identity);
//   * hpose_inverse takes the bare conjugate; minkindr's inverse() is (q.inverse(),
//     -q.inverseRotate(t)) on the Eigen quaternion, whose inverse() is conjugate().coeffs() /
//     squaredNorm() (an ulp of the inverse translation for |q|^2 = 1 +- 1e-16).
struct HPose {
  double qw, qx, qy, qz, tx, ty, tz;
};

inline HPose hpose_from7(const double* p) {
  HPose r;
  r.tx = p[0];
  r.ty = p[1];
  r.tz = p[2];
  r.qw = p[3];
  r.qx = p[4];
  r.qy = p[5];
  r.qz = p[6];
  return r;
}

// Eigen::Quaternion::_transformVector: the rotation of transform_point (amhip_ortho_fold.h), and
// no more -- adding a zero translation would turn a component -0.0 into +0.0
inline V3 hpose_rotate(const HPose& T, const V3& v) {
  const V3 qv = {T.qx, T.qy, T.qz};
  V3 uv = cross3(qv, v);
  uv.x = uv.x + uv.x;
  uv.y = uv.y + uv.y;
  uv.z = uv.z + uv.z;
  const V3 c2 = cross3(qv, uv);
  V3 r;
  r.x = (v.x + T.qw * uv.x) + c2.x;
  r.y = (v.y + T.qw * uv.y) + c2.y;
  r.z = (v.z + T.qw * uv.z) + c2.z;
  return r;
}

// inverse() = (q*, -(q* (x) t))
inline HPose hpose_inverse(const HPose& T) {
  HPose r;
  r.qw = T.qw;
  r.qx = -T.qx;
  r.qy = -T.qy;
  r.qz = -T.qz;
  const V3 t = {T.tx, T.ty, T.tz};
  const V3 rt = hpose_rotate(r, t);
  r.tx = -rt.x;
  r.ty = -rt.y;
  r.tz = -rt.z;
  return r;
}

// A * B = (qA qB, tA + qA (x) tB)
inline HPose hpose_compose(const HPose& A, const HPose& B) {
  HPose r;
  r.qw = A.qw * B.qw - A.qx * B.qx - A.qy * B.qy - A.qz * B.qz;
  r.qx = A.qw * B.qx + A.qx * B.qw + A.qy * B.qz - A.qz * B.qy;
  r.qy = A.qw * B.qy + A.qy * B.qw + A.qz * B.qx - A.qx * B.qz;
  r.qz = A.qw * B.qz + A.qz * B.qw + A.qx * B.qy - A.qy * B.qx;
  const V3 tb = {B.tx, B.ty, B.tz};
  const V3 rt = hpose_rotate(A, tb);
  r.tx = A.tx + rt.x;
  r.ty = A.ty + rt.y;
  r.tz = A.tz + rt.z;
  return r;
}

// ---------------------------------------------------------------------------
// view bounds of a camera with a distortion model
// ---------------------------------------------------------------------------
// Conservative view cone of a camera WITH distortion: the largest normalised
// radius rho = sqrt(x^2 + y^2) / z a landmark can have and still project into
// the image (plus margins).  The reference tests nothing but the image box
// (ortho-backward-grid.cc:164-171), so where the distortion polynomial folds
// back, far off-axis landmarks DO count as visible -- the bound covers that.
// A landmark is visible only if |distort(p)| <= B, B = farthest image corner
// (+1 pixel) in distorted normalised coordinates; |distort(p)| is bounded from
// below by g(|p|), and the supremum of {r : g(r) <= B} is found on a grid with
// a Lipschitz margin per step (so no dip between samples is missed) plus an
// analytic tail.  false = no usable bound (the kernel then tests every frame).
inline bool distorted_view_cone(const amhip_camera& cam, double* cone) {
  double B = 0.0;
  const double us[2] = {-1.0, (double)cam.width}, vs[2] = {-1.0, (double)cam.height};
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const double x = (us[a] - cam.cu) / cam.fu, y = (vs[b] - cam.cv) / cam.fv;
      B = std::max(B, std::sqrt(x * x + y * y));
    }
  B = B * (1.0 + 1e-9) + 1e-9;
  if (cam.distortion == AMHIP_DIST_RADTAN) {
    const double k1 = cam.dist[0], k2 = cam.dist[1];
    const double c = 4.5 * (std::fabs(cam.dist[2]) + std::fabs(cam.dist[3]));  // tangential <= c r^2
    auto g = [&](double r) {
      const double r2 = r * r;
      return r * std::fabs(1.0 + k1 * r2 + k2 * r2 * r2) - c * r2;
    };
    auto lip = [&](double r) {
      const double r2 = r * r;
      return 1.0 + 3.0 * std::fabs(k1) * r2 + 5.0 * std::fabs(k2) * r2 * r2 + 2.0 * c * r;
    };
    const double Rmax = 1e4;
    // tail r >= Rmax: the leading term must dominate for good
    if (k2 != 0.0) {
      const double lead = std::fabs(k2) * Rmax * Rmax * Rmax * Rmax;
      if (!(lead > 2.0 * (std::fabs(k1) * Rmax * Rmax + 1.0 + c * Rmax)) ||
          !(0.5 * lead * Rmax > 2.0 * B))
        return false;
    } else if (k1 != 0.0) {
      const double lead = std::fabs(k1) * Rmax * Rmax;
      if (!(lead > 2.0 * (1.0 + c * Rmax)) || !(0.5 * lead * Rmax > 2.0 * B)) return false;
    } else if (c != 0.0) {
      return false;  // r - c r^2: no bound
    }
    double rstar = 0.0;
    double r = 0.0;
    while (r < Rmax) {
      const double h = r < 20.0 ? 5e-4 : r * 2.5e-5;
      const double rn = r + h;
      if (g(r) <= B + h * lip(rn)) rstar = rn;
      r = rn;
    }
    if (!(rstar < 0.5 * Rmax)) return false;
    *cone = rstar * (1.0 + 1e-6) + 1e-6;
    return true;
  }
  if (cam.distortion == AMHIP_DIST_EQUIDISTANT) {
    const double* k = cam.dist;
    auto td = [&](double th) {
      const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
      return std::fabs(th * (1.0 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8));
    };
    const double half_pi = 1.5707963267948966;
    const double t2 = half_pi * half_pi, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double L = 1.0 + 3.0 * std::fabs(k[0]) * t2 + 5.0 * std::fabs(k[1]) * t4 +
                     7.0 * std::fabs(k[2]) * t6 + 9.0 * std::fabs(k[3]) * t8;
    const double h = 2e-5;
    double tstar = 0.0;
    for (double th = 0.0; th < half_pi; th += h)
      if (td(th) <= B + h * L) tstar = th + h;
    if (!(tstar < half_pi - 2e-3)) return false;  // sees (numerically) the whole half space
    *cone = std::tan(tstar) * (1.0 + 1e-6) + 1e-6;
    return true;
  }
  return false;
}

// Tighter bounds for cameras with a distortion model, given the view cone
// `cone` of distorted_view_cone() (every visible landmark has |p| <= cone * z):
//   ax, ay  outer rectangle: visible => |x| <= ax z and |y| <= ay z.  From
//           x_d = x s(r) + t_x with |t_x| <= c r^2 (radtan; s = the radial
//           factor, t = the tangential terms) resp. x_d = x s(r) (equidistant)
//           and |x_d| <= Bx for a visible landmark:  |x| <= (Bx + c cone^2) / min s.
//   rin     inner cone: |p| <= rin z  =>  visible by a clear margin.  The
//           distorted point of such a landmark has |x_d|, |y_d| <= r |s(r)| + c r^2
//           =: g(r); rin = the largest r with g <= (smallest distance of the
//           principal point to an image edge, normalised) on [0, r].
// Both scans carry a Lipschitz margin per step.  Values of 0 mean "no bound".
inline void distorted_rectangle_and_inner_cone(const amhip_camera& cam, double cone, double* ax,
                                               double* ay, double* rin) {
  *ax = *ay = cone;
  *rin = 0.0;
  const double W = cam.width, H = cam.height;
  // (the same one-pixel allowance as distorted_view_cone)
  const double Bx = std::max(std::fabs(-1.0 - cam.cu), std::fabs(W - cam.cu)) / cam.fu;
  const double By = std::max(std::fabs(-1.0 - cam.cv), std::fabs(H - cam.cv)) / cam.fv;
  const double bmin = std::min(std::min(cam.cu / cam.fu, (W - cam.cu) / cam.fu),
                               std::min(cam.cv / cam.fv, (H - cam.cv) / cam.fv));
  double c = 0.0;
  // s(r): radial factor; ds: an upper bound of |s'| that grows with r
  auto s_of = [&](double r) {
    if (cam.distortion == AMHIP_DIST_RADTAN) {
      const double r2 = r * r;
      return 1.0 + cam.dist[0] * r2 + cam.dist[1] * r2 * r2;
    }
    if (r < 1e-8) return 1.0;
    const double th = std::atan(r);
    const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    return th * (1.0 + cam.dist[0] * t2 + cam.dist[1] * t4 + cam.dist[2] * t6 + cam.dist[3] * t8) / r;
  };
  auto ds_of = [&](double r) {
    if (cam.distortion == AMHIP_DIST_RADTAN)
      return 2.0 * std::fabs(cam.dist[0]) * r + 4.0 * std::fabs(cam.dist[1]) * r * r * r;
    // s = theta_d(theta) / r, theta = atan r, theta_d = theta P(theta^2):
    //   s' = [P (r / (1 + r^2) - theta) + 2 theta^2 P' r / (1 + r^2)] / r^2
    // |theta_d'| <= L, |theta_d| <= L theta <= L r            =>  |s'| <= 2 L / r
    // |r / (1 + r^2) - atan r| <= r^3, theta <= r, |P| <= L   =>  |s'| <= (L + 2 Lp) r
    const double hp = 1.5707963267948966, t2 = hp * hp, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double L = 1.0 + 3.0 * std::fabs(cam.dist[0]) * t2 + 5.0 * std::fabs(cam.dist[1]) * t4 +
                     7.0 * std::fabs(cam.dist[2]) * t6 + 9.0 * std::fabs(cam.dist[3]) * t8;
    const double Lp = std::fabs(cam.dist[0]) + 2.0 * std::fabs(cam.dist[1]) * t2 +
                      3.0 * std::fabs(cam.dist[2]) * t4 + 4.0 * std::fabs(cam.dist[3]) * t6;
    return std::min(2.0 * L / std::max(r, 1e-12), (L + 2.0 * Lp) * r);
  };
  if (cam.distortion == AMHIP_DIST_RADTAN)
    c = 4.5 * (std::fabs(cam.dist[2]) + std::fabs(cam.dist[3]));
  if (!(cone > 0.0) || !(cone < 1e3)) return;
  // ---- outer rectangle: min |s| on [0, cone]
  {
    const int n = 20000;
    const double h = cone / n;
    double smin = 1e300;
    for (int k = 0; k <= n; ++k) {
      const double r = k * h;
      smin = std::min(smin, std::fabs(s_of(r)) - h * ds_of(r + h));
    }
    if (smin > 0.05) {
      const double tx = c * cone * cone;
      *ax = std::min(cone, ((Bx + tx) / smin) * (1.0 + 1e-6) + 1e-6);
      *ay = std::min(cone, ((By + tx) / smin) * (1.0 + 1e-6) + 1e-6);
    }
  }
  // ---- inner cone
  if (bmin > 0.0) {
    const double bound = bmin * (1.0 - 1e-6) - 1e-9;
    const double h = 2e-5;
    double r = 0.0, best = 0.0;
    while (r < cone) {
      const double rn = r + h;
      // g(r) = r |s(r)| + c r^2;  |g'| <= |s| + r |s'| + 2 c r
      const double g = r * std::fabs(s_of(r)) + c * r * r;
      const double lip = std::fabs(s_of(rn)) + h * ds_of(rn) + rn * ds_of(rn) + 2.0 * c * rn;
      if (!(g + h * lip <= bound)) break;
      best = rn;
      r = rn;
    }
    *rin = best;
  }
}

// What amhip_camera_view_bounds reports and the planner culls with (fu, fv > 0).  A camera with a
// distortion model: its view cone, outer rectangle and inner cone; usable false = no cone, and
// then no rectangle either: all zero.  An undistorted one: the image box as ax, ay, nothing else
// (its cull takes the view pyramid itself: plan_ortho_call).
struct ViewBounds {
  double cone, ax, ay, rin;
  bool usable;
};
inline ViewBounds camera_view_bounds(const amhip_camera& cam) {
  ViewBounds b = {0.0, 0.0, 0.0, 0.0, false};
  if (cam.distortion == AMHIP_DIST_NONE) {
    b.ax = std::max(cam.cu, (double)cam.width - cam.cu) / cam.fu;
    b.ay = std::max(cam.cv, (double)cam.height - cam.cv) / cam.fv;
    return b;
  }
  double cone = 0.0;
  if (!distorted_view_cone(cam, &cone)) return b;
  b.cone = cone;
  b.usable = true;
  distorted_rectangle_and_inner_cone(cam, cone, &b.ax, &b.ay, &b.rin);
  return b;
}

// (a few hundred thousand evaluations: kept per camera by the context)
struct ViewBoundsCache {
  bool valid = false;
  amhip_camera cam = {};
  ViewBounds bounds = {};
};
inline const ViewBounds& cached_view_bounds(ViewBoundsCache* cache, const amhip_camera& cam) {
  if (!cache->valid || std::memcmp(&cache->cam, &cam, sizeof(cam)) != 0) {
    cache->cam = cam;
    cache->bounds = camera_view_bounds(cam);
    cache->valid = true;
  }
  return cache->bounds;
}

// ---------------------------------------------------------------------------
// side planes
// ---------------------------------------------------------------------------
// Unit inward normals of four planes through the optical centre, camera frame:
//   left (sx, 0, left_z), right (-sx, 0, right_z), top (0, sy, top_z), bottom (0, -sy, bottom_z).
// The view pyramid of an undistorted pinhole is (fu, cu, W - cu, fv, cv, H - cv): a landmark with
// z > 0 projects into [0, W) x [0, H) only if it is on the inner side of all four (u >= 0, u < W,
// v >= 0, v < H); the rectangle |x| <= ax z, |y| <= ay z is (1, ax, ax, 1, ay, ay).
inline void side_planes(double sx, double left_z, double right_z, double sy, double top_z, double bottom_z,
                        double pl[4][3]) {
  const double n[4][3] = {{sx, 0.0, left_z}, {-sx, 0.0, right_z}, {0.0, sy, top_z}, {0.0, -sy, bottom_z}};
  for (int k = 0; k < 4; ++k) {
    const double len = std::sqrt(n[k][0] * n[k][0] + n[k][1] * n[k][1] + n[k][2] * n[k][2]);
    for (int d = 0; d < 3; ++d) pl[k][d] = n[k][d] / len;
  }
}

// ---------------------------------------------------------------------------
// frame table
// ---------------------------------------------------------------------------
// One buffer, one upload: FramePose[F], then FrameFast[F + 2] (two FramePose slots each; the two
// extra entries carry the camera for exact_view(), doubles 0..5, and the atan table of
// fold_finish(), doubles 8..24).
static_assert(sizeof(FrameFast) == 2 * sizeof(FramePose), "frame table layout");
inline size_t frame_table_slots(size_t F) { return F + 2 * (F + 2); }

struct FrameTable {
  double qdev;   // max | |q|^2 - 1 | over the frames (NaN sticks)
  bool fast_ok;  // every pose takes the margin-guarded fold
};
// table: frame_table_slots(F) entries.  T_C_G[f] = T_G_C[f].inverse() (ortho-backward-grid.cc:157-158;
// the reference recomputes it per cell and frame, the value is the same).  exact_fold: tuning knob
// ortho_exact_fold.
inline FrameTable build_frame_table(const amhip_camera& cam, const double* T_G_C, size_t F, bool exact_fold,
                                    FramePose* table) {
  FrameFast* fast = reinterpret_cast<FrameFast*>(table + F);
  FrameTable r;
  r.qdev = 0.0;
  r.fast_ok = cam.distortion == AMHIP_DIST_NONE && cam.fu > 0.0 && cam.fv > 0.0 && !exact_fold;
  for (size_t f = 0; f < F; ++f) {
    const HPose T = hpose_inverse(hpose_from7(T_G_C + 7 * f));
    table[f].qw = T.qw;
    table[f].qx = T.qx;
    table[f].qy = T.qy;
    table[f].qz = T.qz;
    table[f].tx = T.tx;
    table[f].ty = T.ty;
    table[f].tz = T.tz;
    table[f]._pad = 0.0;
    // (non-unit quaternion / non-finite pose: the whole call takes the exact kernel)
    if (!make_frame_fast(table[f], &fast[f])) r.fast_ok = false;
    const double dev = std::fabs(T.qw * T.qw + T.qx * T.qx + T.qy * T.qy + T.qz * T.qz - 1.0);
    if (!(dev <= r.qdev)) r.qdev = dev;  // (NaN sticks)
  }
  double* camd = reinterpret_cast<double*>(&fast[F]);
  std::memset(camd, 0, 2 * sizeof(FrameFast));
  make_atan_table(camd + 8);
  camd[0] = cam.fu;
  camd[1] = cam.fv;
  camd[2] = cam.cu;
  camd[3] = cam.cv;
  camd[4] = (double)cam.width;
  camd[5] = (double)cam.height;
  return r;
}

// ---------------------------------------------------------------------------
// plan_ortho_call
// ---------------------------------------------------------------------------
// The tuning knobs of the mosaic, a snapshot taken by the caller (the names are the keys).
struct OrthoKnobs {
  bool no_distorted_cull;      // cameras with a distortion model: every frame is tested
  bool no_distorted_prune;     // ... no inner cone
  bool distorted_square_cull;  // ... A/B: the circumscribed square instead of the rectangle
  bool ortho_exact_fold;       // the reference's arithmetic for every pair (build_frame_table)
  bool no_coarse_cull;
  bool ortho_no_prune;
  bool ortho_no_tile_list;     // the dense launch -- A-B and tests
};

// Everything the plan of a call depends on (besides the poses: build_frame_table).
struct OrthoPlanInput {
  amhip_grid_desc grid;                    // the (global) map
  int win_i0, win_j0, win_rows, win_cols;  // the window of it the context owns
  amhip_camera cam;
  size_t F;
  size_t frame_stride, row_step;
  int channels, colored;
  bool zrange_valid;  // the context knows the range of the heights the DSM wrote
  // Ctx::layer_state of the layers the call looks at, before it
  unsigned char state_angle, state_index, state_out, state_nobs;  // (LayerState values)
  OrthoKnobs knobs;
};

// dense: one workgroup per tile, grid (grid_x, grid_y).  tile_list (small batch, big map, the output
// layers materialized): k_ortho_tile_list (builder_grid workgroups of 256 lanes) lists the tiles some
// frame can see into a buffer of list_elems ints, a fixed grid of list_grid workgroups walks them.
struct OrthoLaunch {
  bool tile_list;
  unsigned grid_x, grid_y;
  unsigned list_grid, builder_grid;
  size_t list_elems;
};
struct OrthoPlan {
  OrthoParams p;
  OrthoLaunch launch;
};

inline OrthoPlan plan_ortho_call(const OrthoPlanInput& in, const FrameTable& frames, ViewBoundsCache* cache) {
  const amhip_camera& cam = in.cam;
  OrthoPlan plan;
  OrthoParams& p = plan.p;
  std::memset(&p, 0, sizeof(p));
  grid_bases(in.grid, &p.base_x, &p.base_y);
  p.res = in.grid.resolution;
  p.rows = in.win_rows;
  p.cols = in.win_cols;
  p.i_off = in.win_i0;
  p.j_off = in.win_j0;
  p.fu = cam.fu;
  p.fv = cam.fv;
  p.cu = cam.cu;
  p.cv = cam.cv;
  for (int k = 0; k < 4; ++k) p.dist[k] = cam.dist[k];
  p.width = cam.width;
  p.height = cam.height;
  p.distortion = cam.distortion;
  p.num_frames = static_cast<int>(in.F);
  p.channels = in.channels;
  p.colored = in.colored;
  p.frame_stride = in.frame_stride;
  p.row_step = in.row_step;
  // ---- frame cull: the view pyramid, or the outer rectangle of a camera with a distortion model
  const bool focal_ok = cam.fu > 0.0 && cam.fv > 0.0;
  if (cam.distortion == AMHIP_DIST_NONE) {
    if (focal_ok) {
      p.cull = 1;
      side_planes(cam.fu, cam.cu, (double)cam.width - cam.cu, cam.fv, cam.cv, (double)cam.height - cam.cv, p.pl);
    }
  } else if (focal_ok && !in.knobs.no_distorted_cull) {
    const ViewBounds& b = cached_view_bounds(cache, cam);
    if (b.usable) {
      // every visible landmark has |x| <= ax * z and |y| <= ay * z
      p.cull = 1;
      const bool square = in.knobs.distorted_square_cull;
      side_planes(1.0, square ? b.cone : b.ax, square ? b.cone : b.ax, 1.0, square ? b.cone : b.ay,
                  square ? b.cone : b.ay, p.pl);
      if (!in.knobs.no_distorted_prune) p.r_in = b.rin;
    }
  }
  // ---- layer states (lazy reset): elevation_angle, observation_index and the output layer are
  // either all produced with a fused fill or all materialized
  p.virt_out = (in.state_angle == kLayerLazyInitial && in.state_index == kLayerLazyInitial &&
                in.state_out == kLayerLazyInitial) ? 1 : 0;
  p.radius_scale = 1.0 + 2.0 * frames.qdev;
  if (!(frames.qdev < 0.25)) p.cull = 0;  // not a rotation at all (or NaN): every frame is tested
  // small batches on a big map: most tiles are out of every frame's sight
  p.coarse = (p.cull && in.zrange_valid && in.F <= 64 && !in.knobs.no_coarse_cull) ? 1 : 0;
  // num_observations is zero everywhere while it holds its initial value,
  // filled (0) or not (3): `+= itself` keeps it zero, the kernel neither reads
  // nor writes it and the layer stays in that state
  p.virt_nobs = layer_is_initial((LayerState)in.state_nobs) ? 1 : 0;
  p.prune = (p.cull && (cam.distortion == AMHIP_DIST_NONE || p.r_in > 0.0) && p.virt_nobs &&
             !in.knobs.ortho_no_prune) ? 1 : 0;
  p.fast = frames.fast_ok ? 1 : 0;
  p.fold = make_fold_cam(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height);
  // ---- launch
  OrthoLaunch& l = plan.launch;
  l.grid_x = (unsigned)((p.rows + kTileI - 1) / kTileI);
  l.grid_y = (unsigned)((p.cols + kOrthoTileJ - 1) / kOrthoTileJ);
  const size_t ntiles = (size_t)l.grid_x * (size_t)l.grid_y;
  // (from 16 K tiles: below, dispatching every tile costs less than the list's extra launch.
  // num_observations may stay lazily initial: the kernels neither read nor write it then.)
  l.tile_list = p.coarse && !p.virt_out && ntiles >= 16384 && !in.knobs.ortho_no_tile_list;
  l.list_grid = (unsigned)std::min<size_t>(ntiles, 256 * 16);
  l.builder_grid = (unsigned)((ntiles + 255) / 256);
  l.list_elems = ntiles + 16;
  return plan;
}

}  // namespace amhip

#endif  // AMHIP_ORTHO_PLAN_H_
