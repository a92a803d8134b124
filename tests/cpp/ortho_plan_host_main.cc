// ortho_plan_host_main.cc -- the host-side planner of a backward-grid mosaic call
// (aerial_mapper_amd/csrc/amhip_ortho_plan.h: hpose_*, camera_view_bounds, side_planes,
// build_frame_table, plan_ortho_call) as a stand-alone program.  tests/test_ortho_plan_host.py
// builds it with g++ (-ffp-contract=off, like the library), once plain and once with
// -fsanitize=address,undefined, and runs it as a child process.
//
//   ortho_plan_host_main dump <case file>    every value of every case as text, plus a line of
//                                            branch tags (which branches the case took)
//   ortho_plan_host_main check <case file>   the invariants of a plan; one line per violation, exit
//                                            status 1 if there is any
//
// A case is one line of key=value words behind its kind (tests/golden/ortho_plan/cases.txt):
//   compose  amhip_compose_T_G_C's arithmetic: T_G_B[f] * T_C_B^-1
//   bounds   camera_view_bounds of a camera
//   call     build_frame_table + plan_ortho_call
// Doubles are printed as %a; what lies downstream of libm's atan / tan -- the bounds and planes of
// an equidistant camera, the atan table -- as %.13g, so that the table does not hang on the C
// library's last bit.  The tags are derived here from the inputs and the results, not by
// instrumenting the planner.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "amhip_ortho_plan.h"

using namespace amhip;

typedef std::map<std::string, std::string> Words;

static double num(const Words& w, const char* key, double dflt) {
  const auto it = w.find(key);
  return it == w.end() ? dflt : std::strtod(it->second.c_str(), nullptr);
}
static std::string word(const Words& w, const char* key, const char* dflt) {
  const auto it = w.find(key);
  return it == w.end() ? dflt : it->second;
}

// ---- cameras ------------------------------------------------------------------------------------------
static amhip_camera make_camera(int W, int H, double fu, double fv, double cu, double cv, int model, double k0,
                                double k1, double k2, double k3) {
  amhip_camera c;
  std::memset(&c, 0, sizeof(c));
  c.fu = fu;
  c.fv = fv;
  c.cu = cu;
  c.cv = cv;
  c.width = W;
  c.height = H;
  c.distortion = model;
  c.dist[0] = k0;
  c.dist[1] = k1;
  c.dist[2] = k2;
  c.dist[3] = k3;
  return c;
}
// cam=<name>; the six distorted ones and the half-space fisheye are those of tests/test_camera_bounds.py
static bool camera_by_name(const std::string& n, amhip_camera* c) {
  const int R = AMHIP_DIST_RADTAN, E = AMHIP_DIST_EQUIDISTANT, N = AMHIP_DIST_NONE;
  if (n == "plain") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, N, 0, 0, 0, 0);
  else if (n == "plain_no_focal") *c = make_camera(640, 480, 0.0, 320.0, 210.0, 300.0, N, 0, 0, 0, 0);
  else if (n == "radtan_barrel") *c = make_camera(1920, 1080, 1400.0, 1400.0, 959.5, 539.5, R, -0.28, 0.07, 2e-4, -1e-4);
  else if (n == "radtan_pincushion") *c = make_camera(960, 540, 700.0, 690.0, 470.0, 280.0, R, 0.12, -0.02, -8e-4, 6e-4);
  else if (n == "radtan_folds_back") *c = make_camera(960, 540, 700.0, 690.0, 470.0, 280.0, R, -0.45, 0.0, 0.0, 0.0);
  else if (n == "radtan_off_centre") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, -0.2, 0.03, 1e-3, 2e-3);
  else if (n == "radtan_tangential_only") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, 0.0, 0.0, 1e-3, 2e-3);
  else if (n == "radtan_centre_outside") *c = make_camera(640, 480, 300.0, 320.0, -5.0, 300.0, R, -0.2, 0.03, 1e-3, 2e-3);
  else if (n == "radtan_weak_k1") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, 1e-9, 0.0, 0.0, 0.0);
  else if (n == "radtan_weak_k2") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, 0.1, 1e-12, 0.0, 0.0);
  else if (n == "radtan_dip_at_5000") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, -4e-8, 0.0, 0.0, 0.0);
  else if (n == "radtan_dip_at_1000") *c = make_camera(640, 480, 300.0, 320.0, 210.0, 300.0, R, -1e-6, 0.0, 0.0, 0.0);
  else if (n == "radtan_no_focal") *c = make_camera(640, 480, 300.0, -320.0, 210.0, 300.0, R, -0.2, 0.03, 1e-3, 2e-3);
  else if (n == "equidistant") *c = make_camera(1920, 1080, 1400.0, 1400.0, 959.5, 539.5, E, -0.01, 0.02, -0.005, 0.001);
  else if (n == "equidistant_wide") *c = make_camera(800, 600, 420.0, 420.0, 400.0, 300.0, E, 0.08, -0.03, 0.0, 0.0);
  else if (n == "fisheye_half_space") *c = make_camera(800, 600, 280.0, 280.0, 400.0, 300.0, E, 0.0, 0.0, 0.0, 0.0);
  else return false;
  return true;
}

// a double whose digits may hang on libm (equidistant cameras): 13 significant digits
static void put(const char* name, double v, bool libm) {
  if (libm) std::printf(" %s=%.13g", name, v);
  else std::printf(" %s=%a", name, v);
}

// ---- poses --------------------------------------------------------------------------------------------
// pose=<kind>: frame f of the case.  Built with + - * / sqrt alone (correctly rounded everywhere).
//   identity        no rotation, no translation
//   general         a unit quaternion and a translation that change with f
//   norm=<|q|^2>    the general quaternion scaled to that squared norm (pose=general only)
//   nan             frame 1 (frame 0 when F = 1) has a NaN qy
//   far             translations of 1e6 m
static void make_pose(const std::string& kind, double norm2, int f, int F, double* T7) {
  if (kind == "identity") {
    const double id[7] = {0, 0, 0, 1, 0, 0, 0};
    std::memcpy(T7, id, sizeof(id));
    return;
  }
  double q[4] = {0.9, 0.1 + 0.01 * f, -0.3, 0.2 - 0.02 * f};
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double s = std::sqrt(norm2);
  for (double& v : q) v = v / n * s;
  T7[0] = 10.0 + 3.0 * f;
  T7[1] = -20.0 + 2.0 * f;
  T7[2] = 100.0 + f;
  if (kind == "far") {
    T7[0] += 1e6;
    T7[1] -= 1e6;
  }
  for (int k = 0; k < 4; ++k) T7[3 + k] = q[k];
  if (kind == "nan" && f == (F > 1 ? 1 : 0)) T7[5] = std::numeric_limits<double>::quiet_NaN();
}

static void dump7(const char* name, int f, const double* T7) {
  std::printf("%s[%d]", name, f);
  for (int k = 0; k < 7; ++k) std::printf(" %a", T7[k]);
  std::printf("\n");
}

static void print_tags(const std::vector<std::string>& tags) {
  std::printf("tags");
  for (const std::string& t : tags) std::printf(" %s", t.c_str());
  std::printf("\n");
}

// ---- compose ------------------------------------------------------------------------------------------
static void compose_case(const Words& w) {
  const int F = (int)num(w, "F", 2);
  const std::string tcb = word(w, "tcb", "identity");
  double T_C_B[7];
  make_pose(tcb == "identity" ? "identity" : "general", 1.0, 5, 1, T_C_B);
  const HPose T_B_C = hpose_inverse(hpose_from7(T_C_B));
  for (int f = 0; f < F; ++f) {
    double T_G_B[7];
    make_pose(word(w, "pose", "general"), num(w, "norm", 1.0), f, F, T_G_B);
    const HPose p = hpose_compose(hpose_from7(T_G_B), T_B_C);
    const double o[7] = {p.tx, p.ty, p.tz, p.qw, p.qx, p.qy, p.qz};
    dump7("T_G_C", f, o);
  }
  print_tags({tcb == "identity" ? "compose_identity" : "compose_general"});
}

// ---- bounds -------------------------------------------------------------------------------------------
static void dump_bounds(const amhip_camera& cam, const ViewBounds& b) {
  const bool libm = cam.distortion == AMHIP_DIST_EQUIDISTANT;
  std::printf("bounds usable=%d", b.usable);
  put("cone", b.cone, libm);
  put("ax", b.ax, libm);
  put("ay", b.ay, libm);
  put("rin", b.rin, libm);
  std::printf("\n");
}
static void bounds_tags(const amhip_camera& cam, const ViewBounds& b, std::vector<std::string>* tags) {
  if (cam.distortion == AMHIP_DIST_NONE) {
    tags->push_back("bounds_image_box");
  } else if (b.usable) {
    tags->push_back(cam.distortion == AMHIP_DIST_RADTAN ? "bounds_radtan" : "bounds_equidistant");
    tags->push_back(b.rin > 0.0 ? "inner_cone" : "no_inner_cone");
    if (!(b.cone < 1e3)) tags->push_back("cone_beyond_1e3_no_rectangle");
    else tags->push_back(b.ax < b.cone || b.ay < b.cone ? "rectangle_inside_cone" : "rectangle_is_cone");
  } else if (cam.distortion == AMHIP_DIST_EQUIDISTANT) {
    tags->push_back("no_bound_half_space");
  } else {
    // (the tail test of distorted_view_cone, from the coefficients)
    const double k1 = std::fabs(cam.dist[0]), k2 = std::fabs(cam.dist[1]);
    const double c = 4.5 * (std::fabs(cam.dist[2]) + std::fabs(cam.dist[3]));
    if (k2 != 0.0 && !(k2 * 1e16 > 2.0 * (k1 * 1e8 + 1.0 + c * 1e4))) tags->push_back("no_bound_weak_k2_tail");
    else if (k2 == 0.0 && k1 != 0.0 && !(k1 * 1e8 > 2.0 * (1.0 + c * 1e4))) tags->push_back("no_bound_weak_k1_tail");
    else if (k2 == 0.0 && k1 == 0.0) tags->push_back("no_bound_tangential_only");
    else tags->push_back("no_bound_dip_beyond_half_the_scan");
  }
}

// ---- call ---------------------------------------------------------------------------------------------
static const char* const kKnobNames[] = {"no_distorted_cull", "no_distorted_prune", "distorted_square_cull",
                                         "ortho_exact_fold",  "no_coarse_cull",     "ortho_no_prune",
                                         "ortho_no_tile_list"};
static bool* knob_by_name(OrthoKnobs* k, const std::string& n) {
  bool* const at[] = {&k->no_distorted_cull, &k->no_distorted_prune, &k->distorted_square_cull, &k->ortho_exact_fold,
                      &k->no_coarse_cull,    &k->ortho_no_prune,     &k->ortho_no_tile_list};
  for (int i = 0; i < 7; ++i)
    if (n == kKnobNames[i]) return at[i];
  return nullptr;
}

struct Call {
  OrthoPlanInput in;
  std::vector<double> T_G_C;
  std::string pose, knob;
  double norm2;
};

static bool call_input(const Words& w, Call* c) {
  OrthoPlanInput& in = c->in;
  std::memset(&in, 0, sizeof(in));
  in.grid.rows = (int)num(w, "rows", 128);
  in.grid.cols = (int)num(w, "cols", 64);
  in.grid.resolution = num(w, "res", 0.25);
  in.grid.length_x = in.grid.rows * in.grid.resolution;
  in.grid.length_y = in.grid.cols * in.grid.resolution;
  in.grid.pos_x = num(w, "pos_x", 10.0);
  in.grid.pos_y = num(w, "pos_y", -20.0);
  in.win_i0 = (int)num(w, "i0", 0);
  in.win_j0 = (int)num(w, "j0", 0);
  in.win_rows = (int)num(w, "wrows", in.grid.rows);
  in.win_cols = (int)num(w, "wcols", in.grid.cols);
  if (!camera_by_name(word(w, "cam", "plain"), &in.cam)) return false;
  in.F = (size_t)num(w, "F", 2);
  in.colored = (int)num(w, "colored", 0);
  in.channels = in.colored ? 3 : 1;
  in.row_step = (size_t)num(w, "row_step", (double)in.cam.width * in.channels);
  in.frame_stride = (size_t)num(w, "frame_stride", (double)in.row_step * in.cam.height);
  in.zrange_valid = num(w, "zrange", 1) != 0;
  in.state_angle = (unsigned char)num(w, "angle", 1);
  in.state_index = (unsigned char)num(w, "index", 1);
  in.state_out = (unsigned char)num(w, "out", 1);
  in.state_nobs = (unsigned char)num(w, "nobs", 0);
  c->knob = word(w, "knob", "");
  if (!c->knob.empty()) {
    bool* k = knob_by_name(&in.knobs, c->knob);
    if (!k) return false;
    *k = true;
  }
  c->pose = word(w, "pose", "general");
  c->norm2 = num(w, "norm", 1.0);
  c->T_G_C.resize(7 * in.F);
  for (size_t f = 0; f < in.F; ++f) make_pose(c->pose, c->norm2, (int)f, (int)in.F, &c->T_G_C[7 * f]);
  return true;
}

static void dump_table(const Call& c, const std::vector<FramePose>& table, const FrameTable& ft) {
  const size_t F = c.in.F;
  std::printf("frames qdev=%a fast_ok=%d slots=%zu\n", ft.qdev, ft.fast_ok, table.size());
  // (every frame of a small case; of a large one the first and the last)
  for (size_t f = 0; f < F; ++f) {
    if (F > 4 && f != 0 && f != F - 1) continue;
    const FramePose& T = table[f];
    std::printf("pose[%zu] %a %a %a %a %a %a %a %a\n", f, T.qw, T.qx, T.qy, T.qz, T.tx, T.ty, T.tz, T._pad);
    const double* q = reinterpret_cast<const double*>(&table[F + 2 * f]);
    std::printf("fast[%zu]", f);
    for (int k = 0; k < 16; ++k) std::printf(" %a", q[k]);
    std::printf("\n");
  }
  const double* camd = reinterpret_cast<const double*>(&table[F + 2 * F]);
  std::printf("tail camera");
  for (int k = 0; k < 8; ++k) std::printf(" %a", camd[k]);
  std::printf("\ntail atan");
  for (int k = 8; k < 8 + kAtanTabSize; ++k) std::printf(" %.13g", camd[k]);
  std::printf("\ntail rest");
  for (int k = 8 + kAtanTabSize; k < 32; ++k) std::printf(" %a", camd[k]);
  std::printf("\n");
}

static void dump_plan(const Call& c, const OrthoPlan& plan) {
  const OrthoParams& p = plan.p;
  const bool libm = p.distortion == AMHIP_DIST_EQUIDISTANT;
  std::printf("base_x=%a base_y=%a res=%a rows=%d cols=%d i_off=%d j_off=%d\n", p.base_x, p.base_y, p.res, p.rows,
              p.cols, p.i_off, p.j_off);
  std::printf("fu=%a fv=%a cu=%a cv=%a dist=%a,%a,%a,%a width=%d height=%d distortion=%d\n", p.fu, p.fv, p.cu, p.cv,
              p.dist[0], p.dist[1], p.dist[2], p.dist[3], p.width, p.height, p.distortion);
  std::printf("num_frames=%d channels=%d colored=%d frame_stride=%zu row_step=%zu\n", p.num_frames, p.channels,
              p.colored, p.frame_stride, p.row_step);
  for (int k = 0; k < 4; ++k) {
    std::printf("pl[%d]", k);
    for (int d = 0; d < 3; ++d) std::printf(libm ? " %.13g" : " %a", p.pl[k][d]);
    std::printf("\n");
  }
  std::printf("cull=%d virt_out=%d virt_nobs=%d coarse=%d fast=%d prune=%d radius_scale=%a", p.cull, p.virt_out,
              p.virt_nobs, p.coarse, p.fast, p.prune, p.radius_scale);
  put("r_in", p.r_in, libm);
  std::printf("\nfold %a %a %a %a %a %a %a %a %a\n", p.fold.fu, p.fold.fv, p.fold.cu, p.fold.cv, p.fold.wcu,
              p.fold.hcv, p.fold.kuv, p.fold.kround, p.fold.uv_abs);
  const OrthoLaunch& l = plan.launch;
  std::printf("launch tile_list=%d grid=%u,%u list_grid=%u builder_grid=%u list_elems=%zu\n", l.tile_list, l.grid_x,
              l.grid_y, l.list_grid, l.builder_grid, l.list_elems);
  (void)c;
}

// which branches the case took
static void call_tags(const Call& c, const FrameTable& ft, const OrthoPlan& plan, const ViewBoundsCache& cache,
                      std::vector<std::string>* tags) {
  const OrthoPlanInput& in = c.in;
  const OrthoParams& p = plan.p;
  const bool focal = in.cam.fu > 0.0 && in.cam.fv > 0.0;
  // poses
  tags->push_back("pose_" + c.pose);
  if (in.F == 1) tags->push_back("table_F1");
  if (in.F == 3) tags->push_back("table_F3");
  if (c.norm2 != 1.0 && std::fabs(c.norm2 - 1.0) < 1e-6) tags->push_back(c.norm2 > 1.0 ? "norm_above_keeps_fast" : "norm_below_keeps_fast");
  if (std::fabs(c.norm2 - 1.0) >= 1e-6 && std::fabs(c.norm2 - 1.0) < 0.25)
    tags->push_back(c.norm2 > 1.0 ? "norm_above_refuses_fast" : "norm_below_refuses_fast");
  if (c.pose == "nan" && ft.qdev == ft.qdev) tags->push_back("nan_before_the_last_frame_qdev_finite");
  if (ft.qdev != ft.qdev) tags->push_back("qdev_nan_cull_off");
  else if (!(ft.qdev < 0.25)) tags->push_back("qdev_quarter_cull_off");
  tags->push_back(p.fast ? "fast" : "exact");
  // camera
  if (in.cam.distortion == AMHIP_DIST_NONE) {
    tags->push_back(focal ? "cull_view_pyramid" : "no_cull_no_focal");
  } else if (!focal) {
    tags->push_back("no_cull_distorted_no_focal");
  } else if (!in.knobs.no_distorted_cull) {
    bounds_tags(in.cam, cache.bounds, tags);
  }
  // knobs
  if (!c.knob.empty()) tags->push_back("knob_" + c.knob);
  // layer states
  const int lazy = (in.state_angle == 3) + (in.state_index == 3) + (in.state_out == 3);
  if (lazy == 3) tags->push_back("outputs_all_lazy");
  else if (lazy > 0) tags->push_back("outputs_one_materialized");
  tags->push_back(in.state_nobs == 0 ? "nobs_initial" : in.state_nobs == 3 ? "nobs_lazy" : "nobs_written");
  tags->push_back(p.prune ? "prune" : "no_prune");
  // launch
  const size_t ntiles = (size_t)plan.launch.grid_x * plan.launch.grid_y;
  if (p.coarse) tags->push_back(in.F == 64 ? "coarse_F64" : "coarse");
  else if (in.F == 65) tags->push_back("no_coarse_F65");
  else if (!in.zrange_valid) tags->push_back("no_coarse_no_zrange");
  if (plan.launch.tile_list) tags->push_back(ntiles == 16384 ? "tile_list_16384" : "tile_list");
  else if (ntiles == 16383 && p.coarse && !p.virt_out) tags->push_back("dense_16383");
  else if (ntiles >= 16384 && p.virt_out) tags->push_back("dense_lazy_outputs");
  else if (ntiles >= 16384 && !p.coarse) tags->push_back("dense_no_coarse");
  if (p.rows % kTileI || p.cols % kOrthoTileJ) tags->push_back("partial_tile");
  if (p.i_off || p.j_off) tags->push_back("window_offset");
  if (p.colored) tags->push_back("colored");
}

// ---- the invariants of a plan ("check") ---------------------------------------------------------------
static int g_violations = 0, g_checked = 0;
static void violated(const std::string& name, const char* what) {
  std::printf("%s: %s\n", name.c_str(), what);
  ++g_violations;
}

static void check_call(const std::string& name, const Call& c, const FrameTable& ft, const OrthoPlan& plan,
                       const ViewBoundsCache& cache) {
  static_assert(sizeof(OrthoParams) == 360, "OrthoParams");
  static_assert(sizeof(FrameFast) == 2 * sizeof(FramePose), "frame table layout");
  const OrthoPlanInput& in = c.in;
  const OrthoParams& p = plan.p;
  const OrthoLaunch& l = plan.launch;
  ++g_checked;
  for (int k = 0; k < 4 && p.cull; ++k) {
    const double n = std::sqrt(p.pl[k][0] * p.pl[k][0] + p.pl[k][1] * p.pl[k][1] + p.pl[k][2] * p.pl[k][2]);
    if (!(std::fabs(n - 1.0) <= 4 * std::numeric_limits<double>::epsilon())) violated(name, "a side plane is not of unit length");
  }
  if (p.prune && !(p.cull && p.virt_nobs)) violated(name, "prune without cull and virt_nobs");
  if (p.coarse && !p.cull) violated(name, "coarse without cull");
  if (l.tile_list && !(p.coarse && !p.virt_out)) violated(name, "tile list without coarse or over lazy outputs");
  const size_t ntiles = (size_t)l.grid_x * l.grid_y;
  if (l.list_elems < ntiles + 8) violated(name, "the list buffer does not hold its header and every tile");
  if ((size_t)l.builder_grid * 256 < ntiles) violated(name, "the list builder does not reach every tile");
  if (l.list_grid == 0 || l.list_grid > 256 * 16) violated(name, "the list kernel's grid");
  if ((size_t)l.grid_x * kTileI < (size_t)p.rows || (size_t)l.grid_y * kOrthoTileJ < (size_t)p.cols)
    violated(name, "the dense grid does not cover the window");
  if (p.fast && p.distortion != AMHIP_DIST_NONE) violated(name, "fast with a distortion model");
  const double want = 1.0 + 2.0 * ft.qdev;
  if (!(p.radius_scale == want || (want != want && p.radius_scale != p.radius_scale))) violated(name, "radius_scale");
  if (!(ft.qdev < 0.25) && p.cull) violated(name, "cull with a quaternion that is no rotation");
  const bool fills = in.cam.distortion != AMHIP_DIST_NONE && in.cam.fu > 0.0 && in.cam.fv > 0.0 && !in.knobs.no_distorted_cull;
  if (cache.valid != fills) violated(name, "the camera cache is filled exactly when the distorted cull is on");
  // a second call with the warm cache plans the same
  ViewBoundsCache warm = cache;
  const OrthoPlan again = plan_ortho_call(in, ft, &warm);
  if (std::memcmp(&again.p, &p, sizeof(p)) != 0) violated(name, "a warm cache changes the plan");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string verb = argv[1];
  if (verb != "dump" && verb != "check") return 2;
  std::ifstream file(argv[2]);
  if (!file) return 2;
  std::string line;
  while (std::getline(file, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::stringstream ss(line);
    std::string kind, tok;
    ss >> kind;
    Words w;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) return 2;
      w[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const std::string name = word(w, "name", "?");
    const bool dump = verb == "dump";
    if (dump) std::printf("case %s %s\n", kind.c_str(), name.c_str());
    if (kind == "compose") {
      if (dump) compose_case(w);
    } else if (kind == "bounds") {
      amhip_camera cam;
      if (!camera_by_name(word(w, "cam", "plain"), &cam)) return 2;
      if (!dump) continue;
      const ViewBounds b = camera_view_bounds(cam);
      dump_bounds(cam, b);
      std::vector<std::string> tags;
      bounds_tags(cam, b, &tags);
      print_tags(tags);
    } else if (kind == "call") {
      Call c;
      if (!call_input(w, &c)) return 2;
      std::vector<FramePose> table(frame_table_slots(c.in.F));
      const FrameTable ft = build_frame_table(c.in.cam, c.T_G_C.data(), c.in.F, c.in.knobs.ortho_exact_fold, table.data());
      ViewBoundsCache cache;
      const OrthoPlan plan = plan_ortho_call(c.in, ft, &cache);
      if (!dump) {
        check_call(name, c, ft, plan, cache);
        continue;
      }
      dump_table(c, table, ft);
      if (cache.valid) dump_bounds(c.in.cam, cache.bounds);
      dump_plan(c, plan);
      std::vector<std::string> tags;
      call_tags(c, ft, plan, cache, &tags);
      print_tags(tags);
    } else {
      return 2;
    }
  }
  if (verb == "check") std::printf("%d violations in %d plans\n", g_violations, g_checked);
  return g_violations ? 1 : 0;
}
