// dsm_plan_host_main.cc -- the host-side planner of a DSM call (aerial_mapper_amd/csrc/
// amhip_dsm_plan.h: plan_dsm, plan_gather_classes, rough_policy_step) as a stand-alone program.
// tests/test_dsm_plan_host.py builds it with g++, once plain and once with
// -fsanitize=address,undefined, and runs it as a child process.
//
//   dsm_plan_host_main dump <case file>    every field of every case's plan as text, plus a line of
//                                          branch tags (which branches of the planner the case took)
//   dsm_plan_host_main check <case file>   the invariants of the LDS image and the class caps; one
//                                          line per violation, exit status 1 if there is any
//
// A case is one line of key=value words behind its kind (tests/golden/dsm_plan/cases.txt):
//   plan    one plan_dsm call; with cls=1 also plan_gather_classes on its result
//   policy  a sequence of calls through rough_policy_step
// The tags are derived here from the inputs and the results, not by instrumenting the planner.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "amhip_dsm_plan.h"

using namespace amhip;

typedef std::map<std::string, std::string> Words;

static double num(const Words& w, const char* key, double dflt) {
  const auto it = w.find(key);
  return it == w.end() ? dflt : std::strtod(it->second.c_str(), nullptr);
}
static unsigned long long big(const Words& w, const char* key, unsigned long long dflt) {
  const auto it = w.find(key);
  return it == w.end() ? dflt : std::strtoull(it->second.c_str(), nullptr, 10);
}
static std::string word(const Words& w, const char* key, const char* dflt) {
  const auto it = w.find(key);
  return it == w.end() ? dflt : it->second;
}

static DsmPlanInput plan_input(const Words& w) {
  DsmPlanInput in = {};
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
  in.radius_sq = (int)num(w, "r2", 1);
  in.center_easting = num(w, "ce", 3.0);
  in.center_northing = num(w, "cn", -4.0);
  in.mode = (int)num(w, "mode", 0);
  in.pcl_lambda = (int)num(w, "lambda", 1);
  in.num_points = (size_t)big(w, "n", 1000);
  in.dsm_exact = (int)num(w, "exact", 0);
  in.dsm_exact_now = (int)num(w, "exact_now", 0);
  in.dsm_knn = (int)num(w, "knn", 0);
  in.canon_all = (int)num(w, "canon", 0);
  in.p3_min_points = (size_t)big(w, "p3min", 1u << 20);
  in.p3_target = num(w, "p3target", 1536.0);
  in.p3_cap = (int)num(w, "p3cap", 2048);
  in.knn_global_bins = (int)num(w, "knn_global", 0);
  return in;
}

template <class T>
static void dump_ints(const char* name, const T* v, int n) {
  while (n > 0 && v[n - 1] == 0) --n;  // (the rest is zero)
  std::printf("%s=[", name);
  for (int k = 0; k < n; ++k) std::printf("%s%lld", k ? "," : "", (long long)v[k]);
  std::printf("]\n");
}

static void dump_params(const DsmParams& p) {
  std::printf("base_x=%.17g base_y=%.17g res=%.17g inv_res=%.17g sub_x=%.17g sub_y=%.17g\n", p.base_x, p.base_y,
              p.res, p.inv_res, p.sub_x, p.sub_y);
  std::printf("rows=%d cols=%d i_off=%d j_off=%d pcl_mode=%d only_unfilled=%d canon_all=%d knn_k=%d\n", p.rows,
              p.cols, p.i_off, p.j_off, p.pcl_mode, p.only_unfilled, p.canon_all, p.knn_k);
  std::printf("B=%d M=%d nbx=%d nby=%d nlevels=%d\n", p.B, p.M, p.nbx, p.nby, p.nlevels);
  std::printf("T=[");
  for (int k = 0; k < p.nlevels; ++k) std::printf("%s%.17g", k ? "," : "", p.T[k]);
  std::printf("]\n");
  for (int k = p.nlevels; k < kMaxLevels; ++k)
    if (p.T[k] != 0.0) std::printf("T[%d]=%.17g beyond the ladder\n", k, p.T[k]);
  dump_ints("w", p.w, kMaxLevels);
  std::printf("p3_r1=%d p3_c=%d p3_w=%d p3_n1=%d p3_n2=%d p3_cap=%d mul_B=%u mul_r1=%u mul_w=%u\n", p.p3_r1, p.p3_c,
              p.p3_w, p.p3_n1, p.p3_n2, p.p3_cap, p.mul_B, p.mul_r1, p.mul_w);
  dump_ints("wr", p.wr, 2 * kMaxW0 + 1);
  dump_ints("wr2", p.wr2, 2 * kMaxW0 + 2);
  dump_ints("wrp", p.wrp, kMaxW0 + 1);
  std::printf("lds_ok=%d lds_cap=%d lds_cells=%d tile_j=%d tiles_i=%d tiles_j=%d lds_bytes=%u lds_bytes_f32=%u\n",
              p.lds_ok, p.lds_cap, p.lds_cells, p.tile_j, p.tiles_i, p.tiles_j, p.lds_bytes, p.lds_bytes_f32);
  std::printf("fx_ok=%d fx_S=%d fx_thi=%.9g fx_tlo=%.9g fx_denmax=%.9g fx_epsw=%.9g\n", p.fx_ok, p.fx_S, p.fx_thi,
              p.fx_tlo, p.fx_denmax, p.fx_epsw);
  std::printf("out_i0=%d out_j0=%d out_pitch=%d\n", p.out_i0, p.out_j0, p.out_pitch);
}

// which branches of plan_dsm the case took
static void plan_tags(const DsmPlanInput& in, int rc, const char* why, const DsmParams& p,
                      std::vector<std::string>* tags) {
  if (rc) {
    tags->push_back(std::string(why).find("ladder") != std::string::npos ? "err_ladder" : "err_bins");
    return;
  }
  const bool retry = in.mode == 1 && in.pcl_lambda > 1;
  if (in.mode == 0) tags->push_back(p.nlevels > 2 ? "ladder_long" : "ladder_two");
  else tags->push_back(retry ? "pcl_retry" : "pcl_first");
  // tile shape
  const bool rec_rows = (long long)p.rows + 2LL * p.M <= 65535 && (long long)p.cols + 2LL * p.M <= 65535;
  const bool rec_points = in.num_points < 0xFFFFFFFFull;
  if (!rec_rows) tags->push_back("recfits_rows");
  if (!rec_points) tags->push_back("recfits_points");
  const bool single = in.mode == 0 && !in.dsm_exact && !in.dsm_exact_now && !in.dsm_knn && rec_rows && rec_points;
  const double need16 = region_need(p, 16, in.num_points);
  char shape[64];
  std::snprintf(shape, sizeof(shape), "shape_%d_%d", p.tile_j, p.lds_cap);
  if (p.lds_cap) tags->push_back(shape);  // (0: no LDS image was laid out)
  if (p.lds_cap == 2048 && p.tile_j == 16 && need16 > 2048.0) {
    if (single) tags->push_back("shape_fallback_beyond_7680");
    else if (need16 <= 7680.0) {
      if (in.dsm_exact) tags->push_back("nowide_exact");
      if (in.dsm_exact_now) tags->push_back("nowide_exact_now");
      if (in.dsm_knn) tags->push_back("nowide_knn");
    }
  }
  // lds_ok off
  if (!p.lds_ok) {
    if (p.w[0] > kMaxW0) tags->push_back("ldsoff_w0");
    else if (retry) tags->push_back("ldsoff_pcl_retry");
    else if (p.knn_k && in.knn_global_bins) tags->push_back("ldsoff_knn_global");
    else tags->push_back("ldsoff_bytes");
  }
  // sort plan
  {
    const int r1 = (p.nby + 127) / 128, cmax = 256 / r1;
    if (p.p3_n1) {
      tags->push_back("p3_on");
      if (r1 > 1) tags->push_back("p3_r1_gt1");
      const double raw = (double)in.num_points / ((double)p.nby * in.p3_target) + 0.5;
      if (raw >= (double)cmax + 1.0 && p.p3_c == cmax) tags->push_back("p3_cc_cmax");
      if (raw >= (double)p.nbx + 1.0 && cmax > p.nbx && p.p3_c == p.nbx) tags->push_back("p3_cc_nbx");
      if (in.p3_cap < 64) tags->push_back("p3_cap_lo");
      if (in.p3_cap > 2048) tags->push_back("p3_cap_hi");
    } else if (in.num_points < in.p3_min_points) {
      tags->push_back("p3_off_points");
    } else {
      tags->push_back("p3_off_geometry");
    }
  }
  if (p.mul_B == 0u) tags->push_back("mul_d1");
  if (p.mul_B == 0xFFFFFFFFu) tags->push_back("mul_escape");
  if (p.p3_n1 && p.mul_w == 0xFFFFFFFFu) tags->push_back("mul_w_escape");
  if (p.fx_ok) tags->push_back("fx_on");
}

static unsigned parse_stats(const std::string& s, unsigned* out) {
  unsigned n = 0;
  std::stringstream ss(s);
  std::string item;
  while (n < (unsigned)kListHdr && std::getline(ss, item, ',')) out[n++] = (unsigned)std::strtoul(item.c_str(), nullptr, 10);
  return n;
}

struct ClassCall {
  GatherCallFlags fl;
  size_t n;
  bool have_stats;
  unsigned stats[kListHdr];
  int64_t prev_ntiles;
  bool no_launch_skips;
  std::string sig;  // "match": the signature this very call computes; else "stale"
};

static ClassCall class_call(const Words& w, const DsmPlanInput& in) {
  ClassCall c = {};
  c.fl.fill_untouched = num(w, "fill", 0) != 0;
  c.fl.mask = num(w, "mask", 0) != 0;
  c.fl.unfilled = num(w, "unfilled", 0) != 0;
  c.fl.bin_z_valid = num(w, "binz", 0) != 0;
  c.n = in.num_points;
  const std::string stats = word(w, "stats", "");
  c.have_stats = !stats.empty();
  if (c.have_stats) parse_stats(stats, c.stats);
  c.prev_ntiles = (int64_t)num(w, "prev_ntiles", 0);
  c.no_launch_skips = num(w, "nls", 0) != 0;
  c.sig = word(w, "sig", "stale");
  return c;
}

static GatherClasses run_classes(const DsmParams& p, const ClassCall& c) {
  unsigned long long prev_sig = 12345;
  if (c.sig == "match")
    prev_sig = plan_gather_classes(p, c.n, c.fl, nullptr, 0, 0, false).sig;
  return plan_gather_classes(p, c.n, c.fl, c.have_stats ? c.stats : nullptr, c.prev_ntiles, prev_sig,
                             c.no_launch_skips);
}

static void class_tags(const DsmParams& p, const ClassCall& c, const GatherClasses& g,
                       std::vector<std::string>* tags) {
  tags->push_back(p.tile_j == 16 ? "cls_tj16" : "cls_tj32");
  tags->push_back(g.f32 ? "cls_f32" : "cls_fp64");
  if (g.cap1 == std::min(g.cap0, 2048)) tags->push_back("cls_class1_empty");
  if (g.cap0 == 4096) tags->push_back(g.rej_own ? "rej_own_4096_true" : "rej_own_4096_false");
  if (g.cap0 == 7680) tags->push_back(g.rej_own ? "rej_own_7680_true" : "rej_own_7680_false");
  const unsigned ntiles = (unsigned)p.tiles_i * (unsigned)p.tiles_j;
  const double cells = (double)p.rows * (double)p.cols;
  if (g.sparse) tags->push_back("sparse_on");
  else if (!c.fl.fill_untouched && ntiles == 8192 && (double)c.n * 16.0 < cells) tags->push_back("sparse_off_8192_tiles");
  else if (!c.fl.fill_untouched && ntiles > 8192 && (double)c.n * 16.0 == cells) tags->push_back("sparse_off_16_per_cell");
  else if (c.fl.fill_untouched && ntiles > 8192 && (double)c.n * 16.0 < cells) tags->push_back("sparse_off_fill");
  if (g.use_bin_z && g.cap0 <= 2048 && !g.sparse && c.have_stats && c.prev_ntiles > 0) {
    const double r = (double)c.stats[4] + (double)c.stats[5] + (double)c.stats[6] + (double)c.stats[7];
    if (r * 10.0 == (double)c.prev_ntiles) tags->push_back("rej_dense_at_a_tenth");
    if (g.rej_dense) tags->push_back("rej_dense_above_a_tenth");
  }
  if (!g.f32 && !g.sparse && c.have_stats) {
    const bool empty = c.stats[1] == 0 && c.stats[2] == 0 && c.stats[3] == 0;
    if (g.skip_classes) tags->push_back("skip_classes_on");
    else if (c.sig != "match") tags->push_back("skip_off_stale_signature");
    else if (!empty) tags->push_back("skip_off_counters");
    else if (c.no_launch_skips) tags->push_back("skip_off_no_launch_skips");
  }
}

static void dump_classes(const DsmParams& p, const GatherClasses& g) {
  std::printf("classes f32=%d sparse=%d use_bin_z=%d rej_own=%d rej_dense=%d skip_classes=%d\n", g.f32, g.sparse,
              g.use_bin_z, g.rej_own, g.rej_dense, g.skip_classes);
  // (capf1 / capf2: single-precision images; without them -- fx_ok 0 -- no launch reads the two)
  std::printf("cap0=%d cap1=%d cap2=%d", g.cap0, g.cap1, g.cap2);
  if (p.fx_ok) std::printf(" capf1=%d capf2=%d", g.capf1, g.capf2);
  std::printf(" ccap0=%d ccap1=%d ccap2=%d sig=%llu\n", g.ccap0, g.ccap1, g.ccap2, g.sig);
}

static void print_tags(const std::vector<std::string>& tags) {
  std::printf("tags");
  for (const std::string& t : tags) std::printf(" %s", t.c_str());
  std::printf("\n");
}

// The previous call's counters as dsm_run leaves them: a call that ran the single-precision
// pipeline leaves `rejected` tiles of `ntiles` on the FP64 lists; one that ran FP64 outright leaves
// last_call_f32 false.
static void policy_case(const Words& w) {
  const bool exact = num(w, "exact", 0) != 0, knn = num(w, "knn", 0) != 0, off = num(w, "off", 0) != 0;
  const int calls = (int)num(w, "calls", 20);
  unsigned stats[kListHdr] = {};
  stats[kListRedoOwn] = (unsigned)num(w, "rej_own", 0);
  stats[kListRedoBig] = (unsigned)num(w, "rej_big", 0);
  stats[kListRedoWaveBlock] = (unsigned)num(w, "rej_wave", 0);
  stats[kStatRedoUnlisted] = (unsigned)num(w, "rej_unlisted", 0);
  const int64_t ntiles = (int64_t)num(w, "ntiles", 100);
  const bool have_stats = num(w, "nostats", 0) == 0;
  RoughState s = {0, false, 0};
  std::vector<std::string> tags;
  bool held = false, released = false, any = false;
  std::printf("exact_now hold:");
  for (int k = 0; k < calls; ++k) {
    const int now = rough_policy_step(&s, !(exact || knn || off), have_stats ? stats : nullptr);
    std::printf(" %d/%d", now, s.hold);
    if (held && !now) released = true;
    if (now) held = any = true;
    // (what dsm_run records of this call)
    s.last_ntiles = ntiles;
    s.last_call_f32 = !now && !exact && !knn;
  }
  std::printf("\n");
  const double rejected = rejected_tiles(stats);
  if (exact) tags.push_back("policy_exact_mode");
  else if (knn) tags.push_back("policy_capped_mode");
  else if (off) tags.push_back("policy_switch_off");
  else if (!have_stats) tags.push_back("policy_no_counters");
  else if (any) tags.push_back(released ? "policy_hold_and_release" : "policy_hold");
  else tags.push_back(rejected * 2.0 == (double)ntiles ? "policy_exactly_half" : "policy_smooth");
  print_tags(tags);
}

// ---- the invariants of the LDS image and the class caps ("check") -----------------------------------
static int g_violations = 0, g_checked = 0;
static void violated(const std::string& name, const char* what) {
  std::printf("%s: %s\n", name.c_str(), what);
  ++g_violations;
}
static void check_case(const std::string& name, const Words& w);

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
    if (verb == "check") {
      if (kind == "plan") check_case(name, w);
      continue;
    }
    std::printf("case %s %s\n", kind.c_str(), name.c_str());
    if (kind == "policy") {
      policy_case(w);
      continue;
    }
    if (kind != "plan") return 2;
    const DsmPlanInput in = plan_input(w);
    DsmParams p;
    const char* why = "";
    const int rc = plan_dsm(in, &p, &why);
    std::vector<std::string> tags;
    std::printf("status=%d %s\n", rc, why);
    if (!rc) {
      p.only_unfilled = (int)num(w, "only_unfilled", 0);  // (the adaptive passes' callers set it)
      dump_params(p);
    }
    plan_tags(in, rc, why, p, &tags);
    if (!rc && num(w, "cls", 0) != 0) {
      if (!p.lds_ok) return 3;  // (dsm_run plans classes for the LDS-tiled gather only)
      const ClassCall c = class_call(w, in);
      const GatherClasses g = run_classes(p, c);
      dump_classes(p, g);
      class_tags(p, c, g, &tags);
    }
    print_tags(tags);
  }
  if (verb == "check") std::printf("%d violations in %d plans\n", g_violations, g_checked);
  return g_violations ? 1 : 0;
}

// an image of `cap` points as a launch asks for it: even cap, what the kernel carves ends inside it, it fits a CU
static void check_image(const std::string& name, const DsmParams& p, bool f32, int cap, const char* which) {
  const size_t image = lds_image_bytes(f32, cap, p.lds_cells, p.tile_j);
  const size_t carved = ((size_t)cap + kLdsSpareSlots) * lds_point_bytes(f32) + lds_table_bytes(f32, p.lds_cells, p.tile_j);
  // (FP64: the z array behind the xy array ends inside the point slots)
  const size_t z_end = ((size_t)cap + 1) * 16 + ((size_t)cap + 1) * 8;
  if (cap & 1) violated(name, (std::string(which) + ": odd cap").c_str());
  if (carved > image) violated(name, (std::string(which) + ": the kernel's tables end behind the image").c_str());
  if (!f32 && z_end > ((size_t)cap + kLdsSpareSlots) * kLdsPointBytes64)
    violated(name, (std::string(which) + ": the z array overlaps the cell table").c_str());
  if (image > 160u * 1024u) violated(name, (std::string(which) + ": image above 160 KB").c_str());
  if (image % 16) violated(name, (std::string(which) + ": image not in whole quads").c_str());
}

static void check_case(const std::string& name, const Words& w) {
  const DsmPlanInput in = plan_input(w);
  DsmParams p;
  const char* why = "";
  if (plan_dsm(in, &p, &why)) return;
  ++g_checked;
  if (p.fx_ok && !(p.lds_ok && in.mode == 0 && !in.dsm_exact && !in.dsm_exact_now && !in.dsm_knn))
    violated(name, "fx_ok outside the single-precision mode");
  if (!p.lds_ok) return;
  if ((p.lds_cells + 1) % 4) violated(name, "lds_cells + 1 is no multiple of four");
  if (p.lds_bytes != lds_image_bytes(false, p.lds_cap, p.lds_cells, p.tile_j)) violated(name, "lds_bytes");
  if (p.fx_ok && p.lds_bytes_f32 != lds_image_bytes(true, p.lds_cap, p.lds_cells, p.tile_j))
    violated(name, "lds_bytes_f32");
  if (!p.fx_ok && p.lds_bytes_f32 != 0) violated(name, "lds_bytes_f32 without fx_ok");
  p.only_unfilled = (int)num(w, "only_unfilled", 0);
  const ClassCall c = class_call(w, in);
  const GatherClasses g = run_classes(p, c);
  if (g.cap0 != p.lds_cap) violated(name, "cap0");
  if (!(std::min(g.cap0, 2048) <= g.cap1 && g.cap1 <= g.cap2)) violated(name, "cap0_64 <= cap1 <= cap2");
  if (!(g.cap0 <= g.capf1 && g.capf1 <= g.capf2)) violated(name, "cap0 <= capf1 <= capf2");
  if (g.f32 && !p.fx_ok) violated(name, "f32 without fx_ok");
  if (g.cap0 > 2048 && !p.fx_ok) violated(name, "a wide main launch outside the single-precision mode");
  // every image launch_gathers can ask for (amhip_dsm.hip)
  if (g.cap0 <= 2048 || g.rej_own) check_image(name, p, false, g.cap0, "FP64 main / redo image");
  check_image(name, p, false, std::min(class1_ceiling(p.tile_j), g.cap1), "FP64 class 1");
  check_image(name, p, false, std::min(class2_ceiling(p.tile_j), g.cap2), "FP64 class 2");
  check_image(name, p, false, g.cap2, "FP64 redo with the largest image");
  if (p.fx_ok) {
    check_image(name, p, true, g.cap0, "single-precision main");
    check_image(name, p, true, g.capf1, "single-precision class 1");
    check_image(name, p, true, g.capf2, "single-precision class 2");
  }
}
