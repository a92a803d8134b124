// sort_plan_host_main.cc -- the host-side planner of a dsm_sort call (aerial_mapper_amd/csrc/
// amhip_sort_plan.h: plan_sort_call) as a stand-alone program.  tests/test_sort_plan_host.py builds it
// with g++, once plain and once with -fsanitize=address,undefined, and runs it as a child process.
//
//   sort_plan_host_main dump <case file>    every field of every case's plan as text, plus a line of
//                                           branch tags (which branches of the planner the case took)
//   sort_plan_host_main check <case file>   the invariants of the workspace layout, the LDS images and the
//                                           placement policy; one line per violation, exit status 1 if any
//
// A case is one line of key=value words behind the word `sort` (tests/golden/sort_plan/cases.txt): the
// plan_dsm input in the words of tests/golden/dsm_plan/cases.txt, then the sort call's own:
//   split=0|1|2 nprefix=N    no tiled call / its phase 1 / its phase 2, and the rows in front of the exchange
//   values=1 windowed=1      the call carries values; the context is a window of a tiling
//   one_level=1 runs=0 rcap=N reread=1 nls=1     the five tuning knobs
//   sig=match|stale hostword=0|1 big=N           what the previous call left for the launch policy
// The tags are derived here from the inputs and the results, not by instrumenting the planner.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "amhip_sort_plan.h"

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

// (the grammar of dsm_plan_host_main.cc's `plan` cases)
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

static SortPlanInput sort_input(const Words& w, const DsmPlanInput& in, const DsmParams& p) {
  SortPlanInput s = {};
  s.n = in.num_points;
  s.split_phase = (int)num(w, "split", 0);
  s.split_present = s.split_phase != 0;
  s.split_n_prefix = (size_t)big(w, "nprefix", s.n);
  s.has_values = num(w, "values", 0) != 0;
  s.windowed = num(w, "windowed", 0) != 0;
  s.sort_one_level = num(w, "one_level", 0) != 0;
  s.sort_runs = num(w, "runs", 1) != 0;
  s.p3_rounds_cap = (int)num(w, "rcap", 0);
  s.p3_rounds_reread = num(w, "reread", 0) != 0;
  s.no_launch_skips = num(w, "nls", 0) != 0;
  s.prev_sig = word(w, "sig", "stale") == "match" ? sort_geometry_signature(p) : 12345ull;
  s.have_host_stats = num(w, "hostword", 1) != 0;
  s.prev_big_count = (unsigned)num(w, "big", 0);
  return s;
}

static const char* pipeline_name(SortPipeline k) {
  switch (k) {
    case kSortOneLevel: return "one_level";
    case kSortHaloOnly: return "halo_only";
    case kSortCountDoubles: return "count_doubles";
    case kSortCountRecords: return "count_records";
    case kSortRuns: return "runs";
  }
  return "?";
}
static const char* refusal_name(RunsRefusal r) {
  switch (r) {
    case kRunsTaken: return "taken";
    case kRunsNotThreePass: return "not_three_pass";
    case kRunsRefusedRecords: return "records";
    case kRunsRefusedSplit: return "split";
    case kRunsRefusedWindowed: return "windowed";
    case kRunsRefusedPoints: return "points";
    case kRunsRefusedN1: return "n1";
    case kRunsRefusedN2: return "n2";
    case kRunsRefusedWidth: return "width";
    case kRunsRefusedKnob: return "knob";
  }
  return "?";
}

static void dump_plan(const DsmParams& p, const SortPlan& s) {
  std::printf("nbx=%d nby=%d fx_ok=%d p3_r1=%d p3_c=%d p3_w=%d p3_n1=%d p3_n2=%d p3_cap=%d\n", p.nbx, p.nby, p.fx_ok,
              p.p3_r1, p.p3_c, p.p3_w, p.p3_n1, p.p3_n2, p.p3_cap);
  std::printf("pipeline=%s runs=%s reported=%d rec=%d phase=%d nbins=%zu n_a=%zu\n", pipeline_name(s.pipeline),
              refusal_name(s.runs_refusal), s.reported, (int)s.rec, s.phase, s.nbins, s.n_a);
  std::printf("grids g_a=%zu g_b=%zu gcount=%zu g1=%zu g2=%zu nblocks_scan=%zu grid_pts=%zu scan2=%zu reduce=%zu "
              "range_parts=%zu zref_parts=%zu chunk=%u\n", s.g_a, s.g_b, s.gcount, s.g1, s.g2, s.nblocks_scan,
              s.grid_pts, s.grid_scan2, s.grid_reduce, s.range_parts, s.zref_parts, s.chunk);
  const SortCaps& c = s.cap;
  std::printf("caps sorted=%zu bin_start=%zu tmp_points=%zu rec16=%zu sidx=%zu zref=%zu rec_a=%zu rec_b=%zu zall=%zu "
              "bin_z=%zu rank=%zu scan_partials=%zu zpart=%zu stripe_ws=%zu\n", c.sorted, c.bin_start, c.tmp_points,
              c.rec16, c.sidx, c.zref, c.rec_a, c.rec_b, c.zall, c.bin_z, c.rank, c.scan_partials, c.zpart,
              c.stripe_ws);
  const SortWs& w = s.ws;
  std::printf("ws hist_rows=%zu cnt=%zu start2=%zu cursor2=%zu start1=%zu cursor1=%zu blk2=%zu big_list=%zu tot1=%zu "
              "run1=%zu pre1=%zu seg1=%zu run2=%zu pre2=%zu r1s=%zu p1s=%zu ws_words=%zu\n", w.hist_rows, w.cnt,
              w.start2, w.cursor2, w.start1, w.cursor1, w.blk2, w.big_list, w.tot1, w.run1, w.pre1, w.seg1, w.run2,
              w.pre2, w.r1s, w.p1s, w.ws_words);
  const PlacePolicy& q = s.place;
  std::printf("place geo_sig=%llu want_big=%d skip_lo=%u skip_hi=%u cap_rounds=%d rounds_above=%u reg_max=%u\n",
              q.geo_sig, (int)q.want_big, q.skip_lo, q.skip_hi, q.cap_rounds, q.rounds_above, q.reg_max);
  std::printf("lds count=%zu count_halo=%zu scatter=%zu place=%zu place_big=%zu\n", s.lds_count, s.lds_count_halo,
              s.lds_scatter, s.lds_place, s.lds_place_big);
}

// cap_rounds before the knob: what fits a CU next to the rounds' tables
static int default_cap_rounds(const DsmParams& p, const SortPlan& s) {
  const size_t tables = (4 * (size_t)p.p3_w + 64) * 4 + (s.pipeline == kSortRuns ? 2 * (size_t)kPlaceRunsCache * 4 : 0);
  return (int)std::min<size_t>(kP3BigCap, (kLdsMaxBytes - tables) / (s.rec ? 20 : 24));
}

// which branches of plan_sort_call the case took
static void sort_tags(const SortPlanInput& in, const DsmParams& p, const SortPlan& s, std::vector<std::string>* tags) {
  tags->push_back(pipeline_name(s.pipeline));
  if (s.pipeline == kSortOneLevel) {
    tags->push_back(p.p3_n1 > 0 ? "one_level_by_knob" : "one_level_by_size");
    tags->push_back(s.rec ? "one_level_records" : "one_level_doubles");
  }
  if (s.runs_refusal != kRunsTaken && s.runs_refusal != kRunsNotThreePass)
    tags->push_back(std::string("refused_") + refusal_name(s.runs_refusal));
  if (in.split_present && in.split_phase == 1) tags->push_back("split_phase1");
  if (in.split_present && in.split_phase == 2 && s.phase == 2)
    tags->push_back(s.g_b ? "split_phase2_second_part" : "split_phase2_no_second_part");
  if (in.split_present && in.split_phase == 2 && s.phase == 0) tags->push_back("split_dropped_one_level");
  if (in.has_values) tags->push_back("with_values");
  const bool places = (s.pipeline == kSortRuns || s.pipeline == kSortCountDoubles || s.pipeline == kSortCountRecords) &&
                      s.phase != 1;
  if (places) {
    if (s.rec) tags->push_back("want_big_records");
    else if (!s.place.want_big) tags->push_back("want_big_false");
    else if (in.prev_sig != s.place.geo_sig) tags->push_back("want_big_stale_signature");
    else if (!in.have_host_stats) tags->push_back("want_big_no_host_word");
    else if (in.prev_big_count != 0u) tags->push_back("want_big_count");
    else if (in.no_launch_skips) tags->push_back("want_big_no_launch_skips");
    const int dflt = default_cap_rounds(p, s);
    if (in.p3_rounds_cap != 0) {
      if (in.p3_rounds_cap < 16) tags->push_back("rounds_knob_below_16");
      else if (in.p3_rounds_cap >= dflt) tags->push_back("rounds_knob_at_default");
      else tags->push_back("rounds_knob_applied");
    }
    if (in.p3_rounds_reread) tags->push_back("rounds_reread");
  }
  if (s.pipeline == kSortCountDoubles || s.pipeline == kSortCountRecords) {
    if (s.g_a == 1) tags->push_back("count_grid_floor");
    if (s.g_a == 256) tags->push_back("count_grid_ceiling");
  }
  if (s.pipeline == kSortRuns && s.grid_scan2 == 2048) tags->push_back("scan2_grid_ceiling");
}

static int g_violations = 0, g_checked = 0;
static void check_case(const std::string& name, const DsmParams& p, const SortPlanInput& in, const SortPlan& s);

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
    if (kind != "sort") return 2;
    Words w;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) return 2;
      w[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const std::string name = word(w, "name", "?");
    const DsmPlanInput din = plan_input(w);
    DsmParams p;
    const char* why = "";
    if (plan_dsm(din, &p, &why)) return 3;  // (a sort is planned for a call that has a plan)
    const SortPlanInput in = sort_input(w, din, p);
    const SortPlan s = plan_sort_call(in, p);
    if (verb == "check") {
      check_case(name, p, in, s);
      continue;
    }
    std::printf("case sort %s\n", name.c_str());
    dump_plan(p, s);
    std::vector<std::string> tags;
    sort_tags(in, p, s, &tags);
    std::printf("tags");
    for (const std::string& t : tags) std::printf(" %s", t.c_str());
    std::printf("\n");
  }
  if (verb == "check") std::printf("%d violations in %d plans\n", g_violations, g_checked);
  return g_violations ? 1 : 0;
}

static void violated(const std::string& name, const std::string& what) {
  std::printf("%s: %s\n", name.c_str(), what.c_str());
  ++g_violations;
}

// What each kernel of amhip_sort.hip carves out of its dynamic LDS, spelled out here a second time from
// the kernels' own lines (word offsets, in their order); `end` must agree with the header's *_carved and
// lie inside the image the host asks for.
static size_t carve_scatter() {   // p3_scatter_body
  const size_t s_dest = 6 * (size_t)kP3Chunk, s_cnt = s_dest + kP3Chunk, s_off = s_cnt + kP3MaxKeys,
               s_base = s_off + kP3MaxKeys, s_scan = s_base + kP3MaxKeys;
  return (s_scan + 24) * 4;
}
static size_t carve_scatter_rec() {   // k_dsm_p3_scatter_rec
  const size_t s_dest = (size_t)kRecWords * kRecChunk, s_cnt = s_dest + kRecChunk, s_off = s_cnt + kP3MaxKeys,
               s_base = s_off + kP3MaxKeys, s_scan = s_base + kP3MaxKeys;
  return (s_scan + 24) * 4;
}
static size_t carve_place(int cap, int w, bool bin_z, bool runs) {   // place_subpartition
  const size_t s_bins = 6 * (size_t)cap, s_scan = s_bins + w, s_zlo = s_scan + 24, s_zhi = s_zlo + w;
  const size_t s_cache = s_scan + 24 + (bin_z ? 2 * (size_t)w : 0);
  const size_t tables_end = bin_z ? s_zhi + w : s_scan + 24;
  return std::max(tables_end, runs ? s_cache + 2 * (size_t)kPlaceRunsCache : 0) * 4;
}
static size_t carve_place_rec(int cap, int w) {   // place_records
  const size_t s_bins = (size_t)kRecWords * cap, s_scan = s_bins + w, s_zlo = s_scan + 24, s_zhi = s_zlo + w;
  return (s_zhi + w) * 4;
}
static size_t carve_rounds(int cap, int w, bool rec, bool runs) {   // place_rounds
  const size_t s_bins = (size_t)(rec ? 5 : 6) * cap, s_cur = s_bins + w + 1, s_scan = s_cur + w, s_zlo = s_scan + 24,
               s_zhi = s_zlo + w, s_cache = s_zhi + w;
  return (s_cache + (runs ? 2 * (size_t)kPlaceRunsCache : 0)) * 4;
}

static void check_image(const std::string& name, const char* which, size_t carved_here, size_t carved_header,
                        size_t asked) {
  if (carved_here != carved_header) violated(name, std::string(which) + ": the header's carve is not the kernel's");
  if (carved_here > asked) violated(name, std::string(which) + ": the kernel's last region ends behind the image");
  if (asked > kLdsMaxBytes) violated(name, std::string(which) + ": image above kLdsMaxBytes");
}

static void check_case(const std::string& name, const DsmParams& p, const SortPlanInput& in, const SortPlan& s) {
  ++g_checked;
  const bool three_pass = s.pipeline == kSortCountDoubles || s.pipeline == kSortCountRecords || s.pipeline == kSortRuns;
  const bool runs = s.pipeline == kSortRuns;
  if ((s.reported == AMHIP_SORT_ONE_LEVEL) != !three_pass || (s.reported == AMHIP_SORT_RUNS) != runs)
    violated(name, "reported pipeline");
  if (runs != (s.runs_refusal == kRunsTaken)) violated(name, "runs without kRunsTaken");
  if (!three_pass) {
    if (s.cap.stripe_ws || s.ws.ws_words || s.lds_scatter || s.lds_place) violated(name, "a plan for launches not made");
    if (s.pipeline == kSortOneLevel && s.range_parts != s.grid_pts * 4) violated(name, "range_parts (one level)");
    if (s.pipeline == kSortOneLevel && (s.grid_pts < 1 || s.grid_pts > 4096)) violated(name, "grid_pts");
    return;
  }
  const int n1 = p.p3_n1, n2 = p.p3_n2, nk = n1 * n2;
  // ---- stripe_ws: regions disjoint, in order, inside ws_words
  {
    const SortWs& w = s.ws;
    const size_t rows2 = (s.g1 + (size_t)n1) * (size_t)n2;
    struct { const char* name; size_t at, words; } r[] = {
        {"hist_rows", w.hist_rows, runs ? 0 : s.gcount * (size_t)nk}, {"cnt", w.cnt, (size_t)nk},
        {"start2", w.start2, (size_t)nk + 1}, {"cursor2", w.cursor2, (size_t)nk}, {"start1", w.start1, (size_t)n1 + 1},
        {"cursor1", w.cursor1, (size_t)n1}, {"blk2", w.blk2, (size_t)n1 + 1}, {"big_list", w.big_list, (size_t)nk + 1},
        {"tot1", w.tot1, (size_t)n1}, {"run1", w.run1, (size_t)n1 * w.r1s}, {"pre1", w.pre1, (size_t)n1 * w.p1s},
        {"seg1", w.seg1, (size_t)n1 * w.p1s}, {"run2", w.run2, rows2}, {"pre2", w.pre2, rows2}};
    const int count = runs ? 14 : 8;
    size_t end = 0;
    for (int k = 0; k < count; ++k) {
      if (r[k].at < end) violated(name, std::string("stripe_ws: ") + r[k].name + " overlaps the region in front of it");
      if (k >= 8 && r[k].at % 4) violated(name, std::string("stripe_ws: ") + r[k].name + " is not in whole quads");
      end = r[k].at + r[k].words;
    }
    if (end > w.ws_words) violated(name, "stripe_ws: the last region ends behind ws_words");
    if (s.cap.stripe_ws != w.ws_words) violated(name, "stripe_ws: capacity is not ws_words");
    if (runs && (w.r1s < s.g1 || w.r1s % 4 || w.p1s < s.g1 + 1)) violated(name, "stripe_ws: run table strides");
  }
  // ---- the count pass
  if (!runs) {
    check_image(name, "count", (size_t)nk * 4, lds_count_bytes(nk, false), s.lds_count);
    check_image(name, "count + halo", lds_count_halo_offset(nk) + kHaloStageBytes, lds_count_bytes(nk, true),
                s.lds_count_halo);
    if (lds_count_halo_offset(nk) < (size_t)nk * 4 || lds_count_halo_offset(nk) % 8)
      violated(name, "count + halo: HaloStage overlaps the histogram or is not 8-byte aligned");
    if (s.g_a < 1 || s.g_a > 256 || s.g_b > 256 || s.gcount != s.g_a + s.g_b) violated(name, "count grids");
  }
  if (s.phase == 1) {
    if (s.range_parts || s.lds_scatter || s.lds_place || s.cap.bin_z) violated(name, "phase 1 plans behind the count pass");
    return;
  }
  // ---- scatter
  if (s.rec) check_image(name, "record scatter", carve_scatter_rec(), lds_scatter_rec_carved(), s.lds_scatter);
  else check_image(name, "scatter", carve_scatter(), lds_scatter_carved(), s.lds_scatter);
  if (2 * (size_t)kRunsCache * 4 > (size_t)kP3Chunk * 24) violated(name, "the run table does not fit the points' image");
  if (s.range_parts != s.g1 * (kP3Threads / 64)) violated(name, "range_parts is not the first scatter's waves");
  if (s.g1 != (in.n + s.chunk - 1) / s.chunk || s.g2 != s.g1 + n1) violated(name, "scatter grids");
  // ---- placement
  const PlacePolicy& q = s.place;
  if (q.cap_rounds < 16) violated(name, "cap_rounds below 16");
  if (q.geo_sig != sort_geometry_signature(p)) violated(name, "geo_sig");
  size_t big_a, big_b;  // the big launch's two users: one image of kP3BigCap points, the rounds' image
  if (s.rec) {
    check_image(name, "record placement", carve_place_rec(p.p3_cap, p.p3_w), lds_place_rec_carved(p.p3_cap, p.p3_w),
                s.lds_place);
    big_a = lds_place_rec_bytes(kP3BigCap, p.p3_w);
    big_b = lds_rounds_bytes(q.cap_rounds, p.p3_w, true, false);
    check_image(name, "big record placement", carve_place_rec(kP3BigCap, p.p3_w), lds_place_rec_carved(kP3BigCap, p.p3_w),
                big_a);
    check_image(name, "record rounds", carve_rounds(q.cap_rounds, p.p3_w, true, false),
                (size_t)q.cap_rounds * 20 + lds_rounds_tables_carved(p.p3_w, false), big_b);
  } else {
    check_image(name, "placement", carve_place(p.p3_cap, p.p3_w, false, runs), lds_place_carved(p.p3_cap, p.p3_w, false, runs),
                s.lds_place);
    big_a = lds_place_bytes(kP3BigCap, p.p3_w, false, runs);
    big_b = lds_rounds_bytes(q.cap_rounds, p.p3_w, false, runs);
    check_image(name, "big placement", carve_place(kP3BigCap, p.p3_w, false, runs),
                lds_place_carved(kP3BigCap, p.p3_w, false, runs), big_a);
    check_image(name, "rounds", carve_rounds(q.cap_rounds, p.p3_w, false, runs),
                (size_t)q.cap_rounds * 24 + lds_rounds_tables_carved(p.p3_w, runs), big_b);
    // (with bin ranges, which no doubles pipeline asks for today: the carve still ends inside its image)
    if (carve_place(p.p3_cap, p.p3_w, true, runs) != lds_place_carved(p.p3_cap, p.p3_w, true, runs) ||
        carve_place(p.p3_cap, p.p3_w, true, runs) > lds_place_bytes(p.p3_cap, p.p3_w, true, runs))
      violated(name, "placement with bin ranges");
  }
  if (s.lds_place_big != std::max(big_a, big_b)) violated(name, "lds_place_big is not the larger of its two users");
  // every sub-partition size goes to exactly one of the two launches: the small one leaves (skip_lo, skip_hi],
  // the big one walks the list of those above p3_cap -- when it is launched
  for (int want = 0; want < 2; ++want) {
    unsigned lo, hi;
    place_skips(want != 0, p.p3_cap, &lo, &hi);
    if (want == (int)q.want_big && (lo != q.skip_lo || hi != q.skip_hi)) violated(name, "skip words");
    const unsigned sizes[] = {0u, 1u, (unsigned)p.p3_cap - 1, (unsigned)p.p3_cap, (unsigned)p.p3_cap + 1, (unsigned)kP3BigCap,
                              (unsigned)kP3BigCap + 1, 0x7FFFFFFFu, 0xFFFFFFFFu};
    for (const unsigned size : sizes) {
      const bool small_takes = !(size > lo && size <= hi);
      const bool big_takes = want && size > (unsigned)p.p3_cap;
      if (small_takes == big_takes) violated(name, "a sub-partition size taken by both placement launches or by none");
    }
  }
  if (s.rec && !q.want_big) violated(name, "the record pipeline always launches the big placement");
}
