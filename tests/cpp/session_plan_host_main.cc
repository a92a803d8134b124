// session_plan_host_main.cc -- the pure half of a session call (aerial_mapper_amd/csrc/amhip_session_plan.h) as a
// stand-alone program.  tests/test_session_plan_host.py builds it with g++, once plain and once with
// -fsanitize=address,undefined, and runs it as a child process.
//
//   session_plan_host_main dump <case file>   the arithmetic of windows, halo margin, slices, routing, rectangle
//                                             and staging, and the layer-state transitions, as text
//   session_plan_host_main model <length>     every sequence of <length> events driven through plan_sync_in, the
//                                             three sync_out stages and the layer-state transitions against a
//                                             model of the truth; one line per violation, exit status 1 if any,
//                                             or if one of the plan's actions was never reached
//
// Case lines (tests/golden/session_plan/cases.txt):
//   edges ROWS COLS TILES_I TILES_J      halo RADIUS_SQ RESOLUTION      slices N W
//   route W c00 c01 .. (W * W counts, slice-major)      rect I0 J0 ROWS COLS WIN_ROWS WIN_COLS
//   staging BLOCK LAYERS                 states
//
// The model.  One window, three layers: R is read by the call, A and B are written (B may come out unchanged, like
// num_observations).  A content is a pair of ids (outside, inside the dirty rectangle); its sum IS the pair, the
// initial constant's is (1, 1).  The host holds a content per matrix, the device one per layer; every new content
// takes fresh ids, so nothing is ever equal by accident.  A rectangle download replaces only the inside id: onto
// a matrix that was not the device's content before the call it leaves a pair the device never held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "amhip_session_plan.h"

using namespace amhip;

// ---- dump -----------------------------------------------------------------------------------
static int dump(const char* path) {
  std::ifstream in(path);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream ss(line);
    std::string verb;
    ss >> verb;
    std::printf("%s\n", line.c_str());
    if (verb == "edges") {
      int rows, cols, ti, tj;
      ss >> rows >> cols >> ti >> tj;
      std::vector<int> ei, ej;
      window_edges(rows, ti, 64, &ei);
      window_edges(cols, tj, 32, &ej);
      std::printf("  edges_i");
      for (int v : ei) std::printf(" %d", v);
      std::printf("\n  edges_j");
      for (int v : ej) std::printf(" %d", v);
      std::printf("\n");
      for (int k = 0; k < ti * tj; ++k) {
        const Win w = window_of(ei, ej, k);
        std::printf("  window %d: %d %d %d %d\n", k, w.i0, w.j0, w.rows, w.cols);
      }
    } else if (verb == "halo") {
      int r2;
      double res;
      ss >> r2 >> res;
      std::printf("  margin %.17g\n", halo_margin_m(r2, res));
    } else if (verb == "slices") {
      unsigned long long n;
      int W;
      ss >> n >> W;
      std::printf("  lo");
      for (int k = 0; k <= W; ++k) std::printf(" %zu", slice_lo((size_t)n, k, W));
      std::printf("\n");
    } else if (verb == "route") {
      int W;
      ss >> W;
      std::vector<long long> counts((size_t)W * W);
      for (long long& c : counts) ss >> c;
      const RouteTable t = route_table(counts, W);
      for (int k = 0; k < W; ++k) {
        std::printf("  slice %d: selected %zu offsets", k, t.sel[k]);
        for (int d = 0; d < W; ++d) std::printf(" %llu", t.offs[(size_t)k * W + d]);
        std::printf("\n");
      }
      std::printf("  totals");
      for (int d = 0; d < W; ++d) std::printf(" %zu%s", t.total[d], t.refused(d) ? "(refused)" : "");
      std::printf("\n");
    } else if (verb == "rect") {
      int r[4], rows, cols;
      ss >> r[0] >> r[1] >> r[2] >> r[3] >> rows >> cols;
      std::printf("  partial %d\n", rect_is_partial(r, rows, cols) ? 1 : 0);
    } else if (verb == "staging") {
      unsigned long long block;
      int nl;
      ss >> block >> nl;
      std::printf("  floats %zu\n", rect_staging_floats((size_t)block, nl));
    } else if (verb == "states") {
      for (int v = 0; v < 4; ++v) {
        const LayerState s = (LayerState)v;
        const LayerStep lazy = layer_reset(s, false), eager = layer_reset(s, true), mat = layer_materialize(s),
                        touch = layer_touch(s), init = layer_set_initial(s), claim = layer_claim_output(s);
        std::printf("  state %d: initial %d reset %d/%d eager_reset %d/%d materialize %d/%d touch %d/%d overwrite %d "
                    "set_initial %d/%d claim %d/fused%d\n",
                    v, layer_is_initial(s) ? 1 : 0, lazy.state, lazy.fill, eager.state, eager.fill, mat.state, mat.fill,
                    touch.state, touch.fill, layer_overwrite(s), init.state, init.fill, claim.state, claim.fill);
      }
    } else {
      std::fprintf(stderr, "unknown case: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}

// ---- model ----------------------------------------------------------------------------------
struct Content {
  unsigned out, in;
  bool operator==(const Content& o) const { return out == o.out && in == o.in; }
};
static const Content kConst = {1, 1};
static Hash128 sum_of(const Content& c) {
  Hash128 h;
  h.a = c.out;
  h.b = c.in;
  return h;
}

enum { R = 0, A = 1, B = 2, NL = 3 };

struct World {
  Content host[NL], host_prev[NL], dev[NL];
  LayerState state[NL];
  LayerSync sync[NL];
  bool always_copy;
  unsigned next_id;
  Content fresh() {
    const unsigned v = next_id++;
    return {v, v};
  }
  void set_host(int l, const Content& c) {
    if (c == host[l]) return;
    host_prev[l] = host[l];
    host[l] = c;
  }
};

enum FailAt { kNoFail, kIn0, kIn1, kIn2, kAfter0, kAfter1, kAfter2, kKernel, kPending };
struct Event {
  const char* name;
  int kind;        // 0 edit, 1 call, 2 layers_reset, 3 always_copy
  int layer, how;  // edit: which matrix; 0 new content, 1 the constant, 2 the content it held before
  bool rect, b_changes, staging;
  FailAt fail;
  bool on;
};
static std::vector<Event> g_events;
static bool g_reached[7];
static const char* const kReachName[7] = {"in_have", "in_lazy_reset", "in_upload", "out_none", "out_window", "out_rect",
                                          "out_early"};
static unsigned long long g_violations = 0, g_sequences = 0;
static std::vector<int> g_seq;

static void violation(const char* what, int layer) {
  if (++g_violations > 20) return;
  std::printf("violation: %s (layer %c) after", what, "RAB"[layer]);
  for (int e : g_seq) std::printf(" [%s]", g_events[e].name);
  std::printf("\n");
}
#define EXPECT(cond, what, layer) \
  do {                            \
    if (!(cond)) violation(what, layer); \
  } while (0)

// sync_in of layer l as the driver does it; fail: the enqueue fails (what `before` says is all that was stored)
static InAction model_sync_in(World& w, int l, bool fail) {
  const SyncInPlan p = plan_sync_in(w.sync[l], sum_of(w.host[l]), sum_of(kConst), w.state[l], w.always_copy, l != R);
  w.sync[l] = p.before;
  g_reached[p.action == InAction::kHave ? 0 : p.action == InAction::kLazyReset ? 1 : 2] = true;
  if (p.action == InAction::kUpload) EXPECT(!w.sync[l].device_valid, "device_valid set while an upload is enqueued", l);
  if (fail) {
    if (p.action == InAction::kUpload) w.dev[l] = w.fresh();  // (part of the matrix may have arrived)
    return p.action;
  }
  if (p.action == InAction::kLazyReset) {
    w.state[l] = layer_set_initial(w.state[l]).state;
    w.dev[l] = kConst;
  } else if (p.action == InAction::kUpload) {
    w.state[l] = layer_overwrite(w.state[l]);
    w.dev[l] = w.host[l];
  }
  w.sync[l] = p.after;
  return p.action;
}

// true: the call returned without an error
static bool model_call(World& w, const Event& ev) {
  for (int l = 0; l < NL; ++l) {
    const bool fail = ev.fail == (FailAt)(kIn0 + l);
    model_sync_in(w, l, fail);
    if (fail || ev.fail == (FailAt)(kAfter0 + l)) return false;
  }
  // ---- the kernel is enqueued
  Content before[NL];
  for (int l = 0; l < NL; ++l) {
    EXPECT(w.dev[l] == w.host[l], "(a) the kernel does not see the host matrix's content", l);
    before[l] = w.dev[l];
  }
  EXPECT(!w.sync[A].device_valid && !w.sync[B].device_valid, "(d) device_valid set in front of a writing kernel", A);
  w.state[R] = layer_materialize(w.state[R]).state;
  // (a producer that fills a logically initial layer writes every cell: no rectangle)
  const bool fused = w.state[A] == kLayerLazyInitial || w.state[B] == kLayerLazyInitial;
  const bool rect = ev.rect && !fused;
  for (int l = A; l <= B; ++l) {
    w.state[l] = layer_claim_output(w.state[l]).state;
    if (l == B && !ev.b_changes) continue;
    const Content c = w.fresh();
    w.dev[l] = rect ? Content{w.dev[l].out, c.in} : c;
  }
  if (ev.fail == kKernel) {  // (the kernels fault: nobody knows what the layers hold)
    w.dev[A] = w.fresh();
    w.dev[B] = w.fresh();
    return false;
  }
  // ---- sync_out
  SessionKnobs knobs;
  knobs.always_copy = w.always_copy;
  bool partial = rect_wanted(true, knobs) && rect;
  OutLayer L[2];
  Hash128 consts[NL] = {sum_of(kConst), sum_of(kConst), sum_of(kConst)};
  for (int q = 0; q < 2; ++q) {
    L[q].layer = A + q;
    L[q].want = true;
  }
  plan_out_sums(L, 2, w.sync, consts, w.state, partial, knobs);
  for (int q = 0; q < 2; ++q) {
    const int l = L[q].layer;
    if (L[q].early) {
      g_reached[6] = true;
      out_copy_pending(&w.sync[l]);
    }
    if (L[q].sum) L[q].h = sum_of(w.dev[l]);
    EXPECT(w.always_copy || L[q].sum || w.dev[l] == kConst, "the constant's sum taken for a layer that was written", l);
  }
  partial = partial && ev.staging && rect_staging_floats(16, 2) != 0;
  for (int q = 0; q < 2; ++q) {
    const int l = L[q].layer;
    const OutAction act = plan_out_layer(&L[q], &w.sync[l], partial, w.always_copy);
    g_reached[act == OutAction::kNone ? 3 : act == OutAction::kWindow ? 4 : 5] = true;
    EXPECT(w.sync[l].device_valid == !w.always_copy, "(d) device_valid after the device's own sum", l);
    EXPECT(w.always_copy || w.sync[l].device == sum_of(w.dev[l]), "(d) the recorded device sum is not the layer's", l);
    if (act != OutAction::kNone) EXPECT(!w.sync[l].host_known, "(c) host_known while a download is pending", l);
    if (act == OutAction::kRect) EXPECT(w.host[l] == before[l], "(e) a rectangle onto a matrix that was not the device's", l);
  }
  if (ev.fail == kPending) {  // (a copy fails: the matrices being written hold anything)
    for (int q = 0; q < 2; ++q)
      if (L[q].action != OutAction::kNone) w.set_host(L[q].layer, w.fresh());
    return false;
  }
  for (int q = 0; q < 2; ++q) {
    const int l = L[q].layer;
    if (L[q].action == OutAction::kWindow) w.set_host(l, w.dev[l]);
    if (L[q].action == OutAction::kRect) w.set_host(l, Content{w.host[l].out, w.dev[l].in});
    if (L[q].action != OutAction::kNone) EXPECT(!w.sync[l].host_known, "(c) host_known before the commit", l);
    out_commit(L[q], &w.sync[l], w.always_copy);
    EXPECT(w.host[l] == w.dev[l], "(b) the host matrix does not hold the device layer", l);
    EXPECT(w.always_copy || (w.sync[l].host_known && w.sync[l].host == sum_of(w.host[l])),
           "the host sum on record is not the matrix's", l);
  }
  return true;
}

static void apply(World& w, const Event& ev) {
  if (ev.kind == 0) {
    w.set_host(ev.layer, ev.how == 0 ? w.fresh() : ev.how == 1 ? kConst : w.host_prev[ev.layer]);
  } else if (ev.kind == 2) {
    for (int l = 0; l < NL; ++l) {
      const LayerStep s = layer_reset(w.state[l], false);
      w.state[l] = s.state;
      w.dev[l] = kConst;
      EXPECT(layer_is_initial(s.state), "a reset layer is not initial", l);
    }
  } else if (ev.kind == 3) {
    w.always_copy = ev.on;  // (amhip_session_set_always_copy)
    for (LayerSync& st : w.sync) st.device_valid = st.host_known = false;
  } else {
    Content entry[NL];
    for (int l = 0; l < NL; ++l) entry[l] = w.host[l];
    if (model_call(w, ev)) return;
    // (f) the host puts its matrices back and calls again: the device must be given every one it lost
    World again = w;
    for (int l = 0; l < NL; ++l) again.host[l] = entry[l];
    for (int l = 0; l < NL; ++l) {
      const bool lost = !(again.dev[l] == again.host[l]);
      const InAction act = model_sync_in(again, l, false);
      if (lost) EXPECT(act != InAction::kHave, "(f) a layer the failed call wrote is not uploaded by the retry", l);
      EXPECT(again.dev[l] == again.host[l], "(f) the retry's kernel does not see the restored matrix", l);
    }
  }
}

static void walk(const World& w, int left) {
  if (left == 0) {
    ++g_sequences;
    return;
  }
  for (size_t e = 0; e < g_events.size(); ++e) {
    World next = w;
    g_seq.push_back((int)e);
    apply(next, g_events[e]);
    walk(next, left - 1);
    g_seq.pop_back();
  }
}

static int model(int length) {
  static const char* const edit_names[NL][3] = {{"edit R: new", "edit R: constant", "edit R: earlier"},
                                                {"edit A: new", "edit A: constant", "edit A: earlier"},
                                                {"edit B: new", "edit B: constant", "edit B: earlier"}};
  for (int l = 0; l < NL; ++l)
    for (int how = 0; how < 3; ++how) g_events.push_back({edit_names[l][how], 0, l, how, false, false, true, kNoFail, false});
  g_events.push_back({"call", 1, 0, 0, false, true, true, kNoFail, false});
  g_events.push_back({"call, B unchanged", 1, 0, 0, false, false, true, kNoFail, false});
  g_events.push_back({"call, rectangle", 1, 0, 0, true, true, true, kNoFail, false});
  g_events.push_back({"call, rectangle, B unchanged", 1, 0, 0, true, false, true, kNoFail, false});
  g_events.push_back({"call, rectangle, no staging", 1, 0, 0, true, true, false, kNoFail, false});
  static const char* const fail_names[] = {"", "call fails in sync_in R", "call fails in sync_in A",
                                           "call fails in sync_in B", "call fails after sync_in R",
                                           "call fails after sync_in A", "call fails after sync_in B",
                                           "call fails behind the kernel", "call fails with downloads pending"};
  for (int f = kIn0; f <= kPending; ++f) g_events.push_back({fail_names[f], 1, 0, 0, false, true, true, (FailAt)f, false});
  g_events.push_back({"rectangle call fails with downloads pending", 1, 0, 0, true, true, true, kPending, false});
  g_events.push_back({"layers_reset", 2, 0, 0, false, false, true, kNoFail, false});
  g_events.push_back({"always_copy on", 3, 0, 0, false, false, true, kNoFail, true});
  g_events.push_back({"always_copy off", 3, 0, 0, false, false, true, kNoFail, false});

  World w;
  std::memset(static_cast<void*>(&w), 0, sizeof(w));
  for (int l = 0; l < NL; ++l) {
    w.host[l] = w.host_prev[l] = w.dev[l] = kConst;  // (a fresh session over a fresh map ...)
    w.state[l] = kLayerLazyInitial;                  // (... whose context was reset at creation)
    w.sync[l] = LayerSync();
  }
  w.next_id = 2;
  walk(w, length);
  int missing = 0;
  for (int k = 0; k < 7; ++k)
    if (!g_reached[k]) {
      std::printf("never reached: %s\n", kReachName[k]);
      ++missing;
    }
  std::printf("%llu violations in %llu sequences of %d out of %zu events\n", g_violations, g_sequences, length,
              g_events.size());
  return g_violations || missing ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "dump") == 0) return dump(argv[2]);
  if (argc == 3 && std::strcmp(argv[1], "model") == 0) return model(std::atoi(argv[2]));
  std::fprintf(stderr, "usage: %s dump <case file> | model <length>\n", argv[0]);
  return 2;
}
