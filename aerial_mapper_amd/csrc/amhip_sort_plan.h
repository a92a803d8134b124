// amhip_sort_plan.h -- what the host decides about one dsm_sort call before anything is launched: which of
// the sort's pipelines runs (and why the run pipeline does not), every grid, the element count of every
// buffer, where each table lies in the stripe_ws workspace, the launch policy of the placement pair and the
// bytes of every dynamic-LDS image (plan_sort_call).  Pure functions of their arguments: no HIP, no context,
// no tuning store -- tests/cpp/sort_plan_host_main.cc compiles this header alone.
#ifndef AMHIP_SORT_PLAN_H_
#define AMHIP_SORT_PLAN_H_

#include "amhip_dsm_plan.h"

namespace amhip {

// ---------------------------------------------------------------------------
// compile-time shape of the sort's kernels (amhip_sort.hip)
// ---------------------------------------------------------------------------
constexpr int kP3CountThreads = 1024;
#ifndef AMHIP_P3_THREADS
#define AMHIP_P3_THREADS 512
#endif
#ifndef AMHIP_P3_PER
#define AMHIP_P3_PER 5
#endif
constexpr int kP3Threads = AMHIP_P3_THREADS;
constexpr int kP3Chunk = AMHIP_P3_THREADS * AMHIP_P3_PER;  // points staged per scatter workgroup (2560: 70 KB of LDS, 2 per CU)
constexpr int kP3MaxKeys = 256;
constexpr int kP3PlaceThreads = 256;
// (kP3PlaceMaxCap, the LDS capacity the register-resident placement handles: amhip_dsm_plan.h, plan_sort)
constexpr int kP3PlacePer = kP3PlaceMaxCap / kP3PlaceThreads;
constexpr int kP3BigThreads = 1024;
constexpr int kP3BigPer = 6;
constexpr int kP3BigCap = kP3BigThreads * kP3BigPer;  // 6144 points = 147 KB of LDS
constexpr int kRecWords = 5;  // 20-byte sort records of the single-precision mode
constexpr int kRecPerThread = 6;
constexpr int kRecChunk = kP3Threads * kRecPerThread;
// points a thread of the big placement kernel keeps in registers across the rounds of a
// sub-partition beyond one LDS image (place_rounds): 14 x 24 bytes / 16 x 20 bytes
constexpr int kP3RoundsPer = 14;
constexpr int kP3RoundsPerRec = 16;
constexpr int kRunsCache = 2048;      // runs of a pass-2 segment kept in LDS (more: searched in memory)
constexpr int kPlaceRunsCache = 512;  // run-list rows of a sub-partition kept in LDS by the placement
constexpr size_t kLdsMaxBytes = 160 * 1024 - 512;  // per workgroup on gfx950 (160 KB per CU), a margin kept
constexpr int kScanT = 256;
constexpr int kScanI = 16;
constexpr int kScanE = kScanT * kScanI;
constexpr int kOneLevelThreads = 256;             // k_dsm_bin_count / k_dsm_scatter
constexpr size_t kOneLevelMaxGrid = 256 * 16;
constexpr size_t kCountPointsPerGroup = 8192;     // of a count workgroup, before the grid's floor and ceiling
constexpr size_t kCountMaxGrid = 256;
constexpr size_t kScan2MaxGrid = 2048;
constexpr size_t kRunsMaxPoints = (size_t)1 << 27;   // rows the run tables address with room to spare
constexpr int kRunsMaxWidth = 2048;                  // bins of a column block next to the run lists' 4 KB
constexpr size_t kHaloStageBytes = 16744;            // sizeof(HaloStage) (amhip_sort.hip asserts it)

// ---------------------------------------------------------------------------
// the dynamic-LDS images, in bytes.  Beside each: what its kernel carves, in order, in 32-bit words
// ---------------------------------------------------------------------------
constexpr size_t kWord = sizeof(uint32_t);
constexpr int kLdsSortScanWords = 24;       // block-scan scratch: the last region of every image but the count's
constexpr int kLdsSortScanPadWords = 8;     // padding: the host asks for 32 words where the kernels address 24
constexpr int kLdsRoundsFixedWords = 25;    // place_rounds: the total behind the bin starts + the scan scratch
constexpr int kLdsRoundsPadWords = 39;      // padding: the host asks for 64 words where place_rounds addresses 25
constexpr int kLdsPointBytesDoubles = 24, kLdsPointBytesRecord = kRecWords * 4;

// scatter_pass / k_dsm_p3_scatter, k_dsm_runs_sort1/2:  points 6 * kP3Chunk | dest kP3Chunk | cnt, off, base
// kP3MaxKeys each | scan 24   (the run pipeline's run table, 2 * kRunsCache words, lies in the points)
constexpr size_t lds_scatter_carved() { return ((size_t)kP3Chunk * 7 + 3 * kP3MaxKeys + kLdsSortScanWords) * kWord; }
constexpr size_t lds_scatter_bytes() { return lds_scatter_carved() + kLdsSortScanPadWords * kWord; }
// k_dsm_p3_scatter_rec:  records kRecWords * kRecChunk | dest kRecChunk | cnt, off, base | scan 24
constexpr size_t lds_scatter_rec_carved() {
  return ((size_t)kRecChunk * (kRecWords + 1) + 3 * kP3MaxKeys + kLdsSortScanWords) * kWord;
}
constexpr size_t lds_scatter_rec_bytes() { return lds_scatter_rec_carved() + kLdsSortScanPadWords * kWord; }
// k_dsm_p3_count:  histogram nk   (selecting the halo: histogram nk rounded up to even | HaloStage)
constexpr size_t lds_count_halo_offset(int nk) { return (size_t)((nk + 1) & ~1) * kWord; }
constexpr size_t lds_count_bytes(int nk, bool halo) {
  return halo ? lds_count_halo_offset(nk) + kHaloStageBytes : (size_t)nk * kWord;
}
// place_subpartition:  points 6 * cap | bins w | scan 24 | [zlo w | zhi w] | [run cache 2 * kPlaceRunsCache]
constexpr size_t lds_run_cache_bytes(bool runs) { return runs ? 2 * (size_t)kPlaceRunsCache * kWord : 0; }
constexpr size_t lds_place_carved(int cap, int w, bool bin_z, bool runs) {
  return (size_t)cap * kLdsPointBytesDoubles + ((size_t)w + kLdsSortScanWords + (bin_z ? 2 * (size_t)w : 0)) * kWord +
         lds_run_cache_bytes(runs);
}
constexpr size_t lds_place_bytes(int cap, int w, bool bin_z, bool runs) {
  return lds_place_carved(cap, w, bin_z, runs) + kLdsSortScanPadWords * kWord;
}
// place_records:  records kRecWords * cap | bins w | scan 24 | zlo w | zhi w
constexpr size_t lds_place_rec_carved(int cap, int w) {
  return (size_t)cap * kLdsPointBytesRecord + (3 * (size_t)w + kLdsSortScanWords) * kWord;
}
constexpr size_t lds_place_rec_bytes(int cap, int w) { return lds_place_rec_carved(cap, w) + kLdsSortScanPadWords * kWord; }
// place_rounds:  points (5 | 6) * cap | bin starts w + 1 | cursors w | scan 24 | zlo w | zhi w | [run cache]
constexpr size_t lds_rounds_tables_carved(int w, bool runs) {
  return (4 * (size_t)w + kLdsRoundsFixedWords) * kWord + lds_run_cache_bytes(runs);
}
constexpr size_t lds_rounds_tables_bytes(int w, bool runs) {
  return lds_rounds_tables_carved(w, runs) + kLdsRoundsPadWords * kWord;
}
constexpr size_t lds_rounds_point_bytes(bool rec) { return rec ? kLdsPointBytesRecord : kLdsPointBytesDoubles; }
constexpr size_t lds_rounds_bytes(int cap, int w, bool rec, bool runs) {
  return (size_t)cap * lds_rounds_point_bytes(rec) + lds_rounds_tables_bytes(w, runs);
}
static_assert(2 * kRunsCache * kWord <= (size_t)kP3Chunk * kLdsPointBytesDoubles, "the run table lies in the points' image");

// ---------------------------------------------------------------------------
// plan_sort_call
// ---------------------------------------------------------------------------
enum SortPipeline : int {
  kSortOneLevel = 0,   // one-level counting sort (clouds below the partition sort's threshold)
  kSortHaloOnly,       // phase 1 of a small tiled call: the halo selection in a pass of its own, nothing sorted
  kSortCountDoubles,   // count -> two scatter passes -> placement, on doubles
  kSortCountRecords,   // the same on 20-byte records (the single-precision gather's mode)
  kSortRuns,           // local sorts, runs gathered: no count pass
};
// The run pipeline serves the doubles of a whole, untiled context.  Why a three-pass call keeps the counting
// pipeline: the first of these that holds
enum RunsRefusal : int {
  kRunsTaken = 0,
  kRunsNotThreePass,      // (not asked: the call is no three-pass sort)
  kRunsRefusedRecords,    // the records' zref has to exist before the first is written
  kRunsRefusedSplit,      // tiled call: the halo selection rides on the count pass
  kRunsRefusedWindowed,   // ... and so it does in every window of a tiling
  kRunsRefusedPoints,     // the rows do not fit the run tables' 32-bit addresses with room to spare
  kRunsRefusedN1,
  kRunsRefusedN2,
  kRunsRefusedWidth,      // the run lists' 4 KB of LDS have to fit next to the big placement's image
  kRunsRefusedKnob,       // tuning key sort_runs=0
};

// Everything the plan of a sort call depends on besides the DsmParams.  The tuning values and the previous
// call's placement evidence are a snapshot taken by the caller.
struct SortPlanInput {
  size_t n;
  bool split_present;      // tiled call (SortSplit)
  int split_phase;
  size_t split_n_prefix;
  bool has_values, windowed;
  bool sort_one_level, sort_runs;   // tuning knobs
  int p3_rounds_cap;                // tuning knob (tests): sub-partitions above it are placed in rounds over an image
                                    // of that many points; ignored below 16 or at / above what fits a CU anyway
  bool p3_rounds_reread;            // tuning knob: the rounds re-read the sub-partition, nothing kept in registers
  bool no_launch_skips;             // tuning knob (tests, A-B): the big placement is launched whatever the evidence
  unsigned long long prev_sig;      // geometry signature the pinned word describes
  bool have_host_stats;             // there is a pinned word
  unsigned prev_big_count;          // sub-partitions the previous call left to the big placement kernel
};

// element counts handed to ensure_capacity (0: this pipeline does not ask)
struct SortCaps {
  size_t sorted, bin_start, tmp_points, rec16, sidx, zref, rec_a, rec_b, zall, bin_z, rank, scan_partials, zpart,
      stripe_ws;
};
// stripe_ws, as word offsets: [hist_rows: one histogram row per count workgroup] (counting pipelines), then
// the plan block every three-pass pipeline has, then the run tables (run pipeline)
struct SortWs {
  size_t hist_rows;   // gcount * nk
  size_t cnt;         // nk
  size_t start2;      // nk + 1
  size_t cursor2;     // nk
  size_t start1;      // n1 + 1
  size_t cursor1;     // n1
  size_t blk2;        // n1 + 1
  size_t big_list;    // [count] + up to nk sub-partition ids
  size_t tot1;        // n1, from here on in whole quads
  size_t run1, pre1, seg1;   // n1 rows of r1s / p1s / p1s words
  size_t run2, pre2;         // (g1 + n1) * n2 words each
  size_t r1s, p1s;
  size_t ws_words;
};
constexpr size_t up4(size_t w) { return (w + 3) & ~(size_t)3; }
constexpr size_t kWsPlanPadWords = 64;  // behind the plan block (which ends 3 * n1 + 4 words into 4 * n1 + 64)
constexpr size_t kWsRunsPadWords = 16;  // behind the run tables
inline SortWs sort_workspace(bool runs, size_t gcount, int n1, int n2, size_t g1) {
  SortWs w = {};
  const size_t nk = (size_t)n1 * (size_t)n2;
  w.hist_rows = 0;
  w.cnt = runs ? 0 : gcount * nk;
  w.start2 = w.cnt + nk;
  w.cursor2 = w.start2 + nk + 1;
  w.start1 = w.cursor2 + nk;
  w.cursor1 = w.start1 + n1 + 1;
  w.blk2 = w.cursor1 + n1;
  w.big_list = w.blk2 + n1 + 1;
  const size_t plan_end = w.cnt + 4 * nk + 4 * (size_t)n1 + kWsPlanPadWords;
  if (!runs) {
    w.ws_words = plan_end;
    return w;
  }
  const size_t rows2 = (g1 + (size_t)n1) * (size_t)n2;   // pass 2 has at most g1 + n1 segments
  w.r1s = up4(g1);
  w.p1s = w.r1s + 4;
  w.tot1 = up4(plan_end);
  w.run1 = w.tot1 + up4((size_t)n1);
  w.pre1 = w.run1 + (size_t)n1 * w.r1s;
  w.seg1 = w.pre1 + (size_t)n1 * w.p1s;
  w.run2 = w.seg1 + (size_t)n1 * w.p1s;
  w.pre2 = w.run2 + up4(rows2);
  w.ws_words = w.pre2 + up4(rows2) + kWsRunsPadWords;
  return w;
}

// what a call's pinned launch-policy counters are counters OF: the window's geometry and the sort's plan
inline unsigned long long sort_geometry_signature(const DsmParams& p) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](const void* v, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(v);
    for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  };
  const int ints[] = {p.rows, p.cols, p.M, p.B, p.nbx, p.nby, p.i_off, p.j_off, p.p3_r1, p.p3_c,
                      p.p3_w, p.p3_n1, p.p3_n2, p.p3_cap};
  const double dbls[] = {p.base_x, p.base_y, p.res, p.inv_res, p.sub_x, p.sub_y};
  mix(ints, sizeof(ints));
  mix(dbls, sizeof(dbls));
  return h ? h : 1ull;
}

// The launch policy of the placement pair.  Sub-partitions beyond the placement workgroup's registers (denser
// parts of a non-uniform cloud) are the big kernel's.  On doubles its launch is skipped when the PREVIOUS
// three-pass call of this geometry had none (the scan leaves their number in a pinned word, never waited
// for): the small kernel then keeps nothing back and places a stray over-full sub-partition itself, directly
// (slower, same result) -- the word it leaves brings the big kernel back next call.  The record pipeline
// always launches both.  The small launch leaves (skip_lo, skip_hi] to the big one, whose list holds the
// sub-partitions above p3_cap.
struct PlacePolicy {
  unsigned long long geo_sig;
  bool want_big;
  unsigned skip_lo, skip_hi;
  // sub-partitions beyond one image: rounds over an image of cap_rounds points next to the rounds' tables
  // (place_rounds), their points kept in registers up to reg_max
  int cap_rounds;
  unsigned rounds_above, reg_max;
};
inline void place_skips(bool want_big, int p3_cap, unsigned* skip_lo, unsigned* skip_hi) {
  *skip_lo = want_big ? (unsigned)p3_cap : 0xFFFFFFFFu;
  *skip_hi = 0xFFFFFFFFu;
}
inline PlacePolicy plan_placement(const SortPlanInput& in, const DsmParams& p, bool rec, bool runs) {
  PlacePolicy q = {};
  q.geo_sig = sort_geometry_signature(p);
  q.want_big = rec || !(in.prev_sig == q.geo_sig && in.have_host_stats && in.prev_big_count == 0u) ||
               in.no_launch_skips;
  place_skips(q.want_big, p.p3_cap, &q.skip_lo, &q.skip_hi);
  q.cap_rounds = (int)std::min<size_t>(kP3BigCap, (kLdsMaxBytes - lds_rounds_tables_bytes(p.p3_w, runs)) /
                                                      lds_rounds_point_bytes(rec));
  q.rounds_above = kP3BigCap;
  q.reg_max = 0xFFFFFFFFu;
  if (in.p3_rounds_cap >= 16 && in.p3_rounds_cap < q.cap_rounds) {
    q.cap_rounds = in.p3_rounds_cap;
    q.rounds_above = (unsigned)in.p3_rounds_cap;
  }
  if (in.p3_rounds_reread) q.reg_max = 0u;
  return q;
}

struct SortPlan {
  SortPipeline pipeline;
  RunsRefusal runs_refusal;
  int reported;    // AMHIP_SORT_* (amhip_ctx_dsm_sort_pipeline); ONE_LEVEL also for kSortHaloOnly
  bool rec;        // the record pipeline (the single-precision gather's mode): 16-byte records + rows + zref
  int phase;       // of a tiled three-pass call (1: stops behind the count pass; 2), else 0
  size_t nbins, n_a;   // n_a: rows counted by the first count launch
  // grids
  size_t g_a, g_b, gcount;    // count launches in front of / behind a tiled call's exchange
  size_t g1, g2;              // first scatter (chunks of `chunk` points), second scatter (g1 + n1)
  size_t nblocks_scan, grid_pts;   // one-level sort
  size_t grid_scan2, grid_reduce;  // k_dsm_runs_scan2, k_dsm_p3_reduce_scan
  size_t range_parts;         // height partials the first scatter's waves leave in zpart
  size_t zref_parts;          // height partials k_dsm_zref folds (records)
  unsigned chunk;
  SortCaps cap;
  SortWs ws;
  PlacePolicy place;
  // dynamic LDS
  size_t lds_count, lds_count_halo, lds_scatter, lds_place, lds_place_big;
};

constexpr size_t count_grid(size_t len) {
  return std::min<size_t>(std::max<size_t>((len + kCountPointsPerGroup - 1) / kCountPointsPerGroup, 1), kCountMaxGrid);
}

inline RunsRefusal runs_refusal(const SortPlanInput& in, const DsmParams& p, bool rec, bool split) {
  if (rec) return kRunsRefusedRecords;
  if (split) return kRunsRefusedSplit;
  if (in.windowed) return kRunsRefusedWindowed;
  if (in.n > kRunsMaxPoints) return kRunsRefusedPoints;
  if (p.p3_n1 > kP3MaxKeys) return kRunsRefusedN1;
  if (p.p3_n2 > kP3MaxKeys) return kRunsRefusedN2;
  if (p.p3_w > kRunsMaxWidth) return kRunsRefusedWidth;
  if (!in.sort_runs) return kRunsRefusedKnob;
  return kRunsTaken;
}

inline SortPlan plan_sort_call(const SortPlanInput& in, const DsmParams& p) {
  SortPlan s = {};
  const size_t n = in.n;
  // ---- every pipeline
  s.nbins = (size_t)p.nbx * (size_t)p.nby;
  s.nblocks_scan = (s.nbins + kScanE - 1) / kScanE;
  s.rec = p.fx_ok && !p.pcl_mode && !in.has_values;
  s.place.geo_sig = sort_geometry_signature(p);
  // ([min z, max z] of the binned points: every wave of the first scatter pass leaves a partial)
  s.cap.zpart = 2 * (8 * std::max<size_t>((n + 2047) / 2048 + 1, kOneLevelMaxGrid)) + 16;
  s.cap.sorted = 3 * n;
  s.cap.bin_start = s.nbins + 4;
  if (s.rec) {
    s.cap.rec16 = 4 * n + 16;
    s.cap.sidx = n + 16;
    s.cap.zref = 8;
  }
  s.reported = AMHIP_SORT_ONE_LEVEL;
  s.runs_refusal = kRunsNotThreePass;
  const bool three_pass = p.p3_n1 > 0 && !in.sort_one_level;
  if (!three_pass) {
    if (in.split_present && in.split_phase == 1) {  // small clouds: selection in a pass of its own
      s.pipeline = kSortHaloOnly;
      return s;
    }
    // ---- one-level counting sort (a tiled call's phase 2 is an ordinary call here)
    s.pipeline = kSortOneLevel;
    s.grid_pts = std::min((n + kOneLevelThreads - 1) / kOneLevelThreads, kOneLevelMaxGrid);
    s.range_parts = s.grid_pts * (kOneLevelThreads / 64);
    s.cap.rank = n;
    s.cap.scan_partials = s.nblocks_scan + 4;
    if (s.rec) {
      s.zref_parts = s.grid_pts * (kOneLevelThreads / 64);
      s.cap.zall = 2 * s.zref_parts + 16;
    }
    return s;
  }
  // ---- three-pass partition sort
  const int n1 = p.p3_n1, n2 = p.p3_n2, nk = n1 * n2;
  const bool split = in.split_present;
  s.phase = split ? in.split_phase : 0;
  // (tiled call: the prefix is counted -- and its halo selected -- before the caller's exchange, the received
  // rows after it; each part writes its own histogram rows)
  s.n_a = split ? in.split_n_prefix : n;
  s.g_a = count_grid(s.n_a);
  s.g_b = n > s.n_a ? count_grid(n - s.n_a) : 0;
  s.gcount = s.g_a + s.g_b;
  s.runs_refusal = runs_refusal(in, p, s.rec, split);
  const bool runs = s.runs_refusal == kRunsTaken;
  s.reported = runs ? AMHIP_SORT_RUNS : AMHIP_SORT_COUNT;
  s.pipeline = runs ? kSortRuns : s.rec ? kSortCountRecords : kSortCountDoubles;
  const size_t chunk = s.rec ? kRecChunk : kP3Chunk;
  const size_t g1 = (n + chunk - 1) / chunk;
  s.ws = sort_workspace(runs, s.gcount, n1, n2, g1);
  s.cap.stripe_ws = s.ws.ws_words;
  if (s.rec) {
    s.cap.rec_a = s.cap.rec_b = (size_t)kRecWords * n + 16;
    s.cap.zall = 2 * s.gcount * (kP3CountThreads / 64) + 16;
  } else {
    s.cap.tmp_points = 3 * n;
  }
  if (!runs) {
    s.lds_count = lds_count_bytes(nk, false);
    s.lds_count_halo = lds_count_bytes(nk, true);
    if (s.phase == 1) return s;  // (the second phase comes back for the rest)
    // (the records' reference height: the middle of the range every count workgroup left -- in a tiled call
    // both parts', the second of which may be absent: its rows hold the first call's partials or the
    // initial "empty" pairs)
    if (s.rec) s.zref_parts = (split && !s.g_b ? s.g_a : s.gcount) * (size_t)(kP3CountThreads / 64);
    s.grid_reduce = ((size_t)nk + 63) / 64;
  } else {
    s.grid_scan2 = std::min(((size_t)nk + 15) / 16, kScan2MaxGrid);
  }
  s.chunk = (unsigned)chunk;
  s.g1 = g1;
  s.g2 = g1 + n1;
  s.range_parts = g1 * (kP3Threads / 64);
  s.lds_scatter = s.rec ? lds_scatter_rec_bytes() : lds_scatter_bytes();
  s.place = plan_placement(in, p, s.rec, runs);
  if (s.rec) {
    s.cap.bin_z = 2 * (s.nbins + 4);
    s.lds_place = lds_place_rec_bytes(p.p3_cap, p.p3_w);
    s.lds_place_big = std::max(lds_place_rec_bytes(kP3BigCap, p.p3_w),
                               lds_rounds_bytes(s.place.cap_rounds, p.p3_w, true, false));
  } else {
    s.lds_place = lds_place_bytes(p.p3_cap, p.p3_w, false, runs);
    s.lds_place_big = std::max(lds_place_bytes(kP3BigCap, p.p3_w, false, runs),
                               lds_rounds_bytes(s.place.cap_rounds, p.p3_w, false, runs));
  }
  return s;
}

}  // namespace amhip

#endif  // AMHIP_SORT_PLAN_H_
