// amhip_session_plan.h -- every decision of a session call that needs no device: the contexts' lazy
// layer states, what sync_in / sync_out transfer and what they may believe afterwards, and the
// arithmetic of windows, cloud slices, routing and staging.  Host-only (no HIP header): the driver
// (amhip_session.hip, amhip_api.hip) asks, enqueues what the answer says and stores what it returns;
// tests/cpp/session_plan_host_main.cc drives the same functions against a model of the truth.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace amhip {

// ---- the context's lazy layer state ---------------------------------------------------------
enum LayerState : unsigned char {
  kLayerInitial = 0,   // holds its initial value since the last reset (a reset need not touch it)
  kLayerWritten = 1,   // possibly written
  kLayerHandedOut = 2, // its device pointer was handed out (the caller may write at any time: always refilled)
  kLayerLazyInitial = 3  // logically initial, memory not filled (lazy reset: the next producer kernel fuses the fill)
};

struct LayerStep {
  LayerState state;  // the state afterwards (once the fill, if any, has been launched)
  bool fill;         // the initial value has to be written into the layer's memory first
};

inline bool layer_is_initial(LayerState s) { return s == kLayerInitial || s == kLayerLazyInitial; }

// amhip_layers_reset: an initial layer stays as it is, a written one becomes logically initial
// (eager: filled), a handed-out one is refilled and stays handed out
inline LayerStep layer_reset(LayerState s, bool eager) {
  if (layer_is_initial(s)) return {s, false};
  if (s == kLayerWritten) return eager ? LayerStep{kLayerInitial, true} : LayerStep{kLayerLazyInitial, false};
  return {kLayerHandedOut, true};
}
// the session found the initial constant in the host matrix: the same, never eager
inline LayerStep layer_set_initial(LayerState s) { return layer_reset(s, false); }
// the memory is about to be read or partially written by someone who does not know the lazy state
inline LayerStep layer_materialize(LayerState s) {
  return s == kLayerLazyInitial ? LayerStep{kLayerInitial, true} : LayerStep{s, false};
}
// a partial writer: materialized, then possibly written
inline LayerStep layer_touch(LayerState s) {
  const LayerStep m = layer_materialize(s);
  return {m.state == kLayerInitial ? kLayerWritten : m.state, m.fill};
}
// a full overwrite (upload): no need to fill first
inline LayerState layer_overwrite(LayerState s) { return s == kLayerHandedOut ? s : kLayerWritten; }
// a kernel that produces the whole layer claims it: a logically initial layer is filled by the
// kernel itself (`fill` then means FUSED: nothing is launched), any other is touched
inline LayerStep layer_claim_output(LayerState s) {
  return s == kLayerLazyInitial ? LayerStep{kLayerWritten, true} : LayerStep{layer_touch(s).state, false};
}

// ---- residency by content -----------------------------------------------------------------
struct Hash128 {
  unsigned long long a = 0, b = 0;
  bool operator==(const Hash128& o) const { return a == o.a && b == o.b; }
  bool operator!=(const Hash128& o) const { return !(*this == o); }
};

// What the session knows about one layer of one window.  `device_valid`: the device layer holds
// a matrix with content sum `device`.  It is cleared BEFORE any kernel that writes the layer is
// enqueued and set again only by sync_out, from the device's own sum: a call that fails midway
// leaves it cleared, so the retry uploads the host matrix instead of trusting a half-written
// layer.  `host`: content sum of the host matrix as this session last saw or wrote it;
// `host_known` is false while a download is in flight.
struct LayerSync {
  bool device_valid = false;
  Hash128 device;
  bool host_known = false;
  Hash128 host;
  // sync_in found (or put) the device layer in its lazily-reset initial state AND the host matrix
  // holds that constant: once a kernel has materialised the layer, sync_out downloads it without
  // waiting for its content sum (the sum then runs on a second stream beside the download)
  bool fresh_in = false;
};

struct SessionKnobs {
  bool always_copy = false;   // session_always_copy: every matrix up and down, nothing believed
  bool no_partial = false;    // session_no_partial: always the whole window
  bool serial_sums = false;   // session_serial_sums: no download beside the sums
};

// -- sync_in: host matrix -> window layer, as far as needed
enum class InAction { kHave, kLazyReset, kUpload };
struct SyncInPlan {
  InAction action;
  LayerSync before;  // to store before anything is enqueued (an upload: device_valid cleared)
  LayerSync after;   // to store once the action has been enqueued without an error
};
// host: the matrix's content sum; constant: the sum of the window's initial constant; state: the
// context's layer state now; will_write: the call that follows writes this layer on the device
inline SyncInPlan plan_sync_in(const LayerSync& st, const Hash128& host, const Hash128& constant, LayerState state,
                               bool always_copy, bool will_write) {
  SyncInPlan p;
  p.before = st;
  p.before.host = host;
  p.before.host_known = !always_copy;
  p.before.fresh_in = false;
  p.action = InAction::kUpload;
  bool fresh = false;
  if (!always_copy) {
    const bool host_is_const = host == constant;
    // (a layer in its initial state holds the constant whatever the session last summed: a reset of the
    // context behind the session's back -- amhip_layers_reset on amhip_session_context() -- is honoured)
    if (st.device_valid && st.device == host && (host_is_const || !layer_is_initial(state))) {
      p.action = InAction::kHave;  // the device holds exactly this
      fresh = host_is_const && layer_is_initial(state);
    } else if (host_is_const) {
      // (any matrix with these sums is taken for the initial constant: 2^-128)
      p.action = InAction::kLazyReset;
      fresh = layer_is_initial(layer_set_initial(state).state);
    }
  }
  if (p.action == InAction::kUpload) p.before.device_valid = false;
  p.after = p.before;
  p.after.fresh_in = fresh;
  p.after.device = host;
  // (a layer the next kernel writes is unknown until sync_out has summed it again)
  p.after.device_valid = !always_copy && !will_write;
  return p;
}

// -- sync_out: window layers -> host matrices where the device content differs from the host's.
// The dirty rectangle of the call is asked for only where it can be used ...
inline bool rect_wanted(bool dirty_ok, const SessionKnobs& k) { return dirty_ok && !k.always_copy && !k.no_partial; }
// ... and used when it lies inside the window and covers at most half of it
inline bool rect_is_partial(const int rect[4], int rows, int cols) {
  return rect[2] > 0 && rect[3] > 0 && rect[0] >= 0 && rect[1] >= 0 && rect[0] + rect[2] <= rows &&
         rect[1] + rect[3] <= cols && 2 * (size_t)rect[2] * (size_t)rect[3] <= (size_t)rows * (size_t)cols;
}
// pinned staging for the rectangle of every listed layer, in floats; 0: beyond 1 GiB, the plain way
inline size_t rect_staging_floats(size_t block, int nl) {
  return block * (size_t)nl * 4 > (1ull << 30) ? 0 : block * (size_t)nl;
}

enum class OutAction { kNone, kWindow, kRect };
struct OutLayer {          // one listed layer of a sync_out call
  int layer = 0;
  bool want = false;       // the caller handed a host matrix for it
  bool early = false;      // stage 1: downloaded beside the sums, without waiting for its own
  bool sum = false;        // stage 1: needs a device sum (else: `h` is the constant's)
  OutAction action = OutAction::kNone;  // what was enqueued for it (stage 1: early; stage 2: the rest)
  Hash128 h;               // the device layer's content sum
};

// Stage 1, before the sums: which layers download NOW -- "fresh" ones: the host holds the initial
// constant, the device layer was lazily initial when the call began and a kernel has materialised
// it since; their sums only decide what LATER calls may skip -- and which need a device sum at all.
// sync / constants / states: the window's, by layer id.  Returns: any early layer (the sums then run
// on the second stream).
inline bool plan_out_sums(OutLayer* L, int nl, const LayerSync* sync, const Hash128* constants,
                          const LayerState* states, bool partial, const SessionKnobs& k) {
  bool beside = false;
  for (int q = 0; q < nl; ++q) {
    if (!L[q].want) continue;
    const LayerSync& st = sync[L[q].layer];
    const bool initial = layer_is_initial(states[L[q].layer]);  // nothing wrote it since its (lazy) reset
    L[q].early = !k.always_copy && !partial && !k.serial_sums && st.fresh_in && st.host_known && !initial;
    L[q].sum = !k.always_copy && !initial;
    if (!k.always_copy && initial) L[q].h = constants[L[q].layer];
    beside = beside || L[q].early;
  }
  return beside;
}
// a download is about to be enqueued: until the stream has synchronised without an error the host
// matrix may be stale or half written
inline void out_copy_pending(LayerSync* st) { st->host_known = false; }

// Stage 2, after the sums (L->h) and the staging attempt (`partial` now means: rectangle AND
// staging available): records the device's own sum and decides the download of a layer that did not
// go early.  A rectangle only where the host matrix is what the device layer was BEFORE the call.
inline OutAction plan_out_layer(OutLayer* L, LayerSync* st, bool partial, bool always_copy) {
  const bool host_has_it = !always_copy && st->host_known && st->host == L->h;
  const bool host_is_before = !always_copy && st->host_known && st->host == st->device;
  st->device_valid = !always_copy;
  st->device = L->h;
  if (L->early) return L->action = OutAction::kWindow;
  if (host_has_it) return L->action = OutAction::kNone;
  out_copy_pending(st);
  return L->action = partial && host_is_before ? OutAction::kRect : OutAction::kWindow;
}
// Stage 3, after the stream has synchronised: the host matrix now holds what the device summed
inline void out_commit(const OutLayer& L, LayerSync* st, bool always_copy) {
  if (L.action == OutAction::kNone) return;
  st->host_known = !always_copy;
  st->host = L.h;
}

// ---- windows, slices, routing ---------------------------------------------------------------
struct Win {
  int i0, j0, rows, cols;
};
// n cells cut into `parts`: edges on multiples of `align` (the gather tile: 64 x 32 cells) except at
// the map border, every part at least one cell
inline void window_edges(int n, int parts, int align, std::vector<int>* e) {
  e->assign(1, 0);
  for (int k = 1; k < parts; ++k) {
    int v = (int)std::llround((double)n * k / parts / align) * align;
    v = std::min(std::max(v, e->back() + 1), n - (parts - k));
    e->push_back(v);
  }
  e->push_back(n);
}
// window k = a + b * tiles_i
inline Win window_of(const std::vector<int>& edges_i, const std::vector<int>& edges_j, int k) {
  const int ti = (int)edges_i.size() - 1, a = k % ti, b = k / ti;
  return {edges_i[a], edges_j[b], edges_i[a + 1] - edges_i[a], edges_j[b + 1] - edges_j[b]};
}
// dsm.cc:127-144: the largest squared radius of the ladder -> metres a window grows by
inline double halo_margin_m(int radius_sq, double res) {
  double tmax = (double)radius_sq, lambda = 1.0;
  for (;;) {
    tmax = std::max(tmax, lambda * radius_sq);
    lambda *= 1.1;
    if (lambda * radius_sq > 7.0) break;
  }
  return std::sqrt(tmax) + res;
}
// slice k of an n-point cloud (uploaded to window k's device): [slice_lo(k), slice_lo(k + 1))
inline size_t slice_lo(size_t n, int k, int W) { return n * (size_t)k / (size_t)W; }

constexpr unsigned long long kMaxCallPoints = 0x7FFFFFFFull;  // (the reference indexes results with int)
// counts[k * W + d]: points of slice k that window d needs.  Slice k's selections for window d land
// behind those for windows < d in ONE buffer of sel[k] rows; window d collects total[d] points.
struct RouteTable {
  std::vector<unsigned long long> offs;  // [W][W]
  std::vector<size_t> sel, total;        // [W]
  bool refused(int d) const { return total[d] >= kMaxCallPoints; }
};
inline RouteTable route_table(const std::vector<long long>& counts, int W) {
  RouteTable t;
  t.offs.assign((size_t)W * W, 0ull);
  t.sel.assign(W, 0);
  t.total.assign(W, 0);
  for (int k = 0; k < W; ++k)
    for (int d = 0; d < W; ++d) {
      const size_t c = (size_t)counts[(size_t)k * W + d];
      t.offs[(size_t)k * W + d] = t.sel[k];
      t.sel[k] += c;
      t.total[d] += c;
    }
  return t;
}

}  // namespace amhip
