// amhip_session.hip -- one map served through HOST matrices by one or several GPUs.
//
// The reference's host is ONE C++ process whose state is the GridMap's float matrices
// (main-dsm.cc:103-107, main-ortho-backward-grid.cc:128-141): Dsm::process and
// OrthoBackwardGrid::process read and write them.  A session is what the drop-in classes
// (aerial_mapper_amd/cpp/*.cc) share per map:
//   * windows    the map cut into tiles_i x tiles_j windows, window k on devices[k] (one
//                context each; a device may serve several windows).  A DSM call uploads a
//                slice of the cloud to every device, each selects what every window needs
//                (its cells + the halo margin, k_halo_select) and the selections travel
//                device to device (hipMemcpyPeerAsync: xGMI) -- SURVEY 8e option (i), halo
//                POINTS, inside one process; every window then runs the single-GPU kernels.
//                Frames and poses are replicated; the mosaic needs no exchange.
//   * residency  the layers stay on the devices between calls.  Whether a host matrix still
//                holds what the device holds is decided by CONTENT: two 64-bit sums of a
//                NON-LINEAR mix of (cell bits, cell position) over the matrix -- any single
//                changed cell changes both, and no arithmetic relation between two edits cancels
//                (round 2's sum was linear in the bits: d1 (2 g1 + 1) = -d2 (2 g2 + 1) went
//                unnoticed) --, computed with host threads on the way in and by a kernel on
//                the way out.  Equal -> no transfer;
//                a matrix that holds its initial constant -> a lazy device-side reset instead
//                of an upload; anything else is uploaded.  Outputs the kernels did not change
//                (num_observations: `+= itself`, ortho-backward-grid.cc:183) are not downloaded.
//                tuning knob session_always_copy: every matrix up and down, like round 1.
// What is transferred and what the session may believe afterwards is decided in
// amhip_session_plan.h; this file enqueues what the plan says and stores what it returns.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "amhip_common.h"
#include "amhip_content_sum.h"
#include "amhip_tiff_host.h"

namespace amhip {

// Where the last host-buffer call spent its time (amhip_session_last_profile; window 0's view):
// wall-clock phases on the host, HIP-event times for what the stream did.
struct CallProfile {
  double total_ms = 0, h2d_ms = 0, host_sum_ms = 0, kernel_ms = 0, dev_sum_wait_ms = 0, d2h_ms = 0;
  double up_bytes = 0, down_bytes = 0;
};

constexpr size_t kSumBytes = sizeof(unsigned long long) * 2 * AMHIP_NUM_LAYERS;

// everything of one window
struct Window {
  amhip_ctx* ctx = nullptr;
  Win win = {0, 0, 0, 0};
  int dev = 0;
  LayerSync sync[AMHIP_NUM_LAYERS];
  Hash128 const_hash[AMHIP_NUM_LAYERS];        // content sums of the initial constants
  // DSM routing (W > 1): count, then compact -- a slice's selections for all windows take
  // (points selected) rows, not (slice x windows)
  double* route_out = nullptr;
  size_t route_cap = 0;                        // doubles
  long long* route_counts = nullptr;           // device, W words
  hipEvent_t route_done = nullptr;             // this window's selections are complete
  double* cloud = nullptr;
  size_t cloud_cap = 0;                        // doubles
  unsigned long long* dev_hash = nullptr;      // device scratch: two u64 per layer
  unsigned long long* pin_hash = nullptr;      // its pinned host mirror
  float* pin = nullptr;                        // pinned host staging of partial downloads
  size_t pin_cap = 0;                          // floats
  // a second stream for the content sums that run beside a download, and the events that time a
  // call's kernels / downloads (CallProfile)
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr, ev_s1 = nullptr, ev_d1 = nullptr;
  Ctx* c() const { return &ctx->impl; }
};

struct Session {
  amhip_grid_desc grid;
  int ti = 1;
  std::vector<int> edges_i, edges_j;
  std::vector<Window> windows;
  bool always_copy = false;
  bool verify_partial = false;                 // tuning knob session_verify_partial: re-sum the host matrix
  std::atomic<unsigned long long> up_bytes{0}, down_bytes{0};  // layer traffic (amhip_session_transfer_stats)
  CallProfile prof;
  std::atomic<unsigned long long> prof_down{0};   // (the windows' threads add to it: the call's downloads)
  int W() const { return (int)windows.size(); }
};

static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// tuning knob session_trace: wall time of every phase of a call on stderr (where does a host-matrix
// call spend its time: content sums, uploads, kernels, downloads?)
struct PhaseClock {
  bool on;
  const char* call;
  std::chrono::steady_clock::time_point t0;
  explicit PhaseClock(const char* name)
      : on(tuning_on("session_trace")), call(name), t0(std::chrono::steady_clock::now()) {}
  void mark(const char* phase, hipStream_t wait_for = nullptr, bool wait = false) {
    if (!on) return;
    if (wait) (void)hipStreamSynchronize(wait_for);
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[amhip session] %s: %-28s %8.3f ms\n", call, phase,
                 std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

// ---- content sums (amhip_content_sum.h: cell_mix, host_column_sum) ----------------------
// layer == nullptr: the sums of a window filled with `constant` (no memory is read)
__global__ void __launch_bounds__(256)
k_layer_hash(const float* __restrict__ layer, float constant, int rows, int cols, int i0, int j0,
             int map_rows, unsigned long long* __restrict__ out) {
  unsigned long long a = 0, b = 0;
  const size_t n = (size_t)rows * (size_t)cols;
  const size_t stride = (size_t)gridDim.x * 256;
  const unsigned cbits = __float_as_uint(constant);
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) {
    const int i = (int)(k % (size_t)rows), j = (int)(k / (size_t)rows);
    const unsigned long long g = (unsigned long long)(i0 + i) +
                                 (unsigned long long)(j0 + j) * (unsigned long long)map_rows;
    cell_mix(layer ? __float_as_uint(layer[k]) : cbits, g, &a, &b);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a += __shfl_xor(a, d, 64);
    b += __shfl_xor(b, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, a);
    atomicAdd(out + 1, b);
  }
}

// CPUs this process may keep busy: hardware threads, capped by its affinity mask and by a cgroup
// CPU quota (cpu.max of cgroup v2, cfs_quota_us / cfs_period_us of v1).  *quota_cpus: the quota
// alone (0: none).  A GPU box's pod runs under such a quota: 256 hardware threads, 16 CPUs' worth of
// time per 100 ms (tools/ubench/host_sum_bench.cc: 128 summing threads run 12 ms at 200 GB/s,
// then the whole process is frozen until the period ends).
struct CpuBudget {
  int cpus;
  double quota;
};
static CpuBudget measure_cpu_budget() {
  int n = (int)std::thread::hardware_concurrency();
  if (n <= 0) n = 8;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
  double q = 0.0;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char a[64] = {0};
    double period = 0.0;
    if (std::fscanf(f, "%63s %lf", a, &period) == 2 && period > 0.0 && a[0] >= '0' && a[0] <= '9')
      q = std::atof(a) / period;
    std::fclose(f);
  } else {
    double qu = -1.0, period = 0.0;
    if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
      if (std::fscanf(g, "%lf", &qu) != 1) qu = -1.0;
      std::fclose(g);
    }
    if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(g, "%lf", &period) != 1) period = 0.0;
      std::fclose(g);
    }
    if (qu > 0.0 && period > 0.0) q = qu / period;
  }
  if (q > 0.0) n = std::min(n, std::max(1, (int)std::ceil(q)));
  return {n, q};
}
static int usable_cpus(double* quota_cpus) {
  static const CpuBudget b = measure_cpu_budget();  // (once per process; thread-safe initialisation)
  if (quota_cpus) *quota_cpus = b.quota;
  return b.cpus;
}

// threads for a pass of host threads over `bytes` of matrices
static int host_threads(size_t bytes) {
  if (tuning("session_threads", 0.0) > 0.0) return std::max(1, (int)tuning("session_threads", 0.0));
  unsigned hw = std::thread::hardware_concurrency();
  double quota = 0.0;
  const int cpus = usable_cpus(&quota);
  // (the AVX-512 loop sums 33 GB/s per thread on the pool's EPYCs: a few threads per memory
  // channel group saturate the host's memory, more only burn CPU time in stalls)
  if (host_sum_is_vectorized()) return std::max(1, std::min(cpus, 32));
  // (the scalar mix costs three multiplies per cell, 5 GB/s per thread: 128 threads keep the six
  // matrices of a mosaic call -- 2.4 GB at cfg3 -- near the host's memory bandwidth)
  int T = (int)std::min<unsigned>(hw ? hw : 8u, 128u);
  if (quota > 0.0 && quota < (double)T) {
    // under a CPU quota: a short pass may burst over four times the quota's CPUs (64 threads draw
    // 175 GB/s; more only burn the period's allowance in memory stalls); a pass worth more than
    // ~ 60 % of one period's allowance (100 ms x quota; a thread sums ~ 4.5 GB/s) would get the
    // process frozen mid-way: one thread per CPU of the quota, steadily.  Measured on the pool's
    // boxes (quota 16): cfg3's six matrices 75 - 82 ms per first pass whatever the burst width
    // (32 .. 128), 100 ms at 16 threads; the five 1.6 GB matrices of a 20 000^2 map 180 ms at
    // 128 threads, 150 ms at 16.
    const double cpu_seconds = (double)bytes / 4.5e9;
    T = cpu_seconds <= 0.06 * quota ? std::min(T, 4 * cpus) : cpus;
  } else {
    T = std::min(T, std::max(cpus, 1));
  }
  return std::max(1, T);
}

// per-window sums of `nl` host matrices (column-major, the map's size) with host threads
static void host_hashes(const Session& s, const float* const* mats, int nl,
                        std::vector<Hash128>* out /* [nl][W] */) {
  const int W = s.W(), R = s.grid.rows, Cc = s.grid.cols;
  out->assign((size_t)nl * W, Hash128());
  size_t bytes = 0;
  for (int l = 0; l < nl; ++l)
    if (mats[l]) bytes += (size_t)R * (size_t)Cc * 4;
  const int T = std::max(1, std::min(host_threads(bytes), Cc));
  std::vector<std::vector<Hash128>> part(T, std::vector<Hash128>((size_t)nl * W));
  auto work = [&](int t) {
    const int c0 = (int)((long long)Cc * t / T), c1 = (int)((long long)Cc * (t + 1) / T);
    std::vector<Hash128>& acc = part[t];
    int b = 0;
    for (int j = c0; j < c1; ++j) {
      while (j >= s.edges_j[b + 1]) ++b;
      for (int a = 0; a < s.ti; ++a) {
        const int k = a + b * s.ti;
        const int ia = s.edges_i[a], ib = s.edges_i[a + 1];
        const unsigned long long g0 = (unsigned long long)j * (unsigned long long)R;
        for (int l = 0; l < nl; ++l) {
          if (!mats[l]) continue;
          const unsigned* col = reinterpret_cast<const unsigned*>(mats[l]) + (size_t)j * R;
          host_column_sum(col + ia, (size_t)(ib - ia), g0 + (unsigned long long)ia,
                          &acc[(size_t)l * W + k].a, &acc[(size_t)l * W + k].b);
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  for (int t = 0; t < T; ++t)
    for (size_t q = 0; q < out->size(); ++q) {
      (*out)[q].a += part[t][q].a;
      (*out)[q].b += part[t][q].b;
    }
}

static inline float* map_at(float* base, const Session& s, const Win& w) {
  return base + (size_t)w.i0 + (size_t)w.j0 * (size_t)s.grid.rows;
}
static inline const float* map_at(const float* base, const Session& s, const Win& w) {
  return base + (size_t)w.i0 + (size_t)w.j0 * (size_t)s.grid.rows;
}

// window block <-> map-shaped host matrix (bytes: the grid_map message's payloads are not
// aligned).  A window that spans all rows of the map is ONE contiguous range of both: a plain
// copy instead of a pitched one (the runtime stages pitched copies of pageable memory row by row).
static hipError_t copy_window(void* dst_host_or_dev, const void* src, const Session& s, const Win& w,
                              bool to_host, hipStream_t stream) {
  const size_t col = (size_t)w.rows * 4;
  if (w.rows == s.grid.rows)
    return hipMemcpyAsync(dst_host_or_dev, src, col * (size_t)w.cols,
                          to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, stream);
  return to_host ? hipMemcpy2DAsync(dst_host_or_dev, (size_t)s.grid.rows * 4, src, col, col,
                                    (size_t)w.cols, hipMemcpyDeviceToHost, stream)
                 : hipMemcpy2DAsync(dst_host_or_dev, col, src, (size_t)s.grid.rows * 4, col,
                                    (size_t)w.cols, hipMemcpyHostToDevice, stream);
}

static unsigned long long window_bytes(const Win& w) {
  return (unsigned long long)w.rows * (unsigned long long)w.cols * 4ull;
}

// host matrix -> window layer, as far as needed (asynchronous on the context's stream; the caller
// has made its device current).  will_write: the call that follows writes this layer on the device.
static int sync_in(Session& s, int k, int layer, const float* host, const Hash128& host_hash,
                   bool will_write) {
  Window& x = s.windows[k];
  Ctx* c = x.c();
  LayerSync& st = x.sync[layer];
  const SyncInPlan p =
      plan_sync_in(st, host_hash, x.const_hash[layer], c->layer_state[layer], s.always_copy, will_write);
  st = p.before;
  if (p.action == InAction::kLazyReset) {
    const int rc = ctx_layer_set_initial(c, layer);
    if (rc) return rc;
  } else if (p.action == InAction::kUpload) {
    ctx_overwrite(c, layer);
    AMHIP_TRY(copy_window(c->layers[layer], map_at(host, s, x.win), s, x.win, false, c->stream));
    s.up_bytes += window_bytes(x.win);
  }
  st = p.after;
  return AMHIP_OK;
}

// columns [0, cols) of a packed rows x cols block -> the map-shaped host matrix at (i, j)
static void unpack_block(const float* packed, float* host, const Session& s, int i, int j, int rows,
                         int cols) {
  const size_t bytes = (size_t)rows * (size_t)cols * 4;
  const int T = bytes < (8u << 20) ? 1 : std::min(16, cols);
  auto work = [&](int t) {
    const int c0 = (int)((long long)cols * t / T), c1 = (int)((long long)cols * (t + 1) / T);
    for (int q = c0; q < c1; ++q)
      std::memcpy(host + (size_t)i + (size_t)(j + q) * (size_t)s.grid.rows, packed + (size_t)q * rows,
                  (size_t)rows * 4);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
}

// pinned staging of `need` floats for window x's rectangle downloads; false: none to be had
static bool ensure_pinned(Window& x, size_t need) {
  if (need == 0) return false;
  if (need <= x.pin_cap) return true;
  if (x.pin) (void)hipHostFree(x.pin);
  x.pin = nullptr;
  x.pin_cap = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&x.pin), need * 4, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    x.pin = nullptr;
    return false;
  }
  x.pin_cap = need;
  return true;
}

// the whole window of a layer -> its place in the host matrix, counted
static int download_window(Session& s, Window& x, int layer, float* host) {
  Ctx* c = x.c();
  AMHIP_TRY(copy_window(map_at(host, s, x.win), c->layers[layer], s, x.win, true, c->stream));
  s.down_bytes += window_bytes(x.win);
  s.prof_down += window_bytes(x.win);
  return AMHIP_OK;
}

// stage 1's device work: the sums of the layers that need one (on the second stream when a download
// runs beside them, ordered behind the kernels by their end event), the early downloads on the
// context's stream, and the one wait for the sums
static int run_out_sums(Session& s, Window& x, OutLayer* L, float* const* hosts, int nl, bool beside) {
  Ctx* c = x.c();
  const Win& w = x.win;
  hipStream_t hs = beside ? x.aux_stream : c->stream;
  if (beside) AMHIP_TRY(hipStreamWaitEvent(hs, x.ev_k1, 0));
  AMHIP_TRY(hipMemsetAsync(x.dev_hash, 0, kSumBytes, hs));
  for (int q = 0; q < nl; ++q)
    if (L[q].sum)
      hipLaunchKernelGGL(k_layer_hash, dim3(2048), dim3(256), 0, hs, c->layers[L[q].layer], 0.0f, w.rows,
                         w.cols, w.i0, w.j0, s.grid.rows, x.dev_hash + 2 * q);
  // (pinned: the copy must not block the host)
  AMHIP_TRY(hipMemcpyAsync(x.pin_hash, x.dev_hash, kSumBytes, hipMemcpyDeviceToHost, hs));
  // (a download into pageable memory keeps the calling thread until it is done: the sums are
  // already running on the second stream by then)
  for (int q = 0; q < nl; ++q) {
    if (!L[q].early) continue;
    out_copy_pending(&x.sync[L[q].layer]);
    const int rc = download_window(s, x, L[q].layer, hosts[q]);
    if (rc) return rc;
  }
  // (the downloads' own start, where the sums ran in front of them on the same stream)
  AMHIP_TRY(hipEventRecord(x.ev_s1, c->stream));
  AMHIP_TRY(hipStreamSynchronize(hs));
  for (int q = 0; q < nl; ++q)
    if (L[q].sum) L[q].h = {x.pin_hash[2 * q], x.pin_hash[2 * q + 1]};
  return AMHIP_OK;
}

// tuning knob session_verify_partial (tests): a matrix that took a rectangle must carry the device's sums as a whole
static int verify_rects(Session& s, int k, const OutLayer* L, float* const* hosts, int nl) {
  for (int q = 0; q < nl; ++q) {
    if (L[q].action != OutAction::kRect) continue;
    std::vector<Hash128> hv;
    const float* m[1] = {hosts[q]};
    host_hashes(s, m, 1, &hv);
    if (hv[(size_t)k] != L[q].h)
      return arg_failure("session: a partial download left the host matrix different from the device layer");
  }
  return AMHIP_OK;
}

// the call's profile: window 0's view.  sum_wait_ms: the sums' share of the wall clock, the whole
// wait when nothing was downloaded beside them
static int record_profile(Session& s, Window& x, bool beside, double sum_wait_ms) {
  AMHIP_TRY(hipEventSynchronize(x.ev_d1));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, x.ev_k0, x.ev_k1) == hipSuccess) s.prof.kernel_ms = ms;
  if (hipEventElapsedTime(&ms, beside || s.always_copy ? x.ev_k1 : x.ev_s1, x.ev_d1) == hipSuccess)
    s.prof.d2h_ms = ms;
  (void)hipGetLastError();
  s.prof.dev_sum_wait_ms = beside ? 0.0 : sum_wait_ms;
  return AMHIP_OK;
}

// window layers -> host matrices where the device content differs from what the host holds.
// dirty_ok: the call before was a DSM / backward-mosaic call, whose context knows which cells of
// the window it can have written (ctx_last_dirty): a small cloud's sub-window, the bounding box of
// a small batch's tile list.  A host matrix that equalled the device layer BEFORE the call (what
// sync_in establishes) differs from it only there: that rectangle is downloaded (device -> pinned
// staging -> the matrix's columns) instead of the window -- the incremental use case on a large
// map downloads megabytes instead of gigabytes per call.
// The three stages of amhip_session_plan.h around the two points where the device answers: (1) which
// layers download at once, beside their sums, and which are summed; (2) after the sums, what every
// other layer downloads -- marked "host unknown" BEFORE the copy --; (3) after the stream has
// synchronised, the host matrices are known to hold what the device summed.
// (the caller has made the window's device current)
static int sync_out(Session& s, int k, const int* layers, float* const* hosts, int nl, bool dirty_ok) {
  PhaseClock clock("sync_out");
  Window& x = s.windows[k];
  Ctx* c = x.c();
  int rc;
  const Win& w = x.win;
  const SessionKnobs knobs = {s.always_copy, tuning_on("session_no_partial"), tuning_on("session_serial_sums")};
  OutLayer L[AMHIP_NUM_LAYERS];
  for (int q = 0; q < nl; ++q) {
    L[q].layer = layers[q];
    L[q].want = hosts[q] != nullptr;
  }
  int rect[4] = {0, 0, w.rows, w.cols};
  bool partial = false;
  if (rect_wanted(dirty_ok, knobs)) {
    if ((rc = ctx_last_dirty(c, rect))) return rc;
    partial = rect_is_partial(rect, w.rows, w.cols);
  }
  AMHIP_TRY(hipEventRecord(x.ev_k1, c->stream));  // (the call's kernels end here)
  clock.mark("kernels (wait)", c->stream, true);
  const auto wall0 = std::chrono::steady_clock::now();
  // (1) the sums; beside them, on the context's stream, the downloads that need not wait for them
  const bool beside = plan_out_sums(L, nl, x.sync, x.const_hash, c->layer_state, partial, knobs);
  bool any = beside;
  if (!s.always_copy && (rc = run_out_sums(s, x, L, hosts, nl, beside))) return rc;
  clock.mark("device content sums");
  const double sum_wait_ms = ms_since(wall0);
  // (2) every other layer: downloaded where the device's sum differs from what the host holds
  const size_t block = (size_t)rect[2] * (size_t)rect[3];
  partial = partial && ensure_pinned(x, rect_staging_floats(block, nl));
  for (int q = 0; q < nl; ++q) {
    if (!L[q].want) continue;
    const int l = L[q].layer;
    const OutAction act = plan_out_layer(&L[q], &x.sync[l], partial, s.always_copy);
    if (L[q].early || act == OutAction::kNone) continue;
    if ((rc = ctx_materialize(c, l))) return rc;
    if (act == OutAction::kRect) {
      AMHIP_TRY(hipMemcpy2DAsync(x.pin + block * (size_t)q, (size_t)rect[2] * 4,
                                 c->layers[l] + (size_t)rect[0] + (size_t)rect[1] * (size_t)w.rows,
                                 (size_t)w.rows * 4, (size_t)rect[2] * 4, (size_t)rect[3],
                                 hipMemcpyDeviceToHost, c->stream));
      s.down_bytes += (unsigned long long)block * 4ull;
      s.prof_down += (unsigned long long)block * 4ull;
    } else if ((rc = download_window(s, x, l, hosts[q]))) {
      return rc;
    }
    any = true;
  }
  AMHIP_TRY(hipEventRecord(x.ev_d1, c->stream));
  if (any) AMHIP_TRY(hipStreamSynchronize(c->stream));
  clock.mark("downloads");
  for (int q = 0; q < nl; ++q)
    if (L[q].action == OutAction::kRect)
      unpack_block(x.pin + block * (size_t)q, hosts[q], s, w.i0 + rect[0], w.j0 + rect[1], rect[2], rect[3]);
  clock.mark("unpack");
  if (s.verify_partial && (rc = verify_rects(s, k, L, hosts, nl))) return rc;
  // (3) the stream has synchronised without an error
  for (int q = 0; q < nl; ++q) out_commit(L[q], &x.sync[L[q].layer], s.always_copy);
  return k == 0 ? record_profile(s, x, beside, sum_wait_ms) : AMHIP_OK;
}

template <typename F>
static int for_windows(Session& s, F fn) {
  const int W = s.W();
  std::vector<int> rcs(W, AMHIP_OK);
  std::vector<std::string> msgs(W);
  if (W == 1) return fn(0);
  std::vector<std::thread> th;
  for (int k = 0; k < W; ++k)
    th.emplace_back([&, k]() {
      rcs[k] = fn(k);
      if (rcs[k]) msgs[k] = amhip_last_error();  // (thread-local message)
    });
  for (auto& x : th) x.join();
  for (int k = 0; k < W; ++k)
    if (rcs[k]) {
      set_last_error(msgs[k]);
      return rcs[k];
    }
  return AMHIP_OK;
}

// What every host-matrix call does around its device work: the profile is reset; the host
// matrices are summed (sums()); every window takes in the matrices the call reads or partially
// writes (enter()) and, behind the call's own work, hands back those it wrote (leave()).
struct HostCall {
  Session& s;
  const std::chrono::steady_clock::time_point call0 = std::chrono::steady_clock::now();
  int nin = 0, nout = 0;
  int in_layer[AMHIP_NUM_LAYERS], out_layer[AMHIP_NUM_LAYERS];
  const float* in[AMHIP_NUM_LAYERS];
  bool in_written[AMHIP_NUM_LAYERS];
  float* out[AMHIP_NUM_LAYERS];
  std::vector<Hash128> hh;  // [nin][W]

  HostCall(Session& session, double up_bytes) : s(session) {
    s.prof = CallProfile();
    s.prof_down = 0;
    s.prof.up_bytes = up_bytes;
  }
  // the device needs what `matrix` holds of `layer` (null: not part of this call)
  void reads(int layer, const float* matrix, bool will_write) {
    if (!matrix) return;
    in_layer[nin] = layer;
    in[nin] = matrix;
    in_written[nin++] = will_write;
  }
  // `matrix` has to hold the layer afterwards (null: listed, not handed back)
  void returns(int layer, float* matrix) {
    out_layer[nout] = layer;
    out[nout++] = matrix;
  }
  // content sums of the matrices the call reads, with host threads (always_copy: nothing is compared)
  void sums() {
    const auto t = std::chrono::steady_clock::now();
    if (!s.always_copy) host_hashes(s, in, nin, &hh);
    else hh.assign((size_t)nin * s.W(), Hash128());
    s.prof.host_sum_ms = ms_since(t);
  }
  int enter(int k) {
    int r = ctx_use_device(s.windows[k].c());
    for (int q = 0; q < nin && r == AMHIP_OK; ++q)
      r = sync_in(s, k, in_layer[q], in[q], hh[(size_t)q * s.W() + k], in_written[q]);
    return r;
  }
  // body(k): the call's device work on window k, enqueued on its context's stream
  template <typename Body>
  int leave(int k, bool dirty_ok, Body body) {
    Window& x = s.windows[k];
    AMHIP_TRY(hipEventRecord(x.ev_k0, x.c()->stream));
    int r = body(k);
    if (r == AMHIP_OK) r = sync_out(s, k, out_layer, out, nout, dirty_ok);
    return r ? r : ctx_fetch_status(x.c());
  }
  int done(int rc) {
    s.prof.total_ms = ms_since(call0);
    return rc;
  }
  // the whole of it where nothing runs beside the sums; staged(k): uploads in front of the kernels' clock
  template <typename Staged, typename Body>
  int run(bool dirty_ok, Staged staged, Body body) {
    sums();
    return done(for_windows(s, [&](int k) -> int {
      int r = enter(k);
      if (r == AMHIP_OK) r = staged(k);
      return r ? r : leave(k, dirty_ok, body);
    }));
  }
};

}  // namespace amhip

using namespace amhip;

struct amhip_session {
  amhip::Session impl;
};

// what create_window() made, in any state of completion
static void release_window(Window& x) {
  if (!x.ctx) return;
  (void)ctx_use_device(x.c());
  (void)hipStreamSynchronize(x.c()->stream);
  for (void* p : {(void*)x.route_out, (void*)x.route_counts, (void*)x.cloud, (void*)x.dev_hash})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)x.pin, (void*)x.pin_hash})
    if (p) (void)hipHostFree(p);
  if (x.aux_stream) (void)hipStreamDestroy(x.aux_stream);
  for (hipEvent_t e : {x.route_done, x.ev_k0, x.ev_k1, x.ev_s1, x.ev_d1})
    if (e) (void)hipEventDestroy(e);
  amhip_ctx_destroy(x.ctx);
  x = Window();
}

// window k of the session: its context, the scratch of its content sums, its second stream and
// events, and the sums of its initial constants
static int create_window(Session& s, int k, int device) {
  Window& x = s.windows[k];
  x.win = window_of(s.edges_i, s.edges_j, k);
  x.dev = device;
  int rc = amhip_ctx_create_window(&s.grid, x.win.i0, x.win.j0, x.win.rows, x.win.cols, device, &x.ctx);
  if (rc) return rc;
  Ctx* c = x.c();
  if ((rc = ctx_use_device(c))) return rc;
  if (hipMalloc(reinterpret_cast<void**>(&x.dev_hash), kSumBytes) != hipSuccess)
    return hip_fail(hipGetLastError(), "hipMalloc(session scratch)", __FILE__, __LINE__);
  if (hipHostMalloc(reinterpret_cast<void**>(&x.pin_hash), kSumBytes, hipHostMallocDefault) != hipSuccess)
    return hip_fail(hipGetLastError(), "hipHostMalloc(session scratch)", __FILE__, __LINE__);
  if (hipStreamCreateWithFlags(&x.aux_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&x.ev_k0) != hipSuccess || hipEventCreate(&x.ev_k1) != hipSuccess ||
      hipEventCreate(&x.ev_d1) != hipSuccess || hipEventCreate(&x.ev_s1) != hipSuccess)
    return hip_fail(hipGetLastError(), "session: second stream / timing events", __FILE__, __LINE__);
  // content sums of the window's initial constants: summed on the device without reading
  // memory (the non-linear mix has no closed form)
  hipError_t e = hipMemsetAsync(x.dev_hash, 0, kSumBytes, c->stream);
  for (int l = 0; l < AMHIP_NUM_LAYERS && e == hipSuccess; ++l)
    hipLaunchKernelGGL(k_layer_hash, dim3(1024), dim3(256), 0, c->stream, (const float*)nullptr,
                       ctx_layer_init_value(l), x.win.rows, x.win.cols, x.win.i0, x.win.j0, s.grid.rows,
                       x.dev_hash + 2 * l);
  if (e == hipSuccess) e = hipMemcpyAsync(x.pin_hash, x.dev_hash, kSumBytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(e, "session: content sums of the initial layers", __FILE__, __LINE__);
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l) x.const_hash[l] = {x.pin_hash[2 * l], x.pin_hash[2 * l + 1]};
  return AMHIP_OK;
}

extern "C" {

int amhip_session_create(const amhip_grid_desc* grid, int tiles_i, int tiles_j,
                         const int32_t* devices, amhip_session** out) {
  if (!grid || !out || tiles_i < 1 || tiles_j < 1)
    return arg_failure("amhip_session_create: bad argument");
  if (tiles_i > grid->rows || tiles_j > grid->cols || (long long)tiles_i * tiles_j > 64)
    return arg_failure("amhip_session_create: more windows than the map can be cut into (<= 64)");
  *out = nullptr;
  amhip_session* h = new (std::nothrow) amhip_session();
  if (!h) return AMHIP_ERR_NOMEM;
  Session& s = h->impl;
  s.grid = *grid;
  s.ti = tiles_i;
  s.always_copy = tuning_on("session_always_copy");
  s.verify_partial = tuning_on("session_verify_partial");
  // window edges on multiples of the gather tile (64 x 32 cells) except at the map border
  window_edges(grid->rows, tiles_i, 64, &s.edges_i);
  window_edges(grid->cols, tiles_j, 32, &s.edges_j);
  const int W = tiles_i * tiles_j;
  s.windows.resize(W);
  for (int k = 0; k < W; ++k) {
    const int rc = create_window(s, k, devices ? devices[k] : 0);
    if (rc) {
      amhip_session_destroy(h);
      return rc;
    }
  }
  // direct device-to-device copies where the hardware allows them (xGMI)
  for (int a = 0; a < W; ++a)
    for (int b = 0; b < W; ++b)
      if (s.windows[a].dev != s.windows[b].dev) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, s.windows[a].dev, s.windows[b].dev) == hipSuccess && can &&
            hipSetDevice(s.windows[a].dev) == hipSuccess)
          (void)hipDeviceEnablePeerAccess(s.windows[b].dev, 0);
        (void)hipGetLastError();  // (already enabled is fine)
      }
  *out = h;
  return AMHIP_OK;
}

void amhip_session_destroy(amhip_session* h) {
  if (!h) return;
  for (Window& x : h->impl.windows) release_window(x);
  delete h;
}

int amhip_session_num_windows(const amhip_session* h) { return h ? h->impl.W() : 0; }

amhip_ctx* amhip_session_context(amhip_session* h, int k) {
  if (!h || k < 0 || k >= h->impl.W()) return nullptr;
  return h->impl.windows[k].ctx;
}

int amhip_session_window(const amhip_session* h, int k, int32_t* i0_j0_rows_cols) {
  if (!h || k < 0 || k >= h->impl.W() || !i0_j0_rows_cols)
    return arg_failure("amhip_session_window: bad argument");
  const Win& w = h->impl.windows[k].win;
  const int32_t v[4] = {w.i0, w.j0, w.rows, w.cols};
  std::copy(v, v + 4, i0_j0_rows_cols);
  return AMHIP_OK;
}

int amhip_session_set_always_copy(amhip_session* h, int on) {
  if (!h) return arg_failure("null session");
  h->impl.always_copy = on != 0;
  for (Window& x : h->impl.windows)
    for (LayerSync& st : x.sync) st.device_valid = st.host_known = false;
  return AMHIP_OK;
}

int amhip_session_transfer_stats(const amhip_session* h, uint64_t* uploaded_bytes,
                                 uint64_t* downloaded_bytes) {
  if (!h) return arg_failure("null session");
  if (uploaded_bytes) *uploaded_bytes = h->impl.up_bytes.load();
  if (downloaded_bytes) *downloaded_bytes = h->impl.down_bytes.load();
  return AMHIP_OK;
}

int amhip_session_last_profile(const amhip_session* h, double* out8) {
  if (!h || !out8) return arg_failure("amhip_session_last_profile: null argument");
  const CallProfile& p = h->impl.prof;
  const double v[8] = {p.total_ms, p.h2d_ms, p.host_sum_ms, p.kernel_ms, p.dev_sum_wait_ms, p.d2h_ms, p.up_bytes,
                       (double)h->impl.prof_down.load()};
  std::copy(v, v + 8, out8);
  return AMHIP_OK;
}

int amhip_session_set_dsm_precision(amhip_session* h, int mode) {
  if (!h) return arg_failure("null session");
  for (Window& x : h->impl.windows) {
    const int rc = amhip_ctx_set_dsm_precision(x.ctx, mode);
    if (rc) return rc;
  }
  return AMHIP_OK;
}

// dsm::Dsm::process (dsm.cc:186-201) on host buffers: `elevation` is the GridMap's matrix
// (map rows x cols, column-major), read and written like the reference does.
int amhip_session_dsm_process(amhip_session* h, const double* host_xyz, size_t n, int radius_sq,
                              double center_easting, double center_northing, float* elevation) {
  if (!h) return arg_failure("null session");
  if (n == 0) return AMHIP_OK;  // "Passed empty point cloud to DSM module" (dsm.cc:189-192)
  if (!host_xyz || !elevation) return arg_failure("amhip_session_dsm_process: null buffer");
  if (radius_sq <= 0) return arg_failure("interpolation_radius must be >= 1");
  Session& s = h->impl;
  const int W = s.W();
  // (1) what do the devices already hold of `elevation`?  (host threads; the cloud's upload
  // is enqueued first where there is a single window, so that both overlap)
  HostCall call(s, (double)n * 24.0);
  call.reads(AMHIP_LAYER_ELEVATION, elevation, true);
  call.returns(AMHIP_LAYER_ELEVATION, elevation);
  int rc;
  if (W == 1) {
    PhaseClock clock("dsm");
    Window& x = s.windows[0];
    Ctx* c = x.c();
    if ((rc = ctx_use_device(c))) return rc;
    if (n >= kMaxCallPoints) return arg_failure("more than 2^31-1 points");
    // (a pageable source makes the upload return only once the data is staged; the sums run
    // in a second thread meanwhile)
    std::thread hasher([&]() { call.sums(); });
    const int rc_up = ctx_stage_cloud(c, host_xyz, nullptr, n);
    s.prof.h2d_ms = ms_since(call.call0);
    clock.mark("cloud enqueued");
    hasher.join();
    clock.mark("host content sum");
    if (rc_up) return rc_up;
    if ((rc = call.enter(0))) return rc;
    if ((rc = call.leave(0, true, [&](int) -> int {
          const int r = amhip_dsm_process_dev(x.ctx, c->stage_points, n, radius_sq, center_easting, center_northing);
          if (r == AMHIP_OK) clock.mark("sync_in + dsm enqueued");
          return r;
        })))
      return rc;
    return call.done(AMHIP_OK);
  }

  call.sums();
  // (2) slice k of the cloud goes to window k's device, which COUNTS what every window needs
  // of it (its cells grown by the halo margin) -- one pass without output --
  const double margin = halo_margin_m(radius_sq, s.grid.resolution);
  std::vector<int32_t> wins(4 * (size_t)W);
  for (int d = 0; d < W; ++d) {
    const Win& w = s.windows[d].win;
    const int32_t v[4] = {w.i0, w.j0, w.rows, w.cols};
    std::copy(v, v + 4, &wins[4 * (size_t)d]);
  }
  auto slice = [&](int k) { return slice_lo(n, k + 1, W) - slice_lo(n, k, W); };
  std::vector<long long> counts((size_t)W * W, 0);
  RouteTable route;
  // one selection pass of slice k over destinations [d0, d0 + nd): count only (caps 0) or
  // compacting into window k's route_out at the offsets the counts gave
  auto select_pass = [&](int k, bool count_only) -> int {
    Window& x = s.windows[k];
    Ctx* c = x.c();
    for (int d0 = 0; d0 < W; d0 += kMaxHaloDests) {
      const int nd = std::min(kMaxHaloDests, W - d0);
      HaloParams hp;
      int r = make_halo_params(*c, center_easting, center_northing, &wins[4 * (size_t)d0], nd, margin,
                               0, &hp);
      if (r) return r;
      for (int d = 0; d < nd; ++d) {
        hp.off[d] = count_only ? 0ull : route.offs[(size_t)k * W + d0 + d];
        hp.cap_d[d] = count_only ? 0ull : (unsigned long long)counts[(size_t)k * W + d0 + d];
      }
      if ((r = halo_select_run(c, c->stage_points, slice(k), hp, x.route_out,
                               reinterpret_cast<unsigned long long*>(x.route_counts + d0))))
        return r;
    }
    return AMHIP_OK;
  };
  rc = for_windows(s, [&](int k) -> int {
    Window& x = s.windows[k];
    Ctx* c = x.c();
    int r = call.enter(k);
    if (r) return r;
    if (!x.route_done) AMHIP_TRY(hipEventCreateWithFlags(&x.route_done, hipEventDisableTiming));
    if (slice(k) == 0) return AMHIP_OK;
    if ((r = ctx_stage_cloud(c, host_xyz + 3 * slice_lo(n, k, W), nullptr, slice(k)))) return r;
    if (!x.route_counts)
      AMHIP_TRY(hipMalloc(reinterpret_cast<void**>(&x.route_counts), sizeof(long long) * W));
    if ((r = select_pass(k, true))) return r;
    AMHIP_TRY(hipMemcpyAsync(&counts[(size_t)k * W], x.route_counts, sizeof(long long) * W,
                             hipMemcpyDeviceToHost, c->stream));
    // (the one host synchronisation of the routing: the sizes of everything that follows)
    AMHIP_TRY(hipStreamSynchronize(c->stream));
    return AMHIP_OK;
  });
  if (rc) return rc;
  // (3) the same pass again, now writing: slice k's selections for window d land behind those
  // for windows < d in ONE buffer of (points selected) rows -- not (slice x windows) --, and an
  // event marks them complete; no host synchronisation from here to the DSM's own
  route = route_table(counts, W);
  rc = for_windows(s, [&](int k) -> int {
    Window& x = s.windows[k];
    int r = ctx_use_device(x.c());
    if (r) return r;
    if (slice(k) && route.sel[k]) {
      if ((r = ensure_capacity(&x.route_out, &x.route_cap, 3 * route.sel[k]))) return r;
      if ((r = select_pass(k, false))) return r;
    }
    AMHIP_TRY(hipEventRecord(x.route_done, x.c()->stream));
    return AMHIP_OK;
  });
  if (rc) return rc;
  // (4) every window collects its points from all slices, device to device (xGMI peer copies
  // behind the producers' events), and runs Dsm::process on them
  rc = for_windows(s, [&](int d) -> int {
    Window& x = s.windows[d];
    Ctx* c = x.c();
    int r = ctx_use_device(c);
    if (r) return r;
    const size_t total = route.total[d];
    if (route.refused(d)) return arg_failure("more than 2^31-1 points in one window");
    if (total) {
      if ((r = ensure_capacity(&x.cloud, &x.cloud_cap, 3 * total))) return r;
      size_t off = 0;
      for (int k = 0; k < W; ++k) {
        const Window& from = s.windows[k];
        const size_t cnt = (size_t)counts[(size_t)k * W + d];
        if (!cnt) continue;
        if (k != d) AMHIP_TRY(hipStreamWaitEvent(c->stream, from.route_done, 0));
        const double* src = from.route_out + 3 * (size_t)route.offs[(size_t)k * W + d];
        if (from.dev == x.dev)
          AMHIP_TRY(hipMemcpyAsync(x.cloud + 3 * off, src, cnt * 24, hipMemcpyDeviceToDevice, c->stream));
        else
          AMHIP_TRY(hipMemcpyPeerAsync(x.cloud + 3 * off, x.dev, src, from.dev, cnt * 24, c->stream));
        off += cnt;
      }
    }
    // (no points, no call: no dirty cells on record)
    return call.leave(d, total != 0, [&](int) -> int {
      return total ? amhip_dsm_process_dev(x.ctx, x.cloud, total, radius_sq, center_easting, center_northing)
                   : AMHIP_OK;
    });
  });
  // (a later call may overwrite route_out while a slower peer still reads it: every window
  // finished its copies before its own sync_out returned, and all threads were joined)
  return call.done(rc);
}

// ortho::OrthoBackwardGrid::process (ortho-backward-grid.cc:223-239) on host buffers.
// occl_margin: null = the reference's mosaic; else the occlusion-tested one (one window only).
// blend: null, or the blended mosaic's options (its occlusion switch is what occl_margin says)
static int session_ortho_backward(
    amhip_session* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho, const double* occl_margin,
    const amhip_ortho_blend_opts* blend = nullptr) {
  if (!h || !cam) return arg_failure("null session / camera");
  if (F == 0 || !host_T_G_C || !images || !steps)
    return arg_failure("empty pose / image list (CHECK(!T_G_Bs.empty()))");
  if (cam->width <= 0 || cam->height <= 0) return arg_failure("bad image size");
  if (!elevation || !elevation_angle || !observation_index || !num_observations ||
      !(colored ? colored_ortho : ortho))
    return arg_failure("amhip_session_ortho_backward_process: null layer");
  Session& s = h->impl;
  const size_t row = (size_t)cam->width * (size_t)channels;
  const size_t frame = row * (size_t)cam->height;
  // (the mosaic reads the elevation and writes the other layers, ONE of the two output layers --
  // ortho-backward-grid.cc:186-208 --: the other matrix is neither summed, uploaded nor
  // downloaded; 400 MB of host hashing per call)
  HostCall call(s, (double)frame * (double)F);
  float* const mats[AMHIP_NUM_LAYERS] = {colored ? nullptr : ortho, nullptr,           elevation_angle,
                                         num_observations,          observation_index, colored ? colored_ortho : nullptr};
  for (int l = 0; l < AMHIP_NUM_LAYERS; ++l) {  // (the context's layer order)
    call.reads(l, l == AMHIP_LAYER_ELEVATION ? elevation : mats[l], l != AMHIP_LAYER_ELEVATION);
    if (l != AMHIP_LAYER_ELEVATION) call.returns(l, mats[l]);
  }
  // the frames go up while host threads hash the six matrices
  PhaseClock clock("ortho_backward");
  int rc_up = AMHIP_OK;
  std::string up_msg;
  double up_ms = 0.0;
  std::thread uploader([&]() {
    rc_up = for_windows(s, [&](int k) -> int {
      Ctx* c = s.windows[k].c();
      const int r = ctx_use_device(c);
      return r ? r : ctx_stage_frames(c, images, steps, F, row, (size_t)cam->height);
    });
    if (rc_up) up_msg = amhip_last_error();
    up_ms = ms_since(call.call0);
  });
  call.sums();
  clock.mark("host content sums");
  uploader.join();
  s.prof.h2d_ms = up_ms;
  clock.mark("frames enqueued");
  if (rc_up) {
    set_last_error(up_msg);
    return rc_up;
  }
  return call.done(for_windows(s, [&](int k) -> int {
    int r = call.enter(k);
    if (r) return r;
    if (k == 0) clock.mark("sync_in");
    return call.leave(k, true, [&](int) -> int {
      Window& x = s.windows[k];
      const int rr =
          blend       ? amhip_ortho_backward_process_blend_dev(x.ctx, cam, host_T_G_C, F, x.c()->stage_frames, frame,
                                                               row, channels, colored, blend)
          : occl_margin ? amhip_ortho_backward_process_occl_dev(x.ctx, cam, host_T_G_C, F, x.c()->stage_frames, frame,
                                                              row, channels, colored, *occl_margin)
                      : amhip_ortho_backward_process_dev(x.ctx, cam, host_T_G_C, F, x.c()->stage_frames, frame, row,
                                                         channels, colored);
      if (rr == AMHIP_OK && k == 0) clock.mark("mosaic enqueued");
      return rr;
    });
  }));
}

int amhip_session_ortho_backward_process(
    amhip_session* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho) {
  return session_ortho_backward(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                                elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                                nullptr);
}

int amhip_session_ortho_backward_process_occl(
    amhip_session* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho, double margin_m) {
  if (!h || !cam) return arg_failure("null session / camera");
  if (!(margin_m >= 0.0))
    return arg_failure("occlusion test: margin_m must be >= 0 (+inf is legal: nothing occludes), not negative or NaN");
  if (h->impl.W() != 1)
    return arg_failure(
        "occlusion test: the session holds more than one window and the ray towards the camera leaves "
        "a window; windows need an elevation halo, which is not built yet");
  return session_ortho_backward(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                                elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                                &margin_m);
}

int amhip_session_ortho_backward_process_blend(
    amhip_session* h, const amhip_camera* cam, const double* host_T_G_C, size_t F,
    const uint8_t* const* images, const size_t* steps, int channels, int colored,
    const float* elevation, float* elevation_angle, float* observation_index,
    float* num_observations, float* ortho, float* colored_ortho, const amhip_ortho_blend_opts* opts) {
  if (!h || !cam) return arg_failure("null session / camera");
  if (!opts) return arg_failure("blended mosaic: null options (amhip_ortho_blend_opts)");
  if (opts->sharpness < 0 || opts->sharpness > 4)
    return arg_failure("blended mosaic: sharpness must be 0 .. 4 (the weight is sin^2 .. sin^32 of the view angle)");
  if (opts->occlusion_test) {
    if (!(opts->occlusion_margin_m >= 0.0))
      return arg_failure("occlusion test: margin_m must be >= 0 (+inf is legal: nothing occludes), not negative or NaN");
    if (h->impl.W() != 1)
      return arg_failure(
          "occlusion test: the session holds more than one window and the ray towards the camera leaves "
          "a window; windows need an elevation halo, which is not built yet");
  }
  // (without the occlusion test every window runs it: each context holds its own cells' sums)
  return session_ortho_backward(h, cam, host_T_G_C, F, images, steps, channels, colored, elevation,
                                elevation_angle, observation_index, num_observations, ortho, colored_ortho,
                                opts->occlusion_test ? &opts->occlusion_margin_m : nullptr, opts);
}

// ortho::OrthoFromPcl::process (ortho-from-pcl.cc:20-113) on host buffers: `ortho` = the
// GridMap's matrix.  Every window gets the whole cloud (its binning drops what lies outside the
// window + margin): intensities travel with their points, and this rank-1 "next" path is not
// worth a routing pass of its own.
int amhip_session_ortho_from_pcl_process(amhip_session* h, const double* host_xyz,
                                         const int32_t* host_intensities, size_t n, int radius_sq,
                                         int adaptive, float* ortho) {
  if (!h) return arg_failure("null session");
  if (n == 0 || !host_xyz || !host_intensities || !ortho)
    return arg_failure("empty point cloud / null buffer (CHECK(!pointcloud.empty()))");
  if (n >= kMaxCallPoints) return arg_failure("more than 2^31-1 points");
  Session& s = h->impl;
  HostCall call(s, (double)n * 28.0 * (double)s.W());   // (every window gets the whole cloud)
  call.reads(AMHIP_LAYER_ORTHO, ortho, true);
  call.returns(AMHIP_LAYER_ORTHO, ortho);
  return call.run(
      false, [&](int k) -> int { return ctx_stage_cloud(s.windows[k].c(), host_xyz, host_intensities, n); },
      [&](int k) -> int {
        Ctx* c = s.windows[k].c();
        return amhip_ortho_from_pcl_process_dev(s.windows[k].ctx, c->stage_points, c->stage_values, n, radius_sq,
                                                adaptive);
      });
}

// ---- what leaves the map (formats: amhip_export.hip) ---------------

// grid_map_msgs/GridMap in ROS 1 wire format (AerialGridMap::publishOnce,
// aerial-mapper-grid-map.cc:66-72: setTimestamp + GridMapRosConverter::toMessage + publish):
// the resident layers travel from the devices STRAIGHT into the message buffer -- no host matrix
// in between.  layer_ids[l] = the amhip layer behind message layer l, or -1: then host_layers[l]
// (a rows x cols column-major matrix) is copied, or, if that is null, the layer is NaN (the three
// layers of AerialGridMap the path never touches).
int amhip_session_grid_map_msg(amhip_session* h, uint64_t stamp_ns, const char* frame_id,
                               int num_layers, const char* const* layer_names,
                               const int32_t* layer_ids, const float* const* host_layers,
                               uint8_t* out, size_t cap, size_t* written) {
  if (!h || !frame_id || num_layers < 1 || num_layers > 64 || !layer_names || !layer_ids || !out)
    return arg_failure("amhip_session_grid_map_msg: bad argument");
  Session& s = h->impl;
  for (int l = 0; l < num_layers; ++l)
    if (layer_ids[l] >= AMHIP_NUM_LAYERS) return arg_failure("amhip_session_grid_map_msg: bad layer id");
  std::vector<size_t> at(num_layers);
  int rc = amhip_grid_map_msg_layout(&s.grid, stamp_ns, frame_id, num_layers, layer_names, out, cap,
                                     at.data());
  if (rc) return rc;
  const size_t cells = (size_t)s.grid.rows * (size_t)s.grid.cols;
  // the layers without a device copy are filled by host threads WHILE the others travel
  std::vector<std::thread> fillers;
  {
    std::vector<float> nan_block(std::min<size_t>(cells, 1u << 16), std::nanf(""));
    const size_t nb = nan_block.size();
    auto fill = [&, nb](int l, size_t k0, size_t k1, const std::vector<float>* block) {
      uint8_t* p = out + at[l];  // (not aligned: bytes only)
      if (host_layers && host_layers[l]) {
        std::memcpy(p + 4 * k0, host_layers[l] + k0, 4 * (k1 - k0));
      } else {
        for (size_t k = k0; k < k1; k += nb)
          std::memcpy(p + 4 * k, block->data(), 4 * std::min(nb, k1 - k));
      }
    };
    const auto shared = std::make_shared<std::vector<float>>(std::move(nan_block));
    const int parts = cells >= (size_t(1) << 22) ? 4 : 1;
    for (int l = 0; l < num_layers; ++l) {
      if (layer_ids[l] >= 0) continue;
      for (int q = 0; q < parts; ++q) {
        const size_t k0 = cells * q / parts, k1 = cells * (q + 1) / parts;
        fillers.emplace_back([=]() { fill(l, k0, k1, shared.get()); });
      }
    }
  }
  rc = for_windows(s, [&](int k) -> int {
    Ctx* c = &s.windows[k].ctx->impl;
    int r = ctx_use_device(c);
    if (r) return r;
    const Win& w = s.windows[k].win;
    for (int l = 0; l < num_layers; ++l) {
      const int id = layer_ids[l];
      if (id < 0) continue;
      if ((r = ctx_materialize(c, id))) return r;
      uint8_t* dst = out + at[l] + 4 * ((size_t)w.i0 + (size_t)w.j0 * (size_t)s.grid.rows);
      AMHIP_TRY(copy_window(dst, c->layers[id], s, w, true, c->stream));
    }
    AMHIP_TRY(hipStreamSynchronize(c->stream));
    return AMHIP_OK;
  });
  for (auto& t : fillers) t.join();
  if (rc) return rc;
  if (written) *written = amhip_grid_map_msg_bytes(&s.grid, frame_id, num_layers, layer_names);
  return AMHIP_OK;
}

// The whole map's layer as an image (grid_map_cv's toImage orientation: image row = index 0):
// every window is turned on its own device (k_layer_to_image) and lands in its block of the
// host image.
int amhip_session_layer_to_image(amhip_session* h, int layer, int bgr, float lower, float upper,
                                 uint8_t* host_image, size_t step) {
  if (!h || !host_image || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_session_layer_to_image: bad argument");
  Session& s = h->impl;
  const size_t bpp = bgr ? 3u : 1u;
  if (step < (size_t)s.grid.cols * bpp)
    return arg_failure("amhip_session_layer_to_image: step smaller than an image row");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_session_layer_to_image: upper <= lower");
  return for_windows(s, [&](int k) -> int {
    Ctx* c = &s.windows[k].ctx->impl;
    int r = ctx_use_device(c);
    if (r) return r;
    const Win& w = s.windows[k].win;
    const size_t row = (size_t)w.cols * bpp;
    uint8_t* dev = nullptr;
    AMHIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), row * (size_t)w.rows));
    r = amhip_layer_to_image_dev(s.windows[k].ctx, layer, bgr, lower, upper, dev, row);
    if (r == AMHIP_OK) {
      hipError_t e = hipMemcpy2DAsync(host_image + (size_t)w.i0 * step + (size_t)w.j0 * bpp, step,
                                      dev, row, row, (size_t)w.rows, hipMemcpyDeviceToHost,
                                      c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) r = hip_fail(e, "image download", __FILE__, __LINE__);
    }
    (void)hipFree(dev);
    return r;
  });
}

/* The whole map's layer for a JPEG or PNG writer: the image assembled on the host from every window
 * (amhip_session_layer_to_image), rows packed.  limit: the format's refusal of a map no file of it holds. */
static int session_layer_image(amhip_session* h, const char* limit, int layer, int bgr, float lower, float upper,
                               std::vector<uint8_t>* image, size_t* row) {
  const amhip_grid_desc& g = h->impl.grid;
  if (!image_size_ok(g.rows, g.cols)) return arg_failure(limit);
  *row = (size_t)g.cols * (bgr ? 3u : 1u);
  image->resize(*row * (size_t)g.rows);
  return amhip_session_layer_to_image(h, layer, bgr, lower, upper, image->data(), *row);
}

/* amhip_layer_write_jpeg for the whole map of a session, encoded on the first window's device. */
int amhip_session_layer_write_jpeg(amhip_session* h, int layer, int bgr, float lower, float upper,
                                   int quality, const char* filename) {
  if (!h || !filename || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_session_layer_write_jpeg: bad argument");
  if (quality < 0 || quality > 100)
    return arg_failure("amhip_session_layer_write_jpeg: quality must be 1..100 (0: 95)");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_session_layer_write_jpeg: upper <= lower");
  Session& s = h->impl;
  std::vector<uint8_t> image;
  size_t row = 0;
  const int rc = session_layer_image(h, "amhip_session_layer_write_jpeg: a JPEG file holds 1 x 1 to 65535 x 65535 pixels",
                                     layer, bgr, lower, upper, &image, &row);
  if (rc) return rc;
  return amhip_jpeg_write(s.windows[0].ctx, filename, image.data(), /*on_device=*/0, row, s.grid.cols, s.grid.rows,
                          bgr ? 3 : 1, quality);
}

/* ... and amhip_layer_write_png, the same way */
int amhip_session_layer_write_png(amhip_session* h, int layer, int bgr, float lower, float upper,
                                  const char* filename) {
  if (!h || !filename || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_session_layer_write_png: bad argument");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_session_layer_write_png: upper <= lower");
  Session& s = h->impl;
  std::vector<uint8_t> image;
  size_t row = 0;
  const int rc = session_layer_image(
      h, "amhip_session_layer_write_png: a PNG file of this encoder holds 1 x 1 to 65535 x 65535 pixels", layer, bgr,
      lower, upper, &image, &row);
  if (rc) return rc;
  return amhip_png_write(s.windows[0].ctx, filename, image.data(), /*on_device=*/0, row, s.grid.cols, s.grid.rows,
                         bgr ? 3 : 1);
}

/* amhip_layer_write_geotiff for the whole map of a session: the north-up raster
 * assembled on the host from every window -- the floats themselves for kind 0, the image of
 * amhip_session_layer_to_image for kinds 1 and 2 -- and encoded on the first window's device. */
static int session_layer_write_geotiff(const std::string& kWho, amhip_session* h, int layer, int kind, float lower,
                                       float upper, int tile, int overviews, bool ovr, int utm_zone, int northern,
                                       const char* filename) {
  if (!h || !filename) return arg_failure((std::string(kWho) + "null argument").c_str());
  if (layer < 0 || layer >= AMHIP_NUM_LAYERS) return arg_failure((std::string(kWho) + "layer: no such layer").c_str());
  Session& s = h->impl;
  const size_t rows = (size_t)s.grid.rows, cols = (size_t)s.grid.cols;
  // (the kind and tile rules and their texts are the raster writer's; the size has a text of its own here)
  if (const char* why = tiff::check_kind(kind)) return arg_failure((std::string(kWho) + why).c_str());
  if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535)
    return arg_failure((std::string(kWho) + "width and height must be 1..65535").c_str());
  if (const char* why = tiff::check_tile(tile)) return arg_failure((std::string(kWho) + why).c_str());
  if (utm_zone < 1 || utm_zone > 60) return arg_failure((std::string(kWho) + "utm_zone must be 1..60").c_str());
  if (kind == 1 && !(upper > lower)) return arg_failure((std::string(kWho) + "upper <= lower").c_str());
  int novr = 0;
  if (const char* why = tiff::check_overviews((int)rows, (int)cols, tile, overviews, &novr))
    return arg_failure((std::string(kWho) + why).c_str());
  const amhip_grid_desc& g = s.grid;
  const double gt[6] = {g.pos_x - g.length_x / 2, g.resolution, 0.0, g.pos_y + g.length_y / 2, 0.0, -g.resolution};
  // raster pixel (r, c) is cell (i, j) = (rows - 1 - c, r): width = rows, height = cols
  const size_t px = kind == 0 ? 4u : kind == 1 ? 1u : 3u;
  std::vector<uint8_t> raster(rows * cols * px);
  int rc;
  if (kind == 0) {
    std::vector<float> map(rows * cols);
    rc = for_windows(s, [&](int k) -> int {
      Ctx* c = &s.windows[k].ctx->impl;
      int r = ctx_use_device(c);
      if (r) return r;
      if ((r = ctx_materialize(c, layer))) return r;
      AMHIP_TRY(copy_window(map_at(map.data(), s, s.windows[k].win), c->layers[layer], s, s.windows[k].win, true, c->stream));
      AMHIP_TRY(hipStreamSynchronize(c->stream));
      return AMHIP_OK;
    });
    if (rc) return rc;
    float* out = reinterpret_cast<float*>(raster.data());
    for (size_t r = 0; r < cols; ++r)
      for (size_t c = 0; c < rows; ++c) out[r * rows + c] = map[(rows - 1 - c) + r * rows];
  } else {
    const size_t step = cols * px;
    std::vector<uint8_t> image(rows * step);
    if ((rc = amhip_session_layer_to_image(h, layer, kind == 2, lower, upper, image.data(), step))) return rc;
    for (size_t r = 0; r < cols; ++r)
      for (size_t c = 0; c < rows; ++c) {
        const uint8_t* p = image.data() + (rows - 1 - c) * step + r * px;
        uint8_t* q = raster.data() + (r * rows + c) * px;
        if (kind == 1) {
          q[0] = p[0];
        } else {   // the image is B, G, R
          q[0] = p[2];
          q[1] = p[1];
          q[2] = p[0];
        }
      }
  }
  if (ovr)
    return amhip_geotiff_write_ovr(s.windows[0].ctx, filename, raster.data(), /*on_device=*/0, rows * px, (int)rows, (int)cols,
                                   kind, tile, overviews, gt, utm_zone, northern);
  return amhip_geotiff_write(s.windows[0].ctx, filename, raster.data(), /*on_device=*/0, rows * px, (int)rows, (int)cols, kind,
                             tile, gt, utm_zone, northern);
}

int amhip_session_layer_write_geotiff(amhip_session* h, int layer, int kind, float lower, float upper, int tile,
                                      int utm_zone, int northern, const char* filename) {
  return session_layer_write_geotiff("amhip_session_layer_write_geotiff: ", h, layer, kind, lower, upper, tile, 0, false,
                                     utm_zone, northern, filename);
}

/* ... with `overviews` levels behind level 0: the single context's pyramid of the whole map */
int amhip_session_layer_write_geotiff_ovr(amhip_session* h, int layer, int kind, float lower, float upper, int tile,
                                          int overviews, int utm_zone, int northern, const char* filename) {
  return session_layer_write_geotiff("amhip_session_layer_write_geotiff_ovr: ", h, layer, kind, lower, upper, tile,
                                     overviews, true, utm_zone, northern, filename);
}

/* amhip_layer_read_geotiff for every window of a session, then the layer into the GridMap's host
 * matrix.  Two passes over the windows: every window decodes the chunks under its own cells first
 * (tiff_layer_prepare: no layer, no matrix touched), and only when all of them have succeeded does
 * any of them take the host matrix in (sync_in, as a DSM call does), place the pixels and hand the
 * result back (sync_out), which leaves the content sums agreeing with the matrix. */
static int session_layer_read_geotiff(const char* kWho, amhip_session* h, int layer, const char* filename, int level,
                                      float* matrix) {
  if (!h || !filename || !matrix) return arg_failure((std::string(kWho) + ": null argument").c_str());
  if (layer < 0 || layer >= AMHIP_NUM_LAYERS) return arg_failure((std::string(kWho) + ": layer: no such layer").c_str());
  Session& s = h->impl;
  std::vector<uint8_t> file;
  int rc = read_file(kWho, filename, &file);
  if (rc) return rc;
  std::vector<TiffLayerJob*> jobs(s.W(), nullptr);
  rc = for_windows(s, [&](int k) -> int {
    return tiff_layer_prepare(&s.windows[k].ctx->impl, kWho, layer, file.data(), file.size(), level, &jobs[k]);
  });
  if (rc == AMHIP_OK) {
    HostCall call(s, 0.0);
    call.reads(layer, matrix, true);
    call.returns(layer, matrix);
    rc = call.run(
        false, [](int) -> int { return AMHIP_OK; },
        [&](int k) -> int { return tiff_layer_place(&s.windows[k].ctx->impl, jobs[k]); });
  }
  for (TiffLayerJob* j : jobs) tiff_layer_job_free(j);
  return rc;
}

int amhip_session_layer_read_geotiff(amhip_session* h, int layer, const char* filename, float* matrix) {
  return session_layer_read_geotiff("amhip_session_layer_read_geotiff", h, layer, filename, kTiffFirstIfd, matrix);
}

/* ... from level `level` of the file; -1: every window takes the automatic choice, which
 * depends on the map's resolution only and so is the same level for all of them */
int amhip_session_layer_read_geotiff_level(amhip_session* h, int layer, const char* filename, int level,
                                           float* matrix) {
  static const char kWho[] = "amhip_session_layer_read_geotiff_level";
  if (level < -1)
    return arg_failure((std::string(kWho) + ": level: -1 (automatic) or a level of the file, 0 ..").c_str());
  return session_layer_read_geotiff(kWho, h, layer, filename, level, matrix);
}

}  // extern "C"
