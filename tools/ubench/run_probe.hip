// run_probe.hip -- what does it cost to GATHER short runs on the read side instead of scattering
// them on the write side?  (the sort's run pipeline reads 480 B / 254 B runs at
// 8-byte-aligned addresses where the counting pipeline writes them.)
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/run_probe.hip -o tools/ubench/run_probe
// 1.2 GB of doubles laid out as chunks of 7680 doubles (2560 points), every chunk holding one run
// of L doubles per key (L = 60: 480 B, 128 keys; L = 32: 256 B, 240 keys).  A workgroup owns one
// (key, segment): the key's runs of R consecutive chunks, R * L = 7680 doubles.
//   read  runs -> contiguous (what pass 2 and the placement of the run pipeline do), in two orders:
//         "near"   consecutive workgroups take consecutive KEYS of the same chunks: the lines two
//                  neighbouring runs share are asked for at about the same time
//         "far"    consecutive workgroups take consecutive SEGMENTS of one key: neighbouring runs
//                  are read by workgroups thousands of ids apart
//   write contiguous -> runs (what the counting pipeline's scatter passes do), same two orders
//   copy  contiguous -> contiguous, the same bytes
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)
constexpr int kSeg = 7680;  // doubles a workgroup moves

// mode 0: copy; 1: gather runs; 2: scatter runs.  keys * len == kSeg; chunks == runs_per_wg * segs.
template <int kMode>
__global__ void __launch_bounds__(512) k_runs(const double* __restrict__ src, double* __restrict__ dst,
                                              int keys, int len, int segs, int near) {
  const int wg = blockIdx.x;
  if (wg >= keys * segs) return;
  const int key = near ? wg % keys : wg / segs;
  const int seg = near ? wg / keys : wg % segs;
  const int per = kSeg / len;  // runs of the workgroup (== keys)
  const size_t flat = ((size_t)key * segs + seg) * kSeg;   // the contiguous side
  for (int e = threadIdx.x; e < kSeg; e += 512) {
    const int r = e / len, o = e - r * len;
    const size_t run_at = ((size_t)(seg * per + r) * keys + key) * len + o;   // < chunks * kSeg
    if (kMode == 0) dst[flat + e] = src[flat + e];
    if (kMode == 1) dst[flat + e] = src[run_at];
    if (kMode == 2) dst[run_at] = src[flat + e];
  }
}

int main() {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const size_t cap = (size_t)19456 * kSeg;  // doubles: 1.195 GB
  double *a, *b;
  CK(hipMalloc(&a, cap * 8));
  CK(hipMalloc(&b, cap * 8));
  CK(hipMemset(a, 1, cap * 8));
  CK(hipMemset(b, 2, cap * 8));
  std::printf("%-8s %-6s %-5s %10s %10s %10s\n", "runs", "what", "order", "min ms", "median ms", "TB/s (min)");
  for (int len : {60, 32}) {
    const int keys = kSeg / len, segs = len == 60 ? 152 : 81;   // chunks = keys * segs <= 19456
    const size_t n = (size_t)keys * segs * kSeg;
    if (n > cap) return 1;
    for (int mode = 0; mode < 3; ++mode)
      for (int near = 1; near >= 0; --near) {
        if (mode == 0 && !near) continue;
        std::vector<float> ms;
        for (int it = 0; it < 9; ++it) {
          CK(hipEventRecord(e0));
          const dim3 g(keys * segs), t(512);
          if (mode == 0) hipLaunchKernelGGL(k_runs<0>, g, t, 0, 0, a, b, keys, len, segs, near);
          if (mode == 1) hipLaunchKernelGGL(k_runs<1>, g, t, 0, 0, a, b, keys, len, segs, near);
          if (mode == 2) hipLaunchKernelGGL(k_runs<2>, g, t, 0, 0, a, b, keys, len, segs, near);
          CK(hipGetLastError());
          CK(hipEventRecord(e1));
          CK(hipEventSynchronize(e1));
          float v;
          CK(hipEventElapsedTime(&v, e0, e1));
          if (it >= 2) ms.push_back(v);
        }
        std::sort(ms.begin(), ms.end());
        std::printf("%4d B   %-6s %-5s %10.4f %10.4f %10.2f\n", len * 8,
                    mode == 0 ? "copy" : mode == 1 ? "read" : "write", mode == 0 ? "-" : near ? "near" : "far",
                    ms.front(), ms[ms.size() / 2], 2.0 * n * 8 / (ms.front() * 1e9));
      }
  }
  return 0;
}
