// CPU emulation of the capped DSM mode's sorted set (aerial_mapper_amd/csrc/amhip_knn_set.h): the
// very functions the gather kernels compile, fed one (d2, z) sequence with a run-time k.
// Driven by tests/test_knn_set_host.py through ctypes.
#include "amhip_knn_set.h"

extern "C" {

// Feeds d2[0..n), z[0..n) to knn_add<8> in order; returns the set: out_d2 / out_z (8 entries each,
// the unused ones as knn_init left them), *out_worst, and n as the return value.
int emul_knn_set(int k, int n, const double* d2, const double* z, double* out_d2, double* out_z,
                 double* out_worst) {
  if (k < 1 || k > amhip::kMaxKnn) return -1;
  amhip::KnnSet s;
  amhip::knn_init(&s);
  for (int q = 0; q < n; ++q) amhip::knn_add(&s, k, d2[q], z[q]);
  for (int q = 0; q < amhip::kMaxKnn; ++q) {
    out_d2[q] = s.d2[q];
    out_z[q] = s.z[q];
  }
  *out_worst = s.worst;
  return s.n;
}

// Many sequences in one call (the exhaustive family): sequence t is entries off[t] .. off[t + 1).
// out_d2 / out_z: 8 per sequence, out_worst / out_n: one per sequence.
int emul_knn_set_batch(int k, int nseq, const int* off, const double* d2, const double* z,
                       double* out_d2, double* out_z, double* out_worst, int* out_n) {
  for (int t = 0; t < nseq; ++t) {
    const int r = emul_knn_set(k, off[t + 1] - off[t], d2 + off[t], z + off[t],
                               out_d2 + 8 * t, out_z + 8 * t, out_worst + t);
    if (r < 0) return r;
    out_n[t] = r;
  }
  return 0;
}

}  // extern "C"
