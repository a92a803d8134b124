// amhip_knn_set.h -- the sorted set of the DSM's OPTIONAL capped mode (amhip_ctx_set_dsm_knn;
// not a reference code path): the k nearest points of a cell's search result, kept sorted by
// ascending d2 in registers (nanoflann::KNNResultSet::addPoint, nanoflann.hpp:100-125: a later
// arrival never displaces an equal distance).
//
// Host + device: the gather kernels (amhip_dsm.hip: k_dsm_gather_tiled_knn, k_dsm_gather_knn) and
// the CPU emulation the unit tests drive (tests/cpp/knn_set_emul.cc) compile the same functions.
#ifndef AMHIP_KNN_SET_H_
#define AMHIP_KNN_SET_H_

#ifndef AMHIP_HD   // (as amhip_ortho_fold.h)
#if defined(__HIPCC__)
#define AMHIP_HD __host__ __device__ __forceinline__
#else
#define AMHIP_HD inline
#endif
#endif

namespace amhip {

constexpr int kMaxKnn = 8;
template <int K>
struct KnnSetT {
  double d2[K], z[K];
  double worst;   // d2 of the k-th entry once the set is full, +inf before: what a candidate has to beat
  int n;          // (a scalar of its own: s->d2[k - 1] with a run-time k would move the arrays to scratch memory)
};
typedef KnnSetT<kMaxKnn> KnnSet;

// (K: the registers the set takes, k <= K the cap in force)
template <int K>
AMHIP_HD void knn_add(KnnSetT<K>* s, int k, double d2, double z) {
  if (!(d2 < s->worst)) return;
  // shift the strictly greater entries up (static indices only: the set lives in registers)
  double cd = d2, cz = z;
  bool inserted = false;  // from the insertion point on every entry moves up by one
#pragma unroll
  for (int q = 0; q < K; ++q) {
    if (q < k) {
      const bool here = inserted || q >= s->n || cd < s->d2[q];
      const double od = s->d2[q], oz = s->z[q];
      if (here) {
        s->d2[q] = cd;
        s->z[q] = cz;
        cd = od;
        cz = oz;
        inserted = true;
      }
    }
  }
  if (s->n < k) ++s->n;
  if (s->n == k) {
#pragma unroll
    for (int q = 0; q < K; ++q)
      if (q == k - 1) s->worst = s->d2[q];
  }
}

template <int K>
AMHIP_HD void knn_init(KnnSetT<K>* s) {
  s->n = 0;
  s->worst = __builtin_huge_val();
#pragma unroll
  for (int q = 0; q < K; ++q) s->d2[q] = s->z[q] = 0.0;
}

}  // namespace amhip

#endif  // AMHIP_KNN_SET_H_
