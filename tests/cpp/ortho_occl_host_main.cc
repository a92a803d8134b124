// The occlusion march of the true-ortho mosaic (amhip_ortho_occl.h) on the CPU: the very function
// the kernel calls, compiled alone, under the address and undefined-behaviour sanitizers
// (tests/test_ortho_occlusion_host.py).
//
// usage: ortho_occl_host_main <file>
//   file:   rows cols res nq
//           rows * cols elevations (column-major: cell (i, j) at i + j * rows)
//           nq queries: i j x_c y_c tx ty tz margin zcut
//   numbers are what strtod reads (hex floats, nan, inf); one line "0" or "1" per query.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "amhip_ortho_occl.h"

static bool next_double(FILE* f, double* out) {
  char tok[128];
  if (std::fscanf(f, "%127s", tok) != 1) return false;
  char* end = nullptr;
  *out = std::strtod(tok, &end);
  return end != tok && *end == '\0';
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file>\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  double rows_d, cols_d, res, nq_d;
  if (!next_double(f, &rows_d) || !next_double(f, &cols_d) || !next_double(f, &res) || !next_double(f, &nq_d) ||
      !(rows_d >= 1) || !(cols_d >= 1) || !(rows_d * cols_d <= 1e7) || !(nq_d >= 0) || !(nq_d <= 1e7)) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  const int rows = (int)rows_d, cols = (int)cols_d;
  const long nq = (long)nq_d;
  // (exactly rows * cols floats: a read past the map is the address sanitizer's to find)
  std::vector<float> elevation((size_t)rows * (size_t)cols);
  for (size_t k = 0; k < elevation.size(); ++k) {
    double v;
    if (!next_double(f, &v)) {
      std::fprintf(stderr, "bad elevation %zu\n", k);
      return 2;
    }
    elevation[k] = (float)v;
  }
  for (long q = 0; q < nq; ++q) {
    double a[9];
    for (int k = 0; k < 9; ++k)
      if (!next_double(f, &a[k])) {
        std::fprintf(stderr, "bad query %ld\n", q);
        return 2;
      }
    const int i = (int)a[0], j = (int)a[1];
    if (i < 0 || i >= rows || j < 0 || j >= cols) {
      std::fprintf(stderr, "query %ld: no such cell\n", q);
      return 2;
    }
    const double h = (double)elevation[(size_t)i + (size_t)j * (size_t)rows];
    const bool o = amhip::occl_march(elevation.data(), rows, cols, i, j, a[2], a[3], h, a[4], a[5], a[6], res,
                                     a[7], a[8]);
    std::printf("%d\n", o ? 1 : 0);
  }
  std::fclose(f);
  return 0;
}
