// The arithmetic of the blended mosaic (amhip_ortho_blend.h) on the CPU: the very functions the
// kernel calls, compiled alone, under the address and undefined-behaviour sanitizers
// (tests/test_ortho_blend_host.py).
//
// usage: ortho_blend_host_main <file>
//   file:   nch sharpness npairs          nch: 1 gray, 3 colour (B, G, R)
//           npairs lines: cx cy cz I[0] .. I[nch - 1]     one cell's contributing pairs, in order
//   numbers are what strtod reads (hex floats).  Prints the cell's sums as %a -- wsum, acc[0] ..
//   acc[nch - 1] -- and, when wsum > 0, the bits of the float the output layer gets (%08x).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "amhip_ortho_blend.h"

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
  double head[3];
  for (double& h : head)
    if (!next_double(f, &h)) return 3;
  const int nch = (int)head[0], sharpness = (int)head[1];
  const long npairs = (long)head[2];
  if ((nch != 1 && nch != 3) || sharpness < 0 || sharpness > amhip::kBlendMaxSharpness || npairs < 0) return 3;
  double wsum = 0.0, acc[3] = {0.0, 0.0, 0.0};
  for (long n = 0; n < npairs; ++n) {
    double c[3], px[3];
    for (double& v : c)
      if (!next_double(f, &v)) return 4;
    for (int ch = 0; ch < nch; ++ch)
      if (!next_double(f, &px[ch])) return 4;
    const double zz = c[2] * c[2];
    const double n2 = (c[0] * c[0] + c[1] * c[1]) + zz;
    const double w = amhip::blend_weight(zz, n2, sharpness);
    for (int ch = 0; ch < nch; ++ch) acc[ch] = acc[ch] + w * px[ch];
    wsum = wsum + w;
  }
  std::fclose(f);
  std::printf("%a", wsum);
  for (int ch = 0; ch < nch; ++ch) std::printf(" %a", acc[ch]);
  if (wsum > 0.0) {
    uint32_t bits;
    if (nch == 3) {
      bits = amhip::blend_pack_bgr(amhip::blend_value(acc[0], wsum), amhip::blend_value(acc[1], wsum),
                                   amhip::blend_value(acc[2], wsum));
    } else {
      const float v = (float)amhip::blend_value(acc[0], wsum);
      std::memcpy(&bits, &v, sizeof(bits));
    }
    std::printf(" %08x", bits);
  }
  std::printf("\n");
  return 0;
}
