// jpeg_decode_host_main.cc -- the host-only code of the JPEG decoder (aerial_mapper_amd/csrc/
// amhip_jpeg_decode_host.h: header parser, per-frame descriptor, Huffman decode tables) as a
// stand-alone program.  tests/test_jpeg_decode_host.py builds it with -fsanitize=address,undefined,
// runs it, and compares what it prints with tests/jpeg_decode_reference.py.
//   jpeg_decode_host_main desc <file>...            -> per file the descriptor, its tables and the
//                                                      marks of its scan, or "refused <text>"
//   jpeg_decode_host_main fuzz <seed> <count> <file>...
//        -> per file `count` seeded mutations of its header (one byte changed, or the file cut
//           short), each parsed from a heap buffer of exactly its size; prints "<ok> <refused>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_jpeg_decode_host.h"

using namespace amhip::jpegd;

static bool read_file(const char* name, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(name, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  std::fclose(f);
  return true;
}

static void print_table(const char* name, const HuffTable& t) {
  std::printf("%s.look", name);
  for (int i = 0; i < 256; ++i) std::printf(" %u", t.look[i]);
  std::printf("\n%s.maxcode", name);
  for (int i = 0; i < 18; ++i) std::printf(" %d", t.maxcode[i]);
  std::printf("\n%s.valoffset", name);
  for (int i = 0; i < 17; ++i) std::printf(" %d", t.valoffset[i]);
  std::printf("\n%s.huffval", name);
  for (int i = 0; i < 256; ++i) std::printf(" %u", t.huffval[i]);
  std::printf("\n");
}

// What the entropy kernel relies on when it follows a run of 0xFF inside the scan: the scan ends
// at a 0xFF whose run leads to EOI inside the file, and every run of 0xFF in front of that is
// followed, still inside the scan, by 0x00 (a stuffed byte) or an RSTn.  Counts the RSTn, the
// stuffed bytes and the fill bytes (all but the last 0xFF of a run); false: a bound is broken.
static bool scan_marks(const uint8_t* file, size_t n, const Frame& f, long* rst, long* stuffed, long* fill) {
  *rst = *stuffed = *fill = 0;
  if (f.scan_begin > f.scan_end || f.scan_end + 2 > n || file[f.scan_end] != 0xFF) return false;
  size_t e = (size_t)f.scan_end;
  while (e < n && file[e] == 0xFF) ++e;
  if (e >= n || file[e] != 0xD9) return false;
  for (size_t p = (size_t)f.scan_begin; p < f.scan_end; ++p) {
    if (file[p] != 0xFF) continue;
    size_t k = p + 1;
    while (k < f.scan_end && file[k] == 0xFF) ++k;
    if (k >= f.scan_end) return false;
    if (file[k] == 0x00) ++*stuffed;
    else if (file[k] >= 0xD0 && file[k] <= 0xD7) ++*rst;
    else return false;
    *fill += (long)(k - p - 1);
    p = k;
  }
  return true;
}

static uint64_t next(uint64_t* s) {   // splitmix64
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  char text[160];
  if (!std::strcmp(argv[1], "desc")) {
    for (int a = 2; a < argc; ++a) {
      std::vector<uint8_t> file;
      if (!read_file(argv[a], &file)) return 1;
      // (an exactly sized heap copy: one byte read behind it is an ASan report)
      std::vector<uint8_t> exact(file.begin(), file.end());
      Frame f;
      std::printf("file %s\n", argv[a]);
      if (!parse(exact.data(), exact.size(), &f, text, sizeof(text))) {
        std::printf("refused %s\n", text);
        continue;
      }
      std::printf("size %d %d %d\n", f.width, f.height, f.ncomp);
      std::printf("mcu %d %d %d %d %d\n", f.hmax, f.vmax, f.mcux, f.mcuy, f.restart);
      std::printf("scan %llu %llu\n", (unsigned long long)f.scan_begin, (unsigned long long)f.scan_end);
      for (int c = 0; c < f.ncomp; ++c) {
        std::printf("comp %d %d %d %d %d %u %d %d\n", c, f.comp_h[c], f.comp_v[c], f.comp_bw[c], f.comp_bh[c],
                    f.comp_base[c], f.td[c], f.ta[c]);
        std::printf("quant %d", c);
        for (int i = 0; i < 64; ++i) std::printf(" %u", f.quant[c][i]);
        std::printf("\n");
      }
      std::printf("blocks %u\n", f.comp_base[f.ncomp]);
      long rst, stuffed, fill;
      if (!scan_marks(exact.data(), exact.size(), f, &rst, &stuffed, &fill)) {
        std::printf("bad scan bounds accepted\n");
        return 1;
      }
      std::printf("marks %ld %ld %ld\n", rst, stuffed, fill);
      for (int c = 0; c < f.ncomp; ++c) {
        char name[16];
        std::snprintf(name, sizeof(name), "dc%d", f.td[c]);
        print_table(name, f.dc[f.td[c]]);
        std::snprintf(name, sizeof(name), "ac%d", f.ta[c]);
        print_table(name, f.ac[f.ta[c]]);
      }
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "fuzz") && argc >= 5) {
    uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    const int count = std::atoi(argv[3]);
    long ok = 0, refused = 0, rst, stuffed, fill;
    for (int a = 4; a < argc; ++a) {
      std::vector<uint8_t> file;
      if (!read_file(argv[a], &file)) return 1;
      Frame f;
      if (!parse(file.data(), file.size(), &f, text, sizeof(text))) return 1;
      const size_t header = (size_t)f.scan_begin;
      for (int k = 0; k < count; ++k) {
        const uint64_t r = next(&seed);
        uint8_t* buf;
        size_t n;
        if (r & 1) {   // one header byte changed
          n = file.size();
          buf = static_cast<uint8_t*>(std::malloc(n));
          std::memcpy(buf, file.data(), n);
          buf[(r >> 8) % header] = (uint8_t)(r >> 40);
        } else {       // the file cut short, anywhere from nothing to just behind the header
          n = (r >> 8) % (header + 4);
          buf = static_cast<uint8_t*>(std::malloc(n ? n : 1));
          std::memcpy(buf, file.data(), n);
        }
        text[0] = 0;
        if (parse(buf, n, &f, text, sizeof(text))) {
          // what the kernels rely on
          if (f.scan_begin > f.scan_end || f.scan_end + 2 > n || f.mcux < 1 || f.mcuy < 1 ||
              (f.ncomp != 1 && f.ncomp != 3) || f.comp_base[f.ncomp] == 0 ||
              !scan_marks(buf, n, f, &rst, &stuffed, &fill)) {
            std::printf("bad descriptor accepted\n");
            return 1;
          }
          ++ok;
        } else {
          if (!text[0]) {
            std::printf("refusal without a text\n");
            return 1;
          }
          ++refused;
        }
        std::free(buf);
      }
    }
    std::printf("%ld %ld\n", ok, refused);
    return 0;
  }
  return 2;
}
