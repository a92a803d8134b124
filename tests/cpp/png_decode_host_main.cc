// png_decode_host_main.cc -- the host-only code of the PNG decoder (aerial_mapper_amd/csrc/
// amhip_png_decode_host.h: chunk parser, per-frame descriptor, IDAT spans) as a stand-alone program.
// tests/test_png_decode_host.py builds it with -fsanitize=address,undefined, runs it, and compares
// what it prints with tests/png_decode_reference.py.
//   png_decode_host_main desc <file>...            -> per file the descriptor, its palette, its IDAT
//                                                     spans and the CRC-32 of the joined stream, or
//                                                     "refused <text>"
//   png_decode_host_main fuzz <seed> <count> <file>...
//        -> per file `count` seeded mutations (a byte of the signature, of a chunk's length, type or
//           CRC, or of IHDR / PLTE changed, or the file cut short), each parsed from a heap buffer of
//           exactly its size; prints "<ok> <refused>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_png_decode_host.h"

using namespace amhip::pngd;

static bool read_file(const char* name, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(name, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  std::fclose(f);
  return true;
}

// what the upload relies on: every span lies inside the file, the spans add up to zlen, the stream
// bounds lie inside the joined stream, and the descriptor is one the kernels accept
static bool sound(const Parsed& p, size_t n) {
  size_t total = 0;
  for (const Span& s : p.idat) {
    if (s.begin > n || s.len > n - s.begin) return false;
    total += s.len;
  }
  const Frame& f = p.f;
  if (total != p.zlen || p.zlen < 6 || f.stream_begin != 2 || f.stream_end != p.zlen - 4) return false;
  if (f.width < 1 || f.width > 65535 || f.height < 1 || f.height > 65535) return false;
  if (f.bpp != bytes_per_pixel(f.colour_type) || f.bpp == 0) return false;
  if (f.raw_len != (uint64_t)f.height * (1 + (uint64_t)f.width * f.bpp)) return false;
  if (f.plte_entries < 0 || f.plte_entries > 256 || (f.colour_type == 3 && f.plte_entries == 0)) return false;
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
      Parsed p;
      std::printf("file %s\n", argv[a]);
      if (!parse(exact.data(), exact.size(), &p, text, sizeof(text))) {
        std::printf("refused %s\n", text);
        continue;
      }
      if (!sound(p, exact.size())) {
        std::printf("bad descriptor accepted\n");
        return 1;
      }
      const Frame& f = p.f;
      std::printf("size %d %d %d %d\n", f.width, f.height, f.colour_type, f.bpp);
      std::printf("raw %llu\n", (unsigned long long)f.raw_len);
      std::printf("zlib %llu %llu %llu %u\n", (unsigned long long)p.zlen, (unsigned long long)f.stream_begin,
                  (unsigned long long)f.stream_end, f.adler);
      std::printf("plte %d", f.plte_entries);
      for (int i = 0; i < 3 * f.plte_entries; ++i) std::printf(" %u", f.plte[i]);
      std::printf("\nidat %zu", p.idat.size());
      for (const Span& s : p.idat) std::printf(" %zu %zu", s.begin, s.len);
      std::vector<uint8_t> joined(p.zlen);
      concat(exact.data(), p, joined.data());
      std::printf("\nstream_crc %u\n", crc32(joined.data(), joined.size()));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "fuzz") && argc >= 5) {
    uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    const int count = std::atoi(argv[3]);
    long ok = 0, refused = 0;
    for (int a = 4; a < argc; ++a) {
      std::vector<uint8_t> file;
      if (!read_file(argv[a], &file)) return 1;
      Parsed p;
      if (!parse(file.data(), file.size(), &p, text, sizeof(text))) return 1;
      // the bytes a mutation may hit: the signature, IHDR and PLTE whole, and of every chunk its
      // length, type and CRC
      std::vector<size_t> targets;
      for (size_t i = 0; i < 8; ++i) targets.push_back(i);
      for (size_t at = 8; at + 12 <= file.size();) {
        const size_t L = be32(file.data() + at);
        if (L > file.size() - at - 12) break;
        const bool whole = !std::memcmp(file.data() + at + 4, "IHDR", 4) || !std::memcmp(file.data() + at + 4, "PLTE", 4);
        for (size_t i = 0; i < 8; ++i) targets.push_back(at + i);
        if (whole)
          for (size_t i = 0; i < L; ++i) targets.push_back(at + 8 + i);
        for (size_t i = 0; i < 4; ++i) targets.push_back(at + 8 + L + i);
        at += 12 + L;
      }
      // (also the first bytes of the first IDAT: the zlib header)
      if (!p.idat.empty() && p.idat[0].len >= 2) {
        targets.push_back(p.idat[0].begin);
        targets.push_back(p.idat[0].begin + 1);
      }
      for (int k = 0; k < count; ++k) {
        const uint64_t r = next(&seed);
        uint8_t* buf;
        size_t n;
        if (r & 1) {   // one byte changed
          n = file.size();
          buf = static_cast<uint8_t*>(std::malloc(n));
          std::memcpy(buf, file.data(), n);
          buf[targets[(r >> 8) % targets.size()]] = (uint8_t)(r >> 40);
        } else {       // the file cut short, anywhere
          n = (r >> 8) % (file.size() + 1);
          buf = static_cast<uint8_t*>(std::malloc(n ? n : 1));
          std::memcpy(buf, file.data(), n);
        }
        text[0] = 0;
        if (parse(buf, n, &p, text, sizeof(text))) {
          if (!sound(p, n)) {
            std::printf("bad descriptor accepted\n");
            return 1;
          }
          std::vector<uint8_t> joined(p.zlen);
          concat(buf, p, joined.data());   // (reads every span: ASan sees a span outside the file)
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
