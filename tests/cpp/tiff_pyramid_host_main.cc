// tiff_pyramid_host_main.cc -- the host-only parts of the GeoTIFF pyramid as a
// stand-alone program: the multi-IFD container of amhip_tiff_host.h and the chain walk and level
// rules of amhip_tiff_decode_host.h.  tests/test_geotiff_pyramid_host.py compiles it with
// -fsanitize=address,undefined and runs it as a program.  Every file is parsed from a heap buffer
// of exactly its size, so a read past the end is a report.
//
//   levels FILE...                      per file: "file", "levels N" or "refused TEXT", then per level
//                                       "level K: ..." or "level K refused TEXT"
//   mutate SEED ROUNDS FILE...          seeded byte mutations and truncations of every file, all levels
//                                       parsed; prints the number of parses and of refusals
//   build W H KIND TILE OVERVIEWS       the container for made-up tile sizes (7 + t % 5 + 3 * level):
//                                       "head HEX", "level_at ..", "bytes N", "bound N"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_tiff_decode_host.h"
#include "amhip_tiff_host.h"

using namespace amhip;

static std::vector<uint8_t> read_all(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

static uint64_t bits_of(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}

// every level of the file from an exact-size heap copy; returns the refusals seen; print: the records
static int all_levels(const uint8_t* bytes, size_t len, bool print) {
  uint8_t* file = static_cast<uint8_t*>(std::malloc(len ? len : 1));
  if (len) std::memcpy(file, bytes, len);
  char text[400];
  int refused = 0;
  std::vector<tiffd::Ifd> ifds;
  if (!tiffd::walk_chain(file, len, &ifds, text, sizeof(text))) {
    if (print) std::printf("refused %s\n", text);
    std::free(file);
    return 1;
  }
  const size_t n = tiffd::levels_of(ifds).size();
  if (print) std::printf("levels %zu\n", n);
  for (size_t k = 0; k < n; ++k) {
    tiffd::Parsed P;
    int nl = 0;
    if (!tiffd::parse_level(file, len, (int)k, &P, &nl, text, sizeof(text))) {
      ++refused;
      if (print) std::printf("level %zu refused %s\n", k, text);
      continue;
    }
    if ((size_t)nl != n) std::abort();
    uint64_t sum = 0;
    for (const tiffd::Chunk& c : P.chunks) {
      if (c.offset > len || c.count > len - c.offset) std::abort();   // the parser's promise
      sum += file[c.offset] + (c.count ? file[c.offset + c.count - 1] : 0);   // ... taken at its word
    }
    if (print)
      std::printf("level %zu: %d %d %d %d %u %u %llu %llu %llu %llu %d %zu %llu\n", k, P.width, P.height, P.kind, P.tiled,
                  P.chunk_w, P.chunk_h, (unsigned long long)bits_of(P.gt[0]), (unsigned long long)bits_of(P.gt[1]),
                  (unsigned long long)bits_of(P.gt[3]), (unsigned long long)bits_of(P.gt[5]), P.has_nodata, P.chunks.size(),
                  (unsigned long long)sum);
  }
  if (tiffd::parse_level(file, len, (int)n, nullptr, nullptr, text, sizeof(text))) std::abort();   // no such level
  std::free(file);
  return refused;
}

static uint32_t next_random(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 8;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "levels")) {
    for (int a = 2; a < argc; ++a) {
      const std::vector<uint8_t> f = read_all(argv[a]);
      std::printf("file %s\n", argv[a]);
      all_levels(f.data(), f.size(), true);
    }
    return 0;
  }
  if (argc >= 5 && !std::strcmp(argv[1], "mutate")) {
    uint32_t seed = (uint32_t)std::atoi(argv[2]);
    const int rounds = std::atoi(argv[3]);
    long parses = 0, refusals = 0;
    for (int a = 4; a < argc; ++a) {
      const std::vector<uint8_t> f = read_all(argv[a]);
      // the head of the file is where the IFDs and tables are: most mutations go there
      const size_t head = f.size() < 1024 ? f.size() : 1024;
      for (int r = 0; r < rounds; ++r) {
        std::vector<uint8_t> m = f;
        const uint32_t what = next_random(&seed) % 4;
        if (what == 0) {
          m.resize(next_random(&seed) % (f.size() + 1));   // a truncation
        } else {
          const int n = 1 + (int)(next_random(&seed) % 3);
          for (int k = 0; k < n; ++k) {
            const size_t at = next_random(&seed) % (what == 1 ? head : f.size());
            m[at] = what == 3 ? (uint8_t)(m[at] ^ (1u << (next_random(&seed) % 8))) : (uint8_t)next_random(&seed);
          }
        }
        refusals += all_levels(m.data(), m.size(), false) ? 1 : 0;
        ++parses;
      }
    }
    std::printf("parses %ld refusals %ld\n", parses, refusals);
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "build")) {
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), kind = std::atoi(argv[4]), tile = std::atoi(argv[5]);
    int n = 0;
    if (tiff::check_raster(w, h, kind, tile)) {
      std::printf("refused raster\n");
      return 0;
    }
    if (const char* why = tiff::check_overviews(w, h, tile, std::atoi(argv[6]), &n)) {
      std::printf("refused %s\n", why);
      return 0;
    }
    const std::vector<tiff::Level> levels = tiff::make_levels(w, h, tile, n);
    std::vector<uint64_t> counts;
    for (size_t k = 0; k < levels.size(); ++k)
      for (uint64_t t = 0; t < levels[k].ntiles; ++t) counts.push_back(7 + t % 5 + 3 * k);
    const double gt[6] = {464500.25, 0.5, 0.0, 5272800.75, 0.0, -0.5};
    tiff::Container c;
    if (!tiff::build_pyramid(levels, kind, tile, tiff::make_geo_tags(gt, 32, 1), counts.data(), &c)) {
      std::printf("refused size\n");
      return 0;
    }
    std::printf("head ");
    for (uint8_t b : c.head) std::printf("%02x", b);
    std::printf("\nlevel_at");
    for (uint64_t v : c.level_at) std::printf(" %llu", (unsigned long long)v);
    std::printf("\nbytes %llu\nbound %llu\n", (unsigned long long)c.file_bytes,
                (unsigned long long)tiff::file_bound_ovr(w, h, kind, tile, n));
    if (c.head.size() > tiff::file_bound_ovr(w, h, kind, tile, n)) std::abort();
    // the head is a file of its own as far as the chain goes: walk it
    std::vector<tiffd::Ifd> ifds;
    char text[200];
    if (!tiffd::walk_chain(c.head.data(), c.head.size(), &ifds, text, sizeof(text)) || ifds.size() != levels.size())
      std::abort();
    return 0;
  }
  std::fprintf(stderr, "usage: levels FILE... | mutate SEED ROUNDS FILE... | build W H KIND TILE OVERVIEWS\n");
  return 2;
}
