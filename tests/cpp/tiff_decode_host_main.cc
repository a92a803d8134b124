// tiff_decode_host_main.cc -- the host-only code of the GeoTIFF reader (aerial_mapper_amd/csrc/
// amhip_tiff_decode_host.h: the parser of the first IFD and the chunk table) as a stand-alone program.
// tests/test_geotiff_read_host.py builds it with -fsanitize=address,undefined, runs it, and compares
// what it prints with tests/geotiff_read_reference.py.
//   tiff_decode_host_main desc <file>...   -> per file the descriptor and the chunk table, or
//                                             "refused <text>"
//   tiff_decode_host_main fuzz <seed> <count> <file>...
//        -> per file `count` seeded mutations (a byte of the header, of the IFD or of an out-of-line
//           value changed, or the file cut short), each parsed from a heap buffer of exactly its size,
//           every accepted chunk read through; prints "<ok> <refused>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_tiff_decode_host.h"

using namespace amhip::tiffd;

static bool read_file(const char* name, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(name, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  std::fclose(f);
  return true;
}

// what the upload relies on: the layout implies the chunk table, every chunk lies inside the file
// and is long enough for what the device reads of it; *sum: every chunk's bytes, read
static bool sound(const Parsed& p, const uint8_t* file, size_t n, unsigned* sum) {
  if (p.width < 1 || p.width > (1 << 20) || p.height < 1 || p.height > (1 << 20)) return false;
  if (p.kind < 0 || p.kind > 4 || p.bands != (p.kind == kRgb8 ? 3 : 1)) return false;
  if (p.chunk_w < 1 || p.chunk_h < 1) return false;
  if (p.tiled && (p.chunk_w % 16 || p.chunk_h % 16)) return false;
  if (!p.tiled && (p.chunk_w != (uint32_t)p.width || p.across != 1)) return false;
  if ((uint64_t)p.across * p.chunk_w < (uint64_t)p.width || (uint64_t)p.down * p.chunk_h < (uint64_t)p.height) return false;
  if (p.chunks.size() != (size_t)p.across * p.down) return false;
  if (p.predictor < 1 || p.predictor > 3 || (p.predictor == 3 && p.kind != kF32)) return false;
  uint64_t rows = 0;
  for (size_t t = 0; t < p.chunks.size(); ++t) {
    const Chunk& c = p.chunks[t];
    if (c.offset > n || c.count > n - c.offset) return false;
    if (c.raw_len != (uint64_t)c.rows * p.chunk_w * (uint64_t)pixel_bytes(p.kind)) return false;
    if (p.compression == 1 ? c.count != c.raw_len : c.count < 6) return false;
    for (uint64_t k = 0; k < c.count; ++k) *sum += file[c.offset + k];   // (ASan sees a chunk outside the file)
    if (t % p.across == 0) rows += c.rows;
  }
  if (p.tiled ? rows != (uint64_t)p.down * p.chunk_h : rows != (uint64_t)p.height) return false;
  if (p.has_geo && !(p.gt[1] > 0.0 && p.gt[5] < 0.0)) return false;
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
  char text[200];
  unsigned sum = 0;
  if (!std::strcmp(argv[1], "desc")) {
    for (int a = 2; a < argc; ++a) {
      std::vector<uint8_t> file;
      if (!read_file(argv[a], &file)) return 1;
      // (an exactly sized heap copy: one byte read behind it is an ASan report)
      std::vector<uint8_t> exact(file.begin(), file.end());
      Parsed p;
      std::printf("file %s\n", argv[a]);
      text[0] = 0;
      if (!parse(exact.data(), exact.size(), &p, text, sizeof(text))) {
        std::printf("refused %s\n", text);
        continue;
      }
      if (!sound(p, exact.data(), exact.size(), &sum)) {
        std::printf("bad descriptor accepted\n");
        return 1;
      }
      std::printf("size %d %d %d %d\n", p.width, p.height, p.bands, p.kind);
      std::printf("layout %d %u %u %u %u\n", p.tiled, p.chunk_w, p.chunk_h, p.across, p.down);
      std::printf("coding %d %d\n", p.compression, p.predictor);
      std::printf("geo %d %d %d\n", p.has_geo, p.epsg, p.raster_type);
      std::printf("gt");
      for (int k = 0; k < 6; ++k) {
        uint64_t bits;
        std::memcpy(&bits, &p.gt[k], 8);
        std::printf(" %llu", (unsigned long long)bits);
      }
      uint64_t nd;
      std::memcpy(&nd, &p.nodata, 8);
      std::printf("\nnodata %d %llu\n", p.has_nodata, (unsigned long long)nd);
      std::printf("chunks %zu", p.chunks.size());
      for (const Chunk& c : p.chunks)
        std::printf(" %llu %llu %u", (unsigned long long)c.offset, (unsigned long long)c.count, c.rows);
      std::printf("\n");
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
      // the bytes a mutation may hit: everything in front of the first chunk and behind the last
      // (header, IFD, out-of-line values wherever the writer put them), and every chunk's first two
      size_t lo = file.size(), hi = 0;
      std::vector<size_t> targets;
      for (const Chunk& c : p.chunks) {
        if (c.offset < lo) lo = (size_t)c.offset;
        if (c.offset + c.count > hi) hi = (size_t)(c.offset + c.count);
        targets.push_back((size_t)c.offset);
        targets.push_back((size_t)c.offset + 1);
      }
      for (size_t i = 0; i < lo; ++i) targets.push_back(i);
      for (size_t i = hi; i < file.size(); ++i) targets.push_back(i);
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
          if (!sound(p, buf, n, &sum)) {
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
    std::printf("%ld %ld %u\n", ok, refused, sum & 1u);
    return 0;
  }
  return 2;
}
