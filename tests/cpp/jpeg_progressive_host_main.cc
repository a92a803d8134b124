// jpeg_progressive_host_main.cc -- the host parser of the JPEG decoder (aerial_mapper_amd/csrc/
// amhip_jpeg_decode_host.h) on progressive files, as a stand-alone program.
// tests/test_jpeg_progressive_host.py builds it with -fsanitize=address,undefined, runs it, and
// compares what it prints with tests/jpeg_progressive_reference.py.
//   jpeg_progressive_host_main desc <file>...   -> per file the frame and its scan list, or
//                                                  "refused <text>"
//   jpeg_progressive_host_main fuzz <seed> <count> <file>...
//        -> per file `count` seeded mutations (one byte of a marker segment changed -- headers, DHT,
//           DQT, DRI, SOS -- or the file cut short anywhere), each parsed from a heap buffer of exactly
//           its size; prints "<ok> <refused>"
// Every accepted file, mutated or not, is held to what the entropy kernel relies on (check()).
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

// FNV-1a over the table's numbers, 32 bits each
static uint32_t table_hash(const HuffTable& t) {
  uint32_t h = 2166136261u;
  auto add = [&](uint32_t v) {
    for (int k = 0; k < 4; ++k) {
      h = (h ^ ((v >> (8 * k)) & 255u)) * 16777619u;
    }
  };
  for (int i = 0; i < 256; ++i) add(t.look[i]);
  for (int i = 0; i < 18; ++i) add((uint32_t)t.maxcode[i]);
  for (int i = 0; i < 17; ++i) add((uint32_t)t.valoffset[i]);
  for (int i = 0; i < 256; ++i) add(t.huffval[i]);
  return h;
}

// What the walk relies on: the scans' byte ranges are ordered, disjoint, inside the file, and each
// ends at a 0xFF whose run of 0xFF leads to a marker code inside the file; inside a range every run of
// 0xFF is followed, still inside it, by 0x00 or an RSTn; the scan's fields are in their ranges; its
// block counts fit the frame's planes; every table it names exists;
// and the script brings every coefficient of every component to bit 0, each scan continuing where
// the coefficient stands.  nullptr: all of it holds.
static const char* check(const uint8_t* file, size_t n, const Frame& f, const Progressive& p) {
  if (!f.progressive) return p.scans.empty() && p.tables.empty() ? nullptr : "a scan list beside a baseline frame";
  if (p.scans.empty() || f.scan_count != p.scans.size()) return "scan count";
  if (f.ncomp != 1 && f.ncomp != 3) return "components";
  if (f.mcux < 1 || f.mcuy < 1 || f.comp_base[f.ncomp] == 0) return "layout";
  int bits[3][64];
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) bits[c][k] = -1;
  uint64_t at = 2;
  for (size_t i = 0; i < p.scans.size(); ++i) {
    const Scan& s = p.scans[i];
    if (s.begin < at + 8 || s.begin > s.end || s.end + 2 > n) return "scan range";
    at = s.end;
    if (file[s.end] != 0xFF) return "scan end is no 0xFF";
    size_t e = (size_t)s.end;
    while (e < n && file[e] == 0xFF) ++e;
    if (e >= n || file[e] == 0x00 || (file[e] >= 0xD0 && file[e] <= 0xD7)) return "scan end is no marker";
    for (size_t q = (size_t)s.begin; q < s.end; ++q) {
      if (file[q] != 0xFF) continue;
      size_t k = q + 1;
      while (k < s.end && file[k] == 0xFF) ++k;
      if (k >= s.end) return "a run of 0xFF reaches the scan's end";
      if (file[k] != 0x00 && !(file[k] >= 0xD0 && file[k] <= 0xD7)) return "a marker inside the scan";
      q = k;
    }
    if (s.ns < 1 || s.ns > f.ncomp) return "Ns";
    if (s.ss < 0 || s.se > 63 || s.se < s.ss || (s.ss == 0 && s.se != 0) || (s.ss > 0 && s.ns != 1)) return "band";
    if (s.al < 0 || s.al > 13 || s.ah < 0 || s.ah > 14 || (s.ah && s.al != s.ah - 1)) return "Ah / Al";
    if (s.restart < 0 || s.restart > 65535) return "restart";
    if (s.nx < 1 || s.ny < 1) return "MCU counts";
    for (int k = 0; k < s.ns; ++k) {
      const int c = s.comp[k];
      if (c < 0 || c >= f.ncomp || (k && c <= s.comp[k - 1])) return "component";
      const int h = s.ns > 1 ? f.comp_h[c] : 1, v = s.ns > 1 ? f.comp_v[c] : 1;
      if (s.nx * h > f.comp_bw[c] || s.ny * v > f.comp_bh[c]) return "blocks outside the plane";
      const bool wants_dc = s.ss == 0 && s.ah == 0;
      if (wants_dc != (s.dc_tbl[k] >= 0)) return "DC table";
      if (s.dc_tbl[k] >= (int)p.tables.size()) return "DC table index";
      if (s.ss > 0 && bits[c][0] < 0) return "AC before DC";
      for (int z = s.ss; z <= s.se; ++z) {
        if (s.ah == 0 ? bits[c][z] >= 0 : bits[c][z] != s.ah) return "progression";
        bits[c][z] = s.al;
      }
    }
    for (int k = s.ns; k < 3; ++k)
      if (s.dc_tbl[k] != -1) return "DC table of no component";
    if ((s.ss > 0) != (s.ac_tbl >= 0) || s.ac_tbl >= (int)p.tables.size()) return "AC table";
  }
  for (int c = 0; c < f.ncomp; ++c)
    for (int z = 0; z < 64; ++z)
      if (bits[c][z] != 0) return "a coefficient short of bit 0";
  if (f.scan_begin != p.scans.back().begin || f.scan_end != p.scans.back().end) return "frame's scan range";
  return nullptr;
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
      Progressive p;
      std::printf("file %s\n", argv[a]);
      if (!parse(exact.data(), exact.size(), &f, &p, text, sizeof(text))) {
        std::printf("refused %s\n", text);
        continue;
      }
      if (const char* why = check(exact.data(), exact.size(), f, p)) {
        std::printf("bad descriptor accepted: %s\n", why);
        return 1;
      }
      // (the five-argument parse gives the same frame)
      Frame g;
      if (!parse(exact.data(), exact.size(), &g, text, sizeof(text)) || std::memcmp(&f, &g, sizeof(f))) {
        std::printf("the two parses differ\n");
        return 1;
      }
      std::printf("size %d %d %d %d\n", f.width, f.height, f.ncomp, f.progressive);
      std::printf("mcu %d %d %d %d\n", f.hmax, f.vmax, f.mcux, f.mcuy);
      for (int c = 0; c < f.ncomp; ++c) {
        std::printf("comp %d %d %d %d %d %u\n", c, f.comp_h[c], f.comp_v[c], f.comp_bw[c], f.comp_bh[c], f.comp_base[c]);
        std::printf("quant %d", c);
        for (int i = 0; i < 64; ++i) std::printf(" %u", f.quant[c][i]);
        std::printf("\n");
      }
      std::printf("scans %zu %zu\n", p.scans.size(), p.tables.size());
      for (size_t i = 0; i < p.scans.size(); ++i) {
        const Scan& s = p.scans[i];
        std::printf("scan %zu %llu %llu %d %d %d %d %d %d %d %d %d %d %d", i, (unsigned long long)s.begin,
                    (unsigned long long)s.end, s.ns, s.comp[0], s.comp[1], s.comp[2], s.ss, s.se, s.ah, s.al,
                    s.restart, s.nx, s.ny);
        // the tables by what they hold (0: none)
        for (int k = 0; k < 3; ++k) std::printf(" %u", s.dc_tbl[k] >= 0 ? table_hash(p.tables[s.dc_tbl[k]]) : 0u);
        std::printf(" %u\n", s.ac_tbl >= 0 ? table_hash(p.tables[s.ac_tbl]) : 0u);
      }
      // each distinct table once
      for (size_t i = 0; i < p.tables.size(); ++i)
        for (size_t j = 0; j < i; ++j)
          if (!std::memcmp(&p.tables[i], &p.tables[j], sizeof(HuffTable))) {
            std::printf("a table stored twice\n");
            return 1;
          }
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
      Frame f;
      Progressive p;
      if (!parse(file.data(), file.size(), &f, &p, text, sizeof(text))) return 1;
      // the bytes outside the entropy-coded segments: the header and what lies between the scans
      std::vector<size_t> outside;
      size_t at = 2;
      for (const Scan& s : p.scans) {
        for (size_t q = at; q < s.begin; ++q) outside.push_back(q);
        at = (size_t)s.end;
      }
      if (p.scans.empty())
        for (size_t q = 2; q < f.scan_begin; ++q) outside.push_back(q);
      for (int k = 0; k < count; ++k) {
        const uint64_t r = next(&seed);
        uint8_t* buf;
        size_t n;
        if (r & 3) {   // one byte of a marker segment changed
          n = file.size();
          buf = static_cast<uint8_t*>(std::malloc(n));
          std::memcpy(buf, file.data(), n);
          buf[outside[(r >> 8) % outside.size()]] = (uint8_t)(r >> 40);
        } else {       // the file cut short, anywhere
          n = (r >> 8) % (file.size() + 1);
          buf = static_cast<uint8_t*>(std::malloc(n ? n : 1));
          std::memcpy(buf, file.data(), n);
        }
        text[0] = 0;
        if (parse(buf, n, &f, &p, text, sizeof(text))) {
          if (const char* why = check(buf, n, f, p)) {
            if (f.progressive) {
              std::printf("bad descriptor accepted: %s\n", why);
              return 1;
            }
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
