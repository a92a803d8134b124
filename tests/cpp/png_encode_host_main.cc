// png_encode_host_main.cc -- the host-only code of the PNG encoder (aerial_mapper_amd/csrc/
// amhip_png_encode_host.h: static tables, block planner, container, CRC combine, bounds, argument
// checks) as a stand-alone program.  tests/test_png_encode_host.py builds it with
// -fsanitize=address,undefined, runs it, and compares what it prints and writes with
// tests/png_encode_reference.py and the committed streams.
//   png_encode_host_main tables                 -> the static tables, one line each
//   png_encode_host_main head W H C             -> signature + IHDR and IEND as hex, and the bounds
//   png_encode_host_main crc <file> <split>...  -> per split: the CRC-32 of the whole file put together from
//                                                  the registers of its two parts, and the CRC-32 computed straight
//   png_encode_host_main deflate <in> <out>...  -> per pair: the zlib stream of <in>'s bytes, written to <out>:
//                                                  tokens by rule 4 here, every block through plan_block();
//                                                  prints "<blocks> <stored> <fixed> <dynamic>"
//   png_encode_host_main ext <name>...          -> 1 / 0 per name: does it end in .png
//   png_encode_host_main args                   -> the refusal texts of the argument checks
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_png_encode_host.h"

using namespace amhip::pnge;

static const Tables kTables = make_tables();

static bool read_file(const char* name, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(name, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
  std::fclose(f);
  return true;
}

struct Bits {
  std::vector<uint8_t> out;
  uint64_t acc = 0;
  unsigned n = 0;
  uint64_t total = 0;
  void put(uint32_t v, unsigned len) {
    acc |= (uint64_t)v << n;
    n += len;
    total += len;
    while (n >= 8) {
      out.push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void windup() {
    if (n) {
      out.push_back((uint8_t)acc);
      total += 8 - n;
    }
    acc = 0;
    n = 0;
  }
};

// rule 4, position by position
static void tokens(const std::vector<uint8_t>& d, std::vector<uint16_t>* sym, std::vector<size_t>* pos) {
  const size_t n = d.size();
  size_t i = 0;
  while (i < n) {
    pos->push_back(i);
    if (i > 0 && i + 2 < n && d[i - 1] == d[i] && d[i] == d[i + 1] && d[i] == d[i + 2]) {
      size_t len = 0;
      while (len < kMaxMatch && i + len < n && d[i + len] == d[i - 1]) ++len;
      sym->push_back((uint16_t)(256 + len));
      i += len;
    } else {
      sym->push_back(d[i]);
      ++i;
    }
  }
}

static int deflate(const std::vector<uint8_t>& d, std::vector<uint8_t>* z, int counts[3]) {
  std::vector<uint16_t> sym;
  std::vector<size_t> pos;
  tokens(d, &sym, &pos);
  Bits w;
  w.put(0x78, 8);
  w.put(0x01, 8);
  const size_t nblocks = sym.size() / kBlockSymbols + 1;
  Work* work = new Work;        // (on the heap: the sanitizer sees every index)
  BlockCode* code = new BlockCode;
  for (size_t b = 0; b < nblocks; ++b) {
    const size_t lo = b * kBlockSymbols, hi = lo + kBlockSymbols < sym.size() ? lo + kBlockSymbols : sym.size();
    const size_t byte_lo = lo < sym.size() ? pos[lo] : d.size(), byte_hi = hi < sym.size() ? pos[hi] : d.size();
    const uint32_t last = b + 1 == nblocks;
    std::memset(work, 0, sizeof(*work));
    std::memset(code, 0, sizeof(*code));
    work->lfreq[kEndBlock] = 1;
    for (size_t k = lo; k < hi; ++k) {
      if (sym[k] < 256) {
        ++work->lfreq[sym[k]];
      } else {
        ++work->lfreq[kTables.length_code[sym[k] - 256 - 3] + kLiterals + 1];
        ++work->dfreq[0];
      }
    }
    plan_block(kTables, *work, (uint32_t)(byte_hi - byte_lo), code);
    ++counts[code->type];
    if (code->type == kStored) {
      w.put(last, 3);
      w.windup();
      w.put(code->stored_len, 16);
      w.put(code->stored_len ^ 0xFFFFu, 16);
      for (size_t k = byte_lo; k < byte_hi; ++k) w.put(d[k], 8);
      continue;
    }
    const uint64_t begin = w.total;
    w.put((code->type << 1) + last, 3);
    if (code->header_bits > (kHeaderWords - 1) * 32) return 2;
    for (uint32_t k = 0; k < code->header_bits; k += 32) {
      const uint32_t len = code->header_bits - k < 32 ? code->header_bits - k : 32;
      w.put(len == 32 ? code->header[k / 32] : code->header[k / 32] & ((1u << len) - 1), len);
    }
    uint64_t counted = 3 + code->header_bits;
    for (size_t k = lo; k < hi; ++k) {
      const uint32_t s = sym[k];
      counted += symbol_bits(kTables, code->llen, code->dlen0, s);
      if (s < 256) {
        w.put(code->lcode[s], code->llen[s]);
      } else {
        const uint32_t lc = s - 256 - 3, c = kTables.length_code[lc];
        w.put(code->lcode[c + kLiterals + 1], code->llen[c + kLiterals + 1]);
        if (kTables.extra_lbits[c]) w.put(lc - kTables.base_length[c], kTables.extra_lbits[c]);
        w.put(code->dcode0, code->dlen0);
      }
    }
    w.put(code->lcode[kEndBlock], code->llen[kEndBlock]);
    counted += code->llen[kEndBlock];
    // the planner's bit count is what the offsets pass places the next block by
    if (w.total - begin != code->bits || counted != code->bits) return 3;
  }
  delete work;
  delete code;
  w.windup();
  uint32_t s1 = 1, s2 = 0;
  for (uint8_t v : d) {
    s1 = (s1 + v) % 65521u;
    s2 = (s2 + s1) % 65521u;
  }
  const uint32_t adler = (s2 << 16) | s1;
  for (int k = 3; k >= 0; --k) w.put((adler >> (8 * k)) & 255u, 8);
  if (w.out.size() > zlib_bound(d.size())) return 4;
  *z = w.out;
  return 0;
}

template <typename T>
static void line(const char* name, const T* v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  const Tables& t = kTables;
  if (!std::strcmp(argv[1], "tables")) {
    line("length_code", t.length_code, 256);
    line("base_length", t.base_length, 29);
    line("extra_lbits", t.extra_lbits, 29);
    line("extra_dbits", t.extra_dbits, 30);
    line("extra_blbits", t.extra_blbits, 19);
    line("bl_order", t.bl_order, 19);
    line("fixed_llen", t.fixed_llen, 288);
    line("fixed_lcode", t.fixed_lcode, 288);
    line("fixed_dlen", t.fixed_dlen, 30);
    line("fixed_dcode", t.fixed_dcode, 30);
    line("crc", t.crc, 256);
    line("x2n", t.x2n, 32);
    return 0;
  }
  if (!std::strcmp(argv[1], "head") && argc == 5) {
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), c = std::atoi(argv[4]);
    uint8_t* head = new uint8_t[kFileHead];   // exactly their sizes, on the heap
    uint8_t* tail = new uint8_t[kFileTail];
    write_head_tail(t, w, h, c, head, tail);
    for (uint32_t i = 0; i < kFileHead; ++i) std::printf("%02x", head[i]);
    std::printf("\n");
    for (uint32_t i = 0; i < kFileTail; ++i) std::printf("%02x", tail[i]);
    std::printf("\n%llu %llu %llu\n", (unsigned long long)raw_len(w, h, c),
                (unsigned long long)zlib_bound(raw_len(w, h, c)), (unsigned long long)file_bound(w, h, c));
    delete[] head;
    delete[] tail;
    return 0;
  }
  if (!std::strcmp(argv[1], "crc") && argc >= 3) {
    std::vector<uint8_t> d;
    if (!read_file(argv[2], &d)) return 65;
    for (int a = 3; a < argc; ++a) {
      const size_t split = (size_t)std::strtoull(argv[a], nullptr, 10);
      if (split > d.size()) return 66;
      // the first part from the inverted register, the second from zero, as the frame kernel's lanes do
      const uint32_t ra = crc_run(t, 0xFFFFFFFFu, d.data(), split);
      const uint32_t rb = crc_run(t, 0, d.data() + split, d.size() - split);
      const uint32_t joined = ~(crc_shift(t, ra, d.size() - split) ^ rb);
      std::printf("%u %u\n", joined, crc32(t, d.data(), d.size()));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "deflate") && argc >= 4 && argc % 2 == 0) {
    for (int a = 2; a + 1 < argc; a += 2) {
      std::vector<uint8_t> d, z;
      if (!read_file(argv[a], &d)) return 65;
      int counts[3] = {0, 0, 0};
      const int rc = deflate(d, &z, counts);
      if (rc) return rc;
      FILE* f = std::fopen(argv[a + 1], "wb");
      if (!f || std::fwrite(z.data(), 1, z.size(), f) != z.size()) return 67;
      std::fclose(f);
      std::printf("%d %d %d %d\n", counts[0] + counts[1] + counts[2], counts[0], counts[1], counts[2]);
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "ext")) {
    for (int a = 2; a < argc; ++a) std::printf("%d\n", has_png_extension(argv[a]) ? 1 : 0);
    return 0;
  }
  if (!std::strcmp(argv[1], "args")) {
    auto show = [](const char* s) { std::printf("%s\n", s ? s : "ok"); };
    show(check_image_args(10, 10, 10, 1));
    show(check_image_args(10, 10, 10, 2));
    show(check_image_args(10, 0, 10, 1));
    show(check_image_args(10, 10, 65536, 1));
    show(check_image_args(29, 10, 10, 3));
    show(check_frames_args(2, 10, 10, 3, 30, 300));
    show(check_frames_args(0, 10, 10, 3, 30, 300));
    show(check_frames_args(2, 0, 10, 3, 30, 300));
    show(check_frames_args(2, 10, 65536, 3, 30, 300));
    show(check_frames_args(2, 10, 10, 4, 30, 300));
    show(check_frames_args(2, 10, 10, 3, 29, 300));
    show(check_frames_args(2, 10, 10, 3, 30, 299));
    show(check_frames_args(1, 10, 10, 3, 30, 0));
    return 0;
  }
  return 64;
}
