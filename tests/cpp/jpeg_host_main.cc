// jpeg_host_main.cc -- the host-only code of the JPEG encoder (aerial_mapper_amd/csrc/
// amhip_jpeg_host.h: table scaling, canonical Huffman codes, header writer, size bound, argument
// rules) as a stand-alone program.  tests/test_jpeg_host.py builds it with
// -fsanitize=address,undefined, runs it, and compares what it prints with tests/jpeg_reference.py.
//   jpeg_host_main header <width> <height> <channels> <quality>   -> the header segments, hex
//   jpeg_host_main huff                                            -> every code | length << 16
//   jpeg_host_main bound <width> <height> <channels>               -> the worst-case file size
//   jpeg_host_main check <step> <width> <height> <channels> <quality> -> "ok" or the refusal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amhip_jpeg_host.h"

using namespace amhip::jpeg;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "header") && argc == 6) {
    // a buffer of exactly the size the writer asks for: one byte more written is an ASan report
    std::vector<uint8_t> buf(kMaxHeaderBytes);
    const size_t n = write_header(buf.data(), buf.size(), std::atoi(argv[2]), std::atoi(argv[3]),
                                  std::atoi(argv[4]), std::atoi(argv[5]));
    if (!n || n > buf.size()) return 1;
    // and a buffer one byte short is refused, untouched
    std::vector<uint8_t> small(kMaxHeaderBytes - 1, 0x5A);
    if (write_header(small.data(), small.size(), 8, 8, 3, 95) != 0) return 1;
    for (uint8_t b : small)
      if (b != 0x5A) return 1;
    for (size_t i = 0; i < n; ++i) std::printf("%02x", buf[i]);
    std::printf("\n");
    return 0;
  }
  if (!std::strcmp(argv[1], "huff")) {
    constexpr HuffTables t = make_huff_tables();
    for (int tbl = 0; tbl < 2; ++tbl) {
      for (int i = 0; i < 12; ++i) std::printf("%u ", t.dc[tbl][i]);
      for (int i = 0; i < 256; ++i) std::printf("%u ", t.ac[tbl][i]);
      std::printf("\n");
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "bound") && argc == 5) {
    std::printf("%zu\n", file_bound(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  if (!std::strcmp(argv[1], "check") && argc == 7) {
    const char* why = check_image_args((size_t)std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                       std::atoi(argv[5]), std::atoi(argv[6]));
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  return 2;
}
