// amhip_png_encode_host.h -- the part of the PNG encoder (amhip_png_encode.hip) that needs no
// device: zlib's static tables, the block planner (_tr_flush_block up to the choice of the block
// type, its code tables and its dynamic header), the signature / IHDR / IEND writer, the size bound,
// the CRC-32 table with the x^(2^k) mod P constants of the CRC combine, and the argument checks.  No
// HIP in here: tests/cpp/png_encode_host_main.cc compiles it alone under the address and
// undefined-behaviour sanitizers.  The one concession is AMHIP_PNGE_HD, which marks the functions
// the plan kernel calls as well; it is empty for a host compiler.
//
// The file is defined in DESIGN 4.15: filter Sub on every row; zlib level 1, strategy Z_RLE,
// window 15, memLevel 8; IDAT payloads of 8192 bytes.
#ifndef AMHIP_PNG_ENCODE_HOST_H_
#define AMHIP_PNG_ENCODE_HOST_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define AMHIP_PNGE_HD __host__ __device__ __forceinline__
#else
#define AMHIP_PNGE_HD inline
#endif

namespace amhip {
namespace pnge {

constexpr int kLiterals = 256, kEndBlock = 256, kLCodes = 286, kDCodes = 30, kBlCodes = 19;
constexpr int kHeapSize = 2 * kLCodes + 1;
constexpr int kRep3_6 = 16, kRepZ3_10 = 17, kRepZ11_138 = 18;
constexpr uint32_t kBlockSymbols = 16383;   // lit_bufsize - 1 at memLevel 8
constexpr uint32_t kIdatBytes = 8192;       // libpng's default zbuffer
constexpr uint32_t kMaxMatch = 258;
constexpr uint32_t kFileHead = 33;          // signature + IHDR chunk
constexpr uint32_t kFileTail = 12;          // IEND chunk
// a dynamic block's header behind its three type bits: 14 + 19 * 3 bits, then at most 14 bits (a
// 7-bit code and 7 extra bits) for each of the 286 + 30 lengths
constexpr uint32_t kHeaderWords = (14 + 57 + 316 * 14 + 31) / 32 + 1;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

enum BlockType : uint32_t { kStored = 0, kFixed = 1, kDynamic = 2 };

// tr_static_init()'s tables, the CRC table and x^(2^k) mod P (zlib's x2n_table)
struct Tables {
  uint8_t length_code[256];    // _length_code: match length - 3 -> length code 0..28
  uint8_t base_length[29];
  uint8_t extra_lbits[29];
  uint8_t extra_dbits[30];
  uint8_t extra_blbits[19];
  uint8_t bl_order[19];
  uint8_t fixed_llen[288];
  uint16_t fixed_lcode[288];   // bit-reversed
  uint8_t fixed_dlen[30];
  uint16_t fixed_dcode[30];
  uint32_t crc[256];
  uint32_t x2n[32];
};

constexpr uint32_t bi_reverse(uint32_t code, int len) {
  uint32_t res = 0;
  for (int i = 0; i < len; ++i) {
    res = (res << 1) | (code & 1u);
    code >>= 1;
  }
  return res;
}

// a(x) * b(x) mod P, reflected (zlib's multmodp)
constexpr uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

constexpr Tables make_tables() {
  Tables t = {};
  constexpr uint8_t lbits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 29; ++i) t.extra_lbits[i] = lbits[i];
  for (int i = 0; i < 30; ++i) t.extra_dbits[i] = (uint8_t)(i < 2 ? 0 : i / 2 - 1);
  for (int i = 0; i < 19; ++i) t.extra_blbits[i] = (uint8_t)(i < 16 ? 0 : i == 16 ? 2 : i == 17 ? 3 : 7);
  for (int i = 0; i < 19; ++i) t.bl_order[i] = order[i];
  int length = 0;
  for (int code = 0; code < 28; ++code) {
    t.base_length[code] = (uint8_t)length;
    for (int n = 0; n < (1 << lbits[code]); ++n) t.length_code[length++] = (uint8_t)code;
  }
  t.length_code[255] = 28;
  t.base_length[28] = 0;
  uint32_t count[16] = {};
  for (int n = 0; n < 288; ++n) {
    t.fixed_llen[n] = (uint8_t)(n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8);
    ++count[t.fixed_llen[n]];
  }
  uint32_t next[16] = {};
  uint32_t code = 0;
  for (int bits = 1; bits < 16; ++bits) {
    code = (code + count[bits - 1]) << 1;
    next[bits] = code;
  }
  for (int n = 0; n < 288; ++n) t.fixed_lcode[n] = (uint16_t)bi_reverse(next[t.fixed_llen[n]]++, t.fixed_llen[n]);
  for (int n = 0; n < 30; ++n) {
    t.fixed_dlen[n] = 5;
    t.fixed_dcode[n] = (uint16_t)bi_reverse((uint32_t)n, 5);
  }
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? kCrcPoly ^ (c >> 1) : c >> 1;
    t.crc[i] = c;
  }
  t.x2n[0] = 1u << 30;   // x^1
  for (int n = 1; n < 32; ++n) t.x2n[n] = multmodp(t.x2n[n - 1], t.x2n[n - 1]);
  return t;
}

// x^(8 * bytes) mod P (zlib's x2nmodp(bytes, 3))
AMHIP_PNGE_HD uint32_t x8nmodp(const Tables& t, uint64_t bytes) {
  uint32_t p = 1u << 31;
  unsigned k = 3;
  while (bytes) {
    if (bytes & 1u) p = multmodp(t.x2n[k & 31u], p);
    bytes >>= 1;
    ++k;
  }
  return p;
}

// The CRC register after `n` bytes, from register `reg` (no pre- or post-inversion).
AMHIP_PNGE_HD uint32_t crc_run(const Tables& t, uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) reg = t.crc[(reg ^ p[i]) & 255u] ^ (reg >> 8);
  return reg;
}

// The register after A then B, from the register after A and the register B alone leaves from 0:
// the update is linear, and `bytes_b` zero bytes multiply the register by x^(8 * bytes_b).
AMHIP_PNGE_HD uint32_t crc_shift(const Tables& t, uint32_t reg_a, uint64_t bytes_b) {
  return multmodp(x8nmodp(t, bytes_b), reg_a);
}

// ---- the block planner -------------------------------------------------------------------------
// What one block needs while it is planned: 5.5 KB, the plan kernel's LDS.  freq / len / code of the
// three trees (literal/length, distance, code lengths), then what build_tree() uses for one tree at
// a time.  Every array is indexed at run time, so none may live in registers.
struct Work {
  uint16_t lfreq[kHeapSize], dfreq[2 * kDCodes + 1], blfreq[2 * kBlCodes + 1];
  uint16_t lcode[kLCodes], dcode[kDCodes], blcode[kBlCodes];
  uint16_t heap[kHeapSize], dad[kHeapSize];
  uint16_t bl_count[16], next_code[16];
  uint8_t llen[kHeapSize], dlen[2 * kDCodes + 1], bllen[2 * kBlCodes + 1];
  uint8_t depth[kHeapSize];
  int32_t opt_len, static_len;
};

// what the pack kernel needs of a planned block
struct BlockCode {
  uint32_t type;          // BlockType
  uint32_t bits;          // the block, type bits and end-of-block code included (fixed and dynamic)
  uint32_t header_bits;   // of header[], behind the three type bits (dynamic only)
  uint32_t stored_len;    // the block's bytes of input
  uint16_t lcode[kLCodes];
  uint16_t dcode0;        // distance code 0: every match has distance 1
  uint8_t llen[kLCodes];
  uint8_t dlen0;
  uint8_t pad;
  uint32_t header[kHeaderWords];
};

static_assert(sizeof(BlockCode) == 1448, "a block's share of the scratch (DESIGN 4.15)");

struct TreeDesc {
  uint16_t* freq;
  uint8_t* len;
  uint16_t* code;
  const uint8_t* static_len;   // null: no static tree
  const uint8_t* extra_bits;
  int extra_base, elems, max_length, max_code;
};

// send_bits(): LSB first, whole words; finish() stores what is left
struct WordSink {
  uint32_t* words;
  uint32_t cap, at;
  uint64_t acc;
  uint32_t n, total;
  AMHIP_PNGE_HD void put(uint32_t value, uint32_t len) {
    acc |= (uint64_t)value << n;
    n += len;
    total += len;
    if (n >= 32) {
      if (at < cap) words[at] = (uint32_t)acc;
      ++at;
      acc >>= 32;
      n -= 32;
    }
  }
  AMHIP_PNGE_HD void finish() {
    if (n && at < cap) words[at] = (uint32_t)acc;
  }
};

AMHIP_PNGE_HD bool tree_smaller(const TreeDesc& d, const Work& w, int n, int m) {
  return d.freq[n] < d.freq[m] || (d.freq[n] == d.freq[m] && w.depth[n] <= w.depth[m]);
}

AMHIP_PNGE_HD void pqdownheap(const TreeDesc& d, Work& w, int heap_len, int k) {
  const int v = w.heap[k];
  int j = k << 1;
  while (j <= heap_len) {
    if (j < heap_len && tree_smaller(d, w, w.heap[j + 1], w.heap[j])) ++j;
    if (tree_smaller(d, w, v, w.heap[j])) break;
    w.heap[k] = w.heap[j];
    k = j;
    j <<= 1;
  }
  w.heap[k] = (uint16_t)v;
}

// build_tree() with gen_bitlen() and gen_codes()
AMHIP_PNGE_HD void build_tree(TreeDesc& d, Work& w) {
  int heap_len = 0, heap_max = kHeapSize, max_code = -1;
  for (int n = 0; n < d.elems; ++n) {
    if (d.freq[n] != 0) {
      w.heap[++heap_len] = (uint16_t)(max_code = n);
      w.depth[n] = 0;
    } else {
      d.len[n] = 0;
    }
  }
  while (heap_len < 2) {
    const int node = w.heap[++heap_len] = (uint16_t)(max_code < 2 ? ++max_code : 0);
    d.freq[node] = 1;
    w.depth[node] = 0;
    --w.opt_len;
    if (d.static_len) w.static_len -= d.static_len[node];
  }
  d.max_code = max_code;
  for (int n = heap_len / 2; n >= 1; --n) pqdownheap(d, w, heap_len, n);
  int node = d.elems;
  do {
    const int n = w.heap[1];
    w.heap[1] = w.heap[heap_len--];
    pqdownheap(d, w, heap_len, 1);
    const int m = w.heap[1];
    w.heap[--heap_max] = (uint16_t)n;
    w.heap[--heap_max] = (uint16_t)m;
    d.freq[node] = (uint16_t)(d.freq[n] + d.freq[m]);
    w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
    w.dad[n] = w.dad[m] = (uint16_t)node;
    w.heap[1] = (uint16_t)node++;
    pqdownheap(d, w, heap_len, 1);
  } while (heap_len >= 2);
  w.heap[--heap_max] = w.heap[1];

  // gen_bitlen()
  for (int bits = 0; bits < 16; ++bits) w.bl_count[bits] = 0;
  d.len[w.heap[heap_max]] = 0;
  int overflow = 0;
  for (int h = heap_max + 1; h < kHeapSize; ++h) {
    const int n = w.heap[h];
    int bits = d.len[w.dad[n]] + 1;
    if (bits > d.max_length) {
      bits = d.max_length;
      ++overflow;
    }
    d.len[n] = (uint8_t)bits;
    if (n > max_code) continue;   // not a leaf
    ++w.bl_count[bits];
    const int xbits = n >= d.extra_base ? d.extra_bits[n - d.extra_base] : 0;
    w.opt_len += (int32_t)d.freq[n] * (bits + xbits);
    if (d.static_len) w.static_len += (int32_t)d.freq[n] * (d.static_len[n] + xbits);
  }
  if (overflow > 0) {
    do {
      int bits = d.max_length - 1;
      while (w.bl_count[bits] == 0) --bits;
      --w.bl_count[bits];
      w.bl_count[bits + 1] = (uint16_t)(w.bl_count[bits + 1] + 2);
      --w.bl_count[d.max_length];
      overflow -= 2;
    } while (overflow > 0);
    int h = kHeapSize;
    for (int bits = d.max_length; bits != 0; --bits) {
      int n = w.bl_count[bits];
      while (n != 0) {
        const int m = w.heap[--h];
        if (m > max_code) continue;
        if (d.len[m] != bits) {
          w.opt_len += (bits - (int)d.len[m]) * (int32_t)d.freq[m];
          d.len[m] = (uint8_t)bits;
        }
        --n;
      }
    }
  }
  // gen_codes()
  uint32_t code = 0;
  w.next_code[0] = 0;
  for (int bits = 1; bits < 16; ++bits) {
    code = (code + w.bl_count[bits - 1]) << 1;
    w.next_code[bits] = (uint16_t)code;
  }
  for (int n = 0; n <= max_code; ++n) {
    const int len = d.len[n];
    if (len == 0) continue;
    d.code[n] = (uint16_t)bi_reverse(w.next_code[len]++, len);
  }
}

// The loop scan_tree() and send_tree() share.  emit(symbol, count, repeat): `count` plain codes of a
// length, or one repeat code standing for `count` lengths.  The sentinel behind max_code is a
// length no code has.
template <typename Emit>
AMHIP_PNGE_HD void walk_tree(const uint8_t* len, int max_code, Emit emit) {
  int prevlen = -1, nextlen = len[0], count = 0;
  int max_count = nextlen == 0 ? 138 : 7, min_count = nextlen == 0 ? 3 : 4;
  for (int n = 0; n <= max_code; ++n) {
    const int curlen = nextlen;
    nextlen = n < max_code ? len[n + 1] : 0xFFFF;
    if (++count < max_count && curlen == nextlen) continue;
    if (count < min_count) {
      emit(curlen, count, false);
    } else if (curlen != 0) {
      if (curlen != prevlen) {
        emit(curlen, 1, false);
        --count;
      }
      emit(kRep3_6, count, true);
    } else if (count <= 10) {
      emit(kRepZ3_10, count, true);
    } else {
      emit(kRepZ11_138, count, true);
    }
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) {
      max_count = 138;
      min_count = 3;
    } else if (curlen == nextlen) {
      max_count = 6;
      min_count = 3;
    } else {
      max_count = 7;
      min_count = 4;
    }
  }
}

// _tr_flush_block() for a block whose frequencies stand in w.lfreq (END_BLOCK counted) and
// w.dfreq, every other entry of the three freq arrays zero: the trees, the block type, the bits the
// block takes and, for a dynamic block, send_all_trees() into out->header.
AMHIP_PNGE_HD void plan_block(const Tables& t, Work& w, uint32_t stored_len, BlockCode* out) {
  w.opt_len = 0;
  w.static_len = 0;
  TreeDesc l = {w.lfreq, w.llen, w.lcode, t.fixed_llen, t.extra_lbits, kLiterals + 1, kLCodes, 15, -1};
  TreeDesc d = {w.dfreq, w.dlen, w.dcode, t.fixed_dlen, t.extra_dbits, 0, kDCodes, 15, -1};
  TreeDesc bl = {w.blfreq, w.bllen, w.blcode, nullptr, t.extra_blbits, 0, kBlCodes, 7, -1};
  build_tree(l, w);
  build_tree(d, w);
  // build_bl_tree()
  uint16_t* blfreq = w.blfreq;
  auto count = [blfreq](int sym, int n, bool repeat) { blfreq[sym] = (uint16_t)(blfreq[sym] + (repeat ? 1 : n)); };
  walk_tree(w.llen, l.max_code, count);
  walk_tree(w.dlen, d.max_code, count);
  build_tree(bl, w);
  int max_blindex = kBlCodes - 1;
  while (max_blindex >= 3 && w.bllen[t.bl_order[max_blindex]] == 0) --max_blindex;
  w.opt_len += 3 * (max_blindex + 1) + 5 + 5 + 4;
  uint32_t opt_lenb = (uint32_t)(w.opt_len + 3 + 7) >> 3;
  const uint32_t static_lenb = (uint32_t)(w.static_len + 3 + 7) >> 3;
  if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
  out->stored_len = stored_len;
  out->header_bits = 0;
  out->pad = 0;
  if (stored_len + 4 <= opt_lenb) {
    out->type = kStored;
    out->bits = 0;
    return;
  }
  if (static_lenb == opt_lenb) {
    out->type = kFixed;
    out->bits = (uint32_t)w.static_len + 3;
    for (int n = 0; n < kLCodes; ++n) {
      out->lcode[n] = t.fixed_lcode[n];
      out->llen[n] = t.fixed_llen[n];
    }
    out->dcode0 = t.fixed_dcode[0];
    out->dlen0 = t.fixed_dlen[0];
    return;
  }
  out->type = kDynamic;
  out->bits = (uint32_t)w.opt_len + 3;
  for (int n = 0; n < kLCodes; ++n) {
    out->lcode[n] = n <= l.max_code ? w.lcode[n] : 0;
    out->llen[n] = n <= l.max_code ? w.llen[n] : 0;
  }
  out->dcode0 = w.dcode[0];
  out->dlen0 = w.dlen[0];
  // send_all_trees()
  WordSink s = {out->header, kHeaderWords, 0, 0, 0, 0};
  s.put((uint32_t)(l.max_code + 1 - 257), 5);
  s.put((uint32_t)(d.max_code + 1 - 1), 5);
  s.put((uint32_t)(max_blindex + 1 - 4), 4);
  for (int rank = 0; rank <= max_blindex; ++rank) s.put(w.bllen[t.bl_order[rank]], 3);
  const uint16_t* blcode = w.blcode;
  const uint8_t* bllen = w.bllen;
  WordSink* sp = &s;
  auto send = [blcode, bllen, sp](int sym, int n, bool repeat) {
    if (!repeat) {
      for (int i = 0; i < n; ++i) sp->put(blcode[sym], bllen[sym]);
      return;
    }
    sp->put(blcode[sym], bllen[sym]);
    if (sym == kRep3_6) sp->put((uint32_t)(n - 3), 2);
    else if (sym == kRepZ3_10) sp->put((uint32_t)(n - 3), 3);
    else sp->put((uint32_t)(n - 11), 7);
  };
  walk_tree(w.llen, l.max_code, send);
  walk_tree(w.dlen, d.max_code, send);
  s.finish();
  out->header_bits = s.total;
}

// the bits one symbol takes and its value, LSB first: a literal 0..255, or 256 + length of a match of
// distance 1 (the length code, its extra bits, then distance code 0); at most 15 + 5 + 15 bits
AMHIP_PNGE_HD uint32_t symbol_bits(const Tables& t, const uint8_t* llen, uint32_t dlen0, uint32_t sym) {
  if (sym < 256) return llen[sym];
  const uint32_t code = t.length_code[sym - 256 - 3];
  return (uint32_t)llen[code + kLiterals + 1] + t.extra_lbits[code] + dlen0;
}

// ---- the container ---------------------------------------------------------------------------
inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

inline uint32_t crc32(const Tables& t, const uint8_t* p, size_t n) { return ~crc_run(t, 0xFFFFFFFFu, p, n); }

// signature and IHDR (kFileHead bytes) to head, IEND (kFileTail bytes) to tail
inline void write_head_tail(const Tables& t, int width, int height, int channels, uint8_t* head, uint8_t* tail) {
  static const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  for (int i = 0; i < 8; ++i) head[i] = kSignature[i];
  uint8_t* c = head + 8;
  put_be32(c, 13);
  c[4] = 'I', c[5] = 'H', c[6] = 'D', c[7] = 'R';
  put_be32(c + 8, (uint32_t)width);
  put_be32(c + 12, (uint32_t)height);
  c[16] = 8;
  c[17] = channels == 1 ? 0 : 2;
  c[18] = c[19] = c[20] = 0;
  put_be32(c + 21, crc32(t, c + 4, 17));
  put_be32(tail, 0);
  tail[4] = 'I', tail[5] = 'E', tail[6] = 'N', tail[7] = 'D';
  put_be32(tail + 8, crc32(t, tail + 4, 4));
}

inline uint64_t raw_len(int width, int height, int channels) {
  return (uint64_t)height * (1u + (uint64_t)width * (uint64_t)channels);
}

// the most blocks a frame has: every symbol covers a byte at least, and the last block may be empty
inline uint64_t max_blocks(uint64_t raw) { return raw / kBlockSymbols + 1; }

// The largest zlib stream: a block never takes more than its stored form, which is its bytes, LEN and
// NLEN, and the type bits padded to a byte (at most 5 bytes on top of the data); 2 bytes of header,
// 4 of Adler-32, 1 for the last block's padding.
inline uint64_t zlib_bound(uint64_t raw) { return raw + 5 * max_blocks(raw) + 7; }

// the file around a zlib stream of z bytes
inline uint64_t file_size(uint64_t z) { return kFileHead + z + 12 * ((z + kIdatBytes - 1) / kIdatBytes) + kFileTail; }

inline uint64_t file_bound(int width, int height, int channels) {
  return file_size(zlib_bound(raw_len(width, height, channels)));
}

inline const char* check_image_args(size_t step, int width, int height, int channels) {
  if (channels != 1 && channels != 3) return "channels must be 1 (8UC1) or 3 (8UC3, B G R)";
  if (width < 1 || width > 65535 || height < 1 || height > 65535) return "width and height must be 1..65535";
  if (step < (size_t)width * (size_t)channels) return "step smaller than an image row";
  return nullptr;
}

// a stack of frames; null: fine
inline const char* check_frames_args(size_t F, int width, int height, int channels, size_t row_step,
                                     size_t frame_stride) {
  if (F == 0) return "no frames (F = 0)";
  if (width < 1 || width > 65535) return "width must be 1..65535";
  if (height < 1 || height > 65535) return "height must be 1..65535";
  if (channels != 1 && channels != 3) return "channels must be 1 (8UC1) or 3 (8UC3, B G R)";
  if (row_step < (size_t)width * (size_t)channels) return "row_step smaller than an image row";
  if (F > 1 && frame_stride < (size_t)height * row_step) return "frame_stride smaller than a frame";
  return nullptr;
}

// does the name end in ".png", compared without case as cv::imwrite's encoder lookup compares it
inline bool has_png_extension(const char* name) {
  size_t n = 0;
  while (name[n]) ++n;
  if (n < 4) return false;
  const char* e = name + n - 4;
  auto lower = [](char c) { return (char)(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c); };
  return e[0] == '.' && lower(e[1]) == 'p' && lower(e[2]) == 'n' && lower(e[3]) == 'g';
}

}  // namespace pnge
}  // namespace amhip

#endif  // AMHIP_PNG_ENCODE_HOST_H_
