// amhip_png_decode.hip -- PNG frames, decoded on the GPU: what the second overload of
// io::AerialMapperIO::loadImagesFromFile (aerial-mapper-io.cc:229-249) gets from cv::imread, one
// "<directory><name>.png" per name.  The lossless part is pinned to the real libraries: zlib
// defines inflate, Pillow the pixels (tests/golden/png_decode/); tests/png_decode_reference.py
// restates every rule.  The chunk parser and the per-frame descriptor are host code
// (amhip_png_decode_host.h); the device sees one contiguous zlib stream per frame, never chunk
// framing.
//
// Three kernels per group of frames, on the default stream; the statuses are read back once:
//   1. k_pngd_inflate   RFC 1951, one wave per frame.  The walk (block headers, Huffman codes, extra
//                       bits) is sequential and wave-uniform: every value it branches on is
//                       broadcast from the first lane.  The lanes stage 1 KB of the stream at a
//                       time into LDS, build the code tables there, copy matches and stored bytes
//                       64 at a time, and flush the output.  The 32 KiB window is a ring in LDS;
//                       a match reads it, never global memory.  Every 4096 finished bytes leave
//                       the ring as 256 16-byte stores, and the same pass adds them into the
//                       frame's Adler-32, which is compared with the stream's trailer at the end.
//   2. k_pngd_unfilter  one wave per frame, in place on the raw scanlines: bands of 64 rows, lane r
//                       runs row r of the band one pixel behind lane r - 1 (a skewed wavefront),
//                       so "above" and "above left" arrive from the neighbouring lane and "left"
//                       stays in a register.  Only the first lane's row reads the row above from
//                       memory: the band before wrote it, behind a barrier.
//   3. k_pngd_pixels    one lane per output pixel: alpha dropped, palette looked up, B, G, R or
//                       gray, into the stack layout the JPEG decoder produces.
//
// Bounds: see "What bounds each loop" in DESIGN 4.12.  In short: no byte at or behind the stream's
// end is loaded (they read as 0, and using one of those bits is an error that ends the walk);
// every symbol produces at least one byte or ends its block, every block header takes three real
// bits, and the walk ends as soon as the output passes the scanlines' length; stores to global
// memory cover [0, raw_len rounded up to 16) of the frame's own raw buffer only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_device.h"
#include "amhip_frame_stack.h"
#include "amhip_png_decode_host.h"
#include "amhip_png_inflate.h"

namespace amhip {

namespace {

using pngd::Frame;

constexpr int kWin = 1024;               // stream bytes in LDS (16 per lane)
constexpr int kRing = 32768;             // the deflate window
constexpr int kFlush = 4096;             // bytes that leave the ring at a time
constexpr int kLitBits = 10, kDistBits = 8;   // peeked bits of the two lookup tables
constexpr int kMaxLit = 288, kMaxDist = 32;
constexpr uint32_t kAdlerMod = 65521u;

struct Tables {
  uint16_t len_base[32], len_extra[32], dist_base[32], dist_extra[32];
  uint8_t cl_order[20];
};
constexpr Tables make_tables() {
  Tables t = {};
  // RFC 1951 3.2.5: length codes 257..285, distance codes 0..29
  int base = 3;
  for (int i = 0; i < 28; ++i) {
    const int e = i < 8 ? 0 : (i - 4) / 4;
    t.len_base[i] = (uint16_t)base;
    t.len_extra[i] = (uint16_t)e;
    base += 1 << e;
  }
  t.len_base[28] = 258;
  t.len_extra[28] = 0;
  base = 1;
  for (int i = 0; i < 30; ++i) {
    const int e = i < 4 ? 0 : (i - 2) / 2;
    t.dist_base[i] = (uint16_t)base;
    t.dist_extra[i] = (uint16_t)e;
    base += 1 << e;
  }
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; ++i) t.cl_order[i] = order[i];
  return t;
}
__constant__ Tables d_tables = make_tables();

// One prefix code in LDS: a lookup table over the next `bits` bits of the stream (entry = symbol |
// length << 9, 0: no code that short), and for the longer codes the count per length and the
// symbols in canonical order, walked a bit at a time as zlib's puff does.
struct Code {
  uint16_t* fast;
  uint32_t* count;   // [16]
  uint16_t* sorted;
  int bits;
};

// Builds `c` from n code lengths.  -> the code space left over: 0 complete, > 0 incomplete, < 0
// over-subscribed; *longest = the longest length (0: no code at all).  Every lane takes part.
// place / code: 16 words of LDS each, the next index in `sorted` and the next code per length.
__device__ __forceinline__ int build_code(const uint8_t* lens, int n, const Code& c, uint32_t* place,
                                          uint32_t* code, int lane, int* longest) {
  __syncthreads();
  for (int i = lane; i < (1 << c.bits); i += 64) c.fast[i] = 0;
  if (lane < 16) c.count[lane] = 0;
  __syncthreads();
  for (int s = lane; s < n; s += 64) {
    const int l = lens[s];
    if (l) atomicAdd(&c.count[l], 1u);
  }
  __syncthreads();
  int left = 1, maxlen = 0;
  uint32_t next = 0, at = 0;
#pragma nounroll
  for (int l = 1; l < 16; ++l) {
    const uint32_t k = uni(c.count[l]);
    next <<= 1;
    if (lane == 0) {
      place[l] = at;
      code[l] = next;
    }
    next += k;
    at += k;
    if (left >= 0) left = (left << 1) - (int)k;   // (stays negative once over-subscribed)
    if (k) maxlen = l;
  }
  *longest = maxlen;
  if (left < 0) return left;
  // 64 symbols a round: the lanes whose symbol has length l take consecutive codes, in lane order
  for (int s0 = 0; s0 < n; s0 += 64) {
    __syncthreads();
    const int s = s0 + lane;
    const int mine = s < n ? (int)lens[s] : 0;
    uint32_t rank = 0, took = 0;
    bool last_of_mine = false;
#pragma nounroll
    for (int l = 1; l < 16; ++l) {
      const uint64_t m = __ballot(mine == l);
      if (mine == l) {
        rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        took = (uint32_t)__popcll(m);
        last_of_mine = (m >> lane) == 1ull;
      }
    }
    uint32_t my_place = 0, my_code = 0;
    if (mine) {
      my_place = place[mine];
      my_code = code[mine];
      c.sorted[my_place + rank] = (uint16_t)s;
      if (mine <= c.bits) {
        // deflate packs codes from their most significant bit: the table is indexed by the reverse
        const uint32_t rev = __brev(my_code + rank) >> (32 - mine);
        const uint16_t e = (uint16_t)((uint32_t)s | ((uint32_t)mine << 9));
        for (uint32_t k = rev; k < (1u << c.bits); k += 1u << mine) c.fast[k] = e;
      }
    }
    __syncthreads();
    if (last_of_mine) {
      place[mine] = my_place + took;
      code[mine] = my_code + took;
    }
  }
  __syncthreads();
  return left;
}

// The bit reader of one frame; deflate packs bits from the least significant end.  Everything in
// here is the same in every lane.
struct Reader {
  const uint8_t* at;   // the next byte to load
  int64_t left;        // bytes from there to the stream's end (the Adler-32 trailer); <= 0 behind it
  int32_t o;           // `at` in the LDS window; outside [0, kWin - 8]: stage first
  uint32_t* win;       // LDS, kWin bytes + one word
  uint64_t acc;        // the low `nbits` bits are unread
  int nbits;
  int fake;            // of those, zero bits fed behind the end (always the last ones)
  uint32_t err;

  // kWin bytes from the word that holds `at`; bytes at or behind the end read as 0 and are not loaded
  __device__ __forceinline__ void stage(int lane) {
    __syncthreads();
    o = (int32_t)(reinterpret_cast<uintptr_t>(at) & 3u);   // (the buffer and every stream in it start at a multiple of 16)
    const uint8_t* const base = at - o;
#pragma unroll
    for (int i = 0; i < kWin / 256; ++i) {
      const int64_t rel = 4 * (lane + 64 * i) - o;   // this word's first byte, counted from `at`
      const uint8_t* const q = base + 4 * (lane + 64 * i);
      uint32_t w = 0;
      if (rel + 4 <= left) {
        w = *reinterpret_cast<const uint32_t*>(q);
      } else {
        for (int k = 0; k < 4; ++k)
          if (rel + k < left) w |= (uint32_t)q[k] << (8 * k);   // (never a byte at or behind the end)
      }
      win[lane + 64 * i] = w;
    }
    if (lane == 0) win[kWin / 4] = 0;
    __syncthreads();
  }

  // more than 32 unread bits behind this
  __device__ __forceinline__ void fill(int lane) {
    if (nbits > 32) return;
    if (o < 0 || o + 8 > kWin) stage(lane);
    const uint32_t lo = uni(win[o >> 2]), hi = uni(win[(o >> 2) + 1]);
    const uint32_t v = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (o & 3)));
    acc |= (uint64_t)v << nbits;
    nbits += 32;
    const int real = left <= 0 ? 0 : (left < 4 ? (int)left : 4);
    fake += 8 * (4 - real);
    at += 4;   // (may pass the end by a few bytes: they were fed as zeros and counted in `fake`)
    left -= 4;
    o += 4;
  }
  // moves the load position by n bytes (either way)
  __device__ __forceinline__ void skip(int64_t n) {
    at += n;
    left -= n;
    o = (n > kWin || n < -kWin) ? -1 : o + (int32_t)n;
  }
  __device__ __forceinline__ uint32_t peek(int n) const {
    return (uint32_t)acc & ((1u << n) - 1u);
  }
  __device__ __forceinline__ void drop(int n) {
    acc >>= n;
    nbits -= n;
    if (nbits < fake) err = pngd::kEndsEarly;
  }
  __device__ __forceinline__ uint32_t bits(int n) {   // n <= 16
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  // one symbol of `c`; at most 15 bits.  An undefined pattern sets err.
  __device__ __forceinline__ uint32_t symbol(const Code& c) {
    const uint32_t e = uni(c.fast[peek(c.bits)]);
    if (e) {
      drop((int)(e >> 9));
      return e & 511u;
    }
    int code = 0, first = 0, index = 0;
#pragma nounroll
    for (int l = 1; l < 16; ++l) {   // (at most 15 rounds)
      code |= (int)((acc >> (l - 1)) & 1u);
      const int k = (int)uni(c.count[l]);
      if (code - k < first) {
        drop(l);
        return uni(c.sorted[index + (code - first)]);
      }
      index += k;
      first += k;
      first <<= 1;
      code <<= 1;
    }
    // (15 real bits that no code has; with fewer left, the stream has ended)
    if (!err) err = nbits - 15 < fake ? pngd::kEndsEarly : pngd::kBadCode;
    return 0;
  }
};

__global__ __launch_bounds__(64) void k_pngd_inflate(const uint8_t* __restrict__ stream,
                                                     const Frame* __restrict__ frames, size_t first_frame,
                                                     uint8_t* __restrict__ raw, uint32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
  __shared__ uint32_t win[kWin / 4 + 1];
  __shared__ uint16_t lit_fast[1 << kLitBits], dist_fast[1 << kDistBits];
  __shared__ uint16_t lit_sorted[kMaxLit], dist_sorted[kMaxDist];
  __shared__ uint32_t lit_count[16], dist_count[16], next_place[16], next_code[16];
  __shared__ uint8_t lens[kMaxLit + kMaxDist];
  __shared__ uint8_t* cold_dst;     // what only a flush or the end needs waits in LDS, not in registers
  __shared__ uint32_t cold_adler;
  const int lane = threadIdx.x;
  const Frame* f = frames + (first_frame + blockIdx.x);
  const uint64_t raw_len = f->raw_len;
  if (lane == 0) {
    cold_dst = raw + f->raw_base;
    cold_adler = f->adler;
  }
  const Code lit = {lit_fast, lit_count, lit_sorted, kLitBits};
  const Code dist = {dist_fast, dist_count, dist_sorted, kDistBits};
  const Code clc = {dist_fast, dist_count, dist_sorted, 7};   // the code-length code borrows the distance code's place

  Reader r;
  r.at = stream + f->stream_begin;
  r.left = (int64_t)(f->stream_end - f->stream_begin);
  r.o = -1;   // (nothing staged yet)
  r.win = win;
  r.acc = 0;
  r.nbits = 0;
  r.fake = 0;
  r.err = 0;

  uint64_t out = 0;        // bytes produced; [out rounded down to kFlush, out) are in the ring only
  // Adler-32 as two plain sums: s1 = 1 + sum b[p], s2 = N + sum b[p] * (N - p), both mod 65521; a lane
  // adds its 16-byte granules with the weight (N - p) mod 65521.  No sum can wrap: a term is below
  // 2^28 and a lane sees at most raw_len / 1024 < 2^25 granules.
  uint64_t sum1 = 0, sum2 = 0;

  // [from, upto) out of the ring, from a multiple of kFlush, upto - from <= kFlush, upto <= raw_len:
  // whole 16-byte granules; bytes at or behind `upto` in the last granule are stored as they lie in
  // the ring (the buffer is padded to 16) but stay out of the sums
  auto flush = [&](uint64_t from, uint64_t upto) {
    __syncthreads();
    uint8_t* const dst = cold_dst;
    const uint32_t bytes = (uint32_t)(upto - from);
    const uint32_t weight = (uint32_t)((raw_len - from) % kAdlerMod);
    for (uint32_t g = lane; g < ((bytes + 15u) >> 4); g += 64) {   // (at most kFlush / 16 granules)
      const uint64_t p0 = from + 16ull * g;
      const uint4 v = *reinterpret_cast<const uint4*>(ring + (p0 & (kRing - 1)));
      *reinterpret_cast<uint4*>(dst + p0) = v;
      const uint32_t w0 = (weight + kAdlerMod - 16u * g) % kAdlerMod;   // (16 * g < kFlush < 65521)
      const uint32_t word[4] = {v.x, v.y, v.z, v.w};
      uint32_t s = 0, t = 0;
      const uint32_t live = bytes - 16u * g >= 16u ? 16u : bytes - 16u * g;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t b = (uint32_t)j < live ? (word[j >> 2] >> (8 * (j & 3))) & 255u : 0u;
        s += b;
        t += (uint32_t)j * b;
      }
      sum1 += s;
      // sum of b[j] * (w0 - j) mod 65521, kept non-negative: t <= 120 * 255 < 65521 <= 65521 * (s > 0)
      sum2 += (uint64_t)w0 * s + (s ? kAdlerMod : 0u) - t;
    }
    __syncthreads();
  };
  // after `out` grew by `added` <= kFlush bytes: the kFlush bytes it has completed, if any
  auto flush_if_full = [&](uint32_t added) {
    if (((uint32_t)out & (kFlush - 1)) < added) {
      const uint64_t edge = out & ~(uint64_t)(kFlush - 1);
      flush(edge - kFlush, edge);
    }
  };

  bool last = false;
  while (!last && !r.err) {   // one block a round; a block header takes three real bits
    r.fill(lane);
    last = r.bits(1) != 0;
    const uint32_t btype = r.bits(2);
    if (r.err) break;
    if (btype == 3) {
      r.err = pngd::kBadBlockType;
      break;
    }
    if (btype == 0) {
      // stored: the rest of the byte is dropped; LEN, NLEN; LEN bytes as they are
      r.drop(r.nbits & 7);
      r.fill(lane);
      const uint32_t len = r.bits(16), nlen = r.bits(16);
      if (r.err) break;
      if ((len ^ 0xFFFFu) != nlen) {
        r.err = pngd::kBadStoredLen;
        break;
      }
      // the bytes still in the accumulator go back: the copy reads the stream itself
      r.skip(-(int64_t)(r.nbits >> 3));   // (no fake bit was used, so left >= 0)
      r.acc = 0;
      r.nbits = 0;
      r.fake = 0;
      if ((int64_t)len > r.left) {
        r.err = pngd::kEndsEarly;
        break;
      }
      __syncthreads();
      for (uint32_t k = 0; k < len && !r.err; k += 64) {   // (at most 1024 rounds)
        const uint32_t n = len - k < 64 ? len - k : 64;
        if ((uint32_t)lane < n) ring[(out + lane) & (kRing - 1)] = r.at[k + lane];   // (k + lane < len <= left)
        out += n;
        if (out > raw_len) r.err = pngd::kTooLong;
        else flush_if_full(n);
      }
      r.skip((int64_t)len);
      continue;
    }
    if (btype == 1) {
      // fixed codes (3.2.6): the same builder, from the lengths the RFC states
      __syncthreads();
      for (int s = lane; s < kMaxLit + kMaxDist; s += 64)
        lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    } else {
      const uint32_t hlit = r.bits(5) + 257, hdist = r.bits(5) + 1, hclen = r.bits(4) + 4;
      if (r.err) break;
      if (hlit > 286 || hdist > 30) {
        r.err = pngd::kBadDynHeader;
        break;
      }
      __syncthreads();
      if (lane < 19) lens[lane] = 0;
      __syncthreads();
      for (uint32_t i = 0; i < hclen; ++i) {   // (at most 19)
        r.fill(lane);
        const uint32_t l = r.bits(3);
        if (lane == 0) lens[d_tables.cl_order[i]] = (uint8_t)l;
      }
      if (r.err) break;
      int longest;
      const int left = build_code(lens, 19, clc, next_place, next_code, lane, &longest);
      if (left != 0) {
        r.err = left < 0 ? pngd::kOverSubscribed : pngd::kIncomplete;
        break;
      }
      // HLIT + HDIST lengths as one sequence: a repeat may run from the literal lengths into the
      // distance lengths, not past their end.  Every round stores at least one length.
      const uint32_t total = hlit + hdist;
      uint32_t have = 0, prev = 0;
      while (have < total && !r.err) {
        r.fill(lane);
        const uint32_t s = r.symbol(clc);
        if (r.err) break;
        uint32_t value = s, times = 1;
        if (s == 16) {
          if (have == 0) {
            r.err = pngd::kBadDynHeader;
            break;
          }
          value = prev;
          times = 3 + r.bits(2);
        } else if (s == 17) {
          value = 0;
          times = 3 + r.bits(3);
        } else if (s == 18) {
          value = 0;
          times = 11 + r.bits(7);
        }
        if (r.err) break;
        if (have + times > total) {
          r.err = pngd::kBadDynHeader;
          break;
        }
        // (kept apart from the code-length code's own lengths, which lie in lens[0..18] no longer: the
        // table is built.  Lanes write the run.)
        for (uint32_t k = lane; k < times; k += 64) lens[have + k] = (uint8_t)value;
        have += times;
        prev = value;
      }
      if (r.err) break;
      __syncthreads();
      if (uni(lens[256]) == 0) {
        r.err = pngd::kBadDynHeader;   // no end-of-block code
        break;
      }
      // the distance lengths move behind the literal lengths' full range, so that the two builds
      // do not depend on HLIT
      const uint8_t mine = (uint32_t)lane < hdist ? lens[hlit + lane] : (uint8_t)0;
      __syncthreads();
      if (lane < kMaxDist) lens[kMaxLit + lane] = mine;
      for (uint32_t s = hlit + lane; s < (uint32_t)kMaxLit; s += 64) lens[s] = 0;
    }
    {
      int longest;
      int left = build_code(lens, kMaxLit, lit, next_place, next_code, lane, &longest);
      if (left != 0) {
        r.err = left < 0 ? pngd::kOverSubscribed : pngd::kIncomplete;
        break;
      }
      left = build_code(lens + kMaxLit, kMaxDist, dist, next_place, next_code, lane, &longest);
      // complete, or no distance code at all, or the one code of one bit RFC 1951 allows
      if (left < 0 || (left > 0 && longest > 1)) {
        r.err = left < 0 ? pngd::kOverSubscribed : pngd::kIncomplete;
        break;
      }
    }
    // the block's symbols: a literal is one byte, a match at least three, 256 ends the block
    for (;;) {
      r.fill(lane);
      const uint32_t s = r.symbol(lit);
      uint32_t added = 1;
      if (r.err) break;
      if (s < 256) {
        if (lane == 0) ring[out & (kRing - 1)] = (uint8_t)s;
        out += 1;
      } else if (s == 256) {
        break;
      } else {
        if (s > 285) {
          r.err = pngd::kBadCode;
          break;
        }
        const uint32_t len = d_tables.len_base[s - 257] + r.bits(d_tables.len_extra[s - 257]);
        r.fill(lane);
        const uint32_t ds = r.symbol(dist);
        if (r.err) break;
        if (ds > 29) {
          r.err = pngd::kBadCode;
          break;
        }
        const uint32_t d = d_tables.dist_base[ds] + r.bits(d_tables.dist_extra[ds]);
        if (r.err) break;
        if (d > out) {
          r.err = pngd::kDistTooFar;
          break;
        }
        // byte k of the match is the byte d behind it, so for d < len the last d bytes repeat:
        // every source lies in front of `out` and is in the ring already
        __syncthreads();
        for (uint32_t k0 = 0; k0 < len; k0 += 64) {   // (at most 5 rounds)
          const uint32_t k = k0 + lane;
          if (k < len) {
            const uint32_t back = d >= len ? k : k % d;
            ring[(out + k) & (kRing - 1)] = ring[(out - d + back) & (kRing - 1)];
          }
        }
        out += len;
        added = len;
      }
      if (out > raw_len) {
        r.err = pngd::kTooLong;
        break;
      }
      flush_if_full(added);
    }
  }
  uint32_t err = r.err;
  if (!err && out < raw_len) err = pngd::kTooShort;
  if (!err) {
    if (out & (kFlush - 1)) flush(out & ~(uint64_t)(kFlush - 1), out);   // (out == raw_len: the last, partial piece)
    uint32_t a = (uint32_t)(sum1 % kAdlerMod), b = (uint32_t)(sum2 % kAdlerMod);
    for (int m = 32; m >= 1; m >>= 1) {
      a += (uint32_t)__shfl_xor((int)a, m);
      b += (uint32_t)__shfl_xor((int)b, m);
    }
    const uint32_t s1 = (1u + a) % kAdlerMod;
    const uint32_t s2 = ((uint32_t)(raw_len % kAdlerMod) + b) % kAdlerMod;
    if (((s2 << 16) | s1) != cold_adler) err = pngd::kBadAdler;
  }
  if (lane == 0) status[first_frame + blockIdx.x] = err;
}

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);   // ties: a, then b, then c
}

// a pixel's bytes travel packed in one word, byte k of the pixel in bits 8k..8k+7
__device__ __forceinline__ uint32_t reconstruct(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c, int bpp) {
  uint32_t out = 0;
  for (int k = 0; k < bpp; ++k) {
    const uint32_t xs = (x >> (8 * k)) & 255u, as = (a >> (8 * k)) & 255u, bs = (b >> (8 * k)) & 255u,
                   cs = (c >> (8 * k)) & 255u;
    uint32_t v = xs;
    if (ft == 1) v = xs + as;
    else if (ft == 2) v = xs + bs;
    else if (ft == 3) v = xs + ((as + bs) >> 1);   // (the 9-bit sum)
    else if (ft == 4) v = xs + paeth(as, bs, cs);
    out |= (v & 255u) << (8 * k);
  }
  return out;
}

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p, int bpp) {
  uint32_t v = 0;
  for (int k = 0; k < bpp; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

__global__ __launch_bounds__(64) void k_pngd_unfilter(const Frame* __restrict__ frames, size_t first_frame,
                                                      uint8_t* raw, uint32_t* status) {
  const int lane = threadIdx.x;
  const size_t fi = first_frame + blockIdx.x;
  const Frame* f = frames + fi;
  if (status[fi] != 0) return;   // (the scanlines are not there)
  const int W = f->width, H = f->height, bpp = f->bpp;
  const size_t pitch = 1 + (size_t)W * bpp;
  uint8_t* const base = raw + f->raw_base;
  bool bad = false;
  for (int row0 = 0; row0 < H; row0 += 64) {   // bands, one after another: a band's first row needs the last of the band before
    const int row = row0 + lane;
    const bool have_row = row < H;
    uint8_t* const line = base + (size_t)(have_row ? row : 0) * pitch;
    uint32_t ft = have_row ? line[0] : 0u;
    if (ft > 4) {
      bad = true;
      ft = 0;
    }
    const uint8_t* const above0 = row0 > 0 ? base + (size_t)(row0 - 1) * pitch + 1 : nullptr;
    uint32_t cur = 0, prev_b = 0;
    const int steps = W + 63;
    for (int t = 0; t < steps; ++t) {
      // what lane r - 1 made one step ago is this lane's pixel above
      uint32_t b = (uint32_t)__shfl_up((int)cur, 1);
      const int x = t - lane;
      const bool live = have_row && x >= 0 && x < W;
      if (lane == 0) b = (above0 && live) ? load_pixel(above0 + (size_t)x * bpp, bpp) : 0u;
      if (live) {
        uint8_t* const px = line + 1 + (size_t)x * bpp;
        const uint32_t a = x == 0 ? 0u : cur, c = x == 0 ? 0u : prev_b;
        const uint32_t v = reconstruct(ft, load_pixel(px, bpp), a, b, c, bpp);
        for (int k = 0; k < bpp; ++k) px[k] = (uint8_t)(v >> (8 * k));
        prev_b = b;
        cur = v;
      }
    }
    __syncthreads();   // the band's last row is in memory before the next band's first lane loads it
  }
  if (bad) atomicCAS(&status[fi], 0u, (uint32_t)pngd::kBadFilter);
}

__global__ __launch_bounds__(256) void k_pngd_pixels(const Frame* __restrict__ frames, size_t first_frame,
                                                     const uint8_t* __restrict__ raw, uint8_t* __restrict__ out,
                                                     size_t frame_stride, size_t row_step, int colored,
                                                     uint32_t* status) {
  const size_t fi = first_frame + blockIdx.z;
  const Frame* f = frames + fi;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= f->width || y >= f->height) return;
  const int bpp = f->bpp, ct = f->colour_type;
  const uint8_t* px = raw + f->raw_base + (size_t)y * (1 + (size_t)f->width * bpp) + 1 + (size_t)x * bpp;
  uint32_t R, G, B;
  bool gray_file = false;
  if (ct == 0 || ct == 4) {
    R = G = B = px[0];
    gray_file = true;
  } else if (ct == 3) {
    const int i = px[0];
    if (i >= f->plte_entries) {
      atomicCAS(&status[fi], 0u, (uint32_t)pngd::kBadIndex);
      return;
    }
    R = f->plte[3 * i];
    G = f->plte[3 * i + 1];
    B = f->plte[3 * i + 2];
  } else {
    R = px[0];
    G = px[1];
    B = px[2];
  }
  if (colored) {
    uint8_t* dst = out + fi * frame_stride + (size_t)y * row_step + 3 * (size_t)x;
    dst[0] = (uint8_t)B;
    dst[1] = (uint8_t)G;
    dst[2] = (uint8_t)R;
  } else {
    // png_set_rgb_to_gray(.., 0.299, 0.587) as cv::imread sets it up (adopted, unpinned): exact for R = G = B
    const uint32_t g = gray_file ? R : (9797u * R + 19234u * G + 3737u * B) >> 15;
    out[fi * frame_stride + (size_t)y * row_step + (size_t)x] = (uint8_t)g;
  }
}

size_t round16(size_t n) {
  return (n + 15) & ~(size_t)15;
}

}  // namespace

// (amhip_png_inflate.h: the GeoTIFF reader's chunks are such streams too)
void pngd::launch_inflate(hipStream_t stream, const uint8_t* bytes, const pngd::Frame* frames, size_t first, size_t n,
                          uint8_t* raw, uint32_t* status) {
  hipLaunchKernelGGL(k_pngd_inflate, dim3((unsigned)n), dim3(64), 0, stream, bytes, frames, first, raw, status);
}

namespace {

// The codec description of decode_frame_stack (amhip_frame_stack.h): every frame's IDAT payloads are
// joined into one zlib stream at a multiple of 16; a frame costs its raw scanlines, rounded up to 16.
struct PngStack {
  using Frame = pngd::Frame;
  static constexpr const char* kDecode = "amhip_io_decode_png_frames";
  static constexpr const char* kInfo = "amhip_png_info";
  // MB of raw scanlines per group of frames.  Groups run one after another and each takes as long as
  // its longest stream, so the default holds the demo flags' 249 frames of 1920 x 1080 in one group
  // (0.5 GB gray, 1.5 GB RGB).
  static constexpr const char* kBudgetKey = "pngd_raw_budget_mb";
  static constexpr double kBudgetMB = 4096.0;
  static constexpr size_t kGroupFrames = 32768;   // (grid.z of the per-pixel launch)

  static bool info(const uint8_t* file, size_t len, int* width, int* height, int* channels, char* err,
                   size_t errcap) {
    pngd::Parsed p;
    if (!pngd::parse(file, len, &p, err, errcap)) return false;
    *width = p.f.width;
    *height = p.f.height;
    *channels = (p.f.colour_type == 0 || p.f.colour_type == 4) ? 1 : 3;
    return true;
  }
  static const char* status_text(uint32_t s) { return pngd::status_text(s); }

  std::vector<uint8_t> streams;   // every frame's zlib stream, each at a multiple of 16
  pngd::Parsed parsed;
  DevBuf bytes, raw;

  bool parse(const uint8_t* file, size_t len, Frame* f, char* err, size_t errcap) {
    if (!pngd::parse(file, len, &parsed, err, errcap)) return false;
    const size_t at = streams.size();
    streams.resize(at + round16(parsed.zlen), 0);
    pngd::concat(file, parsed, streams.data() + at);
    *f = parsed.f;
    f->stream_begin += at;
    f->stream_end += at;
    return true;
  }
  size_t cost_bytes(const Frame& f) const { return round16((size_t)f.raw_len); }
  void place(Frame* f, size_t base_bytes, int /*colored*/) { f->raw_base = base_bytes; }
  int upload(const uint8_t* const*, const size_t*, size_t, size_t max_group_bytes, int /*colored*/,
             hipStream_t stream) {
    int rc;
    if ((rc = bytes.alloc(streams.size()))) return rc;
    if ((rc = raw.alloc(max_group_bytes))) return rc;
    AMHIP_TRY(hipMemcpyAsync(bytes.p, streams.data(), streams.size(), hipMemcpyHostToDevice, stream));
    return AMHIP_OK;
  }
  void launch_group(size_t first, size_t n, const StackLaunch<Frame>& s) {
    pngd::launch_inflate(s.stream, bytes.as<uint8_t>(), s.frames, first, n, raw.as<uint8_t>(), s.status);
    hipLaunchKernelGGL(k_pngd_unfilter, dim3((unsigned)n), dim3(64), 0, s.stream, s.frames, first,
                       raw.as<uint8_t>(), s.status);
    hipLaunchKernelGGL(k_pngd_pixels, dim3((unsigned)((s.width + 255) / 256), (unsigned)s.height, (unsigned)n),
                       dim3(256), 0, s.stream, s.frames, first, raw.as<uint8_t>(), s.out, s.frame_stride,
                       s.row_step, s.colored, s.status);
  }
};

}  // namespace

}  // namespace amhip

extern "C" {

int amhip_png_info(const uint8_t* file, size_t len, int* width, int* height, int* channels) {
  return amhip::image_info<amhip::PngStack>(file, len, width, height, channels);
}

int amhip_io_decode_png_frames(int device, const uint8_t* const* files, const size_t* lens, size_t F, int colored,
                               uint8_t** dev_frames, int* width, int* height, size_t* row_step,
                               size_t* frame_stride) {
  return amhip::decode_frame_stack<amhip::PngStack>(device, files, lens, F, colored, dev_frames, width, height,
                                                    row_step, frame_stride);
}

}  // extern "C"
