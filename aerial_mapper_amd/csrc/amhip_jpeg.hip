// amhip_jpeg.hip -- baseline JPEG, encoded on the GPU: what cv::imwrite(filename_mosaic_output,
// result_) leaves behind every batch / updateOrthomosaic (ortho-forward-homography.cc:126-128,188)
// and what save_orthomosaic_jpg / orthomosaic_jpg_filename of the three ortho::Settings ask for.
// The file is the one libjpeg writes at cv::imwrite's / Pillow's settings (quality q, 4:2:0 for
// colour, standard Huffman tables, no optimisation): sequential DCT, 8 bit, one scan, no restart
// markers.  tests/jpeg_reference.py restates it rule by rule and is pinned to libjpeg's own bytes
// (tests/golden/jpeg/); this file must equal the restatement byte for byte.
//
// Five passes, all on the caller's stream, nothing read back but the file's size:
//   1. k_jpeg_blocks    pixels -> quantised coefficients, zigzag order, int16, in the order the scan
//                       codes the blocks (gray: block by block; colour: MCUs of Y00 Y01 Y10 Y11 Cb Cr).
//                       Eight lanes per block: a lane transforms a row, the block goes through LDS,
//                       the same lane transforms a column and quantises it.
//   2. k_jpeg_lengths   one lane per block: the bits its codes take (DC difference against the
//                       previous block of the component, run/size symbols, ZRL, EOB) and the sum of
//                       256 blocks per workgroup.
//   3. k_jpeg_scan_top  one wave walks those sums 64 at a time: 64-bit exclusive prefix sums.
//   4. k_jpeg_pack      one lane per block writes its codes at its bit offset, MSB first.  A 32-bit
//                       word that lies inside one block's bits is stored; a block's first and last
//                       word can be shared with its neighbours and are OR-ed in atomically (the words
//                       are zeroed before).  The last block pads the final byte with 1-bits.
//   5. k_jpeg_ff_count / k_jpeg_scan_top / k_jpeg_stuff: 0xFF bytes per 4096-byte chunk, their
//                       prefix sums, and the copy into the caller's buffer with a 0x00 behind each
//                       0xFF, behind the header segments (built on the host, amhip_jpeg_host.h) and
//                       in front of EOI.  Nothing is written when the file would not fit.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_jpeg_host.h"

namespace amhip {

constexpr int kBlocksPerGroup = 32;   // k_jpeg_blocks: 256 lanes, 8 per block
constexpr int kTile = 256;            // blocks per workgroup of the entropy passes
constexpr int kChunk = 4096;          // bytes per workgroup of the stuffing passes (16 per lane)

__constant__ jpeg::HuffTables d_huff = jpeg::make_huff_tables();

// natural (row-major) index -> zigzag position
struct Unzig {
  uint8_t at[64];
};
constexpr Unzig make_unzig() {
  Unzig u = {};
  for (int z = 0; z < 64; ++z) u.at[jpeg::kZigzag[z]] = (uint8_t)z;
  return u;
}
__constant__ Unzig d_unzig = make_unzig();

// (JpegSource::mode, amhip_common.h)
enum { kGray8 = kJpegGray8, kBgr8 = kJpegBgr8, kBgr16s = kJpegBgr16s };

struct Geom {
  int width, height;
  int colour;        // 0: one component; 1: Y Cb Cr, 4:2:0
  int bw;            // gray: blocks per row; colour: MCUs per row
  unsigned nb;       // blocks in the scan
};

// what the host uploads in front of every call
struct alignas(8) Blob {
  uint16_t divisor[2][64];   // 8 * the quantisation table entry, natural order
  uint32_t header_bytes;
  uint32_t pad[3];
  uint8_t header[jpeg::kMaxHeaderBytes];
};
// device words: [0] bits of the scan, [1] 0xFF bytes in it, [2] the file's size, [3] 1 = does not fit
constexpr int kCtrlWords = 4;

// ---------------------------------------------------------------------------
// pass 1
// ---------------------------------------------------------------------------
template <int kMode>
__device__ __forceinline__ void load_bgr(const uint8_t* __restrict__ px, size_t step, int x, int y,
                                         int* b, int* g, int* r) {
  if (kMode == kBgr8) {
    const uint8_t* p = px + (size_t)y * step + (size_t)x * 3u;
    *b = p[0];
    *g = p[1];
    *r = p[2];
  } else {
    // the mosaic's CV_16SC3 result_, clamped as OrthoForwardHomography::result8() clamps it
    const int16_t* p = reinterpret_cast<const int16_t*>(px + (size_t)y * step) + (size_t)x * 3u;
    *b = min(max((int)p[0], 0), 255);
    *g = min(max((int)p[1], 0), 255);
    *r = min(max((int)p[2], 0), 255);
  }
}

// rgb_ycc_convert (jccolor.c), FIX(x) = (int)(x * 65536 + 0.5)
__device__ __forceinline__ int ycc_y(int b, int g, int r) {
  return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}
__device__ __forceinline__ int ycc_cb(int b, int g, int r) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int ycc_cr(int b, int g, int r) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// one pass of jpeg_fdct_islow (jfdctint.c): CONST_BITS 13, PASS1_BITS 2
template <bool kFirst>
__device__ __forceinline__ void fdct_1d(int* d) {
  constexpr int kShift = kFirst ? 13 - 2 : 13 + 2;
  constexpr int kRound = 1 << (kShift - 1);
  const int t0 = d[0] + d[7], t7 = d[0] - d[7];
  const int t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5];
  const int t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kFirst) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + kRound) >> kShift;
  d[6] = (z1 + t12 * (-15137) + kRound) >> kShift;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * (-16069) + z5;
  z4 = z4 * (-3196) + z5;
  d[7] = (a4 + z1 + z3 + kRound) >> kShift;
  d[5] = (a5 + z2 + z4 + kRound) >> kShift;
  d[3] = (a6 + z2 + z3 + kRound) >> kShift;
  d[1] = (a7 + z1 + z4 + kRound) >> kShift;
}

// a Y block of MCU (mx, my) beyond the component's own block grid only fills the MCU (a dummy)
__device__ __forceinline__ bool y_block_real(const Geom& g, int mx, int my, int k) {
  return 16 * mx + 8 * (k & 1) < g.width && 16 * my + 8 * (k >> 1) < g.height;
}

template <int kMode>
__global__ void __launch_bounds__(256)
k_jpeg_blocks(const uint8_t* __restrict__ px, size_t step, Geom g, const Blob* __restrict__ blob,
              int16_t* __restrict__ coef) {
  __shared__ int s_pass[kBlocksPerGroup][8][9];
  __shared__ __attribute__((aligned(16))) int16_t s_out[kBlocksPerGroup][64];
  __shared__ uint16_t s_div[2][64];
  __shared__ uint8_t s_unzig[64];
  const int t = threadIdx.x;
  if (t < 128) s_div[t >> 6][t & 63] = blob->divisor[t >> 6][t & 63];
  else if (t < 192) s_unzig[t - 128] = d_unzig.at[t - 128];
  const int lb = t >> 3, r = t & 7;
  const unsigned b = blockIdx.x * (unsigned)kBlocksPerGroup + (unsigned)lb;
  const bool live = b < g.nb;
  int d[8];
  int table = 0;
  bool dummy = false;
  if (live) {
    const int W = g.width, H = g.height;
    if (!g.colour) {
      const int x0 = 8 * (int)(b % (unsigned)g.bw), y = min(8 * (int)(b / (unsigned)g.bw) + r, H - 1);
      const uint8_t* row = px + (size_t)y * step;
#pragma unroll
      for (int c = 0; c < 8; ++c) d[c] = (int)row[min(x0 + c, W - 1)] - 128;
    } else {
      const unsigned m = b / 6u;
      const int k = (int)(b - 6u * m);
      const int mx = (int)(m % (unsigned)g.bw), my = (int)(m / (unsigned)g.bw);
      if (k < 4) {
        dummy = !y_block_real(g, mx, my, k);
        const int x0 = 16 * mx + 8 * (k & 1), y = min(16 * my + 8 * (k >> 1) + r, H - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          int bb, gg, rr;
          load_bgr<kMode == kGray8 ? kBgr8 : kMode>(px, step, min(x0 + c, W - 1), y, &bb, &gg, &rr);
          d[c] = ycc_y(bb, gg, rr) - 128;
        }
      } else {
        // h2v2_downsample behind pre_process_data: pixels replicated to the right and down to an
        // even row count, (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 along the row, the
        // DOWNSAMPLED rows replicated down
        table = 1;
        const int cy = min(8 * my + r, (H + 1) / 2 - 1);
        const int ya = min(2 * cy, H - 1), yb = min(2 * cy + 1, H - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int cx = 8 * mx + c;
          const int xa = min(2 * cx, W - 1), xb = min(2 * cx + 1, W - 1);
          int sum = 1 + (cx & 1);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            int bb, gg, rr;
            load_bgr<kMode == kGray8 ? kBgr8 : kMode>(px, step, (q & 1) ? xb : xa, (q & 2) ? yb : ya, &bb,
                                                       &gg, &rr);
            sum += k == 4 ? ycc_cb(bb, gg, rr) : ycc_cr(bb, gg, rr);
          }
          d[c] = (sum >> 2) - 128;
        }
      }
    }
    fdct_1d<true>(d);
#pragma unroll
    for (int c = 0; c < 8; ++c) s_pass[lb][r][c] = d[c];
  }
  __syncthreads();
  if (live) {
    // the same lane, now column r
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s_pass[lb][i][r];
    fdct_1d<false>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // forward_DCT (jcdctmgr.c): (|c| + q / 2) / q with the sign restored, q = 8 * the table entry
      const int nat = 8 * i + r;
      const unsigned q = s_div[table][nat];
      const unsigned a = ((unsigned)abs(d[i]) + (q >> 1)) / q;
      s_out[lb][s_unzig[nat]] = dummy ? (int16_t)0 : (int16_t)(d[i] < 0 ? -(int)a : (int)a);
    }
  }
  __syncthreads();
  if (live)
    reinterpret_cast<uint4*>(coef)[(size_t)b * 8u + (size_t)r] =
        reinterpret_cast<const uint4*>(&s_out[lb][0])[r];
}

// ---------------------------------------------------------------------------
// passes 2 and 4: one walk over a block's symbols, two sinks
// ---------------------------------------------------------------------------
struct EntropyLds {
  uint32_t ac[2][256];
  uint32_t dc[2][12];
  uint32_t wave_sum[4];
};

__device__ __forceinline__ void load_tables(EntropyLds* s) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s->ac[i >> 8][i & 255] = d_huff.ac[i >> 8][i & 255];
  if (threadIdx.x < 24) s->dc[threadIdx.x / 12][threadIdx.x % 12] = d_huff.dc[threadIdx.x / 12][threadIdx.x % 12];
}

// exclusive prefix sum over the workgroup's 256 lanes; *total = the sum of all
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wave_sum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const uint32_t o = __shfl_up(incl, dlt);
    if (lane >= dlt) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = wave_sum[w];
    if (w < wave) base += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }   // a >= 0

// DC of the block the scan coded before Y block (m, k) in its component: dummies carry the DC of the
// block before them (jccoefct.c), so walk back to a real one.  Block 0 of an MCU is always real.
__device__ __forceinline__ int prev_y_dc(const int16_t* __restrict__ coef, const Geom& g, unsigned m, int k) {
  for (;;) {
    if (k == 0) {
      if (m == 0) return 0;
      --m;
      k = 3;
    } else {
      --k;
    }
    if (y_block_real(g, (int)(m % (unsigned)g.bw), (int)(m / (unsigned)g.bw), k))
      return coef[((size_t)m * 6u + (size_t)k) * 64u];
  }
}

// encode_one_block (jchuff.c) of scan block b into `sink.put(code, length)`
template <typename Sink>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ coef, const Geom& g, unsigned b,
                                           const EntropyLds* s, Sink& sink) {
  int table = 0, prev;
  if (!g.colour) {
    prev = b ? coef[(size_t)(b - 1) * 64u] : 0;
  } else {
    const unsigned m = b / 6u;
    const int k = (int)(b - 6u * m);
    if (k < 4) {
      if (!y_block_real(g, (int)(m % (unsigned)g.bw), (int)(m / (unsigned)g.bw), k)) {
        // a dummy: DC difference 0, EOB
        sink.put(s->dc[0][0] & 0xFFFFu, s->dc[0][0] >> 16);
        sink.put(s->ac[0][0] & 0xFFFFu, s->ac[0][0] >> 16);
        return;
      }
      prev = prev_y_dc(coef, g, m, k);
    } else {
      table = 1;
      prev = m ? coef[(size_t)(b - 6u) * 64u] : 0;
    }
  }
  const uint4* p = reinterpret_cast<const uint4*>(coef + (size_t)b * 64u);
  const uint32_t zrl = s->ac[table][0xF0];
  int run = 0;
#pragma unroll 1
  for (int j = 0; j < 8; ++j) {
    const uint4 q = p[j];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = (int)(int16_t)(w[i >> 1] >> (16 * (i & 1)));
      if (j == 0 && i == 0) {
        // the DC difference: category, then its low bits (value - 1 when negative)
        const int diff = v - prev;
        const int cat = bit_length(abs(diff));
        const uint32_t e = s->dc[table][cat];
        const uint32_t low = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
        sink.put(((e & 0xFFFFu) << cat) | low, (e >> 16) + cat);
      } else if (v == 0) {
        ++run;
      } else {
        for (; run > 15; run -= 16) sink.put(zrl & 0xFFFFu, zrl >> 16);
        const int size = bit_length(abs(v));
        const uint32_t e = s->ac[table][(run << 4) | size];
        const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        sink.put(((e & 0xFFFFu) << size) | low, (e >> 16) + size);
        run = 0;
      }
    }
  }
  if (run) sink.put(s->ac[table][0] & 0xFFFFu, s->ac[table][0] >> 16);
}

struct CountSink {
  uint32_t bits;
  __device__ __forceinline__ void put(uint32_t, uint32_t len) { bits += len; }
};

__global__ void __launch_bounds__(kTile)
k_jpeg_lengths(const int16_t* __restrict__ coef, Geom g, uint32_t* __restrict__ bits,
               unsigned long long* __restrict__ tile_sum) {
  __shared__ EntropyLds s;
  load_tables(&s);
  __syncthreads();
  const unsigned b = blockIdx.x * (unsigned)kTile + threadIdx.x;
  CountSink sink = {0};
  if (b < g.nb) {
    walk_block(coef, g, b, &s, sink);
    bits[b] = sink.bits;
  }
  uint32_t total;
  (void)block_excl_scan(sink.bits, s.wave_sum, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// a[0..n) -> its exclusive prefix sums, in place; *total = the sum.  One wave.  scan_bits (may be
// null): the bits of the scan, already on the device -- only the 4096-byte chunks the scan really
// fills are walked (the launch is sized for the worst case, the entries behind are never read).
__global__ void __launch_bounds__(64)
k_jpeg_scan_top(unsigned long long* __restrict__ a, unsigned n, unsigned long long* __restrict__ total,
                const unsigned long long* __restrict__ scan_bits) {
  const unsigned lane = threadIdx.x;
  if (scan_bits) {
    const unsigned long long used = (((*scan_bits + 7ull) >> 3) + (kChunk - 1)) / kChunk;
    if (used < n) n = (unsigned)used;
  }
  unsigned long long carry = 0;
  for (unsigned at = 0; at < n; at += 64) {
    const unsigned long long v = at + lane < n ? a[at + lane] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const uint32_t lo = __shfl_up((uint32_t)incl, dlt), hi = __shfl_up((uint32_t)(incl >> 32), dlt);
      if ((int)lane >= dlt) incl += ((unsigned long long)hi << 32) | lo;
    }
    if (at + lane < n) a[at + lane] = carry + incl - v;
    const uint32_t lo = __shfl((uint32_t)incl, 63), hi = __shfl((uint32_t)(incl >> 32), 63);
    carry += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0) *total = carry;
}

// MSB-first bit writer at bit `off` of a zeroed word array; words are stored byte-swapped so that
// the array's bytes are the stream's bytes
struct BitSink {
  uint32_t* words;
  size_t w;
  unsigned long long acc;
  uint32_t n;      // bits pending in acc, counting the bits in front of `off` in its word
  bool first;
  __device__ __forceinline__ void start(uint32_t* base, unsigned long long off) {
    words = base;
    w = (size_t)(off >> 5);
    n = (uint32_t)(off & 31u);
    acc = 0;
    first = true;
  }
  __device__ __forceinline__ void put(uint32_t code, uint32_t len) {   // len <= 27
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t word = __builtin_bswap32((uint32_t)(acc >> n));
      acc &= (1ull << n) - 1ull;
      // the word `off` lies in may hold a neighbour's bits; every later whole word is this block's
      if (first) atomicOr(words + w, word);
      else words[w] = word;
      first = false;
      ++w;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n) atomicOr(words + w, __builtin_bswap32((uint32_t)(acc << (32 - n))));
  }
};

__global__ void __launch_bounds__(kTile)
k_jpeg_pack(const int16_t* __restrict__ coef, Geom g, const uint32_t* __restrict__ bits,
            const unsigned long long* __restrict__ tile_off, uint32_t* __restrict__ words) {
  __shared__ EntropyLds s;
  load_tables(&s);
  __syncthreads();
  const unsigned b = blockIdx.x * (unsigned)kTile + threadIdx.x;
  const uint32_t mine = b < g.nb ? bits[b] : 0u;
  uint32_t total;
  const uint32_t excl = block_excl_scan(mine, s.wave_sum, &total);
  if (b >= g.nb) return;
  const unsigned long long off = tile_off[blockIdx.x] + excl;
  BitSink sink;
  sink.start(words, off);
  walk_block(coef, g, b, &s, sink);
  if (b == g.nb - 1) {
    // flush_bits (jchuff.c): the last byte is filled with 1-bits
    const uint32_t pad = (8u - (uint32_t)((off + mine) & 7u)) & 7u;
    if (pad) sink.put((1u << pad) - 1u, pad);
  }
  sink.flush();
}

// ---------------------------------------------------------------------------
// pass 5
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t count_ff(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t n = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) n += ((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 0xFFu;
  return n;
}

// (the words behind the scan's last byte are zero: no byte there counts)
__global__ void __launch_bounds__(256)
k_jpeg_ff_count(const uint32_t* __restrict__ words, const unsigned long long* __restrict__ ctrl,
                unsigned long long* __restrict__ chunk_ff) {
  __shared__ uint32_t s_wave[4];
  const unsigned long long nbytes = (ctrl[0] + 7ull) >> 3;
  const unsigned long long at = (unsigned long long)blockIdx.x * kChunk + 16ull * threadIdx.x;
  uint32_t n = 0;
  if (at < nbytes) n = count_ff(reinterpret_cast<const uint4*>(words)[at >> 4]);
  uint32_t total;
  (void)block_excl_scan(n, s_wave, &total);
  if (threadIdx.x == 0) chunk_ff[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
k_jpeg_stuff(const uint32_t* __restrict__ words, unsigned long long* __restrict__ ctrl,
             const unsigned long long* __restrict__ chunk_ff, const Blob* __restrict__ blob,
             uint8_t* __restrict__ out, unsigned long long cap) {
  __shared__ uint32_t s_wave[4];
  const unsigned long long nbytes = (ctrl[0] + 7ull) >> 3;
  const unsigned long long head = blob->header_bytes;
  const unsigned long long size = head + nbytes + ctrl[1] + 2ull;
  const bool fits = size <= cap;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      ctrl[2] = size;
      ctrl[3] = fits ? 0ull : 1ull;
    }
    if (fits) {
      for (unsigned i = threadIdx.x; i < (unsigned)head; i += blockDim.x) out[i] = blob->header[i];
      if (threadIdx.x == 0) {
        out[size - 2] = 0xFF;   // EOI
        out[size - 1] = 0xD9;
      }
    }
  }
  const unsigned long long chunk_at = (unsigned long long)blockIdx.x * kChunk;
  if (!fits || chunk_at >= nbytes) return;
  const unsigned long long at = chunk_at + 16ull * threadIdx.x;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (at < nbytes) v = reinterpret_cast<const uint4*>(words)[at >> 4];
  uint32_t total;
  const uint32_t before = block_excl_scan(at < nbytes ? count_ff(v) : 0u, s_wave, &total);
  if (at >= nbytes) return;
  uint8_t* dst = out + head + at + chunk_ff[blockIdx.x] + before;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const int live = (int)min(16ull, nbytes - at);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < live) {
      const uint8_t byte = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
      *dst++ = byte;
      if (byte == 0xFF) *dst++ = 0;
    }
  }
}

static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
void jpeg_scratch_free(JpegScratch* ws) {
  if (ws->dev) (void)hipFree(ws->dev);
  if (ws->image) (void)hipFree(ws->image);
  if (ws->out) (void)hipFree(ws->out);
  if (ws->pinned) (void)hipHostFree(ws->pinned);
  *ws = JpegScratch();
}

int jpeg_scratch_image(JpegScratch* ws, size_t bytes, uint8_t** out) {
  void* p = ws->image;
  const int rc = ensure_bytes(&p, &ws->image_cap, bytes);
  ws->image = static_cast<uint8_t*>(p);
  *out = ws->image;
  return rc;
}

namespace {

// where one call's buffers lie in the scratch, between its two halves
struct Plan {
  size_t nchunks;
  const Blob* blob;
  unsigned long long* ctrl;
  unsigned long long* chunk;
  uint32_t* words;
  unsigned long long* hres;   // pinned: two words read back
};

// passes 1 - 4 and the 0xFF counts with their prefix sums: everything but the copy into the
// caller's buffer.  Leaves ctrl[0] = bits of the scan, ctrl[1] = 0xFF bytes in it.
int encode_front(hipStream_t stream, JpegScratch* ws, const JpegSource& src, int quality, Plan* plan) {
  if (quality == 0) quality = 95;
  const int channels = src.mode == kGray8 ? 1 : 3;
  Geom g;
  g.width = src.width;
  g.height = src.height;
  g.colour = channels == 3;
  g.bw = g.colour ? (src.width + 15) / 16 : (src.width + 7) / 8;
  const size_t nb = jpeg::scan_blocks(src.width, src.height, channels);
  g.nb = (unsigned)nb;   // (65535^2 / 64 blocks at the most)
  const size_t ntiles = (nb + kTile - 1) / kTile;
  const size_t pack_bytes = round_up(nb * jpeg::kMaxBlockBytes + 1, kChunk);
  const size_t nchunks = pack_bytes / kChunk;
  // scratch: blob | ctrl | coefficients | bits | tile sums | chunk sums | packed words
  size_t at = 0;
  auto carve = [&](size_t n) {
    const size_t a = at;
    at += round_up(n, 256);
    return a;
  };
  const size_t o_blob = carve(sizeof(Blob)), o_ctrl = carve(kCtrlWords * 8), o_coef = carve(nb * 128),
               o_bits = carve(nb * 4), o_tile = carve(ntiles * 8), o_chunk = carve(nchunks * 8),
               o_pack = carve(pack_bytes);
  void* p = ws->dev;
  int rc = ensure_bytes(&p, &ws->cap, at);
  ws->dev = static_cast<uint8_t*>(p);
  if (rc) return rc;
  // pinned: two result words, then the blob
  if (!ws->pinned)
    AMHIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ws->pinned), 16 + sizeof(Blob), hipHostMallocDefault));
  Blob* hb = reinterpret_cast<Blob*>(ws->pinned + 16);
  uint8_t q[2][64];
  jpeg::quant_tables(quality, q);
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) hb->divisor[t][i] = (uint16_t)(8 * q[t][i]);
  hb->header_bytes = (uint32_t)jpeg::write_header(hb->header, sizeof(hb->header), src.width, src.height,
                                                  channels, quality);
  uint8_t* d = ws->dev;
  plan->nchunks = nchunks;
  plan->blob = reinterpret_cast<const Blob*>(d + o_blob);
  plan->ctrl = reinterpret_cast<unsigned long long*>(d + o_ctrl);
  plan->chunk = reinterpret_cast<unsigned long long*>(d + o_chunk);
  plan->words = reinterpret_cast<uint32_t*>(d + o_pack);
  plan->hres = reinterpret_cast<unsigned long long*>(ws->pinned);
  int16_t* coef = reinterpret_cast<int16_t*>(d + o_coef);
  uint32_t* bits = reinterpret_cast<uint32_t*>(d + o_bits);
  unsigned long long* tile = reinterpret_cast<unsigned long long*>(d + o_tile);
  unsigned long long* ctrl = plan->ctrl;
  AMHIP_TRY(hipMemcpyAsync(d + o_blob, hb, sizeof(Blob), hipMemcpyHostToDevice, stream));
  AMHIP_TRY(hipMemsetAsync(plan->words, 0, pack_bytes, stream));
  const dim3 gb((unsigned)((nb + kBlocksPerGroup - 1) / kBlocksPerGroup));
  const uint8_t* px = static_cast<const uint8_t*>(src.dev);
  if (src.mode == kGray8)
    hipLaunchKernelGGL(k_jpeg_blocks<kGray8>, gb, dim3(256), 0, stream, px, src.step, g, plan->blob, coef);
  else if (src.mode == kBgr8)
    hipLaunchKernelGGL(k_jpeg_blocks<kBgr8>, gb, dim3(256), 0, stream, px, src.step, g, plan->blob, coef);
  else
    hipLaunchKernelGGL(k_jpeg_blocks<kBgr16s>, gb, dim3(256), 0, stream, px, src.step, g, plan->blob, coef);
  hipLaunchKernelGGL(k_jpeg_lengths, dim3((unsigned)ntiles), dim3(kTile), 0, stream, coef, g, bits, tile);
  hipLaunchKernelGGL(k_jpeg_scan_top, dim3(1), dim3(64), 0, stream, tile, (unsigned)ntiles, ctrl + 0,
                     static_cast<const unsigned long long*>(nullptr));
  hipLaunchKernelGGL(k_jpeg_pack, dim3((unsigned)ntiles), dim3(kTile), 0, stream, coef, g, bits, tile, plan->words);
  hipLaunchKernelGGL(k_jpeg_ff_count, dim3((unsigned)nchunks), dim3(256), 0, stream, plan->words, ctrl,
                     plan->chunk);
  hipLaunchKernelGGL(k_jpeg_scan_top, dim3(1), dim3(64), 0, stream, plan->chunk, (unsigned)nchunks, ctrl + 1,
                     static_cast<const unsigned long long*>(ctrl));
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

// the copy into dev_out over `chunks` 4096-byte chunks of the scan, then the one read-back: the
// file's size and whether it fitted
int encode_back(hipStream_t stream, const Plan& plan, size_t chunks, uint8_t* dev_out, size_t cap, size_t* bytes) {
  hipLaunchKernelGGL(k_jpeg_stuff, dim3((unsigned)chunks), dim3(256), 0, stream, plan.words, plan.ctrl,
                     plan.chunk, plan.blob, dev_out, (unsigned long long)cap);
  AMHIP_TRY(hipGetLastError());
  AMHIP_TRY(hipMemcpyAsync(plan.hres, plan.ctrl + 2, 16, hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  if (bytes) *bytes = (size_t)plan.hres[0];
  if (plan.hres[1]) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "jpeg: the file takes %llu bytes, the buffer holds %llu (nothing written)",
                  plan.hres[0], (unsigned long long)cap);
    return arg_failure(msg);
  }
  return AMHIP_OK;
}

}  // namespace

int jpeg_encode_run(hipStream_t stream, JpegScratch* ws, const JpegSource& src, int quality,
                    uint8_t* dev_out, size_t cap, size_t* bytes) {
  Plan plan;
  const int rc = encode_front(stream, ws, src, quality, &plan);
  if (rc) return rc;
  return encode_back(stream, plan, plan.nchunks, dev_out, cap, bytes);
}

namespace {

// the file -> host memory.  The scan's size is read back before the last pass, so the scratch's
// output buffer holds the file as it is, not its worst case (a second, 16-byte read-back).
int encode_to_host(hipStream_t stream, JpegScratch* ws, const JpegSource& src, int quality,
                   std::vector<uint8_t>* file) {
  Plan plan;
  int rc = encode_front(stream, ws, src, quality, &plan);
  if (rc) return rc;
  AMHIP_TRY(hipMemcpyAsync(plan.hres, plan.ctrl, 16, hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  const size_t scan_bytes = (size_t)((plan.hres[0] + 7ull) >> 3);
  const size_t size = jpeg::kMaxHeaderBytes + scan_bytes + (size_t)plan.hres[1] + 2;   // (the header: at most)
  void* p = ws->out;
  rc = ensure_bytes(&p, &ws->out_cap, size);
  ws->out = static_cast<uint8_t*>(p);
  if (rc) return rc;
  size_t n = 0;
  if ((rc = encode_back(stream, plan, (scan_bytes + kChunk - 1) / kChunk, ws->out, size, &n))) return rc;
  file->resize(n);
  AMHIP_TRY(hipMemcpyAsync(file->data(), ws->out, n, hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  return AMHIP_OK;
}

// (the status enum has no I/O code: a file that cannot be written is AMHIP_ERR_ARG, as in the
// GeoTiff and point-cloud writers, with errno's text)
int write_failure(const char* what, const char* filename, int err) {
  set_last_error(std::string(what) + ": cannot write " + filename + ": " + std::strerror(err));
  return AMHIP_ERR_ARG;
}

int write_file(const char* what, const char* filename, const std::vector<uint8_t>& file) {
  const int fd = ::open(filename, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return write_failure(what, filename, errno);
  size_t done = 0;
  while (done < file.size()) {
    const ssize_t w = ::write(fd, file.data() + done, file.size() - done);
    if (w < 0 && errno == EINTR) continue;
    if (w < 0) {
      const int err = errno;   // (close() below may change it)
      (void)::close(fd);
      return write_failure(what, filename, err);
    }
    done += (size_t)w;
  }
  if (::close(fd) != 0) return write_failure(what, filename, errno);
  return AMHIP_OK;
}

}  // namespace

int jpeg_write_run(const char* what, hipStream_t stream, JpegScratch* ws, const JpegSource& src,
                   int quality, const char* filename) {
  std::vector<uint8_t> file;
  const int rc = encode_to_host(stream, ws, src, quality, &file);
  if (rc) return rc;
  return write_file(what, filename, file);
}

}  // namespace amhip

using namespace amhip;

extern "C" {

size_t amhip_jpeg_bound(int width, int height, int channels) {
  if (width < 1 || width > 65535 || height < 1 || height > 65535 || (channels != 1 && channels != 3)) return 0;
  return jpeg::file_bound(width, height, channels);
}

int amhip_jpeg_encode_dev(amhip_ctx* h, const uint8_t* dev_pixels, size_t step, int width, int height,
                          int channels, int quality, uint8_t* dev_out, size_t cap, size_t* bytes) {
  if (!h || !dev_pixels || !dev_out || !bytes) return arg_failure("amhip_jpeg_encode_dev: null argument");
  if (const char* why = jpeg::check_image_args(step, width, height, channels, quality))
    return arg_failure((std::string("amhip_jpeg_encode_dev: ") + why).c_str());
  Ctx* c = &h->impl;
  int rc = ctx_use_device(c);
  if (rc) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  const JpegSource src = {dev_pixels, step, width, height, channels == 1 ? kGray8 : kBgr8};
  return jpeg_encode_run(c->stream, &c->jpeg, src, quality, dev_out, cap, bytes);
}

int amhip_jpeg_write(amhip_ctx* h, const char* filename, const uint8_t* pixels, int on_device, size_t step,
                     int width, int height, int channels, int quality) {
  if (!h || !filename || !pixels) return arg_failure("amhip_jpeg_write: null argument");
  if (const char* why = jpeg::check_image_args(step, width, height, channels, quality))
    return arg_failure((std::string("amhip_jpeg_write: ") + why).c_str());
  Ctx* c = &h->impl;
  int rc = ctx_use_device(c);
  if (rc) return rc;
  JpegSource src = {pixels, step, width, height, channels == 1 ? kGray8 : kBgr8};
  if (!on_device) {
    const size_t row = (size_t)width * (size_t)channels;
    uint8_t* dev = nullptr;
    if ((rc = jpeg_scratch_image(&c->jpeg, row * (size_t)height, &dev))) return rc;
    AMHIP_TRY(hipMemcpy2DAsync(dev, row, pixels, step, row, (size_t)height, hipMemcpyHostToDevice, c->stream));
    src.dev = dev;
    src.step = row;
  }
  ScopedTimer timer(c, AMHIP_K_MISC);
  return jpeg_write_run("amhip_jpeg_write", c->stream, &c->jpeg, src, quality, filename);
}

int amhip_layer_write_jpeg(amhip_ctx* h, int layer, int bgr, float lower, float upper, int quality,
                           const char* filename) {
  if (!h || !filename || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_layer_write_jpeg: bad argument");
  if (quality < 0 || quality > 100) return arg_failure("amhip_layer_write_jpeg: quality must be 1..100 (0: 95)");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_layer_write_jpeg: upper <= lower");
  Ctx* c = &h->impl;
  if (c->win_rows < 1 || c->win_cols < 1 || c->win_rows > 65535 || c->win_cols > 65535)
    return arg_failure("amhip_layer_write_jpeg: a JPEG file holds 1 x 1 to 65535 x 65535 pixels");
  int rc = ctx_use_device(c);
  if (rc) return rc;
  const size_t row = (size_t)c->win_cols * (bgr ? 3u : 1u);
  uint8_t* dev = nullptr;
  if ((rc = jpeg_scratch_image(&c->jpeg, row * (size_t)c->win_rows, &dev))) return rc;
  if ((rc = amhip_layer_to_image_dev(h, layer, bgr, lower, upper, dev, row))) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  const JpegSource src = {dev, row, c->win_cols, c->win_rows, bgr ? kBgr8 : kGray8};
  return jpeg_write_run("amhip_layer_write_jpeg", c->stream, &c->jpeg, src, quality, filename);
}

}  // extern "C"
