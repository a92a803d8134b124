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
// A stack of frames (amhip_io_encode_jpeg_frames, amhip_io_write_jpeg_frames) takes the
// same passes once per group of frames: the k_jpegf_* kernels run a pass's body with the frame on
// grid row y, and k_jpegf_offsets lays the group's files end to end.
#include <cstring>
#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_frame_stack.h"
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

// the body of pass 1, for workgroup `group` of one image's grid (k_jpeg_blocks, k_jpegf_blocks)
template <int kMode>
__device__ __forceinline__ void blocks_body(const uint8_t* __restrict__ px, size_t step, const Geom& g,
                                            const Blob* __restrict__ blob, int16_t* __restrict__ coef,
                                            unsigned group) {
  __shared__ int s_pass[kBlocksPerGroup][8][9];
  __shared__ __attribute__((aligned(16))) int16_t s_out[kBlocksPerGroup][64];
  __shared__ uint16_t s_div[2][64];
  __shared__ uint8_t s_unzig[64];
  const int t = threadIdx.x;
  if (t < 128) s_div[t >> 6][t & 63] = blob->divisor[t >> 6][t & 63];
  else if (t < 192) s_unzig[t - 128] = d_unzig.at[t - 128];
  const int lb = t >> 3, r = t & 7;
  const unsigned b = group * (unsigned)kBlocksPerGroup + (unsigned)lb;
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

template <int kMode>
__global__ void __launch_bounds__(256)
k_jpeg_blocks(const uint8_t* __restrict__ px, size_t step, Geom g, const Blob* __restrict__ blob,
              int16_t* __restrict__ coef) {
  blocks_body<kMode>(px, step, g, blob, coef, blockIdx.x);
}

// frame blockIdx.y of a stack: its pixels at px + f * frame_stride, its coefficients at coef + f * nb * 64
template <int kMode>
__global__ void __launch_bounds__(256)
k_jpegf_blocks(const uint8_t* __restrict__ px, size_t step, size_t frame_stride, Geom g,
               const Blob* __restrict__ blob, int16_t* __restrict__ coef) {
  const size_t f = blockIdx.y;
  blocks_body<kMode>(px + f * frame_stride, step, g, blob, coef + f * (size_t)g.nb * 64u, blockIdx.x);
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

// the body of pass 2 for tile `tile` of one image (coef, bits, tile_sum: that image's)
__device__ __forceinline__ void lengths_body(const int16_t* __restrict__ coef, const Geom& g,
                                             uint32_t* __restrict__ bits,
                                             unsigned long long* __restrict__ tile_sum, unsigned tile) {
  __shared__ EntropyLds s;
  load_tables(&s);
  __syncthreads();
  const unsigned b = tile * (unsigned)kTile + threadIdx.x;
  CountSink sink = {0};
  if (b < g.nb) {
    walk_block(coef, g, b, &s, sink);
    bits[b] = sink.bits;
  }
  uint32_t total;
  (void)block_excl_scan(sink.bits, s.wave_sum, &total);
  if (threadIdx.x == 0) tile_sum[tile] = total;
}

__global__ void __launch_bounds__(kTile)
k_jpeg_lengths(const int16_t* __restrict__ coef, Geom g, uint32_t* __restrict__ bits,
               unsigned long long* __restrict__ tile_sum) {
  lengths_body(coef, g, bits, tile_sum, blockIdx.x);
}

// a[0..n) -> its exclusive prefix sums, in place; *total = the sum.  One wave.  scan_bits (may be
// null): the bits of the scan, already on the device -- only the 4096-byte chunks the scan really
// fills are walked (the launch is sized for the worst case, the entries behind are never read).
__device__ __forceinline__ void scan_top_body(unsigned long long* __restrict__ a, unsigned n,
                                              unsigned long long* __restrict__ total,
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

__global__ void __launch_bounds__(64)
k_jpeg_scan_top(unsigned long long* __restrict__ a, unsigned n, unsigned long long* __restrict__ total,
                const unsigned long long* __restrict__ scan_bits) {
  scan_top_body(a, n, total, scan_bits);
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

// the body of pass 4 for tile `tile` of one image; `words`: that image's zeroed packed words
__device__ __forceinline__ void pack_body(const int16_t* __restrict__ coef, const Geom& g,
                                          const uint32_t* __restrict__ bits,
                                          const unsigned long long* __restrict__ tile_off,
                                          uint32_t* __restrict__ words, unsigned tile) {
  __shared__ EntropyLds s;
  load_tables(&s);
  __syncthreads();
  const unsigned b = tile * (unsigned)kTile + threadIdx.x;
  const uint32_t mine = b < g.nb ? bits[b] : 0u;
  uint32_t total;
  const uint32_t excl = block_excl_scan(mine, s.wave_sum, &total);
  if (b >= g.nb) return;
  const unsigned long long off = tile_off[tile] + excl;
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

__global__ void __launch_bounds__(kTile)
k_jpeg_pack(const int16_t* __restrict__ coef, Geom g, const uint32_t* __restrict__ bits,
            const unsigned long long* __restrict__ tile_off, uint32_t* __restrict__ words) {
  pack_body(coef, g, bits, tile_off, words, blockIdx.x);
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

// ---------------------------------------------------------------------------
// a stack of frames (amhip_io_encode_jpeg_frames): the same five passes, frame f of the group on
// grid row f.  Width, height, channels and quality are the call's, so Geom and Blob are shared; a
// frame has its own coefficients, bit counts, tile sums, chunk sums and packed words (every region
// is `n frames x one frame's share`, the packed words a multiple of kChunk per frame: no word and
// no stuffing chunk is shared between two frames) and one control record.
// ---------------------------------------------------------------------------
struct FrameCtrl {
  unsigned long long bits;     // of the frame's scan
  unsigned long long ff;       // 0xFF bytes in it
  unsigned long long size;     // the frame's file
  unsigned long long offset;   // of the file in the group's output
};

// what one frame takes of each region
struct FrameShare {
  unsigned ntiles, nchunks;
  size_t pack_words;   // nchunks * kChunk / 4
};

__global__ void __launch_bounds__(kTile)
k_jpegf_lengths(const int16_t* __restrict__ coef, Geom g, FrameShare fs, uint32_t* __restrict__ bits,
                unsigned long long* __restrict__ tile_sum) {
  const size_t f = blockIdx.y;
  lengths_body(coef + f * (size_t)g.nb * 64u, g, bits + f * (size_t)g.nb, tile_sum + f * (size_t)fs.ntiles,
               blockIdx.x);
}

// one wave per frame.  chunks == 0: the frame's tile sums -> bit offsets, the total -> ctrl.bits;
// chunks != 0: its chunks' 0xFF counts -> their prefix sums, the total -> ctrl.ff.
__global__ void __launch_bounds__(64)
k_jpegf_scan(unsigned long long* __restrict__ a, unsigned per_frame, FrameCtrl* __restrict__ ctrl, int chunks) {
  const size_t f = blockIdx.x;
  scan_top_body(a + f * (size_t)per_frame, per_frame, chunks ? &ctrl[f].ff : &ctrl[f].bits,
                chunks ? &ctrl[f].bits : nullptr);
}

__global__ void __launch_bounds__(kTile)
k_jpegf_pack(const int16_t* __restrict__ coef, Geom g, FrameShare fs, const uint32_t* __restrict__ bits,
             const unsigned long long* __restrict__ tile_off, uint32_t* __restrict__ words) {
  const size_t f = blockIdx.y;
  pack_body(coef + f * (size_t)g.nb * 64u, g, bits + f * (size_t)g.nb, tile_off + f * (size_t)fs.ntiles,
            words + f * fs.pack_words, blockIdx.x);
}

__global__ void __launch_bounds__(256)
k_jpegf_ff_count(const uint32_t* __restrict__ words, FrameShare fs, const FrameCtrl* __restrict__ ctrl,
                 unsigned long long* __restrict__ chunk_ff) {
  __shared__ uint32_t s_wave[4];
  const size_t f = blockIdx.y;
  const unsigned long long nbytes = (ctrl[f].bits + 7ull) >> 3;
  const unsigned long long at = (unsigned long long)blockIdx.x * kChunk + 16ull * threadIdx.x;
  uint32_t n = 0;
  if (at < nbytes) n = count_ff(reinterpret_cast<const uint4*>(words + f * fs.pack_words)[at >> 4]);
  uint32_t total;
  (void)block_excl_scan(n, s_wave, &total);
  if (threadIdx.x == 0) chunk_ff[f * (size_t)fs.nchunks + blockIdx.x] = total;
}

// one wave: every frame's file size, and where the file starts behind the files before it (64 bit)
__global__ void __launch_bounds__(64)
k_jpegf_offsets(FrameCtrl* __restrict__ ctrl, unsigned n, const Blob* __restrict__ blob,
                unsigned long long* __restrict__ sizes) {
  const unsigned lane = threadIdx.x;
  const unsigned long long head = blob->header_bytes;
  unsigned long long carry = 0;
  for (unsigned at = 0; at < n; at += 64) {
    const bool live = at + lane < n;
    const unsigned long long v = live ? head + ((ctrl[at + lane].bits + 7ull) >> 3) + ctrl[at + lane].ff + 2ull : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const uint32_t lo = __shfl_up((uint32_t)incl, dlt), hi = __shfl_up((uint32_t)(incl >> 32), dlt);
      if ((int)lane >= dlt) incl += ((unsigned long long)hi << 32) | lo;
    }
    if (live) {
      ctrl[at + lane].size = v;
      ctrl[at + lane].offset = carry + incl - v;
      sizes[at + lane] = v;
    }
    const uint32_t lo = __shfl((uint32_t)incl, 63), hi = __shfl((uint32_t)(incl >> 32), 63);
    carry += ((unsigned long long)hi << 32) | lo;
  }
}

// header, stuffed scan and EOI of frame blockIdx.y at out + its offset.  `out` holds exactly the
// group's files (it was sized from `sizes`), so there is no capacity to check.
__global__ void __launch_bounds__(256)
k_jpegf_stuff(const uint32_t* __restrict__ words, FrameShare fs, const FrameCtrl* __restrict__ ctrl,
              const unsigned long long* __restrict__ chunk_ff, const Blob* __restrict__ blob,
              uint8_t* __restrict__ out) {
  __shared__ uint32_t s_wave[4];
  const size_t f = blockIdx.y;
  const unsigned long long nbytes = (ctrl[f].bits + 7ull) >> 3;
  const unsigned long long head = blob->header_bytes;
  const unsigned long long size = ctrl[f].size;
  out += ctrl[f].offset;
  if (blockIdx.x == 0) {
    for (unsigned i = threadIdx.x; i < (unsigned)head; i += blockDim.x) out[i] = blob->header[i];
    if (threadIdx.x == 0) {
      out[size - 2] = 0xFF;   // EOI
      out[size - 1] = 0xD9;
    }
  }
  const unsigned long long chunk_at = (unsigned long long)blockIdx.x * kChunk;
  if (chunk_at >= nbytes) return;
  const unsigned long long at = chunk_at + 16ull * threadIdx.x;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (at < nbytes) v = reinterpret_cast<const uint4*>(words + f * fs.pack_words)[at >> 4];
  uint32_t total;
  const uint32_t before = block_excl_scan(at < nbytes ? count_ff(v) : 0u, s_wave, &total);
  if (at >= nbytes) return;
  uint8_t* dst = out + head + at + chunk_ff[f * (size_t)fs.nchunks + blockIdx.x] + before;
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
  if (plan.hres[1]) return capacity_failure("jpeg", plan.hres[0], cap);
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

}  // namespace

int jpeg_write_run(const char* what, hipStream_t stream, JpegScratch* ws, const JpegSource& src,
                   int quality, const char* filename) {
  std::vector<uint8_t> file;
  const int rc = encode_to_host(stream, ws, src, quality, &file);
  if (rc) return rc;
  return write_file(what, filename, file.data(), file.size());
}

// ---------------------------------------------------------------------------
// host: a stack of frames
// ---------------------------------------------------------------------------
namespace {

// One call of amhip_io_encode_jpeg_frames / amhip_io_write_jpeg_frames: the geometry every frame
// shares, the groups (amhip_frame_plan.h: a frame costs its scratch, the budget is the tuning key
// jpege_scratch_budget_mb), the scratch of the largest group and the sizes of all files.
struct FramesEncoder : EncodeGroups {
  Geom g;
  FrameShare fs;
  int channels = 0, quality = 0;
  size_t row_step = 0, fstride = 0, nb = 0, pack_bytes = 0;
  DevBuf blob;

  // where the buffers of a group of n frames lie in the scratch
  struct Layout {
    size_t ctrl, sizes, coef, bits, tile, chunk, pack, total;
  };
  Layout layout(size_t n) const {
    Layout l;
    size_t at = 0;
    auto carve = [&](size_t bytes) {
      const size_t a = at;
      at += round_up(bytes, kChunk);
      return a;
    };
    l.ctrl = carve(n * sizeof(FrameCtrl));
    l.sizes = carve(n * 8);
    l.coef = carve(n * nb * 128);
    l.bits = carve(n * nb * 4);
    l.tile = carve(n * (size_t)fs.ntiles * 8);
    l.chunk = carve(n * (size_t)fs.nchunks * 8);
    l.pack = carve(n * pack_bytes);
    l.total = at;
    return l;
  }
  size_t frame_stride() const { return fstride; }
  // the bytes of the stack that group gi's frames span
  size_t group_span(size_t gi) const { return (group_frames(gi) - 1) * fstride + (size_t)g.height * row_step; }

  // host only: geometry and groups
  void plan(size_t frames, int width, int height, int ch, size_t rstep, size_t stride, int q) {
    channels = ch;
    quality = q ? q : 95;
    row_step = rstep;
    fstride = frames > 1 ? stride : 0;
    g.width = width;
    g.height = height;
    g.colour = ch == 3;
    g.bw = g.colour ? (width + 15) / 16 : (width + 7) / 8;
    nb = jpeg::scan_blocks(width, height, ch);
    g.nb = (unsigned)nb;
    pack_bytes = round_up(nb * jpeg::kMaxBlockBytes + 1, kChunk);
    fs.ntiles = (unsigned)((nb + kTile - 1) / kTile);
    fs.nchunks = (unsigned)(pack_bytes / kChunk);
    fs.pack_words = pack_bytes / 4;
    // a frame's scratch: coefficients, bit counts and packed words of every scan block, its tile
    // and chunk sums, its control record and its size word
    const size_t cost = nb * (128 + 4) + pack_bytes + ((size_t)fs.ntiles + fs.nchunks) * 8 + sizeof(FrameCtrl) + 8;
    plan_uniform(frames, cost, "jpege_scratch_budget_mb", 4096.0, kMaxGroupFrames);
  }

  int open() {
    int rc;
    if ((rc = scratch.alloc(layout(most_group_frames()).total))) return rc;
    if ((rc = blob.alloc(sizeof(Blob)))) return rc;
    Blob hb;
    std::memset(&hb, 0, sizeof(hb));
    uint8_t q[2][64];
    jpeg::quant_tables(quality, q);
    for (int t = 0; t < 2; ++t)
      for (int i = 0; i < 64; ++i) hb.divisor[t][i] = (uint16_t)(8 * q[t][i]);
    hb.header_bytes = (uint32_t)jpeg::write_header(hb.header, sizeof(hb.header), g.width, g.height, channels, quality);
    AMHIP_TRY(hipMemcpy(blob.p, &hb, sizeof(Blob), hipMemcpyHostToDevice));
    return AMHIP_OK;
  }

  // passes 1 - 5 of group gi up to its files' sizes and offsets; `px`: the group's first frame.
  // Reads back the sizes, nothing else.
  int front(size_t gi, const uint8_t* px) {
    const size_t n = group_frames(gi);
    const Layout l = layout(n);
    uint8_t* d = scratch.as<uint8_t>();
    FrameCtrl* ctrl = reinterpret_cast<FrameCtrl*>(d + l.ctrl);
    unsigned long long* dsizes = reinterpret_cast<unsigned long long*>(d + l.sizes);
    int16_t* coef = reinterpret_cast<int16_t*>(d + l.coef);
    uint32_t* bits = reinterpret_cast<uint32_t*>(d + l.bits);
    unsigned long long* tile = reinterpret_cast<unsigned long long*>(d + l.tile);
    unsigned long long* chunk = reinterpret_cast<unsigned long long*>(d + l.chunk);
    uint32_t* words = reinterpret_cast<uint32_t*>(d + l.pack);
    const Blob* b = blob.as<const Blob>();
    AMHIP_TRY(hipMemsetAsync(words, 0, n * pack_bytes, stream));
    const dim3 gb((unsigned)((nb + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)n);
    if (channels == 1)
      hipLaunchKernelGGL(k_jpegf_blocks<kGray8>, gb, dim3(256), 0, stream, px, row_step, fstride, g, b, coef);
    else
      hipLaunchKernelGGL(k_jpegf_blocks<kBgr8>, gb, dim3(256), 0, stream, px, row_step, fstride, g, b, coef);
    const dim3 gt(fs.ntiles, (unsigned)n), gc(fs.nchunks, (unsigned)n);
    hipLaunchKernelGGL(k_jpegf_lengths, gt, dim3(kTile), 0, stream, coef, g, fs, bits, tile);
    hipLaunchKernelGGL(k_jpegf_scan, dim3((unsigned)n), dim3(64), 0, stream, tile, fs.ntiles, ctrl, 0);
    hipLaunchKernelGGL(k_jpegf_pack, gt, dim3(kTile), 0, stream, coef, g, fs, bits, tile, words);
    hipLaunchKernelGGL(k_jpegf_ff_count, gc, dim3(256), 0, stream, words, fs, ctrl, chunk);
    hipLaunchKernelGGL(k_jpegf_scan, dim3((unsigned)n), dim3(64), 0, stream, chunk, fs.nchunks, ctrl, 1);
    hipLaunchKernelGGL(k_jpegf_offsets, dim3(1), dim3(64), 0, stream, ctrl, (unsigned)n, b, dsizes);
    AMHIP_TRY(hipGetLastError());
    AMHIP_TRY(hipMemcpyAsync(sizes.data() + group_begin[gi], dsizes, n * 8, hipMemcpyDeviceToHost, stream));
    AMHIP_TRY(hipStreamSynchronize(stream));
    return AMHIP_OK;
  }

  // ... and the copy of group gi's files to out + at, which holds group_bytes(gi) bytes.  front(gi)
  // ran last.
  int back(size_t gi, uint8_t* out, uint64_t at) {
    const size_t n = group_frames(gi);
    const Layout l = layout(n);
    uint8_t* d = scratch.as<uint8_t>();
    // (a file is its scan and more: no scan has more chunks than the largest file)
    const unsigned chunks = (unsigned)((largest_file(gi) + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(k_jpegf_stuff, dim3(chunks < fs.nchunks ? chunks : fs.nchunks, (unsigned)n), dim3(256), 0,
                       stream, reinterpret_cast<const uint32_t*>(d + l.pack), fs,
                       reinterpret_cast<const FrameCtrl*>(d + l.ctrl),
                       reinterpret_cast<const unsigned long long*>(d + l.chunk), blob.as<const Blob>(), out + at);
    AMHIP_TRY(hipGetLastError());
    return AMHIP_OK;
  }
};

// the argument rules of both entry points (the text names the export and the field), then the plan
int plan_frames(const char* who, FramesEncoder* enc, size_t F, int width, int height, int channels, size_t row_step,
                size_t frame_stride, int quality) {
  auto fail = [who](const std::string& msg) {
    set_last_error(std::string(who) + ": " + msg);
    return AMHIP_ERR_ARG;
  };
  if (F == 0) return fail("no frames (F = 0)");
  if (width < 1 || width > 65535) return fail("width must be 1..65535");
  if (height < 1 || height > 65535) return fail("height must be 1..65535");
  if (channels != 1 && channels != 3) return fail("channels must be 1 (8UC1) or 3 (8UC3, B G R)");
  if (row_step < (size_t)width * (size_t)channels) return fail("row_step smaller than an image row");
  if (F > 1 && frame_stride < (size_t)height * row_step) return fail("frame_stride smaller than a frame");
  if (quality < 0 || quality > 100) return fail("quality must be 1..100 (0: 95)");
  enc->plan(F, width, height, channels, row_step, frame_stride, quality);
  return AMHIP_OK;
}

}  // namespace

// a host image -> the context's image scratch, rows packed; *src then names the copy
int stage_host_image(Ctx* c, int channels, JpegSource* src) {
  const size_t row = (size_t)src->width * (size_t)channels;
  uint8_t* dev = nullptr;
  const int rc = jpeg_scratch_image(&c->jpeg, row * (size_t)src->height, &dev);
  if (rc) return rc;
  AMHIP_TRY(hipMemcpy2DAsync(dev, row, src->dev, src->step, row, (size_t)src->height, hipMemcpyHostToDevice,
                             c->stream));
  src->dev = dev;
  src->step = row;
  return AMHIP_OK;
}

// the context's window of `layer` as an image in its image scratch (amhip_layer_to_image_dev) -> *src;
// limit: the format's refusal of a window no file of it holds
int layer_image_source(amhip_ctx* h, const char* limit, int layer, int bgr, float lower, float upper, JpegSource* src) {
  Ctx* c = &h->impl;
  if (!image_size_ok(c->win_rows, c->win_cols)) return arg_failure(limit);
  int rc = ctx_use_device(c);
  if (rc) return rc;
  const size_t row = (size_t)c->win_cols * (bgr ? 3u : 1u);
  uint8_t* dev = nullptr;
  if ((rc = jpeg_scratch_image(&c->jpeg, row * (size_t)c->win_rows, &dev))) return rc;
  if ((rc = amhip_layer_to_image_dev(h, layer, bgr, lower, upper, dev, row))) return rc;
  *src = JpegSource{dev, row, c->win_cols, c->win_rows, bgr ? kJpegBgr8 : kJpegGray8};
  return AMHIP_OK;
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
  if (!on_device && (rc = stage_host_image(c, channels, &src))) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  return jpeg_write_run("amhip_jpeg_write", c->stream, &c->jpeg, src, quality, filename);
}

int amhip_layer_write_jpeg(amhip_ctx* h, int layer, int bgr, float lower, float upper, int quality,
                           const char* filename) {
  if (!h || !filename || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_layer_write_jpeg: bad argument");
  if (quality < 0 || quality > 100) return arg_failure("amhip_layer_write_jpeg: quality must be 1..100 (0: 95)");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_layer_write_jpeg: upper <= lower");
  JpegSource src;
  const int rc = layer_image_source(h, "amhip_layer_write_jpeg: a JPEG file holds 1 x 1 to 65535 x 65535 pixels", layer,
                                    bgr, lower, upper, &src);
  if (rc) return rc;
  Ctx* c = &h->impl;
  ScopedTimer timer(c, AMHIP_K_MISC);
  return jpeg_write_run("amhip_layer_write_jpeg", c->stream, &c->jpeg, src, quality, filename);
}

int amhip_io_encode_jpeg_frames(int device, const uint8_t* dev_frames, size_t F, int width, int height,
                                int channels, size_t row_step, size_t frame_stride, int quality,
                                uint8_t** dev_files, size_t* offsets) {
  static const char kWho[] = "amhip_io_encode_jpeg_frames";
  return encode_frame_stack<FramesEncoder>(kWho, device, dev_frames, dev_files, offsets, [&](FramesEncoder* enc) {
    return plan_frames(kWho, enc, F, width, height, channels, row_step, frame_stride, quality);
  });
}

int amhip_io_write_jpeg_frames(int device, const uint8_t* frames, int on_device, size_t F, int width,
                               int height, int channels, size_t row_step, size_t frame_stride, int quality,
                               const char* const* filenames) {
  static const char kWho[] = "amhip_io_write_jpeg_frames";
  return write_frame_stack<FramesEncoder>(kWho, device, frames, on_device, filenames, [&](FramesEncoder* enc) {
    return plan_frames(kWho, enc, F, width, height, channels, row_step, frame_stride, quality);
  });
}

}  // extern "C"
