// amhip_png_encode.hip -- PNG files, encoded on the GPU: the file libpng and zlib write for
// cv::imwrite(name, image) when the name ends in .png and no parameter is given.  Filter Sub on
// every row; zlib at level 1 with strategy Z_RLE (window 15, memLevel 8); IDAT payloads of 8192
// bytes; 8UC1 as colour type 0, 8UC3 (B, G, R) as colour type 2, the mosaic's CV_16SC3 clamped to
// 0..255 as result8() clamps it.  Byte for byte what tests/png_encode_reference.py restates and
// what zlib 1.2.11 wrote into tests/golden/png_encode/.  DESIGN 4.15.
//
// Under Z_RLE a match has distance 1, so the tokens are a function of the runs of equal bytes, and
// everything behind the tokens is integer arithmetic per block of 16383 symbols.  A stack of F
// frames (one image: a stack of one) goes through these passes, the frame on the grid's second
// dimension or one workgroup per frame:
//   k_pnge_filter       a lane per 16 bytes of scanline: pixels -> Sub-filtered bytes; per tile of
//                       4096 bytes the two Adler sums and the last run start
//   k_pnge_scan_runs    per frame: the run start every tile inherits (a max-scan), Adler-32
//   k_pnge_tokens<0>    a lane per 16 bytes: which bytes start a symbol (rule 4 per run); counts per tile
//   k_pnge_scan_counts  per frame: every tile's first symbol index, the symbol and block counts
//   k_pnge_tokens<1>    the same walk, now writing the symbols and each block's first byte
//   k_pnge_plan         a wave per block: histogram in LDS, then one lane runs _tr_flush_block's
//                       arithmetic (amhip_png_encode_host.h: plan_block)
//   k_pnge_offsets      a wave per frame: every block's bit offset (a stored block pads to a byte),
//                       the stream's and the file's size, the zlib header and trailer
//   k_pnge_pack         a workgroup per block: code lengths scanned, codes written LSB first; whole
//                       words stored, the words a lane shares with its neighbours atomicOr-ed
//   k_pnge_file_offsets one wave: the files' places in the output
//   k_pnge_frame        a wave per IDAT payload: length, type, 8192 bytes, CRC-32 (a lane per 128
//                       bytes, combined by x^(8n) mod P); signature, IHDR and IEND around them
// Every pass is bounded by its buffer: see the comments at each store.
#include <cstring>
#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_deflate_rle.h"
#include "amhip_frame_stack.h"
#include "amhip_png_encode_host.h"

namespace amhip {

namespace {

using pnge::BlockCode;
using pnge::Tables;
using pnge::Work;

__constant__ Tables d_tables = pnge::make_tables();

using pnge::Bufs;
using pnge::FrameCtrl;
using pnge::kLane;
using pnge::kNoByte;
using pnge::kTile;
using pnge::Share;

constexpr uint32_t kPiece = 128;       // bytes of an IDAT payload per lane of the frame pass

template <typename T, bool kMax>
__device__ __forceinline__ T scan_incl_256(T v, T* sh) {
  const uint32_t tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const T o = tid >= off ? sh[tid - off] : (T)0;
    __syncthreads();
    v = kMax ? (v > o ? v : o) : v + o;
    sh[tid] = v;
    __syncthreads();
  }
  return v;
}

// sample k of a PNG row (R, G, B order for colour) from a source row
template <int kMode>
__device__ __forceinline__ uint32_t sample(const uint8_t* row, uint32_t k) {
  if (kMode == kJpegGray8) return row[k];
  const uint32_t src = (k / 3u) * 3u + (2u - k % 3u);
  if (kMode == kJpegBgr8) return row[src];
  const int v = reinterpret_cast<const int16_t*>(row)[src];
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Pass 1.  Stores: 16 bytes per lane at scan + g0, g0 + 16 <= ntiles * kTile; one word per tile.
template <int kMode>
__global__ void __launch_bounds__(256) k_pnge_filter(const uint8_t* px, Share s, Bufs b) {
  __shared__ uint32_t sh[3];
  const uint32_t tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y;
  if (tid < 3) sh[tid] = 0;
  __syncthreads();
  const uint8_t* frame = px + (size_t)f * s.frame_stride;
  const unsigned long long g0 = (unsigned long long)tile * kTile + tid * kLane;
  uint32_t out[4] = {0, 0, 0, 0};
  uint32_t a = 0, w = 0, last = 0;
  if (g0 < s.raw_len) {
    const unsigned long long left = s.raw_len - g0, tile_left = s.raw_len - (unsigned long long)tile * kTile;
    const uint32_t nv = left < kLane ? (uint32_t)left : kLane, tile_n = tile_left < kTile ? (uint32_t)tile_left : kTile;
    const unsigned long long i0 = g0 ? g0 - 1 : 0;
    uint32_t row = (uint32_t)(i0 / s.row_bytes), col = (uint32_t)(i0 - (unsigned long long)row * s.row_bytes);
    const uint8_t* rp = frame + (size_t)row * s.row_step;
    const uint32_t bpp = (uint32_t)s.bpp;
    auto value = [&]() -> uint32_t {
      uint32_t v = 1;   // the filter byte: Sub
      if (col) {
        const uint32_t k = col - 1;
        v = sample<kMode>(rp, k);
        if (k >= bpp) v -= sample<kMode>(rp, k - bpp);
        v &= 255u;
      }
      if (++col == s.row_bytes) {
        col = 0;
        rp += s.row_step;
      }
      return v;
    };
    uint32_t prev = kNoByte;
    if (g0) prev = value();
#pragma unroll
    for (uint32_t k = 0; k < kLane; ++k) {
      if (k < nv) {
        const uint32_t v = value();
        out[k >> 2] |= v << ((k & 3u) * 8u);
        a += v;
        w += (tile_n - (tid * kLane + k)) * v;   // (at most 4096 * 4097 / 2 * 255 < 2^32 per tile)
        if (v != prev) last = tid * kLane + k + 1;
        prev = v;
      }
    }
  }
  *reinterpret_cast<uint4*>(b.scan + ((size_t)f * s.ntiles + tile) * kTile + tid * kLane) =
      make_uint4(out[0], out[1], out[2], out[3]);
  if (a) atomicAdd(&sh[0], a);
  if (w) atomicAdd(&sh[1], w);
  if (last) atomicMax(&sh[2], last);
  __syncthreads();
  if (tid == 0) {
    const size_t t = (size_t)f * s.ntiles + tile;
    b.tile_a[t] = sh[0];
    b.tile_w[t] = sh[1];
    b.tile_last[t] = sh[2];
  }
}

// Pass 2, a workgroup per frame.  tile_carry[t]: 1 + the start of the run the byte in front of tile
// t lies in (0 for tile 0, which has no such byte).  Adler-32 as two plain sums: byte i weighs
// raw_len - i in the second.
__global__ void __launch_bounds__(256) k_pnge_scan_runs(Share s, Bufs b) {
  __shared__ unsigned long long sh[256];
  const uint32_t tid = threadIdx.x, f = blockIdx.x;
  const size_t t0 = (size_t)f * s.ntiles;
  unsigned long long carry = 0, s1 = 0, s2 = 0;
  for (uint32_t base = 0; base < s.ntiles; base += 256) {
    const uint32_t t = base + tid;
    unsigned long long v = 0;
    if (t < s.ntiles) {
      const uint32_t l = b.tile_last[t0 + t];
      if (l) v = (unsigned long long)t * kTile + l;
      const unsigned long long begin = (unsigned long long)t * kTile, left = s.raw_len - begin;
      const unsigned long long behind = left > kTile ? left - kTile : 0;   // bytes behind the tile
      const unsigned long long a = b.tile_a[t0 + t];
      s1 += a;
      s2 = (s2 + b.tile_w[t0 + t] + (behind % 65521ull) * a) % 65521ull;
    }
    scan_incl_256<unsigned long long, true>(v, sh);
    const unsigned long long before = tid ? sh[tid - 1] : 0;
    if (t < s.ntiles) b.tile_carry[t0 + t] = before > carry ? before : carry;
    carry = sh[255] > carry ? sh[255] : carry;
    __syncthreads();
  }
  scan_incl_256<unsigned long long, false>(s1 % 65521ull, sh);
  const unsigned long long sum1 = sh[255];
  __syncthreads();
  scan_incl_256<unsigned long long, false>(s2, sh);
  if (tid == 0) {
    const uint32_t r1 = (uint32_t)((1ull + sum1) % 65521ull);
    const uint32_t r2 = (uint32_t)((s.raw_len % 65521ull + sh[255]) % 65521ull);
    b.ctrl[f].adler = (r2 << 16) | r1;
  }
}

// the length of the match that starts at byte i (bytes i, i + 1, i + 2 are known to equal d[i - 1]):
// reads d[i + 3 .. min(i + 258, raw)) at the most
__device__ __forceinline__ uint32_t match_length(const uint8_t* d, unsigned long long i, unsigned long long raw) {
  const unsigned long long limit = raw - i < pnge::kMaxMatch ? raw : i + pnge::kMaxMatch;
  const uint32_t v = d[i];
  const unsigned long long pattern = 0x0101010101010101ull * v;
  unsigned long long p = i + 3;
  while (p < limit) {
    if (!(p & 7ull) && p + 8 <= limit) {   // eight aligned bytes at once
      const unsigned long long x = *reinterpret_cast<const unsigned long long*>(d + p) ^ pattern;
      if (x) {
        p += (unsigned long long)(__ffsll((long long)x) - 1) >> 3;
        break;
      }
      p += 8;
    } else {
      if (d[p] != v) break;
      ++p;
    }
  }
  return (uint32_t)(p - i);
}

// Passes 3 and 5.  Rule 4 per run of n equal bytes that starts at s: d[s] is a literal; byte s + 1 + j
// lies in chunk j / 258 at offset o = j % 258; a chunk of 3 bytes or more is a match that starts at
// o = 0, a chunk of 1 or 2 bytes is literals.  So o = 0 starts a symbol (a match if the two bytes
// behind it continue the run), o = 1 starts one only if the run ends with it, o >= 2 never does.
// kEmit = false: tile_cnt.  kEmit = true: sym[index] for every symbol, index < raw_len <= ntiles *
// kTile; block_pos[index / 16383] when that divides, index / 16383 < max_blocks.
template <bool kEmit>
__global__ void __launch_bounds__(256) k_pnge_tokens(const uint8_t* scan, const unsigned long long* tile_carry, uint32_t* tile_cnt,
                                                      const unsigned long long* tile_base, uint16_t* symbols,
                                                      unsigned long long* block_starts, unsigned long long raw,
                                                      uint32_t ntiles, uint32_t max_blocks) {
  __shared__ uint32_t sh[256];
  const uint32_t tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y;
  const size_t t = (size_t)f * ntiles + tile;
  const uint8_t* d = scan + (size_t)f * ntiles * kTile;
  const unsigned long long g0 = (unsigned long long)tile * kTile + tid * kLane;
  const uint32_t nv = g0 >= raw ? 0 : raw - g0 < kLane ? (uint32_t)(raw - g0) : kLane;
  // e[0]: the byte in front, e[1..16]: mine, e[17], e[18]: the two behind
  uint32_t e[19];
  const uint4 q = *reinterpret_cast<const uint4*>(d + g0);   // (inside the buffer: it holds ntiles * kTile bytes)
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
  e[0] = g0 && nv ? d[g0 - 1] : kNoByte;
#pragma unroll
  for (uint32_t k = 0; k < kLane; ++k) e[k + 1] = k < nv ? (qw[k >> 2] >> ((k & 3u) * 8u)) & 255u : kNoByte;
  e[17] = g0 + 16 < raw ? d[g0 + 16] : kNoByte;
  e[18] = g0 + 17 < raw ? d[g0 + 17] : kNoByte;
  // bit k: byte k differs from the byte in front of it (k = 16, 17: the two bytes behind mine); from
  // here on the bytes themselves are not needed
  uint32_t diff = 0;
#pragma unroll
  for (uint32_t k = 0; k < kLane + 2; ++k) diff |= (uint32_t)(e[k + 1] != e[k]) << k;
  const uint32_t valid = (1u << nv) - 1u, heads = diff & valid;
  const uint32_t tl = heads ? tid * kLane + (32u - (uint32_t)__clz((int)heads)) : 0;
  scan_incl_256<uint32_t, true>(tl, sh);
  const uint32_t before = tid ? sh[tid - 1] : 0;
  __syncthreads();
  // o of the byte in front of mine: -1 a run's first byte, else (distance to the run start - 1) % 258
  int o = -1;
  if (nv && !(diff & 1u)) {
    const unsigned long long start = before ? (unsigned long long)tile * kTile + before - 1 : tile_carry[t] - 1;
    const unsigned long long kk = g0 - 1 - start;
    o = kk ? (int)((kk - 1) % pnge::kMaxMatch) : -1;
  }
  uint32_t is_sym = 0, is_match = 0;
#pragma unroll
  for (uint32_t k = 0; k < kLane; ++k) {
    const uint32_t head = (diff >> k) & 1u, more1 = ~(diff >> (k + 1)) & 1u, more2 = ~(diff >> (k + 2)) & 1u;
    o = head ? -1 : (o == -1 || o == (int)pnge::kMaxMatch - 1) ? 0 : o + 1;
    const uint32_t starts = head | (uint32_t)(o == 0) | ((uint32_t)(o == 1) & (more1 ^ 1u));
    is_sym |= starts << k;
    is_match |= ((uint32_t)(o == 0) & more1 & more2) << k;
  }
  is_sym &= valid;
  is_match &= valid;
  const uint32_t mine = __popc(is_sym);
  const uint32_t upto = scan_incl_256<uint32_t, false>(mine, sh);
  if (!kEmit) {
    if (tid == 255) tile_cnt[t] = upto;
    return;
  }
  unsigned long long index = tile_base[t] + (upto - mine);
  unsigned long long block = index / pnge::kBlockSymbols;
  uint32_t in_block = (uint32_t)(index - block * pnge::kBlockSymbols);
  uint16_t* sym = symbols + (size_t)f * ntiles * kTile;
  unsigned long long* block_pos = block_starts + (size_t)f * (max_blocks + 1);
  // (a loop over the set bits, the byte read again from the scanlines: one copy of match_length)
  for (uint32_t left = is_sym; left; left &= left - 1) {
    const uint32_t k = (uint32_t)__ffs((int)left) - 1;
    const unsigned long long i = g0 + k;
    sym[index] = (uint16_t)(((is_match >> k) & 1u) ? 256u + match_length(d, i, raw) : d[i]);
    if (in_block == 0) block_pos[block] = i;
    ++index;
    if (++in_block == pnge::kBlockSymbols) {
      in_block = 0;
      ++block;
    }
  }
}

// Pass 4, a workgroup per frame: tile_base, the counts, and the end of the last block (which holds
// no symbol at all when the symbol count is a multiple of 16383: nobody else writes its start)
__global__ void __launch_bounds__(256) k_pnge_scan_counts(Share s, Bufs b) {
  __shared__ unsigned long long sh[256];
  const uint32_t tid = threadIdx.x, f = blockIdx.x;
  const size_t t0 = (size_t)f * s.ntiles;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < s.ntiles; base += 256) {
    const uint32_t t = base + tid;
    const unsigned long long v = t < s.ntiles ? b.tile_cnt[t0 + t] : 0;
    const unsigned long long upto = scan_incl_256<unsigned long long, false>(v, sh);
    if (t < s.ntiles) b.tile_base[t0 + t] = carry + upto - v;
    carry += sh[255];
    __syncthreads();
  }
  if (tid == 0) {
    // (nsym <= raw_len, so nblocks <= raw_len / 16383 + 1 = max_blocks)
    const unsigned long long nblocks = carry / pnge::kBlockSymbols + 1;
    b.ctrl[f].nsym = carry;
    b.ctrl[f].nblocks = (uint32_t)nblocks;
    unsigned long long* block_pos = b.block_pos + (size_t)f * (s.max_blocks + 1);
    block_pos[nblocks] = s.raw_len;
    if (carry % pnge::kBlockSymbols == 0) block_pos[nblocks - 1] = s.raw_len;
  }
}

// Pass 6, a wave per block.  The histogram by the wave, the trees by one lane: they are a heap walk
// over at most 286 leaves, serial in zlib and serial here; the other blocks of the call run beside it.
__global__ void __launch_bounds__(64) k_pnge_plan(Share s, Bufs b) {
  __shared__ Work w;
  __shared__ uint32_t hist[pnge::kLCodes + 1];   // (the last: matches)
  const uint32_t lane = threadIdx.x, blk = blockIdx.x, f = blockIdx.y;
  const FrameCtrl c = b.ctrl[f];
  if (blk >= c.nblocks) return;
  for (uint32_t n = lane; n < pnge::kLCodes + 1; n += 64) hist[n] = 0;
  for (uint32_t n = lane; n < 2 * pnge::kDCodes + 1; n += 64) w.dfreq[n] = 0;
  for (uint32_t n = lane; n < 2 * pnge::kBlCodes + 1; n += 64) w.blfreq[n] = 0;
  __syncthreads();
  const uint16_t* sym = b.sym + (size_t)f * s.ntiles * kTile;
  const unsigned long long lo = (unsigned long long)blk * pnge::kBlockSymbols;
  const unsigned long long hi = c.nsym - lo < pnge::kBlockSymbols ? c.nsym : lo + pnge::kBlockSymbols;
  for (unsigned long long k = lo + lane; k < hi; k += 64) {
    const uint32_t v = sym[k];
    if (v < 256) {
      atomicAdd(&hist[v], 1u);
    } else {
      atomicAdd(&hist[d_tables.length_code[v - 256 - 3] + pnge::kLiterals + 1], 1u);
      atomicAdd(&hist[pnge::kLCodes], 1u);
    }
  }
  __syncthreads();
  for (uint32_t n = lane; n < pnge::kLCodes; n += 64) w.lfreq[n] = (uint16_t)(n == pnge::kEndBlock ? 1 : hist[n]);
  if (lane == 0) w.dfreq[0] = (uint16_t)hist[pnge::kLCodes];
  __syncthreads();
  if (lane == 0) {
    const unsigned long long* block_pos = b.block_pos + (size_t)f * (s.max_blocks + 1);
    pnge::plan_block(d_tables, w, (uint32_t)(block_pos[blk + 1] - block_pos[blk]),
                     &b.code[(size_t)f * s.max_blocks + blk]);
  }
}

// Pass 7, a wave per frame.  A stored block starts on a byte behind its three type bits, so the
// offsets are a walk, not a sum: 64 blocks are loaded at a time and walked from registers.  Also the
// stream's two header bytes and its Adler-32 (the buffer is zero; the words are shared with the
// first and the last block, so they are OR-ed in).  z: (zlib_bound + 3) / 4 + 2 words.
__global__ void __launch_bounds__(64) k_pnge_offsets(Share s, Bufs b) {
  const uint32_t lane = threadIdx.x, f = blockIdx.x;
  const FrameCtrl c = b.ctrl[f];
  const BlockCode* code = b.code + (size_t)f * s.max_blocks;
  unsigned long long* block_bit = b.block_bit + (size_t)f * s.max_blocks;
  unsigned long long bit = 16;
  for (uint32_t base = 0; base < c.nblocks; base += 64) {
    const uint32_t blk = base + lane;
    uint32_t type = 0, bits = 0, slen = 0;
    if (blk < c.nblocks) {
      type = code[blk].type;
      bits = code[blk].bits;
      slen = code[blk].stored_len;
    }
    unsigned long long mine = 0;
    const uint32_t n = c.nblocks - base < 64 ? c.nblocks - base : 64;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t ty = __shfl(type, (int)j), bi = __shfl(bits, (int)j), sl = __shfl(slen, (int)j);
      if (lane == j) mine = bit;
      bit = ty == pnge::kStored ? ((bit + 3 + 7) & ~7ull) + 32 + 8ull * sl : bit + bi;
    }
    if (blk < c.nblocks) block_bit[blk] = mine;
  }
  if (lane == 0) {
    const unsigned long long trailer = (bit + 7) >> 3, zlen = trailer + 4;
    uint32_t* z = b.z + (size_t)f * s.zwords;
    atomicOr(&z[0], 0x0178u);
    for (uint32_t k = 0; k < 4; ++k) {
      const unsigned long long at = trailer + k;
      atomicOr(&z[at >> 2], ((c.adler >> (24 - 8 * k)) & 255u) << ((at & 3ull) * 8));
    }
    b.ctrl[f].zlen = zlen;
    b.ctrl[f].fsize = pnge::kFileHead + zlen + 12ull * ((zlen + pnge::kIdatBytes - 1) / pnge::kIdatBytes) + pnge::kFileTail;
    b.sizes[f] = b.ctrl[f].fsize;
  }
}

// bits LSB first into zeroed words from an arbitrary bit on.  The first and the last word a lane
// touches may be shared with its neighbours and are OR-ed; every word between is the lane's alone.
struct BitOut {
  uint32_t* z;
  unsigned long long word, acc;
  uint32_t n;
  bool first;
  __device__ __forceinline__ void open(uint32_t* words, unsigned long long bit) {
    z = words;
    word = bit >> 5;
    n = (uint32_t)(bit & 31ull);
    acc = 0;
    first = true;
  }
  __device__ __forceinline__ void put(uint32_t value, uint32_t len) {   // len <= 32
    acc |= (unsigned long long)value << n;
    n += len;
    if (n >= 32) {
      if (first) atomicOr(&z[word], (uint32_t)acc);
      else z[word] = (uint32_t)acc;
      first = false;
      ++word;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void close() {
    if (n && (uint32_t)acc) atomicOr(&z[word], (uint32_t)acc);
  }
};

// Pass 8, a workgroup per block: 64 symbols per lane (the bytes of a stored block likewise), their bit
// counts scanned, then written.  Every bit lies in [block_bit, the next block's block_bit), which
// k_pnge_offsets laid out inside the frame's zlib_bound bytes.
__global__ void __launch_bounds__(256) k_pnge_pack(Share s, Bufs b) {
  __shared__ uint32_t sh[256];
  __shared__ uint16_t lcode[pnge::kLCodes];
  __shared__ uint8_t llen[pnge::kLCodes];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, f = blockIdx.y;
  const FrameCtrl c = b.ctrl[f];
  if (blk >= c.nblocks) return;
  const BlockCode* code = &b.code[(size_t)f * s.max_blocks + blk];
  uint32_t* z = b.z + (size_t)f * s.zwords;
  const unsigned long long bit0 = b.block_bit[(size_t)f * s.max_blocks + blk];
  const uint32_t last = blk + 1 == c.nblocks, type = code->type;
  BitOut o;
  if (type == pnge::kStored) {
    const uint32_t slen = code->stored_len;
    const uint8_t* src = b.scan + (size_t)f * s.ntiles * kTile + b.block_pos[(size_t)f * (s.max_blocks + 1) + blk];
    const unsigned long long body = (bit0 + 3 + 7) & ~7ull;
    const uint32_t per = (slen + 255) / 256, lo = tid * per < slen ? tid * per : slen, hi = lo + per < slen ? lo + per : slen;
    if (tid == 0) {
      o.open(z, bit0);
      o.put(last, 3);
      o.close();
      o.open(z, body);
      o.put(slen & 0xFFFFu, 16);
      o.put(~slen & 0xFFFFu, 16);
    } else {
      o.open(z, body + 32 + 8ull * lo);
    }
    for (uint32_t k = lo; k < hi; ++k) o.put(src[k], 8);
    o.close();
    return;
  }
  for (uint32_t n = tid; n < pnge::kLCodes; n += 256) {
    lcode[n] = code->lcode[n];
    llen[n] = code->llen[n];
  }
  __syncthreads();
  const uint32_t dlen0 = code->dlen0, dcode0 = code->dcode0, header_bits = code->header_bits;
  const uint16_t* sym = b.sym + (size_t)f * s.ntiles * kTile + (unsigned long long)blk * pnge::kBlockSymbols;
  const unsigned long long left = c.nsym - (unsigned long long)blk * pnge::kBlockSymbols;
  const uint32_t cnt = left < pnge::kBlockSymbols ? (uint32_t)left : pnge::kBlockSymbols;
  const uint32_t per = (cnt + 255) / 256, lo = tid * per < cnt ? tid * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
  uint32_t bits = tid == 0 ? 3 + header_bits : 0;
  for (uint32_t k = lo; k < hi; ++k) bits += pnge::symbol_bits(d_tables, llen, dlen0, sym[k]);
  const uint32_t upto = scan_incl_256<uint32_t, false>(bits, sh);
  o.open(z, bit0 + (upto - bits));
  if (tid == 0) {
    o.put((type << 1) + last, 3);
    for (uint32_t k = 0; k < header_bits; k += 32) {
      const uint32_t len = header_bits - k < 32 ? header_bits - k : 32;
      const uint32_t v = code->header[k >> 5];
      o.put(len == 32 ? v : v & ((1u << len) - 1u), len);
    }
  }
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t v = sym[k];
    if (v < 256) {
      o.put(lcode[v], llen[v]);
    } else {
      const uint32_t lc = v - 256 - 3, lcd = d_tables.length_code[lc], x = d_tables.extra_lbits[lcd];
      // the length code and its extra bits: at most 15 + 5 bits in one go
      // (code 28, length 258, has no extra bits and base 0: nothing of lc may follow it)
      const uint32_t extra = x ? lc - d_tables.base_length[lcd] : 0;
      o.put(lcode[lcd + pnge::kLiterals + 1] | (extra << llen[lcd + pnge::kLiterals + 1]),
            llen[lcd + pnge::kLiterals + 1] + x);
      o.put(dcode0, dlen0);
    }
  }
  if (tid == 255) o.put(lcode[pnge::kEndBlock], llen[pnge::kEndBlock]);
  o.close();
}

// Pass 9, one wave: offs[f] = the bytes of the group's files in front of file f
__global__ void __launch_bounds__(64) k_pnge_file_offsets(Bufs b, uint32_t n) {
  const uint32_t lane = threadIdx.x, per = (n + 63) / 64;
  const uint32_t lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
  unsigned long long sum = 0;
  for (uint32_t f = lo; f < hi; ++f) sum += b.sizes[f];
  unsigned long long upto = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long v = __shfl_up(upto, off);
    if ((int)lane >= off) upto += v;
  }
  unsigned long long at = upto - sum;
  for (uint32_t f = lo; f < hi; ++f) {
    b.offs[f] = at;
    at += b.sizes[f];
  }
}

// Pass 10, a wave per IDAT payload p of frame f: the chunk at file + 33 + p * (8192 + 12).  The
// file's bytes are [offs[f], offs[f] + fsize), inside the output the host sized from the sizes.
__global__ void __launch_bounds__(64) k_pnge_frame(Share s, Bufs b, uint8_t* out) {
  __shared__ uint32_t crc_table[256];
  const uint32_t lane = threadIdx.x, p = blockIdx.x, f = blockIdx.y;
  const unsigned long long zlen = b.ctrl[f].zlen;
  const unsigned long long nidat = (zlen + pnge::kIdatBytes - 1) / pnge::kIdatBytes;
  if (p >= nidat) return;
  for (uint32_t n = lane; n < 256; n += 64) crc_table[n] = d_tables.crc[n];
  __syncthreads();
  uint8_t* file = out + b.offs[f];
  const uint8_t* zb = reinterpret_cast<const uint8_t*>(b.z + (size_t)f * s.zwords) + (size_t)p * pnge::kIdatBytes;
  const unsigned long long zleft = zlen - (unsigned long long)p * pnge::kIdatBytes;
  const uint32_t len = zleft < pnge::kIdatBytes ? (uint32_t)zleft : pnge::kIdatBytes;
  uint8_t* chunk = file + pnge::kFileHead + (size_t)p * (pnge::kIdatBytes + 12);
  if (p == 0 && lane < pnge::kFileHead) file[lane] = b.head[lane];
  if (p + 1 == nidat && lane < pnge::kFileTail)
    file[pnge::kFileHead + zlen + 12 * nidat + lane] = b.head[pnge::kFileHead + lane];
  const uint32_t type_word = 0x54414449u;   // "IDAT", first byte lowest
  if (lane < 4) chunk[lane] = (uint8_t)(len >> (24 - 8 * lane));
  else if (lane < 8) chunk[lane] = (uint8_t)(type_word >> (8 * (lane - 4)));
  for (uint32_t k = lane; k < len; k += 64) chunk[8 + k] = zb[k];
  // CRC-32 over the type and the payload: lane 0 starts from the inverted register and takes the
  // type in, every other lane starts from zero; a register with n bytes behind it is multiplied by
  // x^(8n) mod P, and the sum (xor) of all is the register behind the whole chunk
  const uint32_t lo = lane * kPiece < len ? lane * kPiece : len, hi = lo + kPiece < len ? lo + kPiece : len;
  uint32_t reg = 0;
  if (lane == 0) {
    reg = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < 4; ++k) reg = crc_table[(reg ^ (type_word >> (8 * k))) & 255u] ^ (reg >> 8);
  }
  for (uint32_t k = lo; k < hi; ++k) reg = crc_table[(reg ^ zb[k]) & 255u] ^ (reg >> 8);
  if (reg && len - hi) reg = pnge::multmodp(pnge::x8nmodp(d_tables, len - hi), reg);
  for (int off = 32; off >= 1; off >>= 1) reg ^= __shfl_xor(reg, off);
  const uint32_t crc = ~reg;
  if (lane < 4) chunk[8 + len + lane] = (uint8_t)(crc >> (24 - 8 * lane));
}

}  // namespace

int deflate_rle_middle(hipStream_t stream, const Share& s, const Bufs& b, uint32_t n) {
  const dim3 tiles(s.ntiles, n), blocks(s.max_blocks, n);
  hipLaunchKernelGGL(k_pnge_scan_runs, dim3(n), dim3(256), 0, stream, s, b);
  hipLaunchKernelGGL(k_pnge_tokens<false>, tiles, dim3(256), 0, stream, b.scan, b.tile_carry, b.tile_cnt, b.tile_base,
                     b.sym, b.block_pos, s.raw_len, s.ntiles, s.max_blocks);
  hipLaunchKernelGGL(k_pnge_scan_counts, dim3(n), dim3(256), 0, stream, s, b);
  hipLaunchKernelGGL(k_pnge_tokens<true>, tiles, dim3(256), 0, stream, b.scan, b.tile_carry, b.tile_cnt, b.tile_base,
                     b.sym, b.block_pos, s.raw_len, s.ntiles, s.max_blocks);
  hipLaunchKernelGGL(k_pnge_plan, blocks, dim3(64), 0, stream, s, b);
  hipLaunchKernelGGL(k_pnge_offsets, dim3(n), dim3(64), 0, stream, s, b);
  hipLaunchKernelGGL(k_pnge_pack, blocks, dim3(256), 0, stream, s, b);
  AMHIP_TRY(hipGetLastError());
  return AMHIP_OK;
}

namespace {

// One call: the geometry every frame shares, the groups (amhip_frame_plan.h: a frame costs its
// scratch, the budget is the tuning key pnge_scratch_budget_mb), the scratch of the largest group
// and the sizes of all files.  The scratch lives for the call.
struct PngEncoder : EncodeGroups {
  Share s;
  DevBuf head;

  using Layout = pnge::Layout;
  Layout layout(size_t n) const { return pnge::make_layout(s, n); }
  Bufs bufs(const Layout& l) { return pnge::make_bufs(scratch.as<uint8_t>(), l, head.as<const uint8_t>()); }
  size_t frame_stride() const { return (size_t)s.frame_stride; }
  // the bytes of the stack that group gi's frames span
  size_t group_span(size_t gi) const {
    return (group_frames(gi) - 1) * (size_t)s.frame_stride + (size_t)s.height * (size_t)s.row_step;
  }

  // host only: geometry and groups
  void plan(size_t frames, int width, int height, int mode, size_t row_step, size_t frame_stride) {
    s.width = width;
    s.height = height;
    s.mode = mode;
    s.bpp = mode == kJpegGray8 ? 1 : 3;
    s.row_bytes = 1u + (uint32_t)width * (uint32_t)s.bpp;
    pnge::share_set_raw(&s, pnge::raw_len(width, height, s.bpp));
    s.row_step = row_step;
    s.frame_stride = frames > 1 ? frame_stride : 0;
    plan_uniform(frames, layout(1).total, "pnge_scratch_budget_mb", 4096.0, kMaxGroupFrames);
  }

  int open() {
    int rc;
    if ((rc = scratch.alloc(layout(most_group_frames()).total))) return rc;
    if ((rc = head.alloc(pnge::kFileHead + pnge::kFileTail))) return rc;
    static const Tables kTables = pnge::make_tables();
    uint8_t h[pnge::kFileHead + pnge::kFileTail];
    pnge::write_head_tail(kTables, s.width, s.height, s.bpp, h, h + pnge::kFileHead);
    AMHIP_TRY(hipMemcpyAsync(head.p, h, sizeof(h), hipMemcpyHostToDevice, stream));
    AMHIP_TRY(hipStreamSynchronize(stream));   // (h is on the stack)
    return AMHIP_OK;
  }

  // every pass of group gi up to the zlib streams, the files' sizes and their offsets; `px`: the
  // group's first frame.  Reads back the sizes, nothing else.
  int front(size_t gi, const uint8_t* px) {
    const uint32_t n = (uint32_t)group_frames(gi);
    const Layout l = layout(n);
    const Bufs b = bufs(l);
    AMHIP_TRY(hipMemsetAsync(b.z, 0, (size_t)n * (size_t)s.zwords * 4, stream));
    const dim3 tiles(s.ntiles, n);
    if (s.mode == kJpegGray8) hipLaunchKernelGGL(k_pnge_filter<kJpegGray8>, tiles, dim3(256), 0, stream, px, s, b);
    else if (s.mode == kJpegBgr8) hipLaunchKernelGGL(k_pnge_filter<kJpegBgr8>, tiles, dim3(256), 0, stream, px, s, b);
    else hipLaunchKernelGGL(k_pnge_filter<kJpegBgr16s>, tiles, dim3(256), 0, stream, px, s, b);
    const int rc = deflate_rle_middle(stream, s, b, n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pnge_file_offsets, dim3(1), dim3(64), 0, stream, b, n);
    AMHIP_TRY(hipGetLastError());
    AMHIP_TRY(hipMemcpyAsync(sizes.data() + group_begin[gi], b.sizes, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    AMHIP_TRY(hipStreamSynchronize(stream));
    return AMHIP_OK;
  }

  // ... and group gi's files to out + at, which holds group_bytes(gi) bytes.  front(gi) ran last.
  int back(size_t gi, uint8_t* out, uint64_t at) {
    const uint32_t n = (uint32_t)group_frames(gi);
    const Bufs b = bufs(layout(n));
    // (a file is its zlib stream and more: no stream has more payloads than the largest file)
    const unsigned idats = (unsigned)((largest_file(gi) + pnge::kIdatBytes - 1) / pnge::kIdatBytes);
    hipLaunchKernelGGL(k_pnge_frame, dim3(idats, n), dim3(64), 0, stream, s, b, out + at);
    AMHIP_TRY(hipGetLastError());
    return AMHIP_OK;
  }
};

// the argument rules of both stack entry points, then the plan
int plan_frames(const char* who, PngEncoder* enc, size_t F, int width, int height, int channels, size_t row_step,
                size_t frame_stride) {
  if (const char* why = pnge::check_frames_args(F, width, height, channels, row_step, frame_stride)) {
    set_last_error(std::string(who) + ": " + why);
    return AMHIP_ERR_ARG;
  }
  enc->plan(F, width, height, channels == 1 ? kJpegGray8 : kJpegBgr8, row_step, frame_stride);
  return AMHIP_OK;
}

// One image, a stack of one.  dev_out != null: into it, at most cap bytes, nothing written when it
// does not fit.  Otherwise into *host.  *bytes: the file's size.
int png_encode(hipStream_t stream, const JpegSource& src, uint8_t* dev_out, size_t cap, std::vector<uint8_t>* host,
               size_t* bytes) {
  PngEncoder enc;
  enc.stream = stream;
  enc.plan(1, src.width, src.height, src.mode, src.step, 0);
  int rc;
  if ((rc = enc.open())) return rc;
  DevBuf owned;
  rc = encode_groups(
      enc, [&](size_t gi) { return enc.front(gi, static_cast<const uint8_t*>(src.dev)); },
      [&](uint8_t** to, uint64_t*) {
        if (bytes) *bytes = (size_t)enc.sizes[0];
        *to = dev_out;
        if (dev_out) return enc.sizes[0] > cap ? capacity_failure("png", enc.sizes[0], cap) : (int)AMHIP_OK;
        const int r = owned.alloc((size_t)enc.sizes[0]);
        *to = owned.as<uint8_t>();
        return r;
      });
  if (rc) return rc;
  if (!dev_out) {
    host->resize((size_t)enc.sizes[0]);
    AMHIP_TRY(hipMemcpyAsync(host->data(), owned.p, host->size(), hipMemcpyDeviceToHost, stream));
  }
  AMHIP_TRY(hipStreamSynchronize(stream));   // (the scratch goes with this call)
  return AMHIP_OK;
}

}  // namespace

int png_encode_run(hipStream_t stream, const JpegSource& src, uint8_t* dev_out, size_t cap, size_t* bytes) {
  return png_encode(stream, src, dev_out, cap, nullptr, bytes);
}

int png_write_run(const char* what, hipStream_t stream, const JpegSource& src, const char* filename) {
  std::vector<uint8_t> file;
  const int rc = png_encode(stream, src, nullptr, 0, &file, nullptr);
  if (rc) return rc;
  return write_file(what, filename, file.data(), file.size());
}

}  // namespace amhip

using namespace amhip;

extern "C" {

size_t amhip_png_bound(int width, int height, int channels) {
  if (width < 1 || width > 65535 || height < 1 || height > 65535 || (channels != 1 && channels != 3)) return 0;
  return (size_t)pnge::file_bound(width, height, channels);
}

int amhip_png_encode_dev(amhip_ctx* h, const uint8_t* dev_pixels, size_t step, int width, int height,
                         int channels, uint8_t* dev_out, size_t cap, size_t* bytes) {
  if (!h || !dev_pixels || !dev_out || !bytes) return arg_failure("amhip_png_encode_dev: null argument");
  if (const char* why = pnge::check_image_args(step, width, height, channels))
    return arg_failure((std::string("amhip_png_encode_dev: ") + why).c_str());
  Ctx* c = &h->impl;
  int rc = ctx_use_device(c);
  if (rc) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  const JpegSource src = {dev_pixels, step, width, height, channels == 1 ? kJpegGray8 : kJpegBgr8};
  return png_encode_run(c->stream, src, dev_out, cap, bytes);
}

int amhip_png_write(amhip_ctx* h, const char* filename, const uint8_t* pixels, int on_device, size_t step,
                    int width, int height, int channels) {
  if (!h || !filename || !pixels) return arg_failure("amhip_png_write: null argument");
  if (const char* why = pnge::check_image_args(step, width, height, channels))
    return arg_failure((std::string("amhip_png_write: ") + why).c_str());
  Ctx* c = &h->impl;
  int rc = ctx_use_device(c);
  if (rc) return rc;
  JpegSource src = {pixels, step, width, height, channels == 1 ? kJpegGray8 : kJpegBgr8};
  if (!on_device && (rc = stage_host_image(c, channels, &src))) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  return png_write_run("amhip_png_write", c->stream, src, filename);
}

int amhip_layer_write_png(amhip_ctx* h, int layer, int bgr, float lower, float upper, const char* filename) {
  if (!h || !filename || layer < 0 || layer >= AMHIP_NUM_LAYERS)
    return arg_failure("amhip_layer_write_png: bad argument");
  if (!bgr && !(upper > lower)) return arg_failure("amhip_layer_write_png: upper <= lower");
  JpegSource src;
  const int rc = layer_image_source(h, "amhip_layer_write_png: a PNG file of this encoder holds 1 x 1 to 65535 x 65535 pixels",
                                    layer, bgr, lower, upper, &src);
  if (rc) return rc;
  Ctx* c = &h->impl;
  ScopedTimer timer(c, AMHIP_K_MISC);
  return png_write_run("amhip_layer_write_png", c->stream, src, filename);
}

int amhip_io_encode_png_frames(int device, const uint8_t* dev_frames, size_t F, int width, int height,
                               int channels, size_t row_step, size_t frame_stride, uint8_t** dev_files,
                               size_t* offsets) {
  static const char kWho[] = "amhip_io_encode_png_frames";
  return encode_frame_stack<PngEncoder>(kWho, device, dev_frames, dev_files, offsets, [&](PngEncoder* enc) {
    return plan_frames(kWho, enc, F, width, height, channels, row_step, frame_stride);
  });
}

int amhip_io_write_png_frames(int device, const uint8_t* frames, int on_device, size_t F, int width, int height,
                              int channels, size_t row_step, size_t frame_stride, const char* const* filenames) {
  static const char kWho[] = "amhip_io_write_png_frames";
  return write_frame_stack<PngEncoder>(kWho, device, frames, on_device, filenames, [&](PngEncoder* enc) {
    return plan_frames(kWho, enc, F, width, height, channels, row_step, frame_stride);
  });
}

}  // extern "C"
