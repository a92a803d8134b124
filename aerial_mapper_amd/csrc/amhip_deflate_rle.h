// amhip_deflate_rle.h -- what the PNG encoder (amhip_png_encode.hip) and the GeoTIFF encoder
// (amhip_tiff_encode.hip) share: the buffers of the batched zlib level-1 Z_RLE coder of DESIGN 4.15
// and the door to its middle passes.  A "frame" is one independent zlib stream: a PNG image's
// scanlines, or one TIFF tile's predictor bytes.  The producer in front (k_pnge_filter, k_tiff_tile)
// fills `scan` (zero behind raw_len) and, per piece of 4096 bytes, the two Adler sums and the last
// run start; the passes behind it (runs, tokens, counts, plan, offsets, pack) are the PNG encoder's
// kernels, compiled once in its translation unit and launched through deflate_rle_middle().
#ifndef AMHIP_DEFLATE_RLE_H_
#define AMHIP_DEFLATE_RLE_H_

#include "amhip_common.h"
#include "amhip_png_encode_host.h"

namespace amhip {
namespace pnge {

constexpr uint32_t kTile = 4096;       // bytes of a frame per workgroup of the byte passes
constexpr uint32_t kLane = 16;         // ... per lane
constexpr uint32_t kNoByte = 0x100;    // stands for a byte outside the data: equal to none inside

// what every frame of a call shares
struct Share {
  int width, height, bpp, mode;
  uint32_t row_bytes;            // PNG: 1 + width * bpp
  uint32_t ntiles, max_blocks;
  unsigned long long raw_len;    // bytes of a frame
  unsigned long long zwords;     // 32-bit words of a frame's zlib buffer
  unsigned long long row_step, frame_stride;
};

struct FrameCtrl {
  unsigned long long nsym, zlen, fsize;
  uint32_t nblocks, adler;
};

// a group's buffers, frame-major: frame f owns [f * per-frame size, (f + 1) * per-frame size)
struct Bufs {
  uint8_t* scan;                     // ntiles * kTile bytes: the frame's bytes, zero behind raw_len
  uint16_t* sym;                     // ntiles * kTile symbols: 0..255 literal, 256 + length
  uint32_t *tile_last, *tile_cnt, *tile_a, *tile_w;   // ntiles each
  unsigned long long *tile_carry, *tile_base;         // ntiles each
  unsigned long long* block_pos;     // max_blocks + 1: the byte a block starts at
  unsigned long long* block_bit;     // max_blocks: the bit it starts at in the zlib stream
  BlockCode* code;                   // max_blocks
  uint32_t* z;                       // zwords: the zlib stream
  FrameCtrl* ctrl;
  unsigned long long *sizes, *offs;  // one per frame
  const uint8_t* head;               // PNG: kFileHead + kFileTail bytes, shared
};

// where the buffers of a group of n frames lie in one allocation
struct Layout {
  size_t scan, sym, tile32[4], tile64[2], block_pos, block_bit, code, z, ctrl, sizes, offs, total;
};

inline Layout make_layout(const Share& s, size_t n) {
  Layout l;
  size_t at = 0;
  auto carve = [&](size_t bytes) {
    const size_t a = at;
    at += (bytes + 255) / 256 * 256;
    return a;
  };
  const size_t tiles = n * s.ntiles;
  l.scan = carve(tiles * kTile);
  l.sym = carve(tiles * kTile * 2);
  for (size_t& o : l.tile32) o = carve(tiles * 4);
  for (size_t& o : l.tile64) o = carve(tiles * 8);
  l.block_pos = carve(n * ((size_t)s.max_blocks + 1) * 8);
  l.block_bit = carve(n * (size_t)s.max_blocks * 8);
  l.code = carve(n * (size_t)s.max_blocks * sizeof(BlockCode));
  l.z = carve(n * (size_t)s.zwords * 4);
  l.ctrl = carve(n * sizeof(FrameCtrl));
  l.sizes = carve(n * 8);
  l.offs = carve(n * 8);
  l.total = at;
  return l;
}

inline Bufs make_bufs(uint8_t* d, const Layout& l, const uint8_t* head) {
  Bufs b;
  b.scan = d + l.scan;
  b.sym = reinterpret_cast<uint16_t*>(d + l.sym);
  b.tile_last = reinterpret_cast<uint32_t*>(d + l.tile32[0]);
  b.tile_cnt = reinterpret_cast<uint32_t*>(d + l.tile32[1]);
  b.tile_a = reinterpret_cast<uint32_t*>(d + l.tile32[2]);
  b.tile_w = reinterpret_cast<uint32_t*>(d + l.tile32[3]);
  b.tile_carry = reinterpret_cast<unsigned long long*>(d + l.tile64[0]);
  b.tile_base = reinterpret_cast<unsigned long long*>(d + l.tile64[1]);
  b.block_pos = reinterpret_cast<unsigned long long*>(d + l.block_pos);
  b.block_bit = reinterpret_cast<unsigned long long*>(d + l.block_bit);
  b.code = reinterpret_cast<BlockCode*>(d + l.code);
  b.z = reinterpret_cast<uint32_t*>(d + l.z);
  b.ctrl = reinterpret_cast<FrameCtrl*>(d + l.ctrl);
  b.sizes = reinterpret_cast<unsigned long long*>(d + l.sizes);
  b.offs = reinterpret_cast<unsigned long long*>(d + l.offs);
  b.head = head;
  return b;
}

// the geometry of a frame of raw_len bytes (the rest of Share is the producer's business)
inline void share_set_raw(Share* s, unsigned long long raw) {
  s->raw_len = raw;
  s->ntiles = (uint32_t)((raw + kTile - 1) / kTile);
  s->max_blocks = (uint32_t)max_blocks(raw);
  s->zwords = (zlib_bound(raw) + 3) / 4 + 2;
}

}  // namespace pnge

// The middle of the coder for n frames whose producer has run on `stream` and whose zlib buffers
// are zero: k_pnge_scan_runs .. k_pnge_pack (amhip_png_encode.hip).  Behind it ctrl[f].zlen and
// ctrl[f].adler are set and z holds frame f's stream.  Reads s.ntiles, s.max_blocks, s.raw_len and
// s.zwords only.  Asynchronous.
int deflate_rle_middle(hipStream_t stream, const pnge::Share& s, const pnge::Bufs& b, uint32_t n);

}  // namespace amhip

#endif  // AMHIP_DEFLATE_RLE_H_
