// amhip_tiff_encode.hip -- map layers and rasters as tiled Deflate GeoTIFF, compressed on the GPU:
// a classic little-endian TIFF with one IFD (and one more per overview level), square
// tiles, Compression 8 (Adobe Deflate), Predictor 3 for 32-bit float samples and 2 for 8-bit ones, the geo tags of
// amhip_geotiff_write_u8.  Every tile is one zlib stream: byte for byte what zlib 1.2.11 writes for
// the tile's predictor bytes with deflateInit2(1, Z_DEFLATED, 15, 8, Z_RLE), which
// tests/geotiff_reference.py restates and tests/golden/geotiff/ pins.  DESIGN 4.16.
//
// A tile is a "frame" of the batched Z_RLE coder of the PNG encoder (amhip_deflate_rle.h):
//   (k_tovr_reduce  amhip_tiff_overview.hip: the overview levels' rasters, each from the one before it)
//   k_tiff_tile     a workgroup per 4096 predictor bytes of a tile (the tile on blockIdx.y): the rows
//                   of samples it covers go through LDS -- from a layer, reoriented north-up and
//                   converted on the way, or from a row-major raster -- then a lane per 16 bytes:
//                   byte planes and differences; per piece the two Adler sums and the last run start
//   (the coder's middle: k_pnge_scan_runs .. k_pnge_pack, unchanged)
//   k_tiff_offsets  one wave: every stream's length and its place behind the group's first tile
//   k_tiff_gather   a lane per 16 aligned bytes of the file: the streams, tightly packed
// The head of the file (IFD, tables, geo tags) is built on the host from the streams' lengths
// (amhip_tiff_host.h).  Every pass is bounded by its buffer: see the comments at each store.
#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_deflate_rle.h"
#include "amhip_frame_stack.h"
#include "amhip_tiff_host.h"
#include "amhip_tiff_source.h"

namespace amhip {

namespace {

using pnge::Bufs;
using pnge::kLane;
using pnge::kNoByte;
using pnge::kTile;
using pnge::Share;

constexpr uint32_t kStageBytes = 12288;   // the sample rows one piece of 4096 bytes can touch (plan())

// The producer.  Stores: 16 bytes per lane at scan + (f * ntiles + piece) * 4096 + tid * 16, inside
// the group's ntiles * 4096 bytes per tile; one word per piece.  LDS: the rows [row_lo, row_hi] of
// the tile, at most kStageBytes (plan() refuses a geometry that would need more).
template <int kKind, bool kLayer>
__global__ void __launch_bounds__(256) k_tiff_tile(TileSrc src, Share s, Bufs b) {
  constexpr uint32_t kPixel = kKind == tiff::kF32 ? 4u : kKind == tiff::kRgb8 ? 3u : 1u;
  constexpr uint32_t kStride = kKind == tiff::kF32 ? 1u : kPixel;   // of the differencing, in bytes
  __shared__ uint32_t stage[kStageBytes / 4];
  __shared__ uint32_t sh[3];
  uint8_t* stage8 = reinterpret_cast<uint8_t*>(stage);
  // (a launch covers the tiles of one level that a group holds: tile src.first + y of that level's
  // raster is frame src.frame0 + y of the group's buffers)
  const uint32_t tid = threadIdx.x, piece = blockIdx.x, f = src.frame0 + blockIdx.y;
  if (tid < 3) sh[tid] = 0;
  const uint32_t t = src.first + blockIdx.y, ty = t / src.across, tx = t - ty * src.across;
  const uint32_t side = src.side, rb = src.row_bytes, raw = (uint32_t)s.raw_len;
  const uint32_t r0 = ty * side, c0 = tx * side;
  const uint32_t b0 = piece * kTile, b1 = raw - b0 < kTile ? raw : b0 + kTile;   // (piece < ntiles: b0 < raw)
  const uint32_t row_lo = b0 / rb, row_hi = (b1 - 1u) / rb;
  // the rows of samples, a lane per sample: consecutive lanes read consecutive floats of a layer
  // column (backwards) or consecutive pixels of a raster row
  const uint32_t nsamp = (row_hi - row_lo + 1u) * side;
  for (uint32_t q = tid; q < nsamp; q += 256) {
    const uint32_t lr = q / side, x = q - lr * side;
    const uint32_t v = fetch<kKind, kLayer>(src, r0 + row_lo + lr, c0 + x);
    if (kPixel == 4) {
      stage[q] = v;
    } else if (kPixel == 1) {
      stage8[q] = (uint8_t)v;
    } else {
      stage8[3u * q] = (uint8_t)v;
      stage8[3u * q + 1u] = (uint8_t)(v >> 8);
      stage8[3u * q + 2u] = (uint8_t)(v >> 16);
    }
  }
  __syncthreads();
  // byte k of tile row `row` in front of the differencing: f32 in four byte planes, most
  // significant first; else the pixels' bytes.  A row in front of the staged ones (only the byte
  // in front of a piece that starts a row) comes from memory.
  auto plain = [&](uint32_t row, uint32_t k) -> uint32_t {
    if (kKind == tiff::kF32) {
      const uint32_t plane = k / side, x = k - plane * side;
      const uint32_t v = row >= row_lo ? stage[(row - row_lo) * side + x] : fetch<kKind, kLayer>(src, r0 + row, c0 + x);
      return (v >> (8u * (3u - plane))) & 255u;
    }
    if (row >= row_lo) return stage8[(row - row_lo) * rb + k];
    const uint32_t x = k / kPixel;
    return (fetch<kKind, kLayer>(src, r0 + row, c0 + x) >> (8u * (k - x * kPixel))) & 255u;
  };
  auto coded = [&](uint32_t row, uint32_t k) -> uint32_t {
    uint32_t v = plain(row, k);
    if (k >= kStride) v -= plain(row, k - kStride);
    return v & 255u;
  };
  const uint32_t g0 = b0 + tid * kLane;
  uint32_t out[4] = {0, 0, 0, 0};
  uint32_t a = 0, w = 0, last = 0;
  if (g0 < b1) {   // (raw is a multiple of 256: a lane has all of its 16 bytes or none)
    const uint32_t tile_n = b1 - b0;
    const uint32_t row = g0 / rb, k0 = g0 - row * rb, lr = row - row_lo;
    uint32_t prev = kNoByte;
    if (g0) prev = k0 ? coded(row, k0 - 1u) : coded(row - 1u, rb - 1u);
    // (side is a multiple of 16 and so is k0: the 16 bytes lie in one row and, for f32, in one plane)
    uint32_t plane = 0, x0 = k0;
    if (kKind == tiff::kF32) {
      plane = k0 / side;
      x0 = k0 - plane * side;
    }
    const uint32_t shift = 8u * (3u - plane);
    uint32_t before = 0;   // f32: the byte in front of mine, before the differencing
    if (kKind == tiff::kF32 && k0) before = plain(row, k0 - 1u);
#pragma unroll
    for (uint32_t k = 0; k < kLane; ++k) {
      uint32_t v;
      if (kKind == tiff::kF32) {
        const uint32_t cur = (stage[lr * side + x0 + k] >> shift) & 255u;
        v = (cur - before) & 255u;
        before = cur;
      } else {
        v = stage8[lr * rb + k0 + k];
        if (k0 + k >= kStride) v -= stage8[lr * rb + k0 + k - kStride];
        v &= 255u;
      }
      out[k >> 2] |= v << ((k & 3u) * 8u);
      a += v;
      w += (tile_n - (tid * kLane + k)) * v;   // (at most 4096 * 4097 / 2 * 255 < 2^32 per piece)
      if (v != prev) last = tid * kLane + k + 1;
      prev = v;
    }
  }
  *reinterpret_cast<uint4*>(b.scan + ((size_t)f * s.ntiles + piece) * kTile + tid * kLane) =
      make_uint4(out[0], out[1], out[2], out[3]);
  if (a) atomicAdd(&sh[0], a);
  if (w) atomicAdd(&sh[1], w);
  if (last) atomicMax(&sh[2], last);
  __syncthreads();
  if (tid == 0) {
    const size_t p = (size_t)f * s.ntiles + piece;
    b.tile_a[p] = sh[0];
    b.tile_w[p] = sh[1];
    b.tile_last[p] = sh[2];
  }
}

// One wave: sizes[f] = the length of tile f's stream, offs[f] = the bytes of the group's streams in
// front of it.  f < n, the frames the group's buffers hold.
__global__ void __launch_bounds__(64) k_tiff_offsets(Bufs b, uint32_t n) {
  const uint32_t lane = threadIdx.x, per = (n + 63) / 64;
  const uint32_t lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
  unsigned long long sum = 0;
  for (uint32_t f = lo; f < hi; ++f) sum += b.ctrl[f].zlen;
  unsigned long long upto = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long v = __shfl_up(upto, off);
    if ((int)lane >= off) upto += v;
  }
  unsigned long long at = upto - sum;
  for (uint32_t f = lo; f < hi; ++f) {
    const unsigned long long z = b.ctrl[f].zlen;
    b.sizes[f] = z;
    b.offs[f] = at;
    at += z;
  }
}

// Stream f to out + base + offs[f], at whatever alignment that has: a lane per 16-byte aligned block
// of the destination.  A block that lies inside the stream is one 16-byte store, assembled from the
// aligned words of the stream's buffer that cover it (the last of them holds a byte of the stream,
// so it lies inside the buffer's zwords); the blocks at the two ends are written byte by byte, the
// neighbouring streams' bytes in them by their own lanes.  Every byte written lies in
// [base + offs[f], base + offs[f] + sizes[f]), inside the file the host sized from the sizes.
//
// A launch covers the frames first .. first + gridDim.y - 1 of the group, the tiles of one level,
// which follow each other in the file from `base` + offs[first] on; the host passes base modulo 2^64
// (a level's tiles may lie in front of the group's earlier frames), the sum is the true offset.
__global__ void __launch_bounds__(256) k_tiff_gather(Share s, Bufs b, uint8_t* out, unsigned long long base,
                                                     uint32_t first) {
  const uint32_t f = first + blockIdx.y;
  const unsigned long long zlen = b.sizes[f];
  uint8_t* dst = out + (base + b.offs[f]);
  const size_t lead = reinterpret_cast<size_t>(dst) & 15u;   // bytes of the first block in front of the stream
  const unsigned long long blk = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (blk * 16u >= lead + zlen) return;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(b.z + (size_t)f * s.zwords);
  const long long rel = (long long)(blk * 16u) - (long long)lead;   // of the block's first byte in the stream
  if (rel >= 0 && (unsigned long long)rel + 16u <= zlen) {
    const uint32_t sa = (uint32_t)rel & 3u;
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(src + ((unsigned long long)rel & ~3ull));
    uint32_t v[5] = {wp[0], wp[1], wp[2], wp[3], 0};
    if (sa) {
      v[4] = wp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (v[k] >> (8u * sa)) | (v[k + 1] << (32u - 8u * sa));
    }
    *reinterpret_cast<uint4*>(dst + rel) = make_uint4(v[0], v[1], v[2], v[3]);
    return;
  }
  const unsigned long long lo = rel < 0 ? 0 : (unsigned long long)rel;
  const unsigned long long hi = (unsigned long long)(rel + 16) < zlen ? (unsigned long long)(rel + 16) : zlen;
  for (unsigned long long k = lo; k < hi; ++k) dst[k] = src[k];
}

// One call: the levels and their tiles' geometry, the groups (a tile is a frame: it costs its scratch,
// the budget is the tuning key tiffe_scratch_budget_mb), the scratch of the largest group, the
// overview rasters and, in `sizes`, the lengths of all streams.  The tiles of all levels are one
// list -- level 0's, then level 1's, .. -- cut into groups by one budget, so every pass of the coder's
// middle runs once per group; only the producer and the gather, which know where a tile comes from
// and where it goes, run once per level a group holds.
struct TiffEncoder : EncodeGroups {
  Share s = {};
  std::vector<tiff::Level> levels;
  std::vector<TileSrc> srcs;           // per level; level 0: the call's source
  std::vector<uint64_t> dest;          // every tile's place in the file, once the container is built
  DevBuf overviews;                    // the rasters of levels 1.., row-major, tightly packed
  int kind = 0;
  bool layer = false;                  // level 0 comes from a layer

  pnge::Layout layout(size_t n) const { return pnge::make_layout(s, n); }
  Bufs bufs(size_t n) { return pnge::make_bufs(scratch.as<uint8_t>(), layout(n), nullptr); }

  TileSrc source(const void* base, unsigned long long step, int width, int height, uint32_t side) const {
    TileSrc t = {};
    t.base = base;
    t.step = step;
    t.width = width;
    t.height = height;
    t.side = side;
    t.across = ((uint32_t)width + side - 1u) / side;
    t.row_bytes = side * (uint32_t)tiff::pixel_bytes(kind);
    return t;
  }

  // host only: geometry and groups; novr overview levels (>= 0, checked by the caller).  false: a piece
  // could touch more rows than the LDS stage holds (no tile side this writer accepts does).
  bool plan(const void* base, bool from_layer, unsigned long long step, int width, int height, int knd, int tile,
            int novr, float lower, float upper) {
    kind = knd;
    layer = from_layer;
    levels = tiff::make_levels(width, height, tile, novr);
    srcs.assign(levels.size(), TileSrc());
    srcs[0] = source(base, step, width, height, tiff::tile_side(tile));
    srcs[0].lower = lower;
    srcs[0].upper = upper;
    const uint32_t rb = srcs[0].row_bytes;
    // a piece starts anywhere in a row: 4096 bytes touch at most this many rows
    const uint32_t rows = kTile % rb == 0 ? kTile / rb : (kTile + rb - 2) / rb + 1;
    if ((size_t)rows * rb > kStageBytes) return false;
    s.width = width;
    s.height = height;
    s.bpp = tiff::pixel_bytes(kind);
    s.mode = kind;
    s.row_bytes = rb;
    s.row_step = 0;
    s.frame_stride = 0;
    pnge::share_set_raw(&s, tiff::tile_raw(kind, tile));
    plan_uniform((size_t)(levels.back().first + levels.back().ntiles), layout(1).total, "tiffe_scratch_budget_mb",
                 4096.0, kMaxGroupFrames);
    return true;
  }

  size_t raster_bytes(size_t k) const {   // of an overview level, its start kept on a multiple of 16
    return ((size_t)levels[k].width * (size_t)levels[k].height * (size_t)tiff::pixel_bytes(kind) + 15u) & ~(size_t)15u;
  }

  // the scratch of most_group_frames() frames; the overview rasters, each reduced from the level before it
  int open() {
    int rc;
    if ((rc = scratch.alloc(layout(most_group_frames()).total))) return rc;
    if (levels.size() == 1) return AMHIP_OK;
    size_t total = 0;
    for (size_t k = 1; k < levels.size(); ++k) total += raster_bytes(k);
    if ((rc = overviews.alloc(total))) return rc;
    size_t at = 0;
    for (size_t k = 1; k < levels.size(); ++k) {
      uint8_t* raster = overviews.as<uint8_t>() + at;
      if ((rc = tovr_reduce(stream, kind, layer && k == 1, srcs[k - 1], raster))) return rc;
      srcs[k] = source(raster, (unsigned long long)levels[k].width * (unsigned)tiff::pixel_bytes(kind), levels[k].width,
                       levels[k].height, srcs[0].side);
      at += raster_bytes(k);
    }
    return AMHIP_OK;
  }

  template <int kKind>
  void launch_tiles(const dim3& grid, bool from_layer, const TileSrc& ts, const Bufs& b) {
    if (from_layer) hipLaunchKernelGGL((k_tiff_tile<kKind, true>), grid, dim3(256), 0, stream, ts, s, b);
    else hipLaunchKernelGGL((k_tiff_tile<kKind, false>), grid, dim3(256), 0, stream, ts, s, b);
  }

  // fn(level, lo, hi): the frames [lo, hi) of the call's list that group gi holds of `level`
  template <typename Fn>
  int for_segments(size_t gi, Fn fn) {
    const uint64_t g0 = group_begin[gi], g1 = group_begin[gi + 1];
    for (size_t k = 0; k < levels.size(); ++k) {
      const uint64_t l0 = levels[k].first, l1 = l0 + levels[k].ntiles;
      const uint64_t lo = g0 > l0 ? g0 : l0, hi = g1 < l1 ? g1 : l1;
      if (lo >= hi) continue;
      const int rc = fn(k, lo, hi);
      if (rc) return rc;
    }
    return AMHIP_OK;
  }

  // every pass of group gi up to the streams and their lengths, which are read back
  int front(size_t gi) {
    const uint32_t n = (uint32_t)group_frames(gi);
    const Bufs b = bufs(n);
    AMHIP_TRY(hipMemsetAsync(b.z, 0, (size_t)n * (size_t)s.zwords * 4, stream));
    int rc = for_segments(gi, [&](size_t k, uint64_t lo, uint64_t hi) {
      TileSrc ts = srcs[k];
      ts.first = (uint32_t)(lo - levels[k].first);
      ts.frame0 = (uint32_t)(lo - group_begin[gi]);
      const dim3 grid(s.ntiles, (uint32_t)(hi - lo));
      const bool from_layer = layer && k == 0;
      if (kind == tiff::kF32) launch_tiles<tiff::kF32>(grid, from_layer, ts, b);
      else if (kind == tiff::kU8) launch_tiles<tiff::kU8>(grid, from_layer, ts, b);
      else launch_tiles<tiff::kRgb8>(grid, from_layer, ts, b);
      AMHIP_TRY(hipGetLastError());
      return (int)AMHIP_OK;
    });
    if (rc) return rc;
    if ((rc = deflate_rle_middle(stream, s, b, n))) return rc;
    hipLaunchKernelGGL(k_tiff_offsets, dim3(1), dim3(64), 0, stream, b, n);
    AMHIP_TRY(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the lengths are copied as they lie");
    AMHIP_TRY(hipMemcpyAsync(sizes.data() + group_begin[gi], b.sizes, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    AMHIP_TRY(hipStreamSynchronize(stream));
    return AMHIP_OK;
  }

  // every tile's place in the file whose levels start at level_at[k]
  void place_tiles(const std::vector<uint64_t>& level_at) {
    dest.assign(F, 0);
    for (size_t k = 0; k < levels.size(); ++k) {
      uint64_t at = level_at[k];
      for (uint64_t t = levels[k].first; t < levels[k].first + levels[k].ntiles; ++t) {
        dest[t] = at;
        at += sizes[t];
      }
    }
  }

  // ... and group gi's streams into the file at `file`, every level's to its place (place_tiles ran;
  // the driver's running offset holds for a file of one level only and is not used).  front(gi) ran last.
  int back(size_t gi, uint8_t* file, uint64_t) {
    const uint32_t n = (uint32_t)group_frames(gi);
    const Bufs b = bufs(n);
    // (a stream of z bytes behind a lead of at most 15 touches at most (z + 15 + 15) / 16 blocks)
    const unsigned blocks = (unsigned)(((largest_file(gi) + 30) / 16 + 255) / 256);
    return for_segments(gi, [&](size_t, uint64_t lo, uint64_t hi) {
      uint64_t before = 0;   // offs[lo - group_begin[gi]]: the group's streams in front of the segment
      for (uint64_t f = group_begin[gi]; f < lo; ++f) before += sizes[f];
      hipLaunchKernelGGL(k_tiff_gather, dim3(blocks, (uint32_t)(hi - lo)), dim3(256), 0, stream, s, b, file,
                         (unsigned long long)(dest[lo] - before), (uint32_t)(lo - group_begin[gi]));
      AMHIP_TRY(hipGetLastError());
      return (int)AMHIP_OK;
    });
  }
};

// what a call encodes, checked by the callers
struct TiffJob {
  const void* base;
  bool layer;
  unsigned long long step;
  int width, height, kind, tile;
  float lower, upper;
  const double* geotransform;
  int utm_zone, northern;
  int overviews;   // levels behind level 0, resolved (check_overviews)
};

// The whole file.  dev_out != null: into it, at most cap bytes, nothing written when it does not fit.
// dev_out == null: into *owned, allocated at the file's size.  *bytes: the file's size.
int tiff_encode(const char* who, hipStream_t stream, const TiffJob& job, uint8_t* dev_out, size_t cap, DevBuf* owned,
                size_t* bytes) {
  TiffEncoder enc;
  enc.stream = stream;
  if (!enc.plan(job.base, job.layer, job.step, job.width, job.height, job.kind, job.tile, job.overviews, job.lower,
                job.upper))
    return arg_failure((std::string(who) + ": tile: a piece of the tile would not fit the producer's stage").c_str());
  int rc;
  if ((rc = enc.open())) return rc;
  // The tile tables stand in front of the tiles, so the head is built from the streams' lengths and
  // copied in before the first stream follows it.
  tiff::Container file;
  rc = encode_groups(
      enc, [&](size_t gi) { return enc.front(gi); },
      [&](uint8_t** to, uint64_t* at) {
        const tiff::GeoTags geo = tiff::make_geo_tags(job.geotransform, job.utm_zone, job.northern);
        if (!tiff::build_pyramid(enc.levels, job.kind, job.tile, geo, enc.sizes.data(), &file))
          return arg_failure(
              (std::string(who) + ": the file would exceed 4 GB - 1 (BigTIFF is not written; nothing written)").c_str());
        if (bytes) *bytes = (size_t)file.file_bytes;
        *to = dev_out;
        if (dev_out) {
          if (file.file_bytes > cap) return capacity_failure(who, file.file_bytes, cap);
        } else {
          const int r = owned->alloc((size_t)file.file_bytes);
          if (r) return r;
          *to = owned->as<uint8_t>();
        }
        AMHIP_TRY(hipMemcpyAsync(*to, file.head.data(), file.head.size(), hipMemcpyHostToDevice, stream));
        enc.place_tiles(file.level_at);
        *at = file.head.size();
        return (int)AMHIP_OK;
      });
  if (rc) return rc;
  AMHIP_TRY(hipStreamSynchronize(stream));   // (the scratch, the overviews and the head go with this call)
  return AMHIP_OK;
}

// encode, download, write `filename`
int tiff_write(const char* who, hipStream_t stream, const TiffJob& job, const char* filename) {
  DevBuf out;
  size_t bytes = 0;
  int rc = tiff_encode(who, stream, job, nullptr, 0, &out, &bytes);
  if (rc) return rc;
  std::vector<uint8_t> host(bytes);
  AMHIP_TRY(hipMemcpyAsync(host.data(), out.p, bytes, hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  return write_file(who, filename, host.data(), host.size());
}

int bad(const char* who, const char* why) { return arg_failure((std::string(who) + ": " + why).c_str()); }

// the argument errors of a raster call; 0: fine
int check_raster_call(const char* who, size_t step, int width, int height, int kind, int tile,
                      const double* geotransform, int utm_zone) {
  if (const char* why = tiff::check_raster(width, height, kind, tile)) return bad(who, why);
  if (step < (size_t)width * (size_t)tiff::pixel_bytes(kind)) return bad(who, "step smaller than a row");
  if (const char* why = tiff::check_geo(geotransform, utm_zone)) return bad(who, why);
  return AMHIP_OK;
}

// ... and of a layer call on a window of win_rows x win_cols cells
int check_layer_call(const char* who, int layer, int kind, float lower, float upper, int tile, int utm_zone,
                     int win_rows, int win_cols) {
  if (layer < 0 || layer >= AMHIP_NUM_LAYERS) return bad(who, "layer: no such layer");
  // (the raster's width is the window's rows, its height the window's columns)
  if (const char* why = tiff::check_raster(win_rows, win_cols, kind, tile)) return bad(who, why);
  if (utm_zone < 1 || utm_zone > 60) return bad(who, "utm_zone must be 1..60");
  if (kind == tiff::kU8 && !(upper > lower)) return bad(who, "upper <= lower");
  return AMHIP_OK;
}

// the north-up raster of the context's window of `layer`; gt: six doubles to fill
TiffJob layer_job(Ctx* c, int layer, int kind, float lower, float upper, int tile, int utm_zone, int northern,
                  double* gt) {
  const amhip_grid_desc& g = c->grid;
  gt[0] = g.pos_x - g.length_x / 2 + g.resolution * (double)(g.rows - c->win_i0 - c->win_rows);
  gt[1] = g.resolution;
  gt[2] = 0.0;
  gt[3] = g.pos_y + g.length_y / 2 - g.resolution * (double)c->win_j0;
  gt[4] = 0.0;
  gt[5] = -g.resolution;
  return TiffJob{c->layers[layer], true, (unsigned long long)c->win_rows, c->win_rows, c->win_cols, kind, tile,
                 lower, upper, gt, utm_zone, northern};
}

}  // namespace

}  // namespace amhip

using namespace amhip;

namespace {

// The bodies of the exports: `who` is the export's name, overviews as the caller gave it (0 for the
// exports without the argument, which stay what they were).
int geotiff_encode_dev(const char* who, amhip_ctx* h, const void* dev_raster, size_t step, int width, int height,
                       int kind, int tile, int overviews, const double* geotransform, int utm_zone, int northern,
                       uint8_t* dev_out, size_t cap, size_t* bytes) {
  if (!h || !dev_raster || !geotransform || !dev_out || !bytes) return bad(who, "null argument");
  int rc = check_raster_call(who, step, width, height, kind, tile, geotransform, utm_zone);
  if (rc) return rc;
  int novr = 0;
  if (const char* why = tiff::check_overviews(width, height, tile, overviews, &novr)) return bad(who, why);
  Ctx* c = &h->impl;
  if ((rc = ctx_use_device(c))) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  const TiffJob job = {dev_raster, false, step, width, height, kind, tile, 0.0f, 0.0f, geotransform, utm_zone, northern,
                       novr};
  return tiff_encode(who, c->stream, job, dev_out, cap, nullptr, bytes);
}

int geotiff_write(const char* who, amhip_ctx* h, const char* filename, const void* raster, int on_device, size_t step,
                  int width, int height, int kind, int tile, int overviews, const double* geotransform, int utm_zone,
                  int northern) {
  if (!h || !filename || !raster || !geotransform) return bad(who, "null argument");
  int rc = check_raster_call(who, step, width, height, kind, tile, geotransform, utm_zone);
  if (rc) return rc;
  int novr = 0;
  if (const char* why = tiff::check_overviews(width, height, tile, overviews, &novr)) return bad(who, why);
  Ctx* c = &h->impl;
  if ((rc = ctx_use_device(c))) return rc;
  TiffJob job = {raster, false, step, width, height, kind, tile, 0.0f, 0.0f, geotransform, utm_zone, northern, novr};
  DevBuf staged;
  if (!on_device) {
    const size_t row = (size_t)width * (size_t)tiff::pixel_bytes(kind);
    if ((rc = staged.alloc(row * (size_t)height))) return rc;
    AMHIP_TRY(hipMemcpy2DAsync(staged.p, row, raster, step, row, (size_t)height, hipMemcpyHostToDevice, c->stream));
    job.base = staged.p;
    job.step = row;
  }
  ScopedTimer timer(c, AMHIP_K_MISC);
  return tiff_write(who, c->stream, job, filename);
}

// a layer call up to its job; gt: six doubles the job points to
int layer_call(const char* who, amhip_ctx* h, int layer, int kind, float lower, float upper, int tile, int overviews,
               int utm_zone, int northern, double* gt, TiffJob* job) {
  Ctx* c = &h->impl;
  int rc = check_layer_call(who, layer, kind, lower, upper, tile, utm_zone, c->win_rows, c->win_cols);
  if (rc) return rc;
  int novr = 0;
  if (const char* why = tiff::check_overviews(c->win_rows, c->win_cols, tile, overviews, &novr)) return bad(who, why);
  if ((rc = ctx_use_device(c))) return rc;
  if ((rc = ctx_materialize(c, layer))) return rc;
  *job = layer_job(c, layer, kind, lower, upper, tile, utm_zone, northern, gt);
  job->overviews = novr;
  return AMHIP_OK;
}

int layer_encode_geotiff_dev(const char* who, amhip_ctx* h, int layer, int kind, float lower, float upper, int tile,
                             int overviews, int utm_zone, int northern, uint8_t* dev_out, size_t cap, size_t* bytes) {
  if (!h || !dev_out || !bytes) return bad(who, "null argument");
  double gt[6];
  TiffJob job;
  const int rc = layer_call(who, h, layer, kind, lower, upper, tile, overviews, utm_zone, northern, gt, &job);
  if (rc) return rc;
  ScopedTimer timer(&h->impl, AMHIP_K_MISC);
  return tiff_encode(who, h->impl.stream, job, dev_out, cap, nullptr, bytes);
}

int layer_write_geotiff(const char* who, amhip_ctx* h, int layer, int kind, float lower, float upper, int tile,
                        int overviews, int utm_zone, int northern, const char* filename) {
  if (!h || !filename) return bad(who, "null argument");
  double gt[6];
  TiffJob job;
  const int rc = layer_call(who, h, layer, kind, lower, upper, tile, overviews, utm_zone, northern, gt, &job);
  if (rc) return rc;
  ScopedTimer timer(&h->impl, AMHIP_K_MISC);
  return tiff_write(who, h->impl.stream, job, filename);
}

}  // namespace

extern "C" {

size_t amhip_geotiff_bound(int width, int height, int kind, int tile) {
  if (tiff::check_raster(width, height, kind, tile)) return 0;
  return (size_t)tiff::file_bound(width, height, kind, tile);
}

size_t amhip_geotiff_bound_ovr(int width, int height, int kind, int tile, int overviews) {
  int novr = 0;
  if (tiff::check_raster(width, height, kind, tile) || tiff::check_overviews(width, height, tile, overviews, &novr))
    return 0;
  return (size_t)tiff::file_bound_ovr(width, height, kind, tile, novr);
}

int amhip_geotiff_encode_dev(amhip_ctx* h, const void* dev_raster, size_t step, int width, int height, int kind,
                             int tile, const double* geotransform, int utm_zone, int northern, uint8_t* dev_out,
                             size_t cap, size_t* bytes) {
  return geotiff_encode_dev("amhip_geotiff_encode_dev", h, dev_raster, step, width, height, kind, tile, 0, geotransform,
                            utm_zone, northern, dev_out, cap, bytes);
}

int amhip_geotiff_encode_ovr_dev(amhip_ctx* h, const void* dev_raster, size_t step, int width, int height, int kind,
                                 int tile, int overviews, const double* geotransform, int utm_zone, int northern,
                                 uint8_t* dev_out, size_t cap, size_t* bytes) {
  return geotiff_encode_dev("amhip_geotiff_encode_ovr_dev", h, dev_raster, step, width, height, kind, tile, overviews,
                            geotransform, utm_zone, northern, dev_out, cap, bytes);
}

int amhip_geotiff_write(amhip_ctx* h, const char* filename, const void* raster, int on_device, size_t step,
                        int width, int height, int kind, int tile, const double* geotransform, int utm_zone,
                        int northern) {
  return geotiff_write("amhip_geotiff_write", h, filename, raster, on_device, step, width, height, kind, tile, 0,
                       geotransform, utm_zone, northern);
}

int amhip_geotiff_write_ovr(amhip_ctx* h, const char* filename, const void* raster, int on_device, size_t step,
                            int width, int height, int kind, int tile, int overviews, const double* geotransform,
                            int utm_zone, int northern) {
  return geotiff_write("amhip_geotiff_write_ovr", h, filename, raster, on_device, step, width, height, kind, tile,
                       overviews, geotransform, utm_zone, northern);
}

int amhip_layer_encode_geotiff_dev(amhip_ctx* h, int layer, int kind, float lower, float upper, int tile,
                                   int utm_zone, int northern, uint8_t* dev_out, size_t cap, size_t* bytes) {
  return layer_encode_geotiff_dev("amhip_layer_encode_geotiff_dev", h, layer, kind, lower, upper, tile, 0, utm_zone,
                                  northern, dev_out, cap, bytes);
}

int amhip_layer_encode_geotiff_ovr_dev(amhip_ctx* h, int layer, int kind, float lower, float upper, int tile,
                                       int overviews, int utm_zone, int northern, uint8_t* dev_out, size_t cap,
                                       size_t* bytes) {
  return layer_encode_geotiff_dev("amhip_layer_encode_geotiff_ovr_dev", h, layer, kind, lower, upper, tile, overviews,
                                  utm_zone, northern, dev_out, cap, bytes);
}

int amhip_layer_write_geotiff(amhip_ctx* h, int layer, int kind, float lower, float upper, int tile, int utm_zone,
                              int northern, const char* filename) {
  return layer_write_geotiff("amhip_layer_write_geotiff", h, layer, kind, lower, upper, tile, 0, utm_zone, northern,
                             filename);
}

int amhip_layer_write_geotiff_ovr(amhip_ctx* h, int layer, int kind, float lower, float upper, int tile, int overviews,
                                  int utm_zone, int northern, const char* filename) {
  return layer_write_geotiff("amhip_layer_write_geotiff_ovr", h, layer, kind, lower, upper, tile, overviews, utm_zone,
                             northern, filename);
}

}  // extern "C"
