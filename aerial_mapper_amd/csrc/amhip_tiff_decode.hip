// amhip_tiff_decode.hip -- a Deflate GeoTIFF into a device raster or under a map layer, decoded on
// the GPU: the inverse of amhip_tiff_encode.hip for a wider set of files (tiles or strips, five
// sample kinds, Predictor 1 / 2 / 3, Compression 1 / 8 / 32946).  DESIGN 4.17.  The TIFF parser is
// host code (amhip_tiff_decode_host.h); tests/geotiff_read_reference.py restates every rule.
//
// Only the chunks (tiles or strips) that meet the wanted pixel window are uploaded, each at a
// multiple of 16 of the upload buffer, and they run in groups bounded by the tuning key
// tiffd_scratch_budget_mb:
//   1. k_pngd_inflate     (amhip_png_inflate.h) RFC 1951 with the Adler-32 check, one wave per chunk:
//                         a chunk of Compression 8 / 32946 is one zlib stream.  Uncompressed chunks
//                         are copied into the same scratch instead.
//   2. k_tiffd_unpredict  one wave per row of a chunk: the inverse predictor as a wave-level inclusive
//                         scan (DPP) over rounds of 64 samples with the running sum carried from round
//                         to round, then the crop: the samples of the window go into a row-major
//                         north-up raster in the file's sample type.
//   3. k_tiffd_place      (layers only) one lane per cell of the context's window: the pixel the
//                         cell's centre lies in, converted to float, or nothing.
// The statuses are read back once per call, before step 3: a layer is written only when every chunk
// has decoded.
//
// Bounds.  Inflate: as stated in amhip_png_decode.hip; its stores cover [raw_base, raw_base + raw_len
// rounded up to 16) of the group's scratch, which is the sum of exactly those sizes.  Unpredict: a wave
// reads bytes [0, chunk_w * bytes per pixel) of its own row of its own chunk and stores only samples
// whose image position lies in the window, which the host has checked to lie in the raster and in
// dev_out's rows.  Place: a lane reads the raster only after its column and row have passed the
// window test, and writes only its own cell.  Every loop runs a number of rounds fixed by the row's
// length.
#include <cerrno>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_common.h"
#include "amhip_device.h"
#include "amhip_frame_stack.h"
#include "amhip_png_inflate.h"
#include "amhip_tiff_decode_host.h"

namespace amhip {

namespace {

using tiffd::Parsed;

constexpr size_t kMaxGroupChunks = 65535;   // (grid.y of the per-row launch)

// where a selected chunk lies in the image
struct ChunkGeo {
  uint32_t col0, row0;   // its first sample's image position
  uint32_t rows;         // rows it holds
  uint32_t pad;
};

struct Unpredict {
  const uint8_t* raw;           // the group's inflated chunks
  const pngd::Frame* frames;    // raw_base per chunk
  const ChunkGeo* geo;
  const uint32_t* status;
  unsigned long long first;     // the group's first chunk
  uint32_t chunk_w;             // samples per chunk row
  int kind, predictor;
  int wx0, wy0, ww, wh;         // the pixel window
  uint8_t* out;                 // its first pixel
  unsigned long long step;      // bytes between its rows
};

__device__ __forceinline__ uint32_t lane63(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// One wave per chunk row (four rows per workgroup; no LDS, no barrier).  Every loop below is
// wave-uniform -- its bounds depend on the row alone -- so the DPP scan sees all 64 lanes.
__global__ void __launch_bounds__(256) k_tiffd_unpredict(Unpredict u) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t s = (size_t)u.first + blockIdx.y;
  if (u.status[s] != 0) return;   // (the rows are not there)
  const ChunkGeo g = u.geo[s];
  const uint32_t row = blockIdx.x * 4u + wave;
  if (row >= g.rows) return;
  const long long y = (long long)g.row0 + row;
  if (y < u.wy0 || y >= (long long)u.wy0 + u.wh) return;
  // the samples [k_lo, k_hi) of this row lie in the window
  const long long lo = (long long)u.wx0 - g.col0, hi = (long long)u.wx0 + u.ww - g.col0;
  const uint32_t cw = u.chunk_w;
  const uint32_t k_lo = lo < 0 ? 0u : (uint32_t)lo;
  const uint32_t k_hi = hi > (long long)cw ? cw : (hi < 0 ? 0u : (uint32_t)hi);
  if (k_lo >= k_hi) return;
  const int kind = u.kind;
  const uint32_t bpp = kind == tiffd::kF32 ? 4u : kind == tiffd::kU8 ? 1u : kind == tiffd::kRgb8 ? 3u : 2u;
  const uint8_t* src = u.raw + u.frames[s].raw_base + (size_t)row * cw * bpp;   // (a multiple of bpp's power of two)
  // image column g.col0 + k -> byte (g.col0 + k - wx0) * bpp of the output row
  uint8_t* dst = u.out + (size_t)(y - u.wy0) * u.step;
  const long long shift = (long long)g.col0 - u.wx0;

  if (u.predictor == 3) {
    // libtiff's fpAcc: an inclusive byte sum over the row's 4 * cw bytes, then float k is bytes
    // [k], [cw + k], [2 cw + k], [3 cw + k], most significant first.  The sum entering plane p is the
    // total of the planes before it: one pass for the totals, one for the four scans.
    uint32_t t0 = 0, t1 = 0, t2 = 0;
    for (uint32_t k = lane; k < cw; k += 64) {
      t0 += src[k];
      t1 += src[(size_t)cw + k];
      t2 += src[2 * (size_t)cw + k];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      t0 += (uint32_t)__shfl_xor((int)t0, m);
      t1 += (uint32_t)__shfl_xor((int)t1, m);
      t2 += (uint32_t)__shfl_xor((int)t2, m);
    }
    uint32_t c0 = 0, c1 = t0 & 255u, c2 = (t0 + t1) & 255u, c3 = (t0 + t1 + t2) & 255u;
    for (uint32_t k0 = 0; k0 < k_hi; k0 += 64) {
      const uint32_t k = k0 + lane;
      uint32_t a = 0, b = 0;   // two byte sums per word, 16 bits apart: 64 * 255 < 2^16, no sum reaches its neighbour
      if (k < k_hi) {
        a = (uint32_t)src[k] | ((uint32_t)src[2 * (size_t)cw + k] << 16);
        b = (uint32_t)src[(size_t)cw + k] | ((uint32_t)src[3 * (size_t)cw + k] << 16);
      }
      a = wave_incl_scan(a, (int)lane);
      b = wave_incl_scan(b, (int)lane);
      const uint32_t s0 = ((a & 0xFFFFu) + c0) & 255u, s2 = ((a >> 16) + c2) & 255u;
      const uint32_t s1 = ((b & 0xFFFFu) + c1) & 255u, s3 = ((b >> 16) + c3) & 255u;
      c0 = lane63(s0);
      c1 = lane63(s1);
      c2 = lane63(s2);
      c3 = lane63(s3);
      if (k >= k_lo && k < k_hi)
        *reinterpret_cast<uint32_t*>(dst + (size_t)((long long)k + shift) * 4u) = (s0 << 24) | (s1 << 16) | (s2 << 8) | s3;
    }
    return;
  }
  // Predictor 1 and 2 on whole samples; three bands: three interleaved sums
  const bool acc = u.predictor == 2;
  uint32_t carry[3] = {0, 0, 0};
  for (uint32_t k0 = acc ? 0u : (k_lo & ~63u); k0 < k_hi; k0 += 64) {
    const uint32_t k = k0 + lane;
    uint32_t v[3] = {0, 0, 0};
    if (k < k_hi) {
      if (bpp == 4) v[0] = *reinterpret_cast<const uint32_t*>(src + (size_t)k * 4u);
      else if (bpp == 2) v[0] = *reinterpret_cast<const uint16_t*>(src + (size_t)k * 2u);
      else if (bpp == 1) v[0] = src[k];
      else {
        v[0] = src[(size_t)k * 3u];
        v[1] = src[(size_t)k * 3u + 1u];
        v[2] = src[(size_t)k * 3u + 2u];
      }
    }
    if (acc) {
      // (sums modulo 2^32; the 8- and 16-bit ones are cut to their width at the store: 2^8 and 2^16 divide 2^32)
      v[0] = wave_incl_scan(v[0], (int)lane) + carry[0];
      carry[0] = lane63(v[0]);
      if (bpp == 3) {
        v[1] = wave_incl_scan(v[1], (int)lane) + carry[1];
        carry[1] = lane63(v[1]);
        v[2] = wave_incl_scan(v[2], (int)lane) + carry[2];
        carry[2] = lane63(v[2]);
      }
    }
    if (k >= k_lo && k < k_hi) {
      uint8_t* p = dst + (size_t)((long long)k + shift) * bpp;
      if (bpp == 4) *reinterpret_cast<uint32_t*>(p) = v[0];
      else if (bpp == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v[0];
      else if (bpp == 1) p[0] = (uint8_t)v[0];
      else {
        p[0] = (uint8_t)v[0];
        p[1] = (uint8_t)v[1];
        p[2] = (uint8_t)v[2];
      }
    }
  }
}

struct Place {
  double base_x, base_y, res;   // getPosition, as DsmParams
  int rows, cols, i_off, j_off; // the context's window
  double gt0, gt1, gt3, gt5;    // the file's geotransform (pixel areas)
  const uint8_t* raster;        // the decoded pixel window, in the file's sample type
  unsigned long long step;
  int rx0, ry0, rw, rh;         // ... and where it lies in the file
  int kind, has_nodata;
  double nodata;
  int fill;                     // the layer is logically initial: cells that take no pixel get `init`
  float init;
  float* layer;                 // the window's cells, column-major
};

__global__ void __launch_bounds__(256) k_tiffd_place(Place p) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)p.rows * (size_t)p.cols) return;
  const int i = (int)(idx % (size_t)p.rows), j = (int)(idx / (size_t)p.rows);
  // grid_map_core getPosition, as every kernel of the library computes it
  const double x = p.base_x + p.res * (-(double)(i + p.i_off));
  const double y = p.base_y + p.res * (-(double)(j + p.j_off));
  // (IEEE double: this build's `/` is the correctly rounded division, -ffp-contract=off keeps the
  // subtraction apart)
  const double col = floor((x - p.gt0) / p.gt1), row = floor((y - p.gt3) / p.gt5);
  bool have = col >= (double)p.rx0 && col < (double)p.rx0 + (double)p.rw && row >= (double)p.ry0 &&
              row < (double)p.ry0 + (double)p.rh;   // (a NaN fails every comparison)
  float value = 0.0f;
  if (have) {
    const size_t c = (size_t)((long long)col - p.rx0);
    const uint8_t* line = p.raster + (size_t)((long long)row - p.ry0) * p.step;
    if (p.kind == tiffd::kF32) {
      value = reinterpret_cast<const float*>(line)[c];
      have = value == value && !(p.has_nodata && value == (float)p.nodata);
    } else if (p.kind == tiffd::kRgb8) {
      const uint32_t R = line[3 * c], G = line[3 * c + 1], B = line[3 * c + 2];
      value = __uint_as_float((R << 16) | (G << 8) | B);
      have = !(p.has_nodata && (double)R == p.nodata && (double)G == p.nodata && (double)B == p.nodata);
    } else {
      int v;
      if (p.kind == tiffd::kU8) v = line[c];
      else if (p.kind == tiffd::kU16) v = reinterpret_cast<const uint16_t*>(line)[c];
      else v = reinterpret_cast<const int16_t*>(line)[c];
      value = (float)v;   // (exact: |v| < 2^16)
      have = !(p.has_nodata && (double)v == p.nodata);
    }
  }
  if (have) p.layer[idx] = value;
  else if (p.fill) p.layer[idx] = p.init;
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

int bad(const char* who, const std::string& why) { return arg_failure((std::string(who) + ": " + why).c_str()); }

// The pixel window (x0, y0, w, h) of a parsed file -> out (rows `step` bytes apart), asynchronous on
// `stream` up to the read-back of the statuses.  The window lies inside the raster; out and step are
// multiples of the sample's size.  All scratch lives for the call.
// `where`: what stands in front of a chunk's name in an error text ("level 2: " or nothing).
int decode_window(const char* who, const std::string& where, hipStream_t stream, const uint8_t* file, const Parsed& P,
                  int x0, int y0, int w, int h, uint8_t* out, size_t step) {
  // ---- host: the chunks the window meets, their streams packed at multiples of 16 -------------
  const uint32_t cw = P.chunk_w, chh = P.chunk_h;
  const uint32_t tx_lo = P.tiled ? (uint32_t)x0 / cw : 0u, tx_hi = P.tiled ? (uint32_t)(x0 + w - 1) / cw : 0u;
  const uint32_t ty_lo = (uint32_t)y0 / chh, ty_hi = (uint32_t)(y0 + h - 1) / chh;
  std::vector<size_t> sel;
  for (uint32_t ty = ty_lo; ty <= ty_hi; ++ty)
    for (uint32_t tx = tx_lo; tx <= tx_hi; ++tx) sel.push_back((size_t)ty * P.across + tx);
  const size_t S = sel.size();
  const bool deflate = P.compression != 1;
  std::vector<pngd::Frame> frames(S);
  std::vector<ChunkGeo> geo(S);
  std::vector<size_t> cost(S), base(S);
  std::vector<uint8_t> packed;
  if (deflate) {
    size_t total = 0;
    for (size_t k = 0; k < S; ++k) total += round16((size_t)P.chunks[sel[k]].count);
    packed.assign(total, 0);
  }
  size_t at = 0;
  for (size_t k = 0; k < S; ++k) {
    const tiffd::Chunk& c = P.chunks[sel[k]];
    pngd::Frame& f = frames[k];
    std::memset(&f, 0, sizeof(f));
    f.raw_len = c.raw_len;
    if (deflate) {   // (the parser has checked: at least 6 bytes, a zlib header, inside the file)
      std::memcpy(packed.data() + at, file + c.offset, (size_t)c.count);
      const uint8_t* tail = file + c.offset + c.count - 4;
      f.adler = ((uint32_t)tail[0] << 24) | ((uint32_t)tail[1] << 16) | ((uint32_t)tail[2] << 8) | tail[3];
      f.stream_begin = at + 2;
      f.stream_end = at + c.count - 4;
      at += round16((size_t)c.count);
    }
    geo[k].col0 = (uint32_t)(sel[k] % P.across) * (P.tiled ? cw : 0u);
    geo[k].row0 = (uint32_t)(sel[k] / P.across) * chh;
    geo[k].rows = c.rows;
    geo[k].pad = 0;
    cost[k] = round16((size_t)c.raw_len);
  }
  std::vector<size_t> group_begin;
  size_t max_group_bytes = 0;
  plan_groups(cost.data(), S, budget_bytes("tiffd_scratch_budget_mb", 4096.0), kMaxGroupChunks, &group_begin,
              base.data(), &max_group_bytes);
  for (size_t k = 0; k < S; ++k) frames[k].raw_base = base[k];
  // ---- the device --------------------------------------------------------------------------------
  int rc;
  DevBuf bytes, raw, dframes, dgeo, dstatus;
  if (deflate && (rc = bytes.alloc(packed.size()))) return rc;
  if ((rc = raw.alloc(max_group_bytes))) return rc;
  if ((rc = dframes.alloc(S * sizeof(pngd::Frame)))) return rc;
  if ((rc = dgeo.alloc(S * sizeof(ChunkGeo)))) return rc;
  if ((rc = dstatus.alloc(S * sizeof(uint32_t)))) return rc;
  if (deflate) AMHIP_TRY(hipMemcpyAsync(bytes.p, packed.data(), packed.size(), hipMemcpyHostToDevice, stream));
  AMHIP_TRY(hipMemcpyAsync(dframes.p, frames.data(), S * sizeof(pngd::Frame), hipMemcpyHostToDevice, stream));
  AMHIP_TRY(hipMemcpyAsync(dgeo.p, geo.data(), S * sizeof(ChunkGeo), hipMemcpyHostToDevice, stream));
  AMHIP_TRY(hipMemsetAsync(dstatus.p, 0, S * sizeof(uint32_t), stream));
  Unpredict u;
  u.raw = raw.as<uint8_t>();
  u.frames = dframes.as<pngd::Frame>();
  u.geo = dgeo.as<ChunkGeo>();
  u.status = dstatus.as<uint32_t>();
  u.chunk_w = cw;
  u.kind = P.kind;
  u.predictor = P.predictor;
  u.wx0 = x0;
  u.wy0 = y0;
  u.ww = w;
  u.wh = h;
  u.out = out;
  u.step = step;
  for (size_t g = 0; g + 1 < group_begin.size(); ++g) {
    const size_t first = group_begin[g], n = group_begin[g + 1] - first;
    if (deflate) {
      pngd::launch_inflate(stream, bytes.as<uint8_t>(), dframes.as<pngd::Frame>(), first, n, raw.as<uint8_t>(),
                           dstatus.as<uint32_t>());
    } else {
      for (size_t k = first; k < first + n; ++k)   // (count == raw_len, checked by the parser)
        AMHIP_TRY(hipMemcpyAsync(raw.as<uint8_t>() + base[k], file + P.chunks[sel[k]].offset,
                                 (size_t)P.chunks[sel[k]].count, hipMemcpyHostToDevice, stream));
    }
    u.first = first;
    hipLaunchKernelGGL(k_tiffd_unpredict, dim3((chh + 3u) / 4u, (unsigned)n), dim3(256), 0, stream, u);
    AMHIP_TRY(hipGetLastError());
  }
  std::vector<uint32_t> st(S);
  AMHIP_TRY(hipMemcpyAsync(st.data(), dstatus.p, S * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  AMHIP_TRY(hipStreamSynchronize(stream));
  for (size_t k = 0; k < S; ++k)
    if (st[k]) {
      char name[96];
      tiffd::chunk_name(P, sel[k], name, sizeof(name));
      return bad(who, where + name + ": inflate status " + std::to_string(st[k]) + ", " + pngd::status_text(st[k]));
    }
  return AMHIP_OK;
}

bool parse_or_text(const char* who, const uint8_t* file, size_t len, Parsed* P) {
  char text[200];
  if (!tiffd::parse(file, len, P, text, sizeof(text))) {
    bad(who, text);
    return false;
  }
  return true;
}

bool level_or_text(const char* who, const uint8_t* file, size_t len, int level, Parsed* P, int* nlevels = nullptr) {
  char text[320];
  if (!tiffd::parse_level(file, len, level, P, nlevels, text, sizeof(text))) {
    bad(who, text);
    return false;
  }
  return true;
}

void fill_desc(const Parsed& P, amhip_geotiff_desc* desc) {
  std::memset(desc, 0, sizeof(*desc));
  desc->width = P.width;
  desc->height = P.height;
  desc->bands = P.bands;
  desc->kind = P.kind;
  desc->tiled = P.tiled;
  desc->tile_width = P.tiled ? (int32_t)P.chunk_w : 0;
  desc->tile_height = P.tiled ? (int32_t)P.chunk_h : 0;
  desc->rows_per_strip = P.tiled ? 0 : (int32_t)P.chunk_h;
  desc->compression = P.compression;
  desc->predictor = P.predictor;
  desc->has_geo = P.has_geo;
  desc->epsg = P.epsg;
  desc->raster_type = P.raster_type;
  desc->has_nodata = P.has_nodata;
  for (int k = 0; k < 6; ++k) desc->geotransform[k] = P.gt[k];
  desc->nodata = P.nodata;
}

}  // namespace

// One layer call in its two halves (the session runs the first half on every window before the
// second on any): what has been decoded for the context's window, and where it lies in the file.
struct TiffLayerJob {
  Parsed P;
  DevBuf raster;
  size_t step = 0;
  int layer = 0;
  int rx0 = 0, ry0 = 0, rw = 0, rh = 0;   // rw == 0: the file does not reach the window
};

void tiff_layer_job_free(TiffLayerJob* job) { delete job; }

int tiff_layer_prepare(Ctx* c, const char* who, int layer, const uint8_t* file, size_t len, int level,
                       TiffLayerJob** out) {
  *out = nullptr;
  if (layer < 0 || layer >= AMHIP_NUM_LAYERS) return bad(who, "layer: no such layer");
  TiffLayerJob* job = new TiffLayerJob;
  struct Guard {
    TiffLayerJob* j;
    ~Guard() { delete j; }
  } guard = {job};
  std::string where;
  if (level == kTiffFirstIfd) {
    if (!parse_or_text(who, file, len, &job->P)) return AMHIP_ERR_ARG;
  } else {
    if (level < -1) return bad(who, "level: -1 (automatic) or a level of the file, 0 ..");
    if (level == -1) {   // the coarsest level whose pixels are no larger than the map's cells
      std::vector<tiffd::Ifd> ifds;
      char text[200];
      if (!tiffd::walk_chain(file, len, &ifds, text, sizeof(text))) return bad(who, text);
      Parsed base;
      if (!tiffd::parse_ifd(file, len, ifds[0].at, &base, text, sizeof(text))) return bad(who, text);
      level = base.has_geo ? tiffd::auto_level(base, ifds, c->grid.resolution) : 0;
    }
    if (!level_or_text(who, file, len, level, &job->P)) return AMHIP_ERR_ARG;
    where = "level " + std::to_string(level) + ": ";
  }
  const Parsed& P = job->P;
  if (!P.has_geo) return bad(who, "the file has no geo tags (ModelPixelScale + ModelTiepoint or ModelTransformation)");
  if (P.kind == tiffd::kRgb8 && layer != AMHIP_LAYER_COLORED_ORTHO)
    return bad(who, "layer: a three-band file goes to colored_ortho only");
  job->layer = layer;
  // the window's footprint in the file: columns fall with i, rows grow with j
  const amhip_grid_desc& g = c->grid;
  const double base_x = g.pos_x + (0.5 * g.length_x - 0.5 * g.resolution);
  const double base_y = g.pos_y + (0.5 * g.length_y - 0.5 * g.resolution);
  auto col_of = [&](int i) { return std::floor((base_x + g.resolution * (-(double)(i + c->win_i0)) - P.gt[0]) / P.gt[1]); };
  auto row_of = [&](int j) { return std::floor((base_y + g.resolution * (-(double)(j + c->win_j0)) - P.gt[3]) / P.gt[5]); };
  double c_lo = col_of(c->win_rows - 1), c_hi = col_of(0), r_lo = row_of(0), r_hi = row_of(c->win_cols - 1);
  if (c_lo < 0.0) c_lo = 0.0;
  if (r_lo < 0.0) r_lo = 0.0;
  if (c_hi > (double)(P.width - 1)) c_hi = (double)(P.width - 1);
  if (r_hi > (double)(P.height - 1)) r_hi = (double)(P.height - 1);
  if (!(c_lo <= c_hi) || !(r_lo <= r_hi)) {   // (no overlap, or a NaN)
    *out = job;
    guard.j = nullptr;
    return AMHIP_OK;
  }
  job->rx0 = (int)c_lo;
  job->ry0 = (int)r_lo;
  job->rw = (int)c_hi - job->rx0 + 1;
  job->rh = (int)r_hi - job->ry0 + 1;
  int rc;
  if ((rc = ctx_use_device(c))) return rc;
  job->step = ((size_t)job->rw * (size_t)tiffd::pixel_bytes(P.kind) + 3u) & ~(size_t)3u;
  if ((rc = job->raster.alloc(job->step * (size_t)job->rh))) return rc;
  if ((rc = decode_window(who, where, c->stream, file, P, job->rx0, job->ry0, job->rw, job->rh, job->raster.as<uint8_t>(),
                          job->step)))
    return rc;
  *out = job;
  guard.j = nullptr;
  return AMHIP_OK;
}

int tiff_layer_place(Ctx* c, TiffLayerJob* job) {
  if (job->rw == 0) return AMHIP_OK;   // nothing of the file under the window: every cell stays
  int rc;
  if ((rc = ctx_use_device(c))) return rc;
  const Parsed& P = job->P;
  const amhip_grid_desc& g = c->grid;
  Place p;
  p.base_x = g.pos_x + (0.5 * g.length_x - 0.5 * g.resolution);
  p.base_y = g.pos_y + (0.5 * g.length_y - 0.5 * g.resolution);
  p.res = g.resolution;
  p.rows = c->win_rows;
  p.cols = c->win_cols;
  p.i_off = c->win_i0;
  p.j_off = c->win_j0;
  p.gt0 = P.gt[0];
  p.gt1 = P.gt[1];
  p.gt3 = P.gt[3];
  p.gt5 = P.gt[5];
  p.raster = job->raster.as<uint8_t>();
  p.step = job->step;
  p.rx0 = job->rx0;
  p.ry0 = job->ry0;
  p.rw = job->rw;
  p.rh = job->rh;
  p.kind = P.kind;
  p.has_nodata = P.has_nodata;
  p.nodata = P.nodata;
  // a pending lazy reset: this kernel writes the initial value into the cells it leaves alone
  p.fill = c->layer_state[job->layer] == kLayerLazyInitial ? 1 : 0;
  p.init = ctx_layer_init_value(job->layer);
  p.layer = c->layers[job->layer];
  ctx_overwrite(c, job->layer);   // (every cell is defined after the kernel; heights now come from outside)
  ScopedTimer timer(c, AMHIP_K_MISC);
  const size_t cells = (size_t)p.rows * (size_t)p.cols;
  hipLaunchKernelGGL(k_tiffd_place, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, p);
  AMHIP_TRY(hipGetLastError());
  AMHIP_TRY(hipStreamSynchronize(c->stream));   // (the raster goes with the job)
  return AMHIP_OK;
}

}  // namespace amhip

using namespace amhip;

extern "C" {

int amhip_geotiff_info(const uint8_t* file, size_t len, amhip_geotiff_desc* desc) {
  static const char kWho[] = "amhip_geotiff_info";
  if (!file || !desc) return bad(kWho, "null argument");
  Parsed P;
  if (!parse_or_text(kWho, file, len, &P)) return AMHIP_ERR_ARG;
  fill_desc(P, desc);
  return AMHIP_OK;
}

// the pixel window of a parsed level into dev_out: the checks and the call
static int decode_parsed(const char* kWho, const std::string& where, amhip_ctx* h, const uint8_t* file, const Parsed& P,
                         int x0, int y0, int w, int ht, void* dev_out, size_t step) {
  if (x0 < 0 || y0 < 0 || w < 1 || ht < 1 || (long long)x0 + w > P.width || (long long)y0 + ht > P.height)
    return bad(kWho, "the pixel window leaves the raster (" + std::to_string(P.width) + " x " + std::to_string(P.height) + ")");
  const size_t bpp = (size_t)tiffd::pixel_bytes(P.kind), unit = bpp == 3 ? 1 : bpp;
  if (step < (size_t)w * bpp) return bad(kWho, "step smaller than a row");
  if (reinterpret_cast<size_t>(dev_out) % unit || step % unit) return bad(kWho, "dev_out and step must be multiples of the sample's size");
  Ctx* c = &h->impl;
  int rc;
  if ((rc = ctx_use_device(c))) return rc;
  ScopedTimer timer(c, AMHIP_K_MISC);
  return decode_window(kWho, where, c->stream, file, P, x0, y0, w, ht, static_cast<uint8_t*>(dev_out), step);
}

int amhip_geotiff_decode_dev(amhip_ctx* h, const uint8_t* file, size_t len, int x0, int y0, int w, int ht,
                             void* dev_out, size_t step) {
  static const char kWho[] = "amhip_geotiff_decode_dev";
  if (!h || !file || !dev_out) return bad(kWho, "null argument");
  Parsed P;
  if (!parse_or_text(kWho, file, len, &P)) return AMHIP_ERR_ARG;
  return decode_parsed(kWho, "", h, file, P, x0, y0, w, ht, dev_out, step);
}

int amhip_layer_decode_geotiff(amhip_ctx* h, int layer, const uint8_t* file, size_t len) {
  static const char kWho[] = "amhip_layer_decode_geotiff";
  if (!h || !file) return bad(kWho, "null argument");
  Ctx* c = &h->impl;
  TiffLayerJob* job = nullptr;
  int rc = tiff_layer_prepare(c, kWho, layer, file, len, kTiffFirstIfd, &job);
  if (rc) return rc;
  rc = tiff_layer_place(c, job);
  tiff_layer_job_free(job);
  return rc;
}

int amhip_layer_read_geotiff(amhip_ctx* h, int layer, const char* filename) {
  static const char kWho[] = "amhip_layer_read_geotiff";
  if (!h || !filename) return bad(kWho, "null argument");
  std::vector<uint8_t> file;
  int rc = read_file(kWho, filename, &file);
  if (rc) return rc;
  Ctx* c = &h->impl;
  TiffLayerJob* job = nullptr;
  if ((rc = tiff_layer_prepare(c, kWho, layer, file.data(), file.size(), kTiffFirstIfd, &job))) return rc;
  rc = tiff_layer_place(c, job);
  tiff_layer_job_free(job);
  return rc;
}

// ---- levels ------------------------------------------------------------------------

int amhip_geotiff_levels(const uint8_t* file, size_t len, int* n) {
  static const char kWho[] = "amhip_geotiff_levels";
  if (!file || !n) return bad(kWho, "null argument");
  std::vector<tiffd::Ifd> ifds;
  char text[200];
  if (!tiffd::walk_chain(file, len, &ifds, text, sizeof(text))) return bad(kWho, text);
  *n = (int)tiffd::levels_of(ifds).size();
  return AMHIP_OK;
}

int amhip_geotiff_level_info(const uint8_t* file, size_t len, int level, amhip_geotiff_desc* desc) {
  static const char kWho[] = "amhip_geotiff_level_info";
  if (!file || !desc) return bad(kWho, "null argument");
  Parsed P;
  if (!level_or_text(kWho, file, len, level, &P)) return AMHIP_ERR_ARG;
  fill_desc(P, desc);
  return AMHIP_OK;
}

int amhip_geotiff_decode_level_dev(amhip_ctx* h, const uint8_t* file, size_t len, int level, int x0, int y0, int w,
                                   int ht, void* dev_out, size_t step) {
  static const char kWho[] = "amhip_geotiff_decode_level_dev";
  if (!h || !file || !dev_out) return bad(kWho, "null argument");
  Parsed P;
  if (!level_or_text(kWho, file, len, level, &P)) return AMHIP_ERR_ARG;
  return decode_parsed(kWho, "level " + std::to_string(level) + ": ", h, file, P, x0, y0, w, ht, dev_out, step);
}

int amhip_layer_decode_geotiff_level(amhip_ctx* h, int layer, const uint8_t* file, size_t len, int level) {
  static const char kWho[] = "amhip_layer_decode_geotiff_level";
  if (!h || !file) return bad(kWho, "null argument");
  if (level < -1) return bad(kWho, "level: -1 (automatic) or a level of the file, 0 ..");
  Ctx* c = &h->impl;
  TiffLayerJob* job = nullptr;
  int rc = tiff_layer_prepare(c, kWho, layer, file, len, level, &job);
  if (rc) return rc;
  rc = tiff_layer_place(c, job);
  tiff_layer_job_free(job);
  return rc;
}

int amhip_layer_read_geotiff_level(amhip_ctx* h, int layer, const char* filename, int level) {
  static const char kWho[] = "amhip_layer_read_geotiff_level";
  if (!h || !filename) return bad(kWho, "null argument");
  if (level < -1) return bad(kWho, "level: -1 (automatic) or a level of the file, 0 ..");
  std::vector<uint8_t> file;
  int rc = read_file(kWho, filename, &file);
  if (rc) return rc;
  Ctx* c = &h->impl;
  TiffLayerJob* job = nullptr;
  if ((rc = tiff_layer_prepare(c, kWho, layer, file.data(), file.size(), level, &job))) return rc;
  rc = tiff_layer_place(c, job);
  tiff_layer_job_free(job);
  return rc;
}

}  // extern "C"
