// amhip_jpeg_decode.hip -- baseline and progressive JPEG frames, decoded on the GPU: what
// io::AerialMapperIO::loadImagesFromFile (aerial-mapper-io.cc:207-227) gets from cv::imread, one
// file per pose.  The bar is bit identity with libjpeg at its defaults (JDCT_ISLOW, fancy
// upsampling); tests/jpeg_decode_reference.py restates every rule and is pinned to libjpeg's own
// pixels (tests/golden/jpeg_decode/).  The header parser, the per-frame descriptor and the Huffman
// decode tables are host code (amhip_jpeg_decode_host.h).
//
// Three kernels per group of frames, on the default stream; the statuses are read back once:
//   1. k_jpegd_entropy  one wave per frame.  The walk through the scan (Huffman codes, 0xFF 0x00,
//                       RSTn, DC prediction) is sequential and wave-uniform: every value it
//                       branches on is broadcast from the first lane, so it runs on the scalar unit;
//                       the lanes stage 1024 file bytes at a time into LDS (16 per lane, each load
//                       checked against the scan's end), hold the frame's four Huffman tables there,
//                       and flush every finished block as one 128-byte row of int16 coefficients in
//                       natural order (lane k writes the coefficient of zigzag position k).  Blocks are stored plane by
//                       plane, not in scan order.  Parallelism is across the frames of the call.
//      k_jpegd_entropy_prog  the same for a progressive frame (SOF2): one wave walks the frame's scans in
//                       file order into its coefficient blocks (see there).  A call may mix both kinds;
//                       each frame goes to the kernel of its kind, what follows is shared.
//   2. k_jpegd_idct     jpeg_idct_islow, the mirror of k_jpeg_blocks: eight lanes per block, a lane
//                       dequantises and transforms a column, the block goes through LDS, the same
//                       lane transforms a row, adds 128 and clamps.  colored == 0: only Y blocks,
//                       written straight into the cropped output frame.  Otherwise whole-block
//                       component planes.
//   3. k_jpegd_colour   one lane per output pixel: the upsampling rule the frame's sampling selects
//                       (jdsample.c: fullsize, h2v1 fancy, h2v2 fancy, replication when the chroma
//                       plane is at most 2 samples wide) and ycc_rgb_convert -> B, G, R.  A gray
//                       file is replicated.
//
// Bounds: the walk decodes exactly the frame's blocks; a block takes one DC symbol and at most 63 AC
// symbols (every AC symbol moves the coefficient index forward by at least one); a code takes at
// most 16 - 8 steps of the maxcode loop; a refill takes at most 8 bytes.  No byte at or behind the
// scan's end is loaded: they read as 0.  A run of 0xFF fill bytes, in front of a stuffed 0x00 or of
// an RSTn, is followed no further than the scan's end, and so is the search for the RSTn at the end
// of an interval.  An undefined code, a run past coefficient 63, a wrong or missing RSTn and a scan
// that ends early set the frame's status word and end the walk; bytes between the end of an
// interval's data and its RSTn, or between the last block and the EOI, are skipped, as libjpeg
// skips them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "amhip_device.h"
#include "amhip_frame_stack.h"
#include "amhip_jpeg_decode_host.h"

namespace amhip {

namespace {

using jpegd::Frame;
using jpegd::HuffTable;

constexpr int kWindow = 1024;            // file bytes in LDS (16 per lane)
constexpr int kIdctBlocks = 32;          // k_jpegd_idct: 256 lanes, 8 per block

struct Zigzag {
  uint8_t at[64];
};
constexpr Zigzag make_zigzag() {
  Zigzag z = {};
  for (int k = 0; k < 64; ++k) z.at[k] = jpeg::kZigzag[k];
  return z;
}
__constant__ Zigzag d_zigzag = make_zigzag();

// The bit reader of one frame (jpeg_fill_bit_buffer, jdhuff.c).  Everything in here is the same
// in every lane.
struct Reader {
  const uint8_t* files;
  uint8_t* win;        // LDS, kWindow bytes
  uint64_t pos, end;   // next unread byte; the scan's end (EOI)
  uint64_t wbase;      // file offset of win[0]
  uint64_t acc;        // the low `nbits` bits are unread, MSB first
  int nbits;
  int fake;            // of those, zero bits fed behind a marker or the end (always the last ones)
  uint32_t err;

  // (a refill asks for pos and pos + 1 at once; a walk along fill bytes for one byte at a time)
  __device__ __forceinline__ void stage(uint64_t at, int lane) {
    __syncthreads();
    wbase = at;
#pragma unroll
    for (int i = 0; i < kWindow / 64; ++i) {
      const uint64_t q = at + (uint64_t)(lane + 64 * i);
      win[lane + 64 * i] = q < end ? files[q] : (uint8_t)0;   // (never a byte at or behind `end`)
    }
    __syncthreads();
  }

  // the byte at file offset q < end, through the window
  __device__ __forceinline__ uint32_t byte_at(uint64_t q, int lane) {
    if (q < wbase || q >= wbase + kWindow) stage(q, lane);
    return uni(win[q - wbase]);
  }
  // next_marker (jdmarker.c): `at` holds a 0xFF; -> the offset of the first byte behind the run of
  // 0xFF that starts there (at most `end`), and that byte in *code (0xD9 at the end: the EOI).  All
  // but the last 0xFF of the run are fill bytes (T.81 B.1.1.2).
  __device__ __forceinline__ uint64_t behind_ff(uint64_t at, int lane, uint32_t* code) {
    uint64_t k = at + 1;
    uint32_t c = 0xD9u;
    while (k < end) {   // (bounded by the scan's end)
      c = byte_at(k, lane);
      if (c != 0xFFu) break;
      c = 0xD9u;
      ++k;
    }
    *code = c;
    return k;
  }

  // at least 32 unread bits behind this (a code takes at most 16, a value at most 15)
  __device__ __forceinline__ void fill(int lane) {
    while (nbits <= 56) {   // (at most 8 rounds)
      uint32_t b = 0;
      if (pos >= end) {
        fake += 8;
      } else {
        if (pos < wbase || pos + 2 > wbase + kWindow) stage(pos, lane);
        b = uni(win[pos - wbase]);
        if (b == 0xFF) {
          uint32_t b2;
          const uint64_t k = behind_ff(pos, lane, &b2);
          if (b2 == 0) {
            pos = k + 1;   // 0xFF ... 0xFF 0x00 is one data byte 0xFF
          } else {
            b = 0;      // a marker: it stays where it is, zero bits are fed
            fake += 8;
          }
        } else {
          pos += 1;
        }
      }
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(int n) const {
    return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u);
  }
  __device__ __forceinline__ void drop(int n) {
    nbits -= n;
    if (nbits < fake) err = jpegd::kEndsEarly;
  }
  // jpeg_huff_decode: the lookahead table, then the maxcode loop for codes longer than 8 bits
  __device__ __forceinline__ uint32_t symbol(const HuffTable* t) {
    const uint32_t e = uni(t->look[peek(jpegd::kLookahead)]);
    if (e) {
      drop((int)(e >> 8));
      return e & 255u;
    }
    int l = jpegd::kLookahead + 1;
    while (l <= 16 && (int32_t)peek(l) > (int32_t)uni((uint32_t)t->maxcode[l])) ++l;   // (at most 8 rounds)
    if (l > 16) {
      err = jpegd::kBadCode;
      return 0;
    }
    const uint32_t code = peek(l);
    drop(l);
    return uni(t->huffval[(code + (uint32_t)uni((uint32_t)t->valoffset[l])) & 255u]);
  }
  // HUFF_EXTEND: a value below 2^(s-1) is negative
  __device__ __forceinline__ int32_t receive_extend(int s) {
    const int32_t v = (int32_t)peek(s);
    drop(s);
    return v < (1 << (s - 1)) ? v - ((1 << s) - 1) : v;
  }
};

__global__ __launch_bounds__(64) void k_jpegd_entropy(const uint8_t* __restrict__ files,
                                                      const Frame* __restrict__ frames, size_t first_frame,
                                                      int16_t* __restrict__ coef, uint32_t* __restrict__ status) {
  __shared__ HuffTable tbl[4];   // dc 0, dc 1, ac 0, ac 1
  __shared__ uint8_t win[kWindow];
  __shared__ int16_t blk[64];
  const int lane = threadIdx.x;
  const int natural = d_zigzag.at[lane];   // jpeg_natural_order of this lane's zigzag position
  const size_t fi = first_frame + blockIdx.x;
  const Frame* f = frames + fi;
  {
    static_assert(sizeof(HuffTable) % 4 == 0 && offsetof(Frame, dc) % 4 == 0, "tables are copied by words");
    static_assert(offsetof(Frame, ac) == offsetof(Frame, dc) + 2 * sizeof(HuffTable), "dc and ac are adjacent");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(f->dc);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tbl);
    for (int i = lane; i < (int)(4 * sizeof(HuffTable) / 4); i += 64) dst[i] = src[i];
    blk[lane] = 0;
  }
  const int ncomp = (int)uni((uint32_t)f->ncomp);
  const uint32_t mcux = uni((uint32_t)f->mcux), mcuy = uni((uint32_t)f->mcuy);
  const uint32_t restart = uni((uint32_t)f->restart);
  const uint64_t coef_base = f->coef_base;
  Reader r;
  r.files = files;
  r.win = win;
  r.pos = f->scan_begin;
  r.end = f->scan_end;
  r.acc = 0;
  r.nbits = 0;
  r.fake = 0;
  r.err = 0;
  r.stage(r.pos, lane);   // (its barriers cover the tables too)

  uint32_t pred[3] = {0, 0, 0};   // (wraps instead of overflowing on a corrupt file)
  uint32_t todo = restart, next_rst = 0;
  uint32_t mx = 0, my = 0;
  const uint32_t nmcu = mcux * mcuy;
  for (uint32_t mcu = 0; mcu < nmcu && !r.err; ++mcu) {
    if (restart) {
      if (todo == 0) {
        // process_restart: the bits left of the byte are dropped; read_restart_marker: the next
        // marker (next_marker skips what is no 0xFF, and 0xFF 0x00; then any number of 0xFF and the
        // code) must be the expected RSTn; the predictors go back to 0.  p only moves forward and
        // never past the scan's end, where the code reads as EOI.
        r.acc = 0;
        r.nbits = 0;
        r.fake = 0;
        uint64_t p = r.pos, k = r.end;
        uint32_t code = 0xD9u;
        while (p < r.end) {
          if (r.byte_at(p, lane) != 0xFFu) {
            ++p;
            continue;
          }
          k = r.behind_ff(p, lane, &code);
          if (code != 0u) break;
          p = k + 1;
        }
        if (p >= r.end || code != 0xD0u + next_rst) {
          r.err = jpegd::kBadRestart;
          break;
        }
        r.pos = k + 1;
        next_rst = (next_rst + 1) & 7u;
        pred[0] = pred[1] = pred[2] = 0;
        todo = restart;
      }
      --todo;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= ncomp) break;
      const uint32_t ch = uni((uint32_t)f->comp_h[c]), cv = uni((uint32_t)f->comp_v[c]);
      const uint32_t bw = uni((uint32_t)f->comp_bw[c]);
      const HuffTable* dc = &tbl[uni((uint32_t)f->td[c]) & 1u];
      const HuffTable* ac = &tbl[2 + (uni((uint32_t)f->ta[c]) & 1u)];
      const uint32_t nb = ch * cv;   // (1, 2 or 4)
      for (uint32_t k4 = 0; k4 < nb && !r.err; ++k4) {
        const uint32_t bx = k4 % ch, by = k4 / ch;
        r.fill(lane);
        const uint32_t s = r.symbol(dc) & 15u;
        if (s) pred[c] += (uint32_t)r.receive_extend((int)s);
        if (lane == 0) blk[0] = (int16_t)pred[c];
        int k = 1;
        while (k < 64 && !r.err) {   // (every round moves k forward: at most 63)
          r.fill(lane);
          const uint32_t rs = r.symbol(ac);
          const int run = (int)(rs >> 4), size = (int)(rs & 15u);
          if (size == 0) {
            if (run != 15) break;   // EOB
            k += 16;                // ZRL
            continue;
          }
          k += run;
          if (k > 63) {
            r.err = jpegd::kRunPast63;
            break;
          }
          const int32_t v = r.receive_extend(size);
          if (lane == 0) blk[k] = (int16_t)v;   // (zigzag position: the flush puts it in its place)
          ++k;
        }
        // the finished block: one 128-byte row, lane k writes the coefficient of zigzag position k
        const uint64_t b = coef_base + f->comp_base[c] + (uint64_t)(my * cv + by) * bw + (mx * ch + bx);
        __syncthreads();
        coef[b * 64 + natural] = blk[lane];
        blk[lane] = 0;
        __syncthreads();
      }
      if (r.err) break;
    }
    if (++mx == mcux) {
      mx = 0;
      ++my;
    }
  }
  // (what lies between the last block and the EOI is skipped, as next_marker skips it with a
  // warning: the host parser has seen that no other marker is among it)
  if (lane == 0) status[fi] = r.err;
}

// Progressive frames (SOF2; jdphuff.c): one wave per frame walks the frame's scans in file order
// into its coefficient blocks, which the driver has zeroed.  As in k_jpegd_entropy every value the
// walk branches on is the same in all lanes.  A block of an AC scan lives in one register per lane,
// lane k holding the coefficient of zigzag position k (the order the stream speaks in): a
// refinement block is loaded with one 128-byte read and the lanes it has changed store theirs in
// one instruction, a first-scan block needs no read (its band is zero: the host has seen that no
// coefficient is sent first twice) and stores only what it decoded, and a block inside an EOB run
// of a first scan touches no memory at all.  DC scans touch coefficient 0 alone, from lane 0.
// Every coefficient of a block is read and written by one and the same lane in every scan.  The
// scan being walked lies in LDS beside its tables, so that the loops hold only what they change.
//
// What bounds each loop: scans by the frame's scan_count; MCUs by the scan's nx * ny and blocks per
// MCU by ns <= 3 times h * v <= 4, all from the host parser; the table copy by ntab <= 3; Reader's
// loops as in k_jpegd_entropy, with the scan's own end in place of the EOI.  The band loop of an AC
// block refills once per round (57 bits and more) and then either decodes one symbol, which ends
// the block or leads to ++k, or passes at least one coefficient: k <= Se <= 63 bounds it to 63
// symbols and 63 coefficients.  A coefficient is addressed by k alone (a lane number), checked
// against Se before it is used; no index comes from the stream.
__global__ __launch_bounds__(64) void k_jpegd_entropy_prog(const uint8_t* __restrict__ files,
                                                           const Frame* __restrict__ frames,
                                                           const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ script,
                                                           int16_t* coef, uint32_t* __restrict__ status) {
  __shared__ HuffTable tbl[3];   // a DC first scan: one per component of the scan; an AC scan: tbl[0]
  __shared__ uint8_t win[kWindow];
  __shared__ jpegd::Scan cur;    // the scan being walked: its fields are read where they are used
  static_assert(sizeof(jpegd::Scan) % 4 == 0, "the scan is copied by words");
  const int lane = threadIdx.x;
  const int natural = d_zigzag.at[lane];   // jpeg_natural_order of this lane's zigzag position
  // What the block loops seldom need lies in LDS, not in registers: the frame's geometry (block
  // addresses are computed from it in the vector unit), where the script and the frame's status
  // word are, and how far the walk through the script has come (word offsets of its scans).
  __shared__ struct {
    uint64_t coef_base;
    const uint32_t* script;
    uint32_t* status;
    uint32_t comp_base[3], comp_bw[3], comp_h[3], comp_v[3];
    uint32_t next, last;
  } geo;
  constexpr uint32_t kScanWords = (uint32_t)(sizeof(jpegd::Scan) / 4);
  if (lane == 0) {
    const uint32_t fi = list[blockIdx.x];
    const Frame* f = frames + fi;
    geo.coef_base = f->coef_base;
    geo.script = script;
    geo.status = status + fi;
    geo.next = f->scan_first * kScanWords;
    geo.last = (f->scan_first + f->scan_count) * kScanWords;
    for (int c = 0; c < 3; ++c) {
      geo.comp_base[c] = f->comp_base[c];
      geo.comp_bw[c] = (uint32_t)f->comp_bw[c];
      geo.comp_h[c] = (uint32_t)f->comp_h[c];
      geo.comp_v[c] = (uint32_t)f->comp_v[c];
    }
  }
  Reader r;
  r.files = files;
  r.win = win;
  r.err = 0;
  for (;;) {   // (the frame's scans: scan_count rounds)
    __syncthreads();   // (the previous scan and its tables are done with; geo is there)
    const uint32_t at_scan = uni(geo.next);
    if (at_scan >= uni(geo.last) || uni(r.err)) break;
    {
      // (the lanes behind the scan's last word copy that word again)
      const uint32_t w = min((uint32_t)lane, kScanWords - 1u);
      reinterpret_cast<uint32_t*>(&cur)[w] = geo.script[at_scan + w];
    }
    if (lane == 0) geo.next = at_scan + kScanWords;
    __syncthreads();
    const int ns = (int)uni((uint32_t)cur.ns);
    const int ss = (int)uni((uint32_t)cur.ss), se = (int)uni((uint32_t)cur.se);
    const int ah = (int)uni((uint32_t)cur.ah), al = (int)uni((uint32_t)cur.al);
    const int ntab = ss == 0 ? (ah == 0 ? ns : 0) : 1;
    for (int t = 0; t < ntab; ++t) {
      const uint32_t at = uni((uint32_t)(ss == 0 ? cur.dc_tbl[t] : cur.ac_tbl));
      const uint32_t* src = geo.script + at;   // (a table's first word in the script)
      uint32_t* dst = reinterpret_cast<uint32_t*>(tbl + t);
      for (int i = lane; i < (int)(sizeof(HuffTable) / 4); i += 64) dst[i] = src[i];
    }
    r.pos = (uint64_t)uni((uint32_t)cur.begin) | ((uint64_t)uni((uint32_t)(cur.begin >> 32)) << 32);
    r.end = (uint64_t)uni((uint32_t)cur.end) | ((uint64_t)uni((uint32_t)(cur.end >> 32)) << 32);
    r.acc = 0;
    r.nbits = 0;
    r.fake = 0;
    r.stage(r.pos, lane);   // (its barriers cover the tables too)

    uint32_t pred0 = 0, pred1 = 0, pred2 = 0;   // (wrap instead of overflowing on a corrupt file)
    uint32_t eobrun = 0;
    uint32_t todo = uni((uint32_t)cur.restart), next_rst = 0;
    const int32_t p1 = 1 << al, m1 = -(1 << al);
    for (uint32_t my = 0; my < uni((uint32_t)cur.ny) && !uni(r.err); ++my) {
      for (uint32_t mx = 0; mx < uni((uint32_t)cur.nx) && !uni(r.err); ++mx) {
        if (const uint32_t restart = uni((uint32_t)cur.restart)) {
          if (todo == 0) {
            // process_restart / read_restart_marker, the rule of k_jpegd_entropy's MCU loop: the
            // bits left of the byte are dropped, the next marker (what is no 0xFF and 0xFF 0x00
            // pairs skipped; then any number of 0xFF and the code) must be the expected RSTn, whose
            // index starts at 0 in every scan; the predictors and the EOB run go back to 0.  p only
            // moves forward and never past the scan's end, where the code reads as EOI.
            r.acc = 0;
            r.nbits = 0;
            r.fake = 0;
            uint64_t p = r.pos, k = r.end;
            uint32_t code = 0xD9u;
            while (p < r.end) {   // (bounded by the scan's end)
              if (r.byte_at(p, lane) != 0xFFu) {
                ++p;
                continue;
              }
              k = r.behind_ff(p, lane, &code);
              if (code != 0u) break;
              p = k + 1;
            }
            if (p >= r.end || code != 0xD0u + next_rst) {
              r.err = jpegd::kBadRestart;
              break;
            }
            r.pos = k + 1;
            next_rst = (next_rst + 1) & 7u;
            pred0 = pred1 = pred2 = 0;
            eobrun = 0;
            todo = restart;
          }
          --todo;
        }
        if (ss == 0) {
          // ---- DC scans: coefficient 0 of every block of the MCU, from lane 0 ---------------------
#pragma unroll 1
          for (int j = 0; j < ns && !uni(r.err); ++j) {   // (ns <= 3)
            const uint32_t c = uni((uint32_t)cur.comp[j]) & 3u;
            // a scan of one component is not interleaved: one block per MCU (per_scan_setup)
            const uint32_t ch = ns > 1 ? uni(geo.comp_h[c]) : 1u;
            const uint32_t cv = ns > 1 ? uni(geo.comp_v[c]) : 1u;
            const uint32_t nb = ch * cv;   // (1, 2 or 4)
            uint32_t pred = j == 0 ? pred0 : j == 1 ? pred1 : pred2;
            for (uint32_t k4 = 0; k4 < nb && !uni(r.err); ++k4) {
              const uint32_t bx = k4 % ch, by = k4 / ch;
              int16_t* dc = coef + (geo.coef_base + geo.comp_base[c] + (uint64_t)(my * cv + by) * geo.comp_bw[c] + (mx * ch + bx)) * 64;
              r.fill(lane);
              int32_t out;       // (one store for both kinds of DC scan, from lane 0)
              bool put = true;
              if (ah == 0) {
                // decode_mcu_DC_first
                const uint32_t s = r.symbol(&tbl[j]) & 15u;
                if (s) pred += (uint32_t)r.receive_extend((int)s);
                out = (int32_t)(pred << al);
              } else {
                // decode_mcu_DC_refine: one bit
                put = r.peek(1) != 0u;
                r.drop(1);
                out = (int32_t)*dc | p1;
              }
              if (put && lane == 0) *dc = (int16_t)out;
            }
            if (j == 0) pred0 = pred;
            else if (j == 1) pred1 = pred;
            else pred2 = pred;
          }
          continue;
        }
        // ---- AC scans: one component, its real blocks in raster order ------------------------------
        if (ah == 0 && eobrun > 0) {   // decode_mcu_AC_first inside an EOB run: the block stays as it is
          --eobrun;
          continue;
        }
        const uint32_t c = uni((uint32_t)cur.comp[0]) & 3u;
        int16_t* mine = coef + (geo.coef_base + geo.comp_base[c] + (uint64_t)my * geo.comp_bw[c] + mx) * 64 + natural;
        // this lane's coefficient.  A first scan: zero until the scan sends it.
        const int32_t was = ah == 0 ? 0 : (int32_t)*mine;
        int32_t v = was;
        enum { kSymbol, kAdvance, kTail, kDone };
        int phase = eobrun > 0 ? kTail : kSymbol;   // (a refinement block inside an EOB run: corrections only)
        int k = ss, run = 0;
        int32_t fresh = 0;
        while (phase != kDone && !uni(r.err)) {
          r.fill(lane);   // (57 bits and more: a code and its extra bits take at most 31)
          if (phase == kSymbol) {
            if (k > se) break;
            const uint32_t rs = r.symbol(&tbl[0]);
            run = (int)(rs >> 4);
            const int size = (int)(rs & 15u);
            if (size == 0 && run != 15) {
              // EOBn: the run covers this block too
              eobrun = 1u << run;
              if (run) {
                eobrun += r.peek(run);
                r.drop(run);
              }
              phase = kTail;
            } else if (ah == 0) {
              // decode_mcu_AC_first
              if (size) {
                k += run;
                if (k > se) {
                  r.err = jpegd::kRunPastBand;
                  break;
                }
                const int32_t x = r.receive_extend(size);
                if (lane == k) v = (int16_t)((uint32_t)x << al);
                ++k;
              } else {
                k += 16;   // ZRL (past Se: the block ends there)
              }
              continue;
            } else {
              // decode_mcu_AC_refine: a new coefficient of size 1, its sign bit behind the code; or ZRL
              fresh = 0;
              if (size) {
                if (size != 1) {
                  r.err = jpegd::kBadRefinement;
                  break;
                }
                fresh = r.peek(1) ? p1 : m1;
                r.drop(1);
              }
              phase = kAdvance;
            }
          }
          if (phase == kAdvance) {
            // pass `run` zero coefficients, correcting the non-zero ones on the way; stop at the
            // (run + 1)-th zero, or behind Se.  A correction takes one bit; out of bits: refill.
            bool found = false;
            while (k <= se && r.nbits > 0) {
              const int32_t at = __builtin_amdgcn_readlane(v, k);
              if (at != 0) {
                const uint32_t bit = r.peek(1);
                r.drop(1);
                if (bit && (at & p1) == 0 && lane == k) v = (int16_t)(at + (at >= 0 ? p1 : m1));
              } else if (--run < 0) {
                found = true;
                break;
              }
              ++k;
            }
            if (!found && k <= se) continue;
            if (fresh) {
              if (k > se) {
                r.err = jpegd::kRunPastBand;
                break;
              }
              if (lane == k) v = (int16_t)fresh;
            }
            ++k;
            phase = kSymbol;
          } else if (phase == kTail) {
            // the rest of the band inside an EOB run.  A first scan has nothing to correct.
            while (ah != 0 && k <= se && r.nbits > 0) {
              const int32_t at = __builtin_amdgcn_readlane(v, k);
              if (at != 0) {
                const uint32_t bit = r.peek(1);
                r.drop(1);
                if (bit && (at & p1) == 0 && lane == k) v = (int16_t)(at + (at >= 0 ? p1 : m1));
              }
              ++k;
            }
            if (ah == 0 || k > se) {
              --eobrun;
              phase = kDone;
            }
          }
        }
        if (v != was) *mine = (int16_t)v;   // (one store of the lanes the block has changed)
      }
    }
    // (what lies between the scan's last block and its end is skipped: the next scan starts at its
    // own first byte with an empty bit buffer)
  }
  if (lane == 0) *geo.status = r.err;
}

// jpeg_idct_islow's constants (jidctint.c): CONST_BITS = 13, PASS1_BITS = 2
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int64_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373,
                  F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819,
                  F_2_562 = 20995, F_3_072 = 25172;

// one pass of jpeg_idct_islow over d[0..7]; DESCALE by `shift` (rounding half up).  64-bit like the
// C code's JLONG, so that coefficients no real encoder writes cannot overflow.
__device__ __forceinline__ void idct_1d(int64_t d[8], int shift) {
  int64_t z1 = (d[2] + d[6]) * F_0_541;
  const int64_t tmp2 = z1 + d[6] * (-F_1_847);
  const int64_t tmp3 = z1 + d[2] * F_0_765;
  const int64_t tmp0 = (d[0] + d[4]) * ((int64_t)1 << kConstBits);
  const int64_t tmp1 = (d[0] - d[4]) * ((int64_t)1 << kConstBits);
  const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int64_t t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3;
  int64_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int64_t z5 = (z3 + z4) * F_1_175;
  t0 *= F_0_298;
  t1 *= F_2_053;
  t2 *= F_3_072;
  t3 *= F_1_501;
  z1 *= -F_0_899;
  z2 *= -F_2_562;
  z3 *= -F_1_961;
  z4 *= -F_0_390;
  z3 += z5;
  z4 += z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const int64_t half = (int64_t)1 << (shift - 1);
  d[0] = (tmp10 + t3 + half) >> shift;
  d[7] = (tmp10 - t3 + half) >> shift;
  d[1] = (tmp11 + t2 + half) >> shift;
  d[6] = (tmp11 - t2 + half) >> shift;
  d[2] = (tmp12 + t1 + half) >> shift;
  d[5] = (tmp12 - t1 + half) >> shift;
  d[3] = (tmp13 + t0 + half) >> shift;
  d[4] = (tmp13 - t0 + half) >> shift;
}

__global__ __launch_bounds__(256) void k_jpegd_idct(const Frame* __restrict__ frames, size_t first_frame,
                                                    const int16_t* __restrict__ coef,
                                                    uint8_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                    size_t frame_stride, size_t row_step, int colored) {
  __shared__ int32_t tile[kIdctBlocks][64 + 8];   // (+8: rows of neighbouring blocks on other banks)
  const size_t fi = first_frame + blockIdx.y;
  const Frame* f = frames + fi;
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const uint32_t b = blockIdx.x * kIdctBlocks + slot;
  const uint32_t nblocks = colored ? f->comp_base[f->ncomp] : f->comp_base[1];
  const bool live = b < nblocks;
  int c = 0;
  if (live) c = b >= f->comp_base[2] && f->ncomp == 3 ? 2 : (b >= f->comp_base[1] ? 1 : 0);
  int64_t d[8];
  if (live) {
    // columns: lane j holds column j, dequantised
    const int16_t* src = coef + (f->coef_base + b) * 64;
    const uint16_t* q = f->quant[c];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = (int64_t)((int32_t)src[r * 8 + j] * (int32_t)q[r * 8 + j]);
    idct_1d(d, kConstBits - kPass1Bits);
#pragma unroll
    for (int r = 0; r < 8; ++r) tile[slot][r * 8 + j] = (int32_t)d[r];
  }
  __syncthreads();
  if (!live) return;
  // rows: lane j holds row j
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = tile[slot][j * 8 + i];
  idct_1d(d, kConstBits + kPass1Bits + 3);
  uint8_t px[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t v = d[i] + 128;
    px[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
  }
  const uint32_t local = b - f->comp_base[c];
  const uint32_t bw = (uint32_t)f->comp_bw[c];
  const uint32_t by = local / bw, bx = local % bw;
  if (!colored) {
    const uint32_t y = by * 8 + j;
    if (y >= (uint32_t)f->height) return;
    uint8_t* dst = out + fi * frame_stride + (size_t)y * row_step;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t x = bx * 8 + i;
      if (x < (uint32_t)f->width) dst[x] = px[i];
    }
  } else {
    // whole blocks: the plane is bw * 8 wide and comp_bh * 8 high
    uint8_t* dst = planes + f->plane_base + (size_t)f->comp_base[c] * 64 +
                   ((size_t)by * 8 + j) * ((size_t)bw * 8) + (size_t)bx * 8;
    uint2 w;
    w.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    w.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    *reinterpret_cast<uint2*>(dst) = w;
  }
}

// one chroma sample at output pixel (x, y) (jdsample.c).  p: the component's plane, pw bytes per
// row; dw x dh: its real samples (the rest of the plane is block padding).
__device__ __forceinline__ int upsampled(const uint8_t* p, size_t pw, int dw, int dh, int hmax, int vmax,
                                         int x, int y) {
  if (hmax == 1) return p[(size_t)y * pw + x];   // fullsize_upsample
  const int k = x >> 1;
  if (dw <= 2) return p[(size_t)(vmax == 2 ? y >> 1 : y) * pw + k];   // h2v1_upsample / h2v2_upsample
  if (vmax == 1) {
    // h2v1_fancy_upsample
    const uint8_t* row = p + (size_t)y * pw;
    const int a = row[k];
    if (x & 1) return k == dw - 1 ? a : (3 * a + row[k + 1] + 2) >> 2;
    return k == 0 ? a : (3 * a + row[k - 1] + 1) >> 2;
  }
  // h2v2_fancy_upsample: the nearer row 3 : 1 the other; the first and the last real row are their
  // own neighbours
  const int r = y >> 1;
  int nb = (y & 1) ? r + 1 : r - 1;
  nb = nb < 0 ? 0 : nb > dh - 1 ? dh - 1 : nb;
  const uint8_t* r0 = p + (size_t)r * pw;
  const uint8_t* r1 = p + (size_t)nb * pw;
  const int cs = 3 * r0[k] + r1[k];
  if (x & 1) return k == dw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * r0[k + 1] + r1[k + 1] + 7) >> 4;
  return k == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * r0[k - 1] + r1[k - 1] + 8) >> 4;
}

__device__ __forceinline__ uint8_t clamp8(int v) {
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void k_jpegd_colour(const Frame* __restrict__ frames, size_t first_frame,
                                                      const uint8_t* __restrict__ planes,
                                                      uint8_t* __restrict__ out, size_t frame_stride,
                                                      size_t row_step) {
  const size_t fi = first_frame + blockIdx.z;
  const Frame* f = frames + fi;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= f->width || y >= f->height) return;
  const uint8_t* base = planes + f->plane_base;
  const size_t pw0 = (size_t)f->comp_bw[0] * 8;
  const int Y = base[(size_t)y * pw0 + x];
  uint8_t* dst = out + fi * frame_stride + (size_t)y * row_step + 3 * (size_t)x;
  if (f->ncomp == 1) {
    dst[0] = dst[1] = dst[2] = (uint8_t)Y;
    return;
  }
  const int hmax = f->hmax, vmax = f->vmax;
  const int dw = (f->width + hmax - 1) / hmax, dh = (f->height + vmax - 1) / vmax;
  const size_t pw1 = (size_t)f->comp_bw[1] * 8;
  const int cb = upsampled(base + (size_t)f->comp_base[1] * 64, pw1, dw, dh, hmax, vmax, x, y) - 128;
  const int cr = upsampled(base + (size_t)f->comp_base[2] * 64, pw1, dw, dh, hmax, vmax, x, y) - 128;
  // ycc_rgb_convert (jdcolor.c): FIX(1.40200), FIX(1.77200), FIX(0.34414), FIX(0.71414); >> is arithmetic
  const int R = Y + ((91881 * cr + 32768) >> 16);
  const int B = Y + ((116130 * cb + 32768) >> 16);
  const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  dst[0] = clamp8(B);
  dst[1] = clamp8(G);
  dst[2] = clamp8(R);
}

// The codec description of decode_frame_stack (amhip_frame_stack.h): files are uploaded as they are,
// one behind the other; a frame costs its coefficients, 128 bytes per block.
struct JpegStack {
  using Frame = jpegd::Frame;
  static constexpr const char* kDecode = "amhip_io_decode_jpeg_frames";
  static constexpr const char* kInfo = "amhip_jpeg_info";
  // MB of coefficients per group of frames.  Groups run one after another and each takes as long as
  // its longest scan, so the default holds the demo flags' 249 frames of 1920 x 1080 in one group
  // (1.0 GB gray, 1.5 GB 4:2:0, planes half as much again).
  static constexpr const char* kBudgetKey = "jpegd_coef_budget_mb";
  static constexpr double kBudgetMB = 4096.0;
  static constexpr size_t kGroupFrames = 32768;   // (grid.y / grid.z of the per-frame launches)

  static bool info(const uint8_t* file, size_t len, int* width, int* height, int* channels, char* err,
                   size_t errcap) {
    Frame f;
    if (!jpegd::parse(file, len, &f, err, errcap)) return false;
    *width = f.width;
    *height = f.height;
    *channels = f.ncomp;
    return true;
  }
  static const char* status_text(uint32_t s) { return jpegd::status_text(s); }

  size_t total = 0;      // bytes of the files so far
  size_t max_idct = 0;   // most blocks k_jpegd_idct transforms in one frame
  DevBuf bytes, coef, planes;
  // progressive frames (SOF2): their scans and tables, one list each for the call, and per frame of
  // the call where its coefficients lie in the group's scratch
  struct Placed {
    size_t at, bytes;
    bool progressive;
  };
  std::vector<jpegd::Scan> scans;
  std::vector<HuffTable> tables;
  std::vector<uint32_t> prog_list;   // the progressive frames' indices, increasing
  std::vector<Placed> placed;
  size_t parsed = 0;
  DevBuf dscript, dlist;   // the script: every scan of the call, then every table

  bool parse(const uint8_t* file, size_t len, Frame* f, char* err, size_t errcap) {
    jpegd::Progressive prog;
    if (!jpegd::parse(file, len, f, &prog, err, errcap)) return false;
    f->scan_begin += total;
    f->scan_end += total;
    if (f->progressive) {
      f->scan_first = (uint32_t)scans.size();
      for (jpegd::Scan s : prog.scans) {
        s.begin += total;
        s.end += total;
        for (int k = 0; k < 3; ++k)
          if (s.dc_tbl[k] >= 0) s.dc_tbl[k] += (int32_t)tables.size();
        if (s.ac_tbl >= 0) s.ac_tbl += (int32_t)tables.size();
        scans.push_back(s);
      }
      tables.insert(tables.end(), prog.tables.begin(), prog.tables.end());
      prog_list.push_back((uint32_t)parsed);
    }
    ++parsed;
    total += len;
    return true;
  }
  size_t cost_bytes(const Frame& f) const { return (size_t)f.comp_base[f.ncomp] * 128; }
  void place(Frame* f, size_t base_bytes, int colored) {
    f->coef_base = base_bytes / 128;
    f->plane_base = f->coef_base * 64;
    max_idct = std::max(max_idct, (size_t)(colored ? f->comp_base[f->ncomp] : f->comp_base[1]));
    placed.push_back({base_bytes, cost_bytes(*f), f->progressive != 0});
  }
  int upload(const uint8_t* const* files, const size_t* lens, size_t F, size_t max_group_bytes, int colored,
             hipStream_t stream) {
    int rc;
    if ((rc = bytes.alloc(total))) return rc;
    if ((rc = coef.alloc(max_group_bytes))) return rc;
    if (colored && (rc = planes.alloc(max_group_bytes / 2))) return rc;
    size_t at = 0;
    for (size_t i = 0; i < F; ++i) {
      AMHIP_TRY(hipMemcpyAsync(bytes.as<uint8_t>() + at, files[i], lens[i], hipMemcpyHostToDevice, stream));
      at += lens[i];
    }
    if (!prog_list.empty()) {
      // the scans' table numbers become word offsets into the script
      const size_t scan_bytes = scans.size() * sizeof(jpegd::Scan), table_bytes = tables.size() * sizeof(HuffTable);
      if ((scan_bytes + table_bytes) / 4 > 0x7FFFFFFFu) {
        set_last_error(std::string(kDecode) + ": the progressive frames' scans and tables exceed 8 GB");
        return AMHIP_ERR_ARG;
      }
      for (jpegd::Scan& s : scans) {
        for (int k = 0; k < 3; ++k)
          if (s.dc_tbl[k] >= 0) s.dc_tbl[k] = (int32_t)((scan_bytes + (size_t)s.dc_tbl[k] * sizeof(HuffTable)) / 4);
        if (s.ac_tbl >= 0) s.ac_tbl = (int32_t)((scan_bytes + (size_t)s.ac_tbl * sizeof(HuffTable)) / 4);
      }
      if ((rc = dscript.alloc(scan_bytes + table_bytes))) return rc;
      if ((rc = dlist.alloc(prog_list.size() * sizeof(uint32_t)))) return rc;
      AMHIP_TRY(hipMemcpyAsync(dscript.p, scans.data(), scan_bytes, hipMemcpyHostToDevice, stream));
      if (table_bytes)
        AMHIP_TRY(hipMemcpyAsync(dscript.as<uint8_t>() + scan_bytes, tables.data(), table_bytes,
                                 hipMemcpyHostToDevice, stream));
      AMHIP_TRY(hipMemcpyAsync(dlist.p, prog_list.data(), prog_list.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, stream));
    }
    return AMHIP_OK;
  }
  // Each frame goes to the entropy kernel of its kind: the baseline frames of the group run by run of
  // consecutive frames (a call without progressive frames: one launch, as ever), the progressive ones
  // in one launch over their index list, their coefficients zeroed first.
  void launch_entropy(size_t first, size_t n, const StackLaunch<Frame>& s) {
    const size_t last = first + n;
    for (size_t i = first; i < last;) {
      size_t j = i;
      while (j < last && placed[j].progressive == placed[i].progressive) ++j;
      if (placed[i].progressive)
        (void)hipMemsetAsync(coef.as<uint8_t>() + placed[i].at, 0,
                             placed[j - 1].at + placed[j - 1].bytes - placed[i].at, s.stream);
      else
        hipLaunchKernelGGL(k_jpegd_entropy, dim3((unsigned)(j - i)), dim3(64), 0, s.stream, bytes.as<uint8_t>(),
                           s.frames, i, coef.as<int16_t>(), s.status);
      i = j;
    }
    const size_t lo = std::lower_bound(prog_list.begin(), prog_list.end(), (uint32_t)first) - prog_list.begin();
    const size_t hi = std::lower_bound(prog_list.begin(), prog_list.end(), (uint32_t)last) - prog_list.begin();
    if (hi > lo)
      hipLaunchKernelGGL(k_jpegd_entropy_prog, dim3((unsigned)(hi - lo)), dim3(64), 0, s.stream, bytes.as<uint8_t>(),
                         s.frames, dlist.as<uint32_t>() + lo, dscript.as<uint32_t>(), coef.as<int16_t>(), s.status);
  }
  void launch_group(size_t first, size_t n, const StackLaunch<Frame>& s) {
    launch_entropy(first, n, s);
    hipLaunchKernelGGL(k_jpegd_idct, dim3((unsigned)((max_idct + kIdctBlocks - 1) / kIdctBlocks), (unsigned)n),
                       dim3(256), 0, s.stream, s.frames, first, coef.as<int16_t>(), planes.as<uint8_t>(), s.out,
                       s.frame_stride, s.row_step, s.colored);
    if (s.colored)
      hipLaunchKernelGGL(k_jpegd_colour, dim3((unsigned)((s.width + 255) / 256), (unsigned)s.height, (unsigned)n),
                         dim3(256), 0, s.stream, s.frames, first, planes.as<uint8_t>(), s.out, s.frame_stride,
                         s.row_step);
  }
};

}  // namespace

}  // namespace amhip

extern "C" {

int amhip_jpeg_info(const uint8_t* file, size_t len, int* width, int* height, int* channels) {
  return amhip::image_info<amhip::JpegStack>(file, len, width, height, channels);
}

int amhip_io_decode_jpeg_frames(int device, const uint8_t* const* files, const size_t* lens, size_t F, int colored,
                                uint8_t** dev_frames, int* width, int* height, size_t* row_step,
                                size_t* frame_stride) {
  return amhip::decode_frame_stack<amhip::JpegStack>(device, files, lens, F, colored, dev_frames, width, height,
                                                     row_step, frame_stride);
}

int amhip_io_download_frames(const uint8_t* dev_frames, size_t num_bytes, uint8_t* host_frames) {
  if (num_bytes == 0) return AMHIP_OK;
  if (!dev_frames || !host_frames) {
    amhip::set_last_error("amhip_io_download_frames: null argument");
    return AMHIP_ERR_ARG;
  }
  AMHIP_TRY(hipMemcpy(host_frames, dev_frames, num_bytes, hipMemcpyDeviceToHost));
  return AMHIP_OK;
}

}  // extern "C"
