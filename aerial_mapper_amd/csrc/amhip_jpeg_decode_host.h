// amhip_jpeg_decode_host.h -- the host-only part of the JPEG decoder (amhip_jpeg_decode.hip): the
// header parser (jdmarker.c: read_markers, get_sof, get_sos, get_dht, get_dqt, get_dri), the
// per-frame descriptor the kernels read, and the Huffman decode tables in libjpeg's shape
// (jpeg_make_d_derived_tbl, jdhuff.c).  No HIP in here: tests/cpp/jpeg_decode_host_main.cc compiles
// it alone under the address and undefined-behaviour sanitizers.
//
// Accepted: baseline sequential DCT (SOF0), 8 bit, Huffman, one scan; one component, or Y Cb Cr
// with Y sampled 1x1, 2x1 or 2x2 and chroma 1x1; 8-bit quantisation tables; Huffman table ids 0
// and 1; optional DRI; APPn / COM skipped; 0xFF fill bytes in front of any marker, in the header
// and in the scan (where a run of 0xFF followed by 0x00 is one data byte 0xFF); any bytes between
// the last block and EOI; bytes behind EOI ignored.  Also accepted: progressive DCT (SOF2), 8 bit,
// Huffman, the same components, Huffman table ids 0..3: the whole marker sequence up to EOI becomes
// a scan list (Progressive), DHT / DQT / DRI / COM / APPn may stand between scans, a component's
// quantisation table is the one in effect at its first scan.  Its script is held to libjpeg's rules
// (start_pass_phuff_decoder) and must bring every coefficient to bit 0.  Everything else is refused
// with a text that names the marker or field, under SOF2 the scan as well.  Every read is checked
// against the file's length.
#ifndef AMHIP_JPEG_DECODE_HOST_H_
#define AMHIP_JPEG_DECODE_HOST_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "amhip_jpeg_host.h"

namespace amhip {
namespace jpegd {

constexpr int kLookahead = 8;  // HUFF_LOOKAHEAD (jdhuff.h)

// d_derived_tbl: look[peek of 8 bits] = length << 8 | symbol for codes of at most 8 bits, 0 for
// longer ones; maxcode[l] = the largest code of length l (-1: none), maxcode[17] a sentinel;
// valoffset[l] = huffval index of the first code of length l minus that code.  908 bytes.
struct HuffTable {
  uint16_t look[256];
  int32_t maxcode[18];
  int32_t valoffset[17];
  uint8_t huffval[256];
};

// what the kernels need of one file.  Offsets are into the buffer that holds the call's files.
struct Frame {
  int32_t width, height;
  int32_t ncomp;            // 1 or 3
  int32_t hmax, vmax;       // Y's sampling factors as the scan codes them (1 x 1 for one component)
  int32_t mcux, mcuy;       // MCUs across and down
  int32_t restart;          // MCUs per restart interval, 0: none
  uint64_t scan_begin;      // first entropy-coded byte
  uint64_t scan_end;        // the EOI marker: no byte at or behind it is read
  int32_t comp_h[3], comp_v[3];    // blocks per MCU
  int32_t comp_bw[3], comp_bh[3];  // the component's plane in blocks (whole MCUs)
  uint32_t comp_base[4];    // first block of each plane in the frame's block list; [ncomp] = total
  int32_t td[3], ta[3];     // Huffman tables of each component
  uint64_t coef_base;       // the frame's first block in the coefficient scratch
  uint64_t plane_base;      // the frame's first byte in the plane scratch
  uint16_t quant[3][64];    // per component, natural order
  HuffTable dc[2], ac[2];   // SOF0: the tables of the one scan
  int32_t progressive;      // SOF2: the walk follows the scan list, td / ta / dc / ac / restart unused
  uint32_t scan_first, scan_count;   // ... its scans in the call's list
};

// jpeg_make_d_derived_tbl; false when the counts do not describe a prefix code
inline bool make_table(const uint8_t bits[16], const uint8_t* vals, int nvals, HuffTable* t) {
  std::memset(t, 0, sizeof(*t));
  for (int l = 0; l < 18; ++l) t->maxcode[l] = -1;
  for (int i = 0; i < nvals; ++i) t->huffval[i] = vals[i];
  int32_t code = 0;
  int p = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    if (n) {
      if (code + n > (1 << l)) return false;
      t->valoffset[l] = p - code;
      if (l <= kLookahead)
        for (int i = 0; i < n; ++i) {
          const int lo = (code + i) << (kLookahead - l);
          for (int k = 0; k < (1 << (kLookahead - l)); ++k)
            t->look[lo + k] = (uint16_t)((l << 8) | vals[p + i]);
        }
      p += n;
      code += n;
      t->maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0xFFFFF;
  return true;
}

inline const char* sof_name(int m) {
  switch (m) {
    case 0xC1: return "SOF1 (extended sequential)";
    case 0xC2: return "SOF2 (progressive)";
    case 0xC3: return "SOF3 (lossless)";
    case 0xC5: return "SOF5";
    case 0xC6: return "SOF6";
    case 0xC7: return "SOF7";
    case 0xC8: return "JPG";
    case 0xC9: return "SOF9 (arithmetic)";
    case 0xCA: return "SOF10 (arithmetic)";
    case 0xCB: return "SOF11 (arithmetic)";
    case 0xCC: return "DAC (arithmetic)";
    case 0xCD: return "SOF13";
    case 0xCE: return "SOF14";
    case 0xCF: return "SOF15";
  }
  return nullptr;
}

// per_scan_setup (jdinput.c): MCU counts, the planes' sizes and the block list.  A scan of one
// component is not interleaved: one block per MCU, 8 x 8 MCUs, whatever SOF0 declares.
inline void layout(Frame* f, const int h[3], const int v[3]) {
  if (f->ncomp == 1) {
    f->hmax = f->vmax = 1;
    f->comp_h[0] = f->comp_v[0] = 1;
  } else {
    f->hmax = h[0];
    f->vmax = v[0];
    for (int c = 0; c < 3; ++c) {
      f->comp_h[c] = h[c];
      f->comp_v[c] = v[c];
    }
  }
  f->mcux = (f->width + 8 * f->hmax - 1) / (8 * f->hmax);
  f->mcuy = (f->height + 8 * f->vmax - 1) / (8 * f->vmax);
  uint32_t base = 0;
  for (int c = 0; c < f->ncomp; ++c) {
    f->comp_bw[c] = f->mcux * f->comp_h[c];
    f->comp_bh[c] = f->mcuy * f->comp_v[c];
    f->comp_base[c] = base;
    base += (uint32_t)f->comp_bw[c] * (uint32_t)f->comp_bh[c];   // (<= 1.5 * 8192^2: fits)
  }
  for (int c = f->ncomp; c < 4; ++c) f->comp_base[c] = base;
}

// One scan of a progressive file (SOF2), as the entropy kernel walks it.  Offsets are into the buffer
// that holds the call's files, table indices into the list of the file's tables (the driver turns
// them into word offsets into the script it uploads: every scan of the call, then every table).
struct Scan {
  uint64_t begin;        // first entropy-coded byte
  uint64_t end;          // the 0xFF of the marker that ends the segment: no byte at or behind it is read
  int32_t ns;            // components in the scan (1: not interleaved)
  int32_t comp[3];       // their indices in the frame, increasing
  int32_t ss, se, ah, al;
  int32_t restart;       // the scan's MCUs per restart interval as DRI stood at this SOS, 0: none
  int32_t dc_tbl[3];     // per component of the scan; -1: the scan decodes no DC symbol
  int32_t ac_tbl;        // -1: a DC scan
  int32_t nx, ny;        // the scan's MCUs across and down: whole MCUs when interleaved, else the
                         // component's real blocks (per_scan_setup, jdinput.c)
};

// what a progressive file adds to its Frame: the scans in file order and every table they use, once
struct Progressive {
  std::vector<Scan> scans;
  std::vector<HuffTable> tables;
};

// The whole marker sequence.  SOF0: up to the first entropy-coded byte, and the EOI at the file's
// end.  SOF2: every scan up to EOI into *prog, the script checked as start_pass_phuff_decoder
// (jdphuff.c) checks it, and stricter: what libjpeg only warns about is refused, and so is a file
// whose scans leave any coefficient short of bit 0.  Returns true and fills *f (scan_begin /
// scan_end relative to `file`, of a progressive file those of its last scan; coef_base / plane_base
// left 0), or false with a text in err.
inline bool parse(const uint8_t* file, size_t len, Frame* f, Progressive* prog, char* err, size_t errcap) {
  auto fail = [&](const char* fmt, int a, int b) {
    if (err && errcap) std::snprintf(err, errcap, fmt, a, b);
    return false;
  };
  std::memset(f, 0, sizeof(*f));
  prog->scans.clear();
  prog->tables.clear();
  if (!file || len < 4 || file[0] != 0xFF || file[1] != 0xD8) return fail("no SOI", 0, 0);
  bool have_q[4] = {false, false, false, false};
  bool have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
  std::vector<HuffTable> cur(8);   // [class * 4 + id], as the DHTs so far define them
  int pooled[2][4];                // ... and where prog->tables holds that definition, -1: not yet
  bool high_id = false;            // a DHT with id 2 or 3 was seen: legal under SOF2 only
  uint16_t q[4][64];
  int id[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, h[3] = {1, 1, 1}, v[3] = {1, 1, 1};
  bool have_sof = false, progressive = false;
  bool latched[3] = {false, false, false};   // latch_quant_tables (jdinput.c)
  int bits[3][64];                           // coef_bits: the Al each coefficient has reached, -1: not sent
  int restart = 0;
  int adobe_transform = -1;
  for (int c = 0; c < 2; ++c)
    for (int t = 0; t < 4; ++t) pooled[c][t] = -1;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) bits[c][k] = -1;
  size_t p = 2;
  for (;;) {
    const bool between = !prog->scans.empty();   // behind a progressive file's first scan
    if (between) {
      if (p + 2 > len) return fail("no EOI", 0, 0);
    } else if (p + 4 > len) {
      return fail("no SOS", 0, 0);
    }
    if (file[p] != 0xFF) return fail("marker expected at byte %d", (int)p, 0);
    const int m = file[p + 1];
    if (m == 0xFF) {   // fill byte
      ++p;
      continue;
    }
    if (m == 0xD9) {
      if (between) break;
      return fail("no SOS", 0, 0);
    }
    if (p + 4 > len) return fail("no EOI", 0, 0);
    const size_t L = ((size_t)file[p + 2] << 8) | file[p + 3];
    if (L < 2 || p + 2 + L > len) return fail("segment %02X runs past the file", m, 0);
    const uint8_t* pl = file + p + 4;
    const size_t n = L - 2;
    if (between && !(m == 0xC4 || m == 0xDB || m == 0xDD || m == 0xDA || m == 0xFE || (m >= 0xE0 && m <= 0xEF)))
      return fail("SOF2 (progressive): marker %02X between scans", m, 0);
    if (m == 0xC0 || m == 0xC2) {
      // (the texts of both frame types name SOF0 where the rule is SOF0's: one set of words)
      if (have_sof) return fail(m == 0xC0 ? "second SOF0" : "second SOF2 (progressive)", 0, 0);
      if (n < 6 || n != 6 + 3 * (size_t)pl[5]) return fail("SOF0: bad length", 0, 0);
      if (pl[0] != 8) return fail("SOF0: %d-bit samples", pl[0], 0);
      f->height = (pl[1] << 8) | pl[2];
      f->width = (pl[3] << 8) | pl[4];
      if (f->height < 1 || f->width < 1) return fail("SOF0: zero width or height", 0, 0);
      if (pl[5] != 1 && pl[5] != 3) return fail("SOF0: %d components", pl[5], 0);
      f->ncomp = pl[5];
      for (int c = 0; c < f->ncomp; ++c) {
        id[c] = pl[6 + 3 * c];
        h[c] = pl[7 + 3 * c] >> 4;
        v[c] = pl[7 + 3 * c] & 15;
        tq[c] = pl[8 + 3 * c];
        if (h[c] < 1 || h[c] > 4 || v[c] < 1 || v[c] > 4 || tq[c] > 3)
          return fail("SOF0: bad sampling factors or table id", 0, 0);
      }
      if (f->ncomp == 3) {
        const bool y_ok = (h[0] == 1 && v[0] == 1) || (h[0] == 2 && v[0] == 1) || (h[0] == 2 && v[0] == 2);
        if (!y_ok || h[1] != 1 || v[1] != 1 || h[2] != 1 || v[2] != 1)
          return fail("SOF0: sampling factors other than 4:4:4, 4:2:2, 4:2:0", 0, 0);
        if (id[0] == 'R' && id[1] == 'G' && id[2] == 'B') return fail("SOF0: component ids R G B", 0, 0);
        if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) {
          if (m == 0xC2) return fail("SOF2 (progressive): a component id twice", 0, 0);
        }
      }
      have_sof = true;
      progressive = m == 0xC2;
      f->progressive = progressive ? 1 : 0;
      if (!progressive && high_id) return fail("DHT: bad table class, id or length", 0, 0);
      if (progressive) layout(f, h, v);
    } else if (sof_name(m)) {
      if (err && errcap) std::snprintf(err, errcap, "marker %s", sof_name(m));
      return false;
    } else if (m == 0xDB) {
      size_t at = 0;
      while (at < n) {
        if (pl[at] >> 4) return fail("DQT: 16-bit table", 0, 0);
        const int t = pl[at] & 15;
        if (t > 3 || at + 65 > n) return fail("DQT: bad table id or length", 0, 0);
        for (int z = 0; z < 64; ++z) q[t][jpeg::kZigzag[z]] = pl[at + 1 + z];
        have_q[t] = true;
        at += 65;
      }
    } else if (m == 0xC4) {
      size_t at = 0;
      while (at < n) {
        // ids 2 and 3: SOF2 only (T.81 B.2.4.2).  A DHT may precede SOF: then SOF0 refuses them.
        const int top = have_sof && !progressive ? 1 : 3;
        if (at + 17 > n || (pl[at] >> 4) > 1 || (pl[at] & 15) > top)
          return fail("DHT: bad table class, id or length", 0, 0);
        const int cls = pl[at] >> 4, th = pl[at] & 15;
        if (th > 1) high_id = true;
        int nv = 0;
        for (int i = 0; i < 16; ++i) nv += pl[at + 1 + i];
        if (nv > 256 || at + 17 + (size_t)nv > n) return fail("DHT: bad symbol count", 0, 0);
        if (cls == 0)
          for (int i = 0; i < nv; ++i)
            if (pl[at + 17 + i] > 15) return fail("DHT: DC symbol above 15", 0, 0);
        if (!make_table(pl + at + 1, pl + at + 17, nv, &cur[cls * 4 + th]))
          return fail("DHT: codes do not fit", 0, 0);
        have_h[cls][th] = true;
        pooled[cls][th] = -1;
        at += 17 + (size_t)nv;
      }
    } else if (m == 0xDD) {
      if (n != 2) return fail("DRI: bad length", 0, 0);
      restart = (pl[0] << 8) | pl[1];
    } else if (m == 0xEE && n >= 12 && std::memcmp(pl, "Adobe", 5) == 0) {
      adobe_transform = pl[11];
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
      // APPn, COM: skipped
    } else if (m == 0xDA && !progressive) {
      if (!have_sof) return fail("SOS before SOF0", 0, 0);
      if (n < 1 || n != 4 + 2 * (size_t)pl[0]) return fail("SOS: bad length", 0, 0);
      if (pl[0] != f->ncomp) return fail("SOS: several scans (%d of %d components)", pl[0], f->ncomp);
      for (int c = 0; c < f->ncomp; ++c) {
        if (pl[1 + 2 * c] != id[c]) return fail("SOS: component order", 0, 0);
        f->td[c] = pl[2 + 2 * c] >> 4;
        f->ta[c] = pl[2 + 2 * c] & 15;
        if (f->td[c] > 1 || f->ta[c] > 1) return fail("SOS: Huffman table id above 1", 0, 0);
        if (!have_h[0][f->td[c]] || !have_h[1][f->ta[c]]) return fail("SOS: missing Huffman table", 0, 0);
        if (!have_q[tq[c]]) return fail("SOS: missing quantisation table", 0, 0);
        std::memcpy(f->quant[c], q[tq[c]], sizeof(q[0]));
      }
      if (pl[n - 3] != 0 || pl[n - 2] != 63 || pl[n - 1] != 0)
        return fail("SOS: not a sequential scan (Ss, Se, Ah/Al)", 0, 0);
      if (adobe_transform == 0 && f->ncomp == 3) return fail("Adobe transform 0 (RGB)", 0, 0);
      f->restart = restart;
      for (int t = 0; t < 2; ++t) {
        f->dc[t] = cur[t];
        f->ac[t] = cur[4 + t];
      }
      f->scan_begin = p + 2 + L;
      break;
    } else if (m == 0xDA) {
      // get_sos (jdmarker.c) and start_pass_phuff_decoder (jdphuff.c); every text names the scan
      const int si = (int)prog->scans.size();
      if (n < 1 || n != 4 + 2 * (size_t)pl[0]) return fail("SOF2 (progressive): scan %d: bad SOS length", si, 0);
      Scan s;
      std::memset(&s, 0, sizeof(s));
      s.ns = pl[0];
      if (s.ns < 1 || s.ns > f->ncomp)
        return fail("SOF2 (progressive): scan %d: Ns = %d, more components than the frame defines", si, s.ns);
      s.ss = pl[n - 3];
      s.se = pl[n - 2];
      s.ah = pl[n - 1] >> 4;
      s.al = pl[n - 1] & 15;
      // (a sequential scan under SOF2, which libjpeg refuses too, keeps the words this file shape
      // has always been refused with: the baseline restatement's)
      if (s.ss == 0 && s.se == 63 && pl[n - 1] == 0) return fail("marker SOF2 (progressive)", 0, 0);
      if (s.ss == 0 && s.se != 0) return fail("SOF2 (progressive): scan %d: Ss = 0 with Se = %d", si, s.se);
      if (s.ss > 0 && s.ns != 1) return fail("SOF2 (progressive): scan %d: Ss > 0 with Ns = %d", si, s.ns);
      if (s.se < s.ss || s.se > 63) return fail("SOF2 (progressive): scan %d: Se = %d below Ss or above 63", si, s.se);
      if (s.al > 13) return fail("SOF2 (progressive): scan %d: Al = %d above 13", si, s.al);
      if (s.ah != 0 && s.al != s.ah - 1)
        return fail("SOF2 (progressive): scan %d: Ah = %d with Al other than Ah - 1", si, s.ah);
      for (int k = 0; k < 3; ++k) s.dc_tbl[k] = -1;
      s.ac_tbl = -1;
      for (int k = 0; k < s.ns; ++k) {
        int c = 0;
        while (c < f->ncomp && id[c] != pl[1 + 2 * k]) ++c;
        if (c == f->ncomp)
          return fail("SOF2 (progressive): scan %d: component id %d the frame does not define", si, pl[1 + 2 * k]);
        if (k && c <= s.comp[k - 1]) return fail("SOF2 (progressive): scan %d: component order", si, 0);
        s.comp[k] = c;
        if (!latched[c]) {
          if (!have_q[tq[c]]) return fail("SOS: missing quantisation table", 0, 0);
          std::memcpy(f->quant[c], q[tq[c]], sizeof(q[0]));
          latched[c] = true;
        }
        if (s.ss > 0 && bits[c][0] < 0)
          return fail("SOF2 (progressive): scan %d: AC scan of component %d before its DC scan", si, c);
        for (int z = s.ss; z <= s.se; ++z) {
          if (s.ah == 0 && bits[c][z] >= 0)
            return fail("SOF2 (progressive): scan %d: coefficient %d sent first twice (Ah = 0)", si, z);
          if (s.ah != 0 && bits[c][z] < 0)
            return fail("SOF2 (progressive): scan %d: coefficient %d refined before its first scan (Ah)", si, z);
          if (s.ah != 0 && bits[c][z] != s.ah)
            return fail("SOF2 (progressive): scan %d: Ah = %d is not the coefficient's current Al", si, s.ah);
          bits[c][z] = s.al;
        }
        // the tables the scan uses, as they stand: a DC refinement scan decodes no symbol
        const int cls = s.ss == 0 ? 0 : 1;
        const int th = cls ? pl[2 + 2 * k] & 15 : pl[2 + 2 * k] >> 4;
        if (cls == 0 && s.ah != 0) continue;
        if (th > 3 || !have_h[cls][th])
          return fail("SOF2 (progressive): scan %d: Huffman table id %d the file does not define", si, th);
        if (pooled[cls][th] < 0) {
          size_t t = 0;
          while (t < prog->tables.size() && std::memcmp(&prog->tables[t], &cur[cls * 4 + th], sizeof(HuffTable))) ++t;
          if (t == prog->tables.size()) prog->tables.push_back(cur[cls * 4 + th]);
          pooled[cls][th] = (int)t;
        }
        if (cls) s.ac_tbl = pooled[cls][th];
        else s.dc_tbl[k] = pooled[cls][th];
      }
      if (adobe_transform == 0 && f->ncomp == 3) return fail("Adobe transform 0 (RGB)", 0, 0);
      s.restart = restart;
      if (s.ns > 1) {
        s.nx = f->mcux;
        s.ny = f->mcuy;
      } else {
        const int c = s.comp[0];
        const int ch = f->ncomp == 1 ? 1 : h[c], cv = f->ncomp == 1 ? 1 : v[c];
        const int hm = f->ncomp == 1 ? 1 : f->hmax, vm = f->ncomp == 1 ? 1 : f->vmax;
        s.nx = ((f->width * ch + hm - 1) / hm + 7) / 8;
        s.ny = ((f->height * cv + vm - 1) / vm + 7) / 8;
      }
      // the entropy-coded segment ends at the first marker that is neither a stuffed 0xFF 0x00 nor an
      // RSTn (next_marker); only fill bytes lie between that 0xFF and the marker's code
      s.begin = p + 2 + L;
      size_t at = (size_t)s.begin;
      for (;;) {
        const uint8_t* ff = at < len ? static_cast<const uint8_t*>(std::memchr(file + at, 0xFF, len - at)) : nullptr;
        if (!ff) return fail("no EOI", 0, 0);
        const size_t run = (size_t)(ff - file);
        size_t k = run + 1;
        while (k < len && file[k] == 0xFF) ++k;
        if (k >= len) return fail("no EOI", 0, 0);
        if (file[k] == 0x00 || (file[k] >= 0xD0 && file[k] <= 0xD7)) {
          at = k + 1;
          continue;
        }
        s.end = run;
        break;
      }
      prog->scans.push_back(s);
      p = (size_t)s.end;
      continue;
    } else {
      return fail("marker %02X", m, 0);
    }
    p += 2 + L;
  }
  if (progressive) {
    // EOI.  libjpeg decodes a file that stops short of full precision, and smooths its blocks
    // (jdcoefct.c: decompress_smooth_data); that is not reproduced: such a file is refused.
    for (int c = 0; c < f->ncomp; ++c)
      for (int z = 0; z < 64; ++z)
        if (bits[c][z] != 0)
          return fail("SOF2 (progressive): the file ends before coefficient %d of component %d has reached bit 0", z, c);
    f->scan_begin = prog->scans.back().begin;
    f->scan_end = prog->scans.back().end;
    f->scan_count = (uint32_t)prog->scans.size();
    return true;
  }
  // The scan ends at the first marker behind it that is neither a stuffed 0xFF 0x00 nor an RSTn: that
  // must be EOI (jdmarker.c: next_marker).  What follows EOI is ignored, as libjpeg ignores it.
  size_t at = (size_t)f->scan_begin;
  for (;;) {
    const uint8_t* ff = at < len ? static_cast<const uint8_t*>(std::memchr(file + at, 0xFF, len - at)) : nullptr;
    if (!ff) return fail("no EOI", 0, 0);
    const size_t run = (size_t)(ff - file);   // (first 0xFF of a run of fill bytes)
    size_t k = run + 1;
    while (k < len && file[k] == 0xFF) ++k;
    if (k >= len) return fail("no EOI", 0, 0);
    const int m = file[k];
    if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) {
      at = k + 1;
      continue;
    }
    if (m != 0xD9) return fail("marker %02X behind the scan (several scans?)", m, 0);
    f->scan_end = run;
    break;
  }
  layout(f, h, v);
  return true;
}

// ... for a caller that wants the frame alone (the size of a file, a baseline descriptor)
inline bool parse(const uint8_t* file, size_t len, Frame* f, char* err, size_t errcap) {
  Progressive prog;
  return parse(file, len, f, &prog, err, errcap);
}

// status words the entropy kernel leaves per frame
enum Status : uint32_t {
  kOk = 0,
  kBadCode = 1,        // an undefined Huffman code
  kRunPast63 = 2,      // a run past coefficient 63
  kBadRestart = 3,     // a wrong or missing RSTn
  kEndsEarly = 4,      // the scan ends before its last block
  // (5 was "bytes left behind the last block": libjpeg skips them, and so does the walk.  Retired,
  // not reused.)
  kRunPastBand = 6,    // SOF2: a run past the end of the scan's band (Se)
  kBadRefinement = 7,  // SOF2: a refinement scan's new coefficient of a size other than 1
};

inline const char* status_text(uint32_t s) {
  switch (s) {
    case kOk: return "ok";
    case kBadCode: return "an undefined Huffman code";
    case kRunPast63: return "a run past coefficient 63";
    case kBadRestart: return "a wrong or missing RSTn marker";
    case kEndsEarly: return "the scan ends before its last block";
    case kRunPastBand: return "a run past the end of the scan's band";
    case kBadRefinement: return "a refinement coefficient of a size other than 1";
  }
  return "unknown status";
}

}  // namespace jpegd
}  // namespace amhip

#endif  // AMHIP_JPEG_DECODE_HOST_H_
