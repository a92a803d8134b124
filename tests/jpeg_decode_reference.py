"""NumPy restatement of libjpeg's baseline decoder at its defaults (JDCT_ISLOW, fancy upsampling):
what cv::imread / Pillow's Image.open give for a sequential 8-bit Huffman file of one scan, gray or
Y Cb Cr with Y sampled 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), with or without restart markers.

Every rule names the libjpeg function it restates (libjpeg-turbo file names).  Integer arithmetic
only (int64; >> on negative numbers is arithmetic, as libjpeg's RIGHT_SHIFT).  Pinned: the .npz files
beside the fixtures of tests/golden/jpeg_decode/ hold what the real library decodes, and
tests/test_jpeg_decode_reference.py compares bit for bit.  This module is the yardstick of the GPU
decoder (aerial_mapper_amd/csrc/amhip_jpeg_decode.hip).

Not restated: the C code's wraparound of samples beyond the range table (corrupt coefficients);
samples are clamped, as libjpeg-turbo's SIMD IDCT clamps them (pinned up to an IDCT output of
+-1303 by the fixtures of tests/golden/jpeg_decode/streams/; beyond that the SIMD code's 16-bit
intermediates leave the plain rule).  EXIF orientation is not applied.  Deliberately stricter than
libjpeg, which warns and goes on: a scan that ends early, a wrong RSTn index.
"""
import numpy as np

from jpeg_reference import ZIGZAG, huff_codes

LOOKAHEAD = 8   # HUFF_LOOKAHEAD (jdhuff.h)


class Refused(ValueError):
    """a file outside the accepted shape: the text names the marker or field"""


class Corrupt(ValueError):
    """an entropy-coded segment that does not decode"""


# ---------------------------------------------------------------------------
# header (jdmarker.c: read_markers, get_sof, get_sos, get_dht, get_dqt, get_dri)
# ---------------------------------------------------------------------------


class HuffTable(object):
    """jpeg_make_d_derived_tbl (jdhuff.c): look[256] = length << 8 | symbol for codes of at most 8
    bits (0: longer); maxcode[l] the largest code of length l (-1: none), maxcode[17] a sentinel;
    valoffset[l] = index of the first symbol of length l minus its code; huffval the symbols."""

    def __init__(self, bits, vals):
        self.bits, self.vals = list(bits), list(vals)
        if sum(bits) > 256 or sum(bits) != len(vals):
            raise Refused("DHT: bad symbol count")
        self.look = [0] * 256
        self.maxcode = [-1] * 18
        self.valoffset = [0] * 17
        self.huffval = list(vals) + [0] * (256 - len(vals))
        code, p = 0, 0
        for l in range(1, 17):
            n = bits[l - 1]
            if n:
                if code + n > (1 << l):
                    raise Refused("DHT: codes do not fit")
                self.valoffset[l] = p - code
                for i in range(n):
                    if l <= LOOKAHEAD:
                        lo = (code + i) << (LOOKAHEAD - l)
                        for k in range(1 << (LOOKAHEAD - l)):
                            self.look[lo + k] = (l << 8) | vals[p + i]
                p += n
                code += n
                self.maxcode[l] = code - 1
            code <<= 1
        self.maxcode[17] = 0xFFFFF
        assert huff_codes(bits, vals) is not None


class Header(object):
    """width, height; comps: list of dicts (id, h, v, tq, td, ta); qtables {id: natural-order 64};
    huff {(class, id): HuffTable}; restart (MCUs per interval, 0: none); scan_begin, scan_end: the
    byte range of the entropy-coded segment; channels = len(comps)"""
    pass


_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)",
              0xC5: "SOF5", 0xC6: "SOF6", 0xC7: "SOF7", 0xC9: "SOF9 (arithmetic)", 0xCA: "SOF10 (arithmetic)",
              0xCB: "SOF11 (arithmetic)", 0xCD: "SOF13", 0xCE: "SOF14", 0xCF: "SOF15", 0xC8: "JPG",
              0xCC: "DAC (arithmetic)"}


def parse_header(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    h = Header()
    h.qtables, h.huff, h.restart, h.comps = {}, {}, 0, None
    adobe_transform = None
    p = 2
    while True:
        if p + 4 > n:
            raise Refused("no SOS")
        if data[p] != 0xFF:
            raise Refused("marker expected at byte %d" % p)
        m = data[p + 1]
        if m == 0xFF:      # fill byte
            p += 1
            continue
        if m == 0xD9:
            raise Refused("no SOS")
        length = (data[p + 2] << 8) | data[p + 3]
        if length < 2 or p + 2 + length > n:
            raise Refused("segment %02X runs past the file" % m)
        pl = data[p + 4:p + 2 + length]
        if m == 0xC0:
            if h.comps is not None:
                raise Refused("second SOF0")
            if len(pl) < 6 or len(pl) != 6 + 3 * pl[5]:
                raise Refused("SOF0: bad length")
            if pl[0] != 8:
                raise Refused("SOF0: %d-bit samples" % pl[0])
            h.height, h.width = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4]
            if h.height < 1 or h.width < 1:
                raise Refused("SOF0: zero width or height")
            if pl[5] not in (1, 3):
                raise Refused("SOF0: %d components" % pl[5])
            h.comps = [dict(id=pl[6 + 3 * i], h=pl[7 + 3 * i] >> 4, v=pl[7 + 3 * i] & 15, tq=pl[8 + 3 * i])
                       for i in range(pl[5])]
            for c in h.comps:
                if not (1 <= c["h"] <= 4 and 1 <= c["v"] <= 4) or c["tq"] > 3:
                    raise Refused("SOF0: bad sampling factors or table id")
            if len(h.comps) == 3:
                s = [(c["h"], c["v"]) for c in h.comps]
                if s[0] not in ((1, 1), (2, 1), (2, 2)) or s[1] != (1, 1) or s[2] != (1, 1):
                    raise Refused("SOF0: sampling factors other than 4:4:4, 4:2:2, 4:2:0")
                if [c["id"] for c in h.comps] == [ord("R"), ord("G"), ord("B")]:
                    raise Refused("SOF0: component ids R G B")
        elif m in _SOF_NAMES:
            raise Refused("marker %s" % _SOF_NAMES[m])
        elif m == 0xDB:
            q = 0
            while q < len(pl):
                if pl[q] >> 4:
                    raise Refused("DQT: 16-bit table")
                if (pl[q] & 15) > 3 or q + 65 > len(pl):
                    raise Refused("DQT: bad table id or length")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(pl[q + 1:q + 65], np.uint8)
                h.qtables[pl[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(pl):
                if q + 17 > len(pl) or (pl[q] >> 4) > 1 or (pl[q] & 15) > 1:
                    raise Refused("DHT: bad table class, id or length")
                bits = list(pl[q + 1:q + 17])
                nv = sum(bits)
                if nv > 256 or q + 17 + nv > len(pl):
                    raise Refused("DHT: bad symbol count")
                vals = list(pl[q + 17:q + 17 + nv])
                if (pl[q] >> 4) == 0 and any(v > 15 for v in vals):
                    raise Refused("DHT: DC symbol above 15")
                h.huff[(pl[q] >> 4, pl[q] & 15)] = HuffTable(bits, vals)
                q += 17 + nv
        elif m == 0xDD:
            if len(pl) != 2:
                raise Refused("DRI: bad length")
            h.restart = (pl[0] << 8) | pl[1]
        elif m == 0xEE and pl[:5] == b"Adobe" and len(pl) >= 12:
            adobe_transform = pl[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDA:
            if h.comps is None:
                raise Refused("SOS before SOF0")
            if len(pl) < 1 or len(pl) != 4 + 2 * pl[0]:
                raise Refused("SOS: bad length")
            if pl[0] != len(h.comps):
                raise Refused("SOS: several scans (%d of %d components)" % (pl[0], len(h.comps)))
            for i, c in enumerate(h.comps):
                if pl[1 + 2 * i] != c["id"]:
                    raise Refused("SOS: component order")
                c["td"], c["ta"] = pl[2 + 2 * i] >> 4, pl[2 + 2 * i] & 15
                if c["td"] > 1 or c["ta"] > 1:
                    raise Refused("SOS: Huffman table id above 1")
                if (0, c["td"]) not in h.huff or (1, c["ta"]) not in h.huff:
                    raise Refused("SOS: missing Huffman table")
                if c["tq"] not in h.qtables:
                    raise Refused("SOS: missing quantisation table")
            if tuple(pl[-3:]) != (0, 63, 0):
                raise Refused("SOS: not a sequential scan (Ss, Se, Ah/Al)")
            if adobe_transform == 0 and len(h.comps) == 3:
                raise Refused("Adobe transform 0 (RGB)")
            h.scan_begin = p + 2 + length
            break
        else:
            raise Refused("marker %02X" % m)
        p += 2 + length
    # next_marker (jdmarker.c): the scan ends at the first marker behind it that is neither a stuffed
    # 0xFF 0x00 nor an RSTn; it must be EOI, and what follows EOI is ignored
    at = h.scan_begin
    while True:
        run = data.find(b"\xff", at)
        if run < 0:
            raise Refused("no EOI")
        k = run + 1
        while k < n and data[k] == 0xFF:
            k += 1
        if k >= n:
            raise Refused("no EOI")
        m = data[k]
        if m == 0 or 0xD0 <= m <= 0xD7:
            at = k + 1
            continue
        if m != 0xD9:
            raise Refused("marker %02X behind the scan (several scans?)" % m)
        h.scan_end = run
        break
    h.channels = len(h.comps)
    return h


def layout(h):
    """per_scan_setup (jdinput.c): -> hmax, vmax, mcux, mcuy, [(h, v) per component as coded].  A
    scan of one component is not interleaved: one block per MCU, 8 x 8 MCUs, whatever SOF0 says."""
    if len(h.comps) == 1:
        return 1, 1, (h.width + 7) // 8, (h.height + 7) // 8, [(1, 1)]
    hmax, vmax = h.comps[0]["h"], h.comps[0]["v"]
    return (hmax, vmax, (h.width + 8 * hmax - 1) // (8 * hmax), (h.height + 8 * vmax - 1) // (8 * vmax),
            [(c["h"], c["v"]) for c in h.comps])


# ---------------------------------------------------------------------------
# entropy decoding (jdhuff.c: decode_mcu, jpeg_fill_bit_buffer, jpeg_huff_decode, process_restart)
# ---------------------------------------------------------------------------


class Counters(object):
    def __init__(self):
        self.slow_codes = 0       # codes longer than the lookahead (the maxcode loop)
        self.restarts = 0         # RSTn markers passed
        self.rst_wraps = 0        # ... of which n went from 7 back to 0
        self.stuffed = 0          # 0xFF 0x00 pairs read as one byte
        self.fill_bytes = 0       # 0xFF fill bytes skipped in front of a stuffed 0x00 or an RSTn
        self.before_rst = 0       # bytes skipped between the end of an interval's data and its RSTn
        self.trailing = 0         # bytes between the last block and EOI (libjpeg warns and skips them)
        self.slow_by_length = np.zeros(17, np.int64)   # slow codes of each length 9..16
        self.max_dc_size = self.max_ac_size = 0        # the largest SSSS seen (merge with max, not +)
        self.at_63 = 0            # coefficients stored at zigzag 63 (such a block has no EOB)
        self.zrls = 0             # ZRL symbols
        self.zrl_past_63 = 0      # ZRLs that carry the index past 63 (the block ends there)


def entropy_decode(data, h, counters=None):
    """-> [coefficients of component c: (blocks down, blocks across, 64) int64, natural order,
    whole MCUs (padding blocks are what the scan codes for them)]"""
    cnt = counters if counters is not None else Counters()
    hmax, vmax, mcux, mcuy, samp = layout(h)
    planes = [np.zeros((mcuy * v, mcux * hh, 64), np.int64) for (hh, v) in samp]
    end = h.scan_end
    st = dict(pos=h.scan_begin, acc=0, nbits=0, fake=0)
    zz = [int(v) for v in ZIGZAG]

    def fill():
        # jpeg_fill_bit_buffer: a run of 0xFF and then 0x00 is one data byte 0xFF (all but the last
        # 0xFF of the run are fill bytes, T.81 B.1.1.2); at a marker (or behind the end) no byte is
        # consumed and zero bits are fed.  The run is followed no further than the scan's end.
        while st["nbits"] <= 56:
            pos = st["pos"]
            b = 0
            if pos >= end:
                st["fake"] += 8
            else:
                b = data[pos]
                if b == 0xFF:
                    k = pos + 1
                    while k < end and data[k] == 0xFF:
                        k += 1
                    b2 = data[k] if k < end else 0xD9
                    if b2 == 0:
                        st["pos"] = k + 1
                        cnt.stuffed += 1
                        cnt.fill_bytes += k - pos - 1
                    else:
                        b = 0
                        st["fake"] += 8
                else:
                    st["pos"] = pos + 1
            st["acc"] = ((st["acc"] << 8) | b) & ((1 << 64) - 1)
            st["nbits"] += 8

    def peek(nb):
        return (st["acc"] >> (st["nbits"] - nb)) & ((1 << nb) - 1)

    def drop(nb):
        st["nbits"] -= nb
        if st["nbits"] < st["fake"]:
            raise Corrupt("the scan ends early")

    def symbol(t):
        e = t.look[peek(LOOKAHEAD)]
        if e:
            drop(e >> 8)
            return e & 255
        cnt.slow_codes += 1
        l = LOOKAHEAD + 1
        while l <= 16 and peek(l) > t.maxcode[l]:
            l += 1
        if l > 16:
            raise Corrupt("undefined Huffman code")
        cnt.slow_by_length[l] += 1
        code = peek(l)
        drop(l)
        return t.huffval[(code + t.valoffset[l]) & 255]

    def receive_extend(s):
        # HUFF_EXTEND: a value below 2^(s-1) is negative
        v = peek(s)
        drop(s)
        return v - ((1 << s) - 1) if v < (1 << (s - 1)) else v

    pred = [0] * len(samp)
    todo = h.restart
    next_rst = 0
    for my in range(mcuy):
        for mx in range(mcux):
            if h.restart:
                if todo == 0:
                    # process_restart: discard the bits left of the byte; read_restart_marker /
                    # next_marker: skip to the next marker (bytes that are not 0xFF, 0xFF 0x00 pairs:
                    # "extraneous bytes", a warning; then any number of 0xFF and the code), which
                    # must be the next RSTn; predictors back to 0.  Stricter than libjpeg in one
                    # thing: a wrong index is an error (jpeg_resync_to_restart guesses and goes on).
                    st["acc"] = st["nbits"] = st["fake"] = 0
                    pos, code = st["pos"], None
                    while pos < end:
                        if data[pos] != 0xFF:
                            pos += 1
                            cnt.before_rst += 1
                            continue
                        k = pos + 1
                        while k < end and data[k] == 0xFF:
                            k += 1
                        if k >= end:
                            break
                        if data[k] != 0:
                            code = data[k]
                            break
                        cnt.before_rst += 1          # (a stuffed 0xFF among them)
                        cnt.stuffed += 1
                        cnt.fill_bytes += k - pos - 1
                        pos = k + 1
                    if code != 0xD0 + next_rst:
                        raise Corrupt("wrong or missing RST%d" % next_rst)
                    cnt.fill_bytes += k - pos - 1
                    st["pos"] = k + 1
                    cnt.restarts += 1
                    next_rst = (next_rst + 1) & 7
                    cnt.rst_wraps += next_rst == 0
                    pred = [0] * len(samp)
                    todo = h.restart
                todo -= 1
            for ci, (hh, v) in enumerate(samp):
                c = h.comps[ci]
                dc, ac = h.huff[(0, c["td"])], h.huff[(1, c["ta"])]
                for by in range(v):
                    for bx in range(hh):
                        row = planes[ci][my * v + by, mx * hh + bx]
                        fill()
                        s = symbol(dc)
                        cnt.max_dc_size = max(cnt.max_dc_size, s)
                        if s:
                            fill()
                            pred[ci] += receive_extend(s)
                        row[0] = pred[ci]
                        k = 1
                        while k < 64:
                            fill()
                            rs = symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break      # EOB
                                k += 16        # ZRL (past 63: the loop ends, as decode_mcu's does)
                                cnt.zrls += 1
                                cnt.zrl_past_63 += k > 63
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt("run past coefficient 63")
                            cnt.max_ac_size = max(cnt.max_ac_size, s)
                            cnt.at_63 += k == 63
                            row[zz[k]] = receive_extend(s)
                            k += 1
    # what lies between the last block and EOI is skipped whatever it is (next_marker: "extraneous
    # bytes before marker", a warning); the header parser has seen that no other marker is among it
    cnt.trailing += end - st["pos"]
    cnt.scan_bits_left = st["nbits"] - st["fake"]
    return planes


# ---------------------------------------------------------------------------
# IDCT (jidctint.c: jpeg_idct_islow)
# ---------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(d, shift):
    """one pass of jpeg_idct_islow along axis -2 (the 8 inputs d[..., k, :]).  The all-zero-AC
    shortcut of the C code gives the same bits and is not restated."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., k, :] for k in range(8))
    z1 = (i2 + i6) * F_0_541
    tmp2 = z1 + i6 * (-F_1_847)
    tmp3 = z1 + i2 * F_0_765
    tmp0 = (i0 + i4) << CONST_BITS
    tmp1 = (i0 - i4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961), z4 * (-F_0_390)
    z3, z4 = z3 + z5, z4 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([_descale(o, shift) for o in out], axis=-2)


class IdctCounters(object):
    def __init__(self):
        self.clamped_low = self.clamped_high = 0
        self.lowest = self.highest = 0   # extremes of the IDCT's output before + 128 (merge with min / max)


def idct_islow(coef, qtable, counters=None):
    """coef (..., 64) natural order, qtable (64,) natural order -> (..., 8, 8) samples 0..255:
    dequantise, columns (descale by CONST_BITS - PASS1_BITS = 11), rows (CONST_BITS + PASS1_BITS + 3
    = 18), + 128, clamp (the range_limit table)"""
    d = (coef * qtable).reshape(coef.shape[:-1] + (8, 8))
    ws = _idct_1d(d, CONST_BITS - PASS1_BITS)                         # columns: along the row index
    px = _idct_1d(ws.swapaxes(-1, -2), CONST_BITS + PASS1_BITS + 3).swapaxes(-1, -2) + 128
    if counters is not None:
        counters.lowest = min(counters.lowest, int(px.min()) - 128)
        counters.highest = max(counters.highest, int(px.max()) - 128)
        counters.clamped_low += int((px < 0).sum())
        counters.clamped_high += int((px > 255).sum())
    return np.clip(px, 0, 255)


def component_planes(h, coefs, counters=None, only_first=False):
    """-> [plane (8 * blocks down, 8 * blocks across) int64]: whole blocks, padding included"""
    out = []
    for ci, c in enumerate(h.comps):
        if only_first and ci:
            break
        px = idct_islow(coefs[ci], h.qtables[c["tq"]], counters)       # (R, C, 8, 8)
        r, cc = px.shape[:2]
        out.append(px.transpose(0, 2, 1, 3).reshape(8 * r, 8 * cc))
    return out


# ---------------------------------------------------------------------------
# upsampling (jdsample.c) and colour (jdcolor.c)
# ---------------------------------------------------------------------------


class SampleCounters(object):
    def __init__(self):
        self.replicated = self.h2v1_fancy = self.h2v2_fancy = self.fullsize = 0


def _fancy_row(cs, three, first, last_bias, even_bias, odd_bias, shift):
    """the horizontal triangle filter shared by h2v1_fancy_upsample and h2v2_fancy_upsample"""
    dw = cs.shape[1]
    out = np.empty((cs.shape[0], 2 * dw), np.int64)
    left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
    right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out[:, 0::2] = (three * cs + left + even_bias) >> shift
    out[:, 1::2] = (three * cs + right + odd_bias) >> shift
    out[:, 0] = first(cs[:, 0])
    out[:, -1] = (cs[:, -1] * (three + 1) + last_bias) >> shift
    return out


def upsample(plane, width, height, hmax, vmax, counters=None):
    """a 1 x 1 chroma plane -> (height, width): fullsize_upsample, h2v1_fancy_upsample or
    h2v2_fancy_upsample; plain replication (h2v1_upsample, h2v2_upsample) when the component is at
    most 2 samples wide (jinit_upsampler: downsampled_width > 2)"""
    cnt = counters if counters is not None else SampleCounters()
    dw = (width + hmax - 1) // hmax
    dh = (height + vmax - 1) // vmax
    p = plane[:dh, :dw]
    if hmax == 1 and vmax == 1:
        cnt.fullsize += 1
        return p
    if dw <= 2:
        cnt.replicated += 1
        return np.repeat(np.repeat(p, vmax, axis=0), hmax, axis=1)[:height, :width]
    if vmax == 1:
        cnt.h2v1_fancy += 1
        # out[2k] = (3 in[k] + in[k-1] + 1) >> 2, out[2k+1] = (3 in[k] + in[k+1] + 2) >> 2; ends copied
        out = _fancy_row(p, 3, lambda v: v, 0, 1, 2, 2)
        out[:, -1] = p[:, -1]
        return out[:, :width]
    cnt.h2v2_fancy += 1
    # colsum = 3 * row + neighbour (above for the upper output row, below for the lower; the first
    # and last REAL rows are their own neighbours), then 3 : 1 across with biases 8 and 7
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for par, nb in ((0, above), (1, below)):
        cs = 3 * p + nb
        out[par::2] = _fancy_row(cs, 3, lambda v: (4 * v + 8) >> 4, 7, 8, 7, 4)
    return out[:height, :width]


FIX_1_40200, FIX_1_77200, FIX_0_34414, FIX_0_71414 = 91881, 116130, 22554, 46802


def ycc_to_bgr(y, cb, cr):
    """ycc_rgb_convert (jdcolor.c, build_ycc_rgb_table): FIX(x) = (int)(x * 65536 + 0.5)"""
    cb, cr = cb - 128, cr - 128
    r = y + ((FIX_1_40200 * cr + 32768) >> 16)
    b = y + ((FIX_1_77200 * cb + 32768) >> 16)
    g = y + ((-FIX_0_34414 * cb - FIX_0_71414 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255)


# ---------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------


class Decoded(object):
    """header; coefs (per component, plane order); gray (H, W) uint8: the file's one component or
    its Y plane (cv::IMREAD_GRAYSCALE: JCS_GRAYSCALE); bgr (H, W, 3) uint8 (cv::IMREAD_COLOR)"""
    pass


def decode(data, counters=None):
    """counters: None or an object whose .entropy / .idct / .sample are Counters / IdctCounters /
    SampleCounters to be added to"""
    data = bytes(data)
    out = Decoded()
    h = out.header = parse_header(data)
    out.coefs = entropy_decode(data, h, getattr(counters, "entropy", None))
    planes = component_planes(h, out.coefs, getattr(counters, "idct", None))
    hmax, vmax = layout(h)[:2]
    y = planes[0][:h.height, :h.width]
    out.gray = y.astype(np.uint8)
    if len(planes) == 1:
        out.bgr = np.repeat(out.gray[..., None], 3, axis=-1)
    else:
        sc = getattr(counters, "sample", None)
        cb = upsample(planes[1], h.width, h.height, hmax, vmax, sc)
        cr = upsample(planes[2], h.width, h.height, hmax, vmax, sc)
        out.bgr = ycc_to_bgr(y, cb, cr).astype(np.uint8)
    return out


def decode_pixels(data, colored):
    d = decode(data)
    return d.bgr if colored else d.gray


class AllCounters(object):
    def __init__(self):
        self.entropy, self.idct, self.sample = Counters(), IdctCounters(), SampleCounters()
