"""The PNG decoder (aerial_mapper_amd/csrc/amhip_png_decode.hip, amhip_png_decode_host.h) restated
rule by rule in plain python, in the manner of tests/jpeg_decode_reference.py: the chunk parser with
the library's refusal texts, inflate (RFC 1951) symbol by symbol, Adler-32, the five filters and the
pixel rules.  Counters record which rules a file exercises; tests/png_decode_inputs.py asserts that
the fixture family reaches all of them.

Pinned: inflate to zlib.decompress, raw pixels and B, G, R to Pillow (tests/test_png_decode_reference.py).
Not pinned: gray from a colour file, libpng's png_set_rgb_to_gray(.., 0.299, 0.587) as cv::imread
sets it up, restated as (9797 R + 19234 G + 3737 B) >> 15 -- adopted, unpinned."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}

# amhip::pngd::status_text
STATUS = {
    "bad_code": "an undefined Huffman code",
    "over_subscribed": "an over-subscribed set of code lengths",
    "incomplete": "an incomplete set of code lengths",
    "bad_dyn_header": "a dynamic block's header is out of range (HLIT, HDIST, a repeat, or no end-of-block code)",
    "bad_block_type": "block type 3",
    "bad_stored_len": "a stored block's LEN is not ~NLEN",
    "dist_too_far": "a distance that reaches behind the first output byte",
    "ends_early": "the stream ends before its final block does",
    "too_short": "the stream holds fewer bytes than the image's scanlines",
    "too_long": "the stream holds more bytes than the image's scanlines",
    "bad_filter": "a filter type above 4",
    "bad_adler": "an Adler-32 mismatch",
    "bad_index": "a palette index outside PLTE",
}


class Refused(Exception):
    """the host parser's refusal, with the library's text"""


class Corrupt(Exception):
    """an error the device finds, with the library's text"""


class Counters(object):
    def __init__(self):
        self.blocks = [0, 0, 0]           # stored, fixed, dynamic
        self.filters = [0, 0, 0, 0, 0]
        self.length_codes = set()         # 257..285
        self.dist_codes = set()           # 0..29
        self.repeats = set()              # (16 | 17 | 18, count)
        self.repeat_crossed = 0           # a repeat that ran from the literal into the distance lengths
        self.ring_wraps = 0               # the output passed a multiple of 32768
        self.long_codes = 0               # symbols whose code is longer than the lookup table's bits
        self.max_code_length = 0
        self.overlapping = 0              # matches with distance < length
        self.single_dist_code = 0
        self.no_dist_code = 0
        self.paeth_picks = set()          # "a", "b", "c" on ties and otherwise
        self.average_carry = 0            # Average with a + b >= 256

    def add(self, o):
        for k, v in vars(o).items():
            mine = getattr(self, k)
            if isinstance(v, set):
                mine |= v
            elif isinstance(v, list):
                setattr(self, k, [a + b for a, b in zip(mine, v)])
            elif k == "max_code_length":
                self.max_code_length = max(mine, v)
            else:
                setattr(self, k, mine + v)


class Header(object):
    pass


def _chunk_name(t):
    return "".join(chr(c) if ord("A") <= c <= ord("z") else "?" for c in t)


def parse(data):
    """amhip::pngd::parse -> Header (width, height, colour_type, bpp, plte, idat spans, stream, adler)"""
    data = bytes(data)
    n = len(data)
    if n < 8 or data[:8] != SIGNATURE:
        raise Refused("no PNG signature")
    h = Header()
    h.idat, h.plte = [], b""
    p = 8
    have_ihdr = have_plte = have_iend = idat_open = idat_closed = False
    while not have_iend:
        if p == n:
            raise Refused("no IDAT chunk" if not h.idat else "no IEND chunk")
        if n - p < 8:
            raise Refused("truncated chunk header at byte %d" % p)
        L = struct.unpack(">I", data[p:p + 4])[0]
        t = data[p + 4:p + 8]
        if L + 12 > n - p:
            if L > 0x7FFFFFFF or L > n:
                raise Refused("chunk %s: its length runs past the file" % _chunk_name(t))
            raise Refused("chunk %s: truncated" % _chunk_name(t))
        pl = data[p + 8:p + 8 + L]
        if not have_ihdr and t != b"IHDR":
            raise Refused("IHDR is not the first chunk")
        if t in (b"IHDR", b"PLTE", b"IDAT", b"IEND"):
            if zlib.crc32(t + pl) != struct.unpack(">I", data[p + 8 + L:p + 12 + L])[0]:
                raise Refused("chunk %s: bad CRC" % _chunk_name(t))
        elif not (t[0] & 0x20):
            raise Refused("unknown critical chunk %s" % _chunk_name(t))
        if idat_open and t != b"IDAT":
            idat_open, idat_closed = False, True
        if t == b"IHDR":
            if have_ihdr:
                raise Refused("second IHDR")
            if L != 13:
                raise Refused("IHDR: length %d" % L)
            w, hh, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", pl)
            if not (1 <= w <= 65535 and 1 <= hh <= 65535):
                raise Refused("IHDR: width or height outside 1..65535")
            if ct not in BPP:
                raise Refused("IHDR: colour type %d" % ct)
            if depth != 8:
                raise Refused("IHDR: bit depth %d" % depth)
            if comp:
                raise Refused("IHDR: compression method %d" % comp)
            if flt:
                raise Refused("IHDR: filter method %d" % flt)
            if lace:
                raise Refused("IHDR: interlace method %d (Adam7)" % lace)
            h.width, h.height, h.colour_type, h.bpp = w, hh, ct, BPP[ct]
            h.raw_len = hh * (1 + w * h.bpp)
            have_ihdr = True
        elif t == b"PLTE":
            if have_plte:
                raise Refused("second PLTE")
            if h.idat or idat_closed:
                raise Refused("PLTE behind IDAT")
            if L == 0 or L % 3 or L > 768:
                raise Refused("PLTE: length %d" % L)
            h.plte = pl
            have_plte = True
        elif t == b"IDAT":
            if idat_closed:
                raise Refused("IDAT behind another chunk: the run of IDAT chunks is interrupted")
            idat_open = True
            h.idat.append((p + 8, L))
        elif t == b"IEND":
            have_iend = True
        p += 12 + L
    if not h.idat:
        raise Refused("no IDAT chunk")
    if h.colour_type == 3 and not have_plte:
        raise Refused("colour type 3 without a PLTE chunk")
    h.stream = b"".join(data[b:b + l] for b, l in h.idat)
    h.zlen = len(h.stream)
    if h.zlen < 6:
        raise Refused("IDAT: %d bytes are no zlib stream" % h.zlen)
    cmf, flg = h.stream[0], h.stream[1]
    if cmf & 15 != 8:
        raise Refused("zlib header: compression method %d" % (cmf & 15))
    if cmf >> 4 > 7:
        raise Refused("zlib header: CINFO %d" % (cmf >> 4))
    if (cmf * 256 + flg) % 31:
        raise Refused("zlib header: FCHECK")
    if flg & 0x20:
        raise Refused("zlib header: FDICT set")
    h.adler = struct.unpack(">I", h.stream[-4:])[0]
    h.plte_entries = len(h.plte) // 3
    return h


# ---- RFC 1951 ------------------------------------------------------------------------------------
def _bases(n, free, first, step):
    base, extra, b = [], [], first
    for i in range(n):
        e = 0 if i < free else (i - free + step) // step
        base.append(b)
        extra.append(e)
        b += 1 << e
    return base, extra


LEN_BASE, LEN_EXTRA = _bases(28, 8, 3, 4)
LEN_BASE.append(258)
LEN_EXTRA.append(0)
DIST_BASE, DIST_EXTRA = _bases(30, 4, 1, 2)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FAST_BITS = {"lit": 10, "dist": 8, "cl": 7}


class _Bits(object):
    def __init__(self, data):
        self.data, self.pos = data, 0          # pos in bits

    def take(self, n):
        v = 0
        for k in range(n):
            byte = self.pos >> 3
            if byte >= len(self.data):
                raise Corrupt(STATUS["ends_early"])
            v |= ((self.data[byte] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


class _Code(object):
    """canonical code from lengths; .left: 0 complete, > 0 incomplete, < 0 over-subscribed"""

    def __init__(self, lens):
        self.count = [0] * 16
        for l in lens:
            if l:
                self.count[l] += 1
        self.longest = max([l for l in range(16) if self.count[l]] or [0])
        left = 1
        for l in range(1, 16):
            left = (left << 1) - self.count[l]
            if left < 0:
                break
        self.left = left
        self.sorted = [s for l in range(1, 16) for s, x in enumerate(lens) if x == l]

    def decode(self, bits):
        """-> (symbol, code length); the walk zlib's puff does"""
        code = first = index = 0
        for l in range(1, 16):
            code |= bits.take(1)
            k = self.count[l]
            if code - k < first:
                return self.sorted[index + code - first], l
            index += k
            first = (first + k) << 1
            code <<= 1
        raise Corrupt(STATUS["bad_code"])


def _check_set(code, what):
    if code.left < 0:
        raise Corrupt(STATUS["over_subscribed"])
    if code.left > 0:
        # complete, or -- for the distance code only -- no code at all or the one code of one bit
        if what != "dist" or code.longest > 1:
            raise Corrupt(STATUS["incomplete"])


def inflate(data, expected, c=None):
    """data: the deflate stream (no zlib header, no trailer); expected: the scanlines' length.
    -> bytes of exactly that length, or Corrupt with the library's text"""
    c = c if c is not None else Counters()
    bits = _Bits(data)
    out = bytearray()

    def grew(before):
        if len(out) > expected:
            raise Corrupt(STATUS["too_long"])
        c.ring_wraps += len(out) // 32768 - before // 32768

    last = False
    while not last:
        last = bits.take(1) == 1
        btype = bits.take(2)
        if btype == 3:
            raise Corrupt(STATUS["bad_block_type"])
        c.blocks[btype] += 1
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            ln, nln = bits.take(16), bits.take(16)
            if ln ^ 0xFFFF != nln:
                raise Corrupt(STATUS["bad_stored_len"])
            at = bits.pos >> 3
            if at + ln > len(data):
                raise Corrupt(STATUS["ends_early"])
            for k in range(0, ln, 64):
                before = len(out)
                out += data[at + k:at + min(k + 64, ln)]
                grew(before)
            bits.pos += 8 * ln
            continue
        if btype == 1:
            lit = _Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
            dist = _Code([5] * 32)
        else:
            hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            if hlit > 286 or hdist > 30:
                raise Corrupt(STATUS["bad_dyn_header"])
            cl = [0] * 19
            for i in range(hclen):
                cl[CL_ORDER[i]] = bits.take(3)
            clc = _Code(cl)
            _check_set(clc, "cl")
            lens = []
            while len(lens) < hlit + hdist:
                s, _ = clc.decode(bits)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Corrupt(STATUS["bad_dyn_header"])
                    value, times = lens[-1], 3 + bits.take(2)
                elif s == 17:
                    value, times = 0, 3 + bits.take(3)
                else:
                    value, times = 0, 11 + bits.take(7)
                if len(lens) + times > hlit + hdist:
                    raise Corrupt(STATUS["bad_dyn_header"])
                c.repeats.add((s, times))
                if len(lens) < hlit < len(lens) + times:
                    c.repeat_crossed += 1
                lens += [value] * times
            if lens[256] == 0:
                raise Corrupt(STATUS["bad_dyn_header"])
            lit = _Code(lens[:hlit] + [0] * (288 - hlit))
            _check_set(lit, "lit")
            dist = _Code(lens[hlit:])
            _check_set(dist, "dist")
            if dist.left > 0:
                if dist.longest == 0:
                    c.no_dist_code += 1
                else:
                    c.single_dist_code += 1
        while True:
            s, l = lit.decode(bits)
            c.max_code_length = max(c.max_code_length, l)
            c.long_codes += l > FAST_BITS["lit"]
            before = len(out)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise Corrupt(STATUS["bad_code"])
                ln = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                ds, l = dist.decode(bits)
                c.max_code_length = max(c.max_code_length, l)
                c.long_codes += l > FAST_BITS["dist"]
                if ds > 29:
                    raise Corrupt(STATUS["bad_code"])
                d = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                if d > len(out):
                    raise Corrupt(STATUS["dist_too_far"])
                c.length_codes.add(s)
                c.dist_codes.add(ds)
                c.overlapping += d < ln
                # byte k of the match is the byte d behind it: for d < ln the last d bytes repeat
                start = len(out) - d
                for k in range(ln):
                    out.append(out[start + (k if d >= ln else k % d)])
            grew(before)
    if len(out) < expected:
        raise Corrupt(STATUS["too_short"])
    return bytes(out)


def adler32(data):
    s1, s2 = 1, 0
    for b in data:
        s1 = (s1 + b) % 65521
        s2 = (s2 + s1) % 65521
    return (s2 << 16) | s1


def _paeth(a, b, cc, c):
    p = a + b - cc
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
    if pa <= pb and pa <= pc:      # ties: a, then b, then c
        if c is not None:
            c.paeth_picks.add("a tie" if (pa == pb or pa == pc) else "a")
        return a
    if pb <= pc:
        if c is not None:
            c.paeth_picks.add("b tie" if pb == pc else "b")
        return b
    if c is not None:
        c.paeth_picks.add("c")
    return cc


def unfilter(raw, width, height, bpp, c=None):
    """the filtered scanlines -> (height, width * bpp) uint8"""
    c = c if c is not None else Counters()
    pitch = width * bpp
    out = np.zeros((height, pitch), np.uint8)
    prev = [0] * pitch
    for y in range(height):
        ft = raw[y * (pitch + 1)]
        if ft > 4:
            raise Corrupt(STATUS["bad_filter"])
        c.filters[ft] += 1
        line = raw[y * (pitch + 1) + 1:(y + 1) * (pitch + 1)]
        cur = [0] * pitch
        for i in range(pitch):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            cc = prev[i - bpp] if i >= bpp else 0
            x = line[i]
            if ft == 0:
                v = x
            elif ft == 1:
                v = x + a
            elif ft == 2:
                v = x + b
            elif ft == 3:
                c.average_carry += a + b >= 256
                v = x + ((a + b) >> 1)      # the 9-bit sum
            else:
                v = x + _paeth(a, b, cc, c)
            cur[i] = v & 255
        out[y] = cur
        prev = cur
    return out


def pixels(h, rows):
    """rows: (height, width * bpp) unfiltered -> (gray (H, W), bgr (H, W, 3)) uint8"""
    px = rows.reshape(h.height, h.width, h.bpp).astype(np.uint32)
    ct = h.colour_type
    if ct in (0, 4):
        g = px[:, :, 0].astype(np.uint8)
        return g, np.repeat(g[:, :, None], 3, axis=2)
    if ct == 3:
        idx = px[:, :, 0]
        if int(idx.max()) >= h.plte_entries:
            raise Corrupt(STATUS["bad_index"])
        pal = np.frombuffer(h.plte, np.uint8).reshape(-1, 3).astype(np.uint32)
        rgb = pal[idx]
    else:
        rgb = px[:, :, :3]
    R, G, B = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
    gray = ((9797 * R + 19234 * G + 3737 * B) >> 15).astype(np.uint8)      # adopted, unpinned
    return gray, np.stack([B, G, R], axis=2).astype(np.uint8)


class Decoded(object):
    pass


def decode(data, c=None):
    """the whole decoder -> .header, .raw (filtered scanlines), .rows (unfiltered), .gray, .bgr"""
    c = c if c is not None else Counters()
    d = Decoded()
    d.header = h = parse(data)
    d.raw = inflate(h.stream[2:-4], h.raw_len, c)
    if adler32(d.raw) != h.adler:
        raise Corrupt(STATUS["bad_adler"])
    d.rows = unfilter(d.raw, h.width, h.height, h.bpp, c)
    d.gray, d.bgr = pixels(h, d.rows)
    d.counters = c
    return d


def decode_pixels(data, colored):
    d = decode(data)
    return d.bgr if colored else d.gray
