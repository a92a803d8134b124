"""The PNG file the GPU encoder (amhip_png_encode.hip) has to write, restated on the host.

What cv::imwrite leaves when no PNG parameter is given: filter Sub on every row, and zlib at
Z_BEST_SPEED with strategy Z_RLE, window 15, memLevel 8.  Under Z_RLE the token sequence is a pure
function of the runs of equal bytes, and everything behind the tokens is integer arithmetic per
block of 16383 symbols, so the whole stream can be restated without zlib.  The rules, and the zlib
1.2.11 function each restates:

  1 container            png_write_IHDR / png_write_IDAT (zbuffer 8192) / png_write_IEND
  2 scanlines            png_write_find_filter with PNG_FILTER_SUB alone
  3 zlib stream          deflate()'s header for level 1 (78 01), adler32()
  4 tokens               deflate_rle()
  5 blocks               _tr_tally() (lit_bufsize - 1 = 16383), FLUSH_BLOCK at Z_FINISH
  6 per block            _tr_flush_block(): build_tree / pqdownheap / gen_bitlen / gen_codes,
                         build_bl_tree / scan_tree / send_tree / send_all_trees, compress_block,
                         _tr_stored_block, bi_windup

Nothing in here calls zlib's deflate; zlib_rle_stream() below is the library itself, for the tests
that compare the two.
"""
import struct
import zlib

import numpy as np

LITERALS = 256
END_BLOCK = 256
L_CODES = 286
D_CODES = 30
BL_CODES = 19
HEAP_SIZE = 2 * L_CODES + 1
REP_3_6, REPZ_3_10, REPZ_11_138 = 16, 17, 18
BLOCK_SYMBOLS = 16383          # lit_bufsize - 1 at memLevel 8
IDAT_BYTES = 8192              # libpng's default zbuffer
MAX_MATCH = 258

EXTRA_LBITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
EXTRA_DBITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
EXTRA_BLBITS = [0] * 16 + [2, 3, 7]
BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def bi_reverse(code, length):
    res = 0
    for _ in range(length):
        res = (res << 1) | (code & 1)
        code >>= 1
    return res


def _static_init():
    """tr_static_init()"""
    base_length = [0] * 29
    length_code = [0] * 256
    length = 0
    for code in range(28):
        base_length[code] = length
        for _ in range(1 << EXTRA_LBITS[code]):
            length_code[length] = code
            length += 1
    assert length == 256
    length_code[255] = 28
    ltree_len = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    bl_count = [0] * 16
    for n in ltree_len:
        bl_count[n] += 1
    ltree_code = gen_codes(ltree_len, 287, bl_count)
    dtree_len = [5] * D_CODES
    dtree_code = [bi_reverse(n, 5) for n in range(D_CODES)]
    return base_length, length_code, ltree_len, ltree_code, dtree_len, dtree_code


def gen_codes(lens, max_code, bl_count):
    """gen_codes(): the bit-reversed codes of lens[0 .. max_code]"""
    next_code = [0] * 16
    code = 0
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lens)
    for n in range(max_code + 1):
        ln = lens[n]
        if ln == 0:
            continue
        codes[n] = bi_reverse(next_code[ln], ln)
        next_code[ln] += 1
    return codes


class Tree:
    """one of a block's three trees: what build_tree() reads and leaves"""

    def __init__(self, elems, static_len, extra_bits, extra_base, max_length):
        self.elems = elems
        self.static_len = static_len
        self.extra_bits = extra_bits
        self.extra_base = extra_base
        self.max_length = max_length
        self.freq = [0] * HEAP_SIZE
        self.len = [0] * HEAP_SIZE
        self.code = [0] * HEAP_SIZE
        self.max_code = -1
        self.repaired = False


class Block:
    """deflate_state's tree part for one block"""

    def __init__(self):
        self.opt_len = 0
        self.static_len = 0
        self.l = Tree(L_CODES, STATIC_LTREE_LEN, EXTRA_LBITS, LITERALS + 1, 15)
        self.d = Tree(D_CODES, STATIC_DTREE_LEN, EXTRA_DBITS, 0, 15)
        self.bl = Tree(BL_CODES, None, EXTRA_BLBITS, 0, 7)
        self.l.freq[END_BLOCK] = 1


def build_tree(s, t):
    """build_tree() with pqdownheap(), gen_bitlen() and gen_codes()"""
    freq, lens = t.freq, t.len
    heap = [0] * HEAP_SIZE
    depth = [0] * HEAP_SIZE
    dad = [0] * HEAP_SIZE
    heap_len = 0
    heap_max = HEAP_SIZE
    max_code = -1
    for n in range(t.elems):
        if freq[n] != 0:
            heap_len += 1
            heap[heap_len] = max_code = n
            depth[n] = 0
        else:
            lens[n] = 0
    while heap_len < 2:
        if max_code < 2:
            max_code += 1
            node = max_code
        else:
            node = 0
        heap_len += 1
        heap[heap_len] = node
        freq[node] = 1
        depth[node] = 0
        s.opt_len -= 1
        if t.static_len is not None:
            s.static_len -= t.static_len[node]
    t.max_code = max_code

    def smaller(n, m):
        return freq[n] < freq[m] or (freq[n] == freq[m] and depth[n] <= depth[m])

    def pqdownheap(k):
        v = heap[k]
        j = k << 1
        while j <= heap_len:
            if j < heap_len and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k = j
            j <<= 1
        heap[k] = v

    for n in range(heap_len // 2, 0, -1):
        pqdownheap(n)
    node = t.elems
    while True:
        n = heap[1]
        heap[1] = heap[heap_len]
        heap_len -= 1
        pqdownheap(1)
        m = heap[1]
        heap_max -= 1
        heap[heap_max] = n
        heap_max -= 1
        heap[heap_max] = m
        freq[node] = freq[n] + freq[m]
        depth[node] = max(depth[n], depth[m]) + 1
        dad[n] = dad[m] = node
        heap[1] = node
        node += 1
        pqdownheap(1)
        if heap_len < 2:
            break
    heap_max -= 1
    heap[heap_max] = heap[1]

    # gen_bitlen()
    bl_count = [0] * 16
    max_length = t.max_length
    lens[heap[heap_max]] = 0
    overflow = 0
    for h in range(heap_max + 1, HEAP_SIZE):
        n = heap[h]
        bits = lens[dad[n]] + 1
        if bits > max_length:
            bits = max_length
            overflow += 1
        lens[n] = bits
        if n > max_code:
            continue
        bl_count[bits] += 1
        xbits = t.extra_bits[n - t.extra_base] if n >= t.extra_base else 0
        s.opt_len += freq[n] * (bits + xbits)
        if t.static_len is not None:
            s.static_len += freq[n] * (t.static_len[n] + xbits)
    if overflow > 0:
        t.repaired = True
        while True:
            bits = max_length - 1
            while bl_count[bits] == 0:
                bits -= 1
            bl_count[bits] -= 1
            bl_count[bits + 1] += 2
            bl_count[max_length] -= 1
            overflow -= 2
            if overflow <= 0:
                break
        h = HEAP_SIZE
        for bits in range(max_length, 0, -1):
            n = bl_count[bits]
            while n != 0:
                h -= 1
                m = heap[h]
                if m > max_code:
                    continue
                if lens[m] != bits:
                    s.opt_len += (bits - lens[m]) * freq[m]
                    lens[m] = bits
                n -= 1
    t.code = gen_codes(lens, max_code, bl_count)


def _walk_tree(lens, max_code, emit):
    """the loop scan_tree() and send_tree() share; emit(kind, curlen, count)"""
    prevlen = -1
    nextlen = lens[0]
    count = 0
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for n in range(max_code + 1):
        curlen = nextlen
        nextlen = lens[n + 1] if n < max_code else 0xFFFF   # the sentinel behind max_code
        count += 1
        if count < max_count and curlen == nextlen:
            continue
        if count < min_count:
            emit("plain", curlen, count)
        elif curlen != 0:
            if curlen != prevlen:
                emit("plain", curlen, 1)
                count -= 1
            emit("rep", REP_3_6, count)
        elif count <= 10:
            emit("rep", REPZ_3_10, count)
        else:
            emit("rep", REPZ_11_138, count)
        count = 0
        prevlen = curlen
        if nextlen == 0:
            max_count, min_count = 138, 3
        elif curlen == nextlen:
            max_count, min_count = 6, 3
        else:
            max_count, min_count = 7, 4


def scan_tree(s, lens, max_code, stats=None):
    def emit(kind, sym, count):
        s.bl.freq[sym] += count if kind == "plain" else 1
        if kind == "rep" and stats is not None:
            stats.repeats.add((sym, count))
    _walk_tree(lens, max_code, emit)
    if stats is not None:
        # the runs of equal code lengths the walk met: (the length is zero, the run's length)
        at = 0
        while at <= max_code:
            end = at
            while end <= max_code and lens[end] == lens[at]:
                end += 1
            stats.len_runs.add((lens[at] == 0, end - at))
            at = end


class BitWriter:
    """send_bits(): LSB first"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, length):
        self.acc |= value << self.n
        self.n += length
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def windup(self):
        if self.n:
            self.out.append(self.acc & 255)
        self.acc = 0
        self.n = 0

    def bit_length(self):
        return len(self.out) * 8 + self.n


def send_tree(w, s, lens, max_code):
    def emit(kind, sym, count):
        if kind == "plain":
            for _ in range(count):
                w.bits(s.bl.code[sym], s.bl.len[sym])
        else:
            w.bits(s.bl.code[sym], s.bl.len[sym])
            if sym == REP_3_6:
                w.bits(count - 3, 2)
            elif sym == REPZ_3_10:
                w.bits(count - 3, 3)
            else:
                w.bits(count - 11, 7)
    _walk_tree(lens, max_code, emit)


def tokens(d):
    """deflate_rle(): the symbols of the whole input.  0..255 a literal, 256 + length a match of
    distance 1.  Returns (symbols, the byte each starts at)."""
    d = np.frombuffer(bytes(d), np.uint8)
    n = d.size
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
    ends = np.concatenate((starts[1:], [n]))
    long_runs = np.flatnonzero(ends - starts >= 4)
    if long_runs.size == 0:
        return d.astype(np.int32), np.arange(n, dtype=np.int64)
    sym, pos = [], []
    at = 0
    for r in long_runs:
        s0, e = int(starts[r]), int(ends[r])
        # everything up to and with the run's first byte: literals
        sym.append(d[at:s0 + 1].astype(np.int32))
        pos.append(np.arange(at, s0 + 1, dtype=np.int64))
        p = s0 + 1
        rest = e - p
        ms, mp = [], []
        while rest >= 3:                  # greedy: 258 while at least 3 remain, then what is left
            ln = min(rest, MAX_MATCH)
            ms.append(256 + ln)
            mp.append(p)
            p += ln
            rest -= ln
        sym.append(np.array(ms, np.int32))
        pos.append(np.array(mp, np.int64))
        at = p
    sym.append(d[at:].astype(np.int32))
    pos.append(np.arange(at, n, dtype=np.int64))
    return np.concatenate(sym), np.concatenate(pos)


class Stats:
    """what a stream reached, for the fixture generator's counts"""

    def __init__(self):
        self.block_types = []          # per block: "stored" / "fixed" / "dynamic"
        self.block_bits = []           # the bit offset each block starts at
        self.lcodes = []
        self.dcodes = []
        self.max_blindex = []
        self.repeats = set()           # (repeat code, the lengths it stands for)
        self.len_runs = set()          # (zero length, run) of equal code lengths in a tree
        self.repaired_l = self.repaired_bl = False
        self.tie = False
        self.symbols = 0
        self.match_lengths = set()
        self.boundary_in_run = False
        self.no_match_block = self.one_match_block = False


def deflate_rle(d, stats=None):
    """rules 4 to 6: the deflate data of `d`"""
    d = bytes(d)
    sym, pos = tokens(d)
    nsym = int(sym.size)
    if stats is not None:
        stats.symbols = nsym
        stats.match_lengths = set(int(v) - 256 for v in np.unique(sym[sym >= 256]))
    w = BitWriter()
    nblocks = nsym // BLOCK_SYMBOLS + 1
    for b in range(nblocks):
        lo = b * BLOCK_SYMBOLS
        hi = min(lo + BLOCK_SYMBOLS, nsym)
        last = 1 if b == nblocks - 1 else 0
        byte_lo = int(pos[lo]) if lo < nsym else len(d)
        byte_hi = int(pos[hi]) if hi < nsym else len(d)
        stored_len = byte_hi - byte_lo
        bs = sym[lo:hi]
        s = Block()
        # _tr_tally()
        lit = bs[bs < 256]
        mt = bs[bs >= 256] - 256
        for v, c in zip(*np.unique(lit, return_counts=True)):
            s.l.freq[int(v)] += int(c)
        for v, c in zip(*np.unique(mt, return_counts=True)):
            s.l.freq[LENGTH_CODE[int(v) - 3] + LITERALS + 1] += int(c)
        s.d.freq[0] += int(mt.size)
        # _tr_flush_block()
        build_tree(s, s.l)
        build_tree(s, s.d)
        scan_tree(s, s.l.len, s.l.max_code, stats)
        scan_tree(s, s.d.len, s.d.max_code, stats)
        build_tree(s, s.bl)
        max_blindex = BL_CODES - 1
        while max_blindex >= 3 and s.bl.len[BL_ORDER[max_blindex]] == 0:
            max_blindex -= 1
        s.opt_len += 3 * (max_blindex + 1) + 5 + 5 + 4
        opt_lenb = (s.opt_len + 3 + 7) >> 3
        static_lenb = (s.static_len + 3 + 7) >> 3
        if stats is not None:
            stats.block_bits.append(w.bit_length())
            stats.lcodes.append(s.l.max_code + 1)
            stats.dcodes.append(s.d.max_code + 1)
            stats.max_blindex.append(max_blindex)
            stats.repaired_l |= s.l.repaired
            stats.repaired_bl |= s.bl.repaired
            stats.tie |= static_lenb == opt_lenb
            stats.no_match_block |= mt.size == 0 and hi > lo
            stats.one_match_block |= mt.size == 1
            if 0 < lo < nsym and byte_lo > 0 and d[byte_lo] == d[byte_lo - 1]:
                stats.boundary_in_run = True
        if static_lenb <= opt_lenb:
            opt_lenb = static_lenb
        if stored_len + 4 <= opt_lenb:
            kind = "stored"
            w.bits((0 << 1) + last, 3)
            w.windup()
            w.bits(stored_len, 16)
            w.bits(stored_len ^ 0xFFFF, 16)
            w.out += d[byte_lo:byte_hi]
        else:
            if static_lenb == opt_lenb:
                kind = "fixed"
                w.bits((1 << 1) + last, 3)
                lcode, llen, dcode, dlen = STATIC_LTREE_CODE, STATIC_LTREE_LEN, STATIC_DTREE_CODE, STATIC_DTREE_LEN
            else:
                kind = "dynamic"
                w.bits((2 << 1) + last, 3)
                # send_all_trees()
                w.bits(s.l.max_code + 1 - 257, 5)
                w.bits(s.d.max_code + 1 - 1, 5)
                w.bits(max_blindex + 1 - 4, 4)
                for rank in range(max_blindex + 1):
                    w.bits(s.bl.len[BL_ORDER[rank]], 3)
                send_tree(w, s, s.l.len, s.l.max_code)
                send_tree(w, s, s.d.len, s.d.max_code)
                lcode, llen, dcode, dlen = s.l.code, s.l.len, s.d.code, s.d.len
            # compress_block()
            for v in bs.tolist():
                if v < 256:
                    w.bits(lcode[v], llen[v])
                else:
                    lc = v - 256 - 3
                    code = LENGTH_CODE[lc]
                    w.bits(lcode[code + LITERALS + 1], llen[code + LITERALS + 1])
                    if EXTRA_LBITS[code]:
                        w.bits(lc - BASE_LENGTH[code], EXTRA_LBITS[code])
                    w.bits(dcode[0], dlen[0])
            w.bits(lcode[END_BLOCK], llen[END_BLOCK])
        if stats is not None:
            stats.block_types.append(kind)
    w.windup()
    return bytes(w.out)


def adler32(d):
    """adler32(), as the two plain sums"""
    d = np.frombuffer(bytes(d), np.uint8).astype(np.uint64)
    n = d.size
    s1 = (1 + int(d.sum())) % 65521
    s2 = (n + int((d * np.arange(n, 0, -1, dtype=np.uint64) % np.uint64(65521)).sum())) % 65521
    return (s2 << 16) | s1


def zlib_stream(raw, stats=None):
    """rule 3"""
    return b"\x78\x01" + deflate_rle(raw, stats) + struct.pack(">I", adler32(raw))


def zlib_rle_stream(raw):
    """the library itself, as cv::imwrite sets it up"""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(bytes(raw)) + c.flush()


def scanlines(pixels):
    """rule 2.  pixels: (h, w) gray or (h, w, 3) B, G, R, uint8"""
    px = np.ascontiguousarray(pixels, dtype=np.uint8)
    if px.ndim == 2:
        px = px[:, :, None]
    else:
        px = px[:, :, ::-1]
    h, w, c = px.shape
    row = px.reshape(h, w * c).astype(np.int16)
    sub = row.copy()
    sub[:, c:] -= row[:, :-c]
    out = np.zeros((h, 1 + w * c), np.uint8)
    out[:, 0] = 1
    out[:, 1:] = (sub & 255).astype(np.uint8)
    return out.tobytes()


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def frame_file(width, height, channels, zstream):
    """rule 1 around a finished zlib stream"""
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 0 if channels == 1 else 2, 0, 0, 0))]
    assert len(zstream) > 0
    for at in range(0, len(zstream), IDAT_BYTES):
        out.append(chunk(b"IDAT", zstream[at:at + IDAT_BYTES]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def encode(pixels, stats=None):
    """the whole file"""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    channels = 1 if px.ndim == 2 else 3
    return frame_file(w, h, channels, zlib_stream(scanlines(px), stats))


def clamp16(result):
    """the mosaic's CV_16SC3 result_, as result8() clamps it"""
    return np.clip(np.asarray(result), 0, 255).astype(np.uint8)


STATIC_LTREE_LEN = STATIC_DTREE_LEN = None
BASE_LENGTH, LENGTH_CODE, STATIC_LTREE_LEN, STATIC_LTREE_CODE, STATIC_DTREE_LEN, STATIC_DTREE_CODE = _static_init()
