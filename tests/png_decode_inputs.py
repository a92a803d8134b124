"""Inputs of the PNG decoder's tests.  Run as a script it is the GENERATOR of tests/golden/png_decode/:
every fixture as <name>.png with its expected pixels beside it in <name>.npz (gray, bgr), written
once and committed, so that no test depends on the local zlib's choice of bytes.  Imported, it hands
the committed files to the tests and builds, from its own writers alone (no zlib stream in them), the
files the host parser must refuse and the streams on which the device must report an error.

Three small writers: chunk() / png() for the container, filter_rows() forcing a filter type per row,
and DeflateWriter, which writes a deflate stream symbol by symbol (the analogue of ScanWriter in
tests/jpeg_decode_inputs.py).  Expected pixels come from Pillow and from zlib.decompress of the
concatenated IDAT plus tests/png_decode_reference.py's few lines of unfiltering; the generator
asserts that the restatement agrees with both, and that the family reaches every block type, filter
type, length code and distance code, a ring wrap, codes of 15 bits and every repeat count at its
edges."""
import os
import struct
import zlib

import numpy as np

import png_decode_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_decode")
MODE = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}


# ---- the container ---------------------------------------------------------------------------------
def chunk(ctype, payload=b"", crc=None):
    crc = zlib.crc32(ctype + payload) if crc is None else crc
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", crc & 0xFFFFFFFF)


def ihdr(w, h, ct, depth=8, comp=0, flt=0, lace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, comp, flt, lace))


def split_at(stream, cuts):
    """the stream cut at the given offsets -> list of pieces (an offset given twice: an empty piece)"""
    cuts = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def png(w, h, ct, stream, plte=None, pieces=None, before=(), between=(), tail=b""):
    """signature, IHDR, `before`, PLTE, `between`, the IDAT pieces, IEND, `tail`"""
    out = R.SIGNATURE + ihdr(w, h, ct) + b"".join(before)
    if plte is not None:
        out += chunk(b"PLTE", plte)
    out += b"".join(between)
    for piece in (pieces if pieces is not None else [stream]):
        out += chunk(b"IDAT", piece)
    return out + chunk(b"IEND") + tail


def zwrap(deflate, raw, cinfo=7):
    """a zlib stream around deflate data: CMF, FLG with a valid FCHECK, the Adler-32 of `raw`"""
    cmf = 8 | (cinfo << 4)
    flg = (31 - (cmf * 256) % 31) % 31
    return bytes([cmf, flg]) + deflate + struct.pack(">I", zlib.adler32(raw))


# ---- the filters -----------------------------------------------------------------------------------
def filter_rows(rows, bpp, types):
    """rows: (H, W * bpp) uint8; types: one filter type per row -> the filtered scanlines"""
    rows = np.asarray(rows, np.uint8)
    H, pitch = rows.shape
    out = bytearray()
    prev = np.zeros(pitch, np.int32)
    for y in range(H):
        cur = rows[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if pitch > bpp else np.zeros(pitch, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if pitch > bpp else np.zeros(pitch, np.int32)
        if pitch <= bpp:
            a = np.zeros(pitch, np.int32)
            c = np.zeros(pitch, np.int32)
        b = prev
        t = types[y]
        if t == 0:
            pred = 0
        elif t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


# ---- deflate, symbol by symbol -------------------------------------------------------------------------
def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lengths(n):
    """n >= 2 symbols -> a complete code of two neighbouring lengths (the longer ones last)"""
    k = n.bit_length() - 1
    longer = 2 * (n - (1 << k))
    return [k] * (n - longer) + [k + 1] * longer


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_LENS = [4] * 13 + [5] * 6          # all 19 symbols of the code-length code, complete


def match(length, dist, len_sym=None, dist_sym=None):
    """('m', length symbol, extra value, distance symbol, extra value); the canonical symbols unless given
    (length 258 can also be written as symbol 284 with all extra bits set)"""
    if len_sym is None:
        len_sym = 285 if length == 258 else max(s for s in range(257, 285) if R.LEN_BASE[s - 257] <= length)
    if dist_sym is None:
        dist_sym = max(s for s in range(30) if R.DIST_BASE[s] <= dist)
    le, de = length - R.LEN_BASE[len_sym - 257], dist - R.DIST_BASE[dist_sym]
    assert 0 <= le < (1 << R.LEN_EXTRA[len_sym - 257]) or le == 0, (length, len_sym)
    assert 0 <= de < (1 << R.DIST_EXTRA[dist_sym]) or de == 0, (dist, dist_sym)
    return ("m", len_sym, le, dist_sym, de)


def rle_ops(seq):
    """code lengths -> ops of the code-length alphabet, longest repeats first: (symbol, extra value)"""
    ops, i = [], 0
    while i < len(seq):
        v = seq[i]
        run = 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            n = min(run, 138)
            ops.append((18, n - 11))
        elif v == 0 and run >= 3:
            n = min(run, 10)
            ops.append((17, n - 3))
        elif v != 0 and run >= 4:
            ops.append((v, 0))
            n = 1 + min(run - 1, 6)
            ops.append((16, n - 1 - 3))
        else:
            n = 1
            ops.append((v, 0))
        i += n
    return ops


class DeflateWriter(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.stored_offsets = set()       # bit offsets (mod 8) at which a stored block's padding began

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):
        code, length = cl
        for k in range(length - 1, -1, -1):        # Huffman codes go in from their most significant bit
            self.bits((code >> k) & 1, 1)

    def stored(self, data, final=False, nlen=None):
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.stored_offsets.add(self.bitpos() % 8)
        if self.n:
            self.bits(0, 8 - self.n)
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data

    def _symbols(self, symbols, lit, dist):
        for s in symbols:
            if isinstance(s, tuple):
                _, ls, le, ds, de = s
                self.code(lit[ls])
                self.bits(le, R.LEN_EXTRA[ls - 257] if ls <= 285 else 0)
                self.code(dist[ds])
                self.bits(de, R.DIST_EXTRA[ds] if ds <= 29 else 0)
            else:
                self.code(lit[s])
        self.code(lit[256])

    def fixed(self, symbols, final=False):
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self._symbols(symbols, canonical(FIXED_LIT), canonical(FIXED_DIST))

    def dynamic(self, symbols, lit_lens, dist_lens, final=False, ops=None, hlit=None, hdist=None, cl_lens=None):
        """lit_lens: HLIT lengths (at least 257), dist_lens: HDIST lengths (at least 1); ops: how the
        lengths are written (default: rle_ops over both as one sequence)"""
        hlit = len(lit_lens) if hlit is None else hlit
        hdist = len(dist_lens) if hdist is None else hdist
        cl_lens = CL_LENS if cl_lens is None else cl_lens
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(19 - 4, 4)
        for s in R.CL_ORDER:
            self.bits(cl_lens[s], 3)
        clc = canonical(cl_lens)
        for sym, extra in (rle_ops(list(lit_lens) + list(dist_lens)) if ops is None else ops):
            self.code(clc[sym])
            if sym >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
        if symbols is not None:
            self._symbols(symbols, canonical(list(lit_lens)), canonical(list(dist_lens)))

    def finish(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


# ---- contents --------------------------------------------------------------------------------------
def image(content, w, h, bpp, seed=0):
    """(h, w * bpp) uint8"""
    rng = np.random.default_rng(1000 * w + 10 * h + bpp + seed)
    if content == "noise":
        return rng.integers(0, 256, (h, w * bpp), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w * bpp]
    if content == "ramp":
        return ((x * 3 + y * 5) & 255).astype(np.uint8)
    # smooth with a little noise: matches and literals both
    return (((x // max(bpp, 1)) * 2 + y * 3 + rng.integers(0, 3, (h, w * bpp))) & 255).astype(np.uint8)


def palette(n, seed=0):
    return np.random.default_rng(77 + n + seed).integers(0, 256, 3 * n, dtype=np.uint8).tobytes()


def zdeflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(raw) + c.flush()


def _cycle(h, start=0):
    return [(start + y) % 5 for y in range(h)]


# ---- the fixtures (generator only) -----------------------------------------------------------------
def _build_fixtures():
    """{name: bytes}"""
    out = {}

    def put(name, w, h, ct, rows, types, stream_of=None, plte=None, **kw):
        raw = filter_rows(rows, R.BPP[ct], types)
        stream = zdeflate(raw) if stream_of is None else stream_of(raw)
        assert zlib.decompress(stream) == raw, name
        out[name] = png(w, h, ct, stream, plte=plte, **kw)
        return raw, stream

    # sizes
    for (w, h) in [(1, 1), (1, 7), (7, 1), (2, 2), (17, 17), (64, 3), (129, 47)]:
        put("size_%dx%d_gray" % (w, h), w, h, 0, image("noise", w, h, 1), _cycle(h))
    put("noise_200x190_gray", 200, 190, 0, image("noise", 200, 190, 1), _cycle(190))
    # colour types; palettes of 1, 2 and 256 entries
    for (w, h) in [(129, 47), (1, 1)]:
        for ct in (0, 2, 3, 4, 6):
            n = 256 if w > 1 else 1
            rows = image("mixed", w, h, R.BPP[ct], seed=ct)
            if ct == 3:
                rows = (rows.astype(np.int32) % n).astype(np.uint8)
            put("ct%d_%dx%d" % (ct, w, h), w, h, ct, rows, _cycle(h, ct), plte=palette(n) if ct == 3 else None)
    put("palette2_17x17", 17, 17, 3, image("noise", 17, 17, 1) % 2, _cycle(17), plte=palette(2))
    # filters: each on every row, and cycling for every bpp (first-row and first-pixel cases)
    for t in range(5):
        put("filter%d_17x17_rgb" % t, 17, 17, 2, image("noise", 17, 17, 3, seed=t), [t] * 17)
    for ct in (0, 4, 2, 6):
        for start in (3, 4):     # Average and Paeth on the first row
            put("filter_cycle%d_17x17_bpp%d" % (start, R.BPP[ct]), 17, 17, ct, image("noise", 17, 17, R.BPP[ct], seed=9),
                _cycle(17, start))
    # zlib's own streams
    rows = image("mixed", 129, 47, 3, seed=5)
    variants = {"level0": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
                "fixed": dict(strategy=zlib.Z_FIXED), "rle": dict(strategy=zlib.Z_RLE),
                "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY), "filtered": dict(strategy=zlib.Z_FILTERED),
                "wbits9": dict(wbits=9)}
    for name, kw in variants.items():
        put("z_%s_129x47_rgb" % name, 129, 47, 2, rows, _cycle(47), stream_of=lambda raw, kw=kw: zdeflate(raw, **kw))
    # Pillow's writer
    try:
        import io
        from PIL import Image
        for name, kw in (("pillow_default", {}), ("pillow_optimize", dict(optimize=True))):
            buf = io.BytesIO()
            Image.fromarray(rows.reshape(47, 129, 3), "RGB").save(buf, "PNG", **kw)
            out["%s_129x47_rgb" % name] = buf.getvalue()
    except ImportError:
        pass
    # IDAT splits
    rows = image("mixed", 64, 3, 3, seed=2)
    raw = filter_rows(rows, 3, [4, 3, 1])
    stream = zdeflate(raw)
    assert (stream[2] >> 1) & 3 == 2      # a dynamic block: its header takes far more than 4 bytes
    out["idat_one_64x3_rgb"] = png(64, 3, 2, stream)
    out["idat_bytes_64x3_rgb"] = png(64, 3, 2, stream, pieces=[stream[k:k + 1] for k in range(len(stream))])
    out["idat_in_header_64x3_rgb"] = png(64, 3, 2, stream, pieces=split_at(stream, [1, 6]))
    out["idat_empty_piece_64x3_rgb"] = png(64, 3, 2, stream, pieces=split_at(stream, [40, 40, len(stream) - 3]))
    # chunk-level shapes
    text = chunk(b"tEXt", b"Comment\0" + bytes(64992))
    assert len(text) == 65012
    out["chunks_ancillary_17x17_p"] = png(
        17, 17, 3, zwrap_rows(image("noise", 17, 17, 1) % 2, 1, _cycle(17)), plte=palette(2),
        before=[chunk(b"gAMA", struct.pack(">I", 45455), crc=12345), chunk(b"sRGB", b"\0")],
        between=[chunk(b"tRNS", b"\x00\xff"), text, chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))],
        tail=b"bytes behind IEND" + bytes(40))
    out.update(_hand_coded())
    return out


def zwrap_rows(rows, bpp, types):
    return zdeflate(filter_rows(rows, bpp, types))


def _literal_dynamic(w, raw, final=True):
    """raw as literals in one dynamic block over all 286 / 30 symbols"""
    w.dynamic(list(raw), complete_lengths(286), complete_lengths(30), final=final)


def _hand_coded():
    out = {}
    rng = np.random.default_rng(4242)
    # 1. length 258 at distance 32768, on 200 x 190 gray (38 190 bytes of scanlines, filter None)
    raw = bytearray(rng.integers(0, 256, 38190, dtype=np.uint8).tobytes())
    for p in range(0, 38190, 201):
        raw[p] = 0
    raw[196] = 0                       # lands on a filter byte of the copy: 32768 + 196 = 164 * 201
    raw[32768:32768 + 258] = raw[0:258]
    for p in range(0, 38190, 201):
        assert raw[p] <= 4
    w = DeflateWriter()
    w.dynamic(list(raw[:32768]) + [match(258, 32768)] + list(raw[32768 + 258:]), complete_lengths(286),
              complete_lengths(30), final=True)
    out["hand_len258_dist32768_200x190_gray"] = png(200, 190, 0, zwrap(w.finish(), bytes(raw)))
    # 2. every length code and every distance code, extra bits all zeros and all ones; bytes 0..4
    # everywhere, so that whatever a copy puts on a filter byte is a filter type
    raw = bytearray(rng.integers(0, 5, 32768, dtype=np.uint8).tobytes())
    syms = list(raw)
    lens_list = [(s, e) for s in range(257, 286) for e in (0, (1 << R.LEN_EXTRA[s - 257]) - 1)]
    dist_list = [(s, e) for s in range(30) for e in (0, (1 << R.DIST_EXTRA[s]) - 1)]
    for k, (ds, de) in enumerate(dist_list):
        ls, le = lens_list[k % len(lens_list)]
        ln, d = R.LEN_BASE[ls - 257] + le, R.DIST_BASE[ds] + de
        syms.append(("m", ls, le, ds, de))
        start = len(raw) - d
        for i in range(ln):
            raw.append(raw[start + (i if d >= ln else i % d)])
    fill = 38190 - len(raw)
    assert fill > 0
    tail = rng.integers(0, 5, fill, dtype=np.uint8).tobytes()
    raw += tail
    syms += list(tail)
    w = DeflateWriter()
    w.dynamic(syms, complete_lengths(286), complete_lengths(30), final=True)
    out["hand_all_codes_200x190_gray"] = png(200, 190, 0, zwrap(w.finish(), bytes(raw)))
    # 3. distance 1 with lengths 258 and 3: runs of zeros (17 x 17 gray: 306 bytes)
    raw = bytes(306)
    w = DeflateWriter()
    w.fixed([0, match(258, 1), match(3, 1)] + [0] * 44, final=True)
    out["hand_dist1_runs_17x17_gray"] = png(17, 17, 0, zwrap(w.finish(), raw))
    # 4. a dynamic block with one distance code (one bit, RFC 1951 3.2.7), and one with none
    lit = [0] * 286
    lit[0], lit[256], lit[285], lit[257] = 1, 2, 3, 3
    w = DeflateWriter()
    w.dynamic([0, match(258, 1), match(3, 1)] + [0] * 44, lit, [1], final=True)
    out["hand_one_dist_code_17x17_gray"] = png(17, 17, 0, zwrap(w.finish(), raw))
    rows = image("noise", 17, 17, 1, seed=3)
    raw = filter_rows(rows, 1, [0] * 17)
    w = DeflateWriter()
    w.dynamic(list(raw), complete_lengths(257), [0], final=True)
    out["hand_no_dist_code_17x17_gray"] = png(17, 17, 0, zwrap(w.finish(), raw))
    # 5. code lengths up to 15: literals 0..14 and the end of block on a chain 1, 2, .., 14, 15, 15
    rows = (rng.integers(0, 15, (17, 17))).astype(np.uint8)
    raw = filter_rows(rows, 1, [0] * 17)
    lit = [0] * 257
    for s in range(14):
        lit[s] = s + 1
    lit[14] = lit[256] = 15
    w = DeflateWriter()
    w.dynamic(list(raw), lit, [0], final=True)
    out["hand_len15_codes_17x17_gray"] = png(17, 17, 0, zwrap(w.finish(), raw))
    # 6. repeat codes at their smallest and largest counts, and a 16 that runs from the literal lengths
    # into the distance lengths
    lit = [0] * 286
    for s in range(7):
        lit[s] = 6
    for s in range(145, 149):
        lit[s] = 5
    lit[160] = lit[171] = 8
    lit[256] = 7
    lit[283] = lit[284] = lit[285] = 2
    dist = [2, 2, 2, 2]
    ops = [(6, 0), (16, 3), (18, 127), (5, 0), (16, 0), (18, 0), (8, 0), (17, 7), (8, 0), (17, 0)]
    ops += [(0, 0)] * 81 + [(7, 0)] + [(0, 0)] * 26 + [(2, 0), (16, 2), (2, 0)]
    alphabet = np.array(list(range(7)) + list(range(145, 149)) + [160, 171], np.uint8)
    rows = alphabet[rng.integers(0, len(alphabet), (17, 17))]
    raw = filter_rows(rows, 1, [0] * 17)
    w = DeflateWriter()
    w.dynamic(list(raw), lit, dist, final=True, ops=ops)
    out["hand_repeats_17x17_gray"] = png(17, 17, 0, zwrap(w.finish(), raw))
    # 7. blocks: an empty fixed block that is not the last in front of the data, an empty stored block,
    # one of 65535 bytes, a stored block entered at each of the 8 bit offsets, a dynamic block, a fixed
    # one: 256 x 256 gray, 65 792 bytes of scanlines
    y, x = np.mgrid[0:256, 0:256]
    rows = (144 + ((x * 7 + y * 13) % 112)).astype(np.uint8)     # (literals of 9 bits in the fixed code)
    raw = filter_rows(rows, 1, [0] * 256)
    w = DeflateWriter()
    w.fixed([])
    w.stored(b"")
    w.stored(raw[:65535])
    at = 65535
    for k in range(8):
        guard = 0
        while (w.bitpos() + 3) % 8 != k:
            w.fixed([raw[at]])          # 18 or 19 bits: shifts the offset
            at += 1
            guard += 1
            assert guard < 32
        w.stored(raw[at:at + 7])
        at += 7
    assert w.stored_offsets == set(range(8)), w.stored_offsets
    _literal_dynamic(w, raw[at:at + 60], final=False)
    at += 60
    w.fixed(list(raw[at:]), final=True)
    out["hand_blocks_256x256_gray"] = png(256, 256, 0, zwrap(w.finish(), raw))
    return out


# ---- built in memory: what must be refused, what the device must report ----------------------------------
def _base():
    """17 x 17 RGB, Paeth, literals in fixed blocks: (raw, zlib stream, file)"""
    rows = image("noise", 17, 17, 3, seed=11)
    raw = filter_rows(rows, 3, [4] * 17)
    w = DeflateWriter()
    w.fixed(list(raw), final=True)
    stream = zwrap(w.finish(), raw)
    return raw, stream, png(17, 17, 2, stream)


def good_17x17():
    """a good frame to stand beside the bad ones"""
    return _base()[2]


def refusals():
    """{what: (file bytes, a word the refusal's text must contain)}"""
    raw, stream, good = _base()
    body = lambda *chunks: R.SIGNATURE + b"".join(chunks)
    idat, iend = chunk(b"IDAT", stream), chunk(b"IEND")
    out = {}
    for depth in (1, 2, 4, 16):
        out["bit depth %d" % depth] = (body(ihdr(17, 17, 0, depth=depth), idat, iend), "bit depth %d" % depth)
    out["Adam7"] = (body(ihdr(17, 17, 2, lace=1), idat, iend), "Adam7")
    out["colour type 5"] = (body(ihdr(17, 17, 5), idat, iend), "colour type 5")
    out["width 0"] = (body(ihdr(0, 17, 2), idat, iend), "width or height")
    out["height 65536"] = (body(ihdr(17, 65536, 2), idat, iend), "width or height")
    out["compression method 1"] = (body(ihdr(17, 17, 2, comp=1), idat, iend), "compression method")
    out["filter method 1"] = (body(ihdr(17, 17, 2, flt=1), idat, iend), "filter method")
    out["bad signature"] = (b"\x89PNG\r\n\x1a\r" + good[8:], "signature")
    out["IHDR not first"] = (body(chunk(b"gAMA", bytes(4)), ihdr(17, 17, 2), idat, iend), "IHDR is not the first")
    out["IHDR of 12 bytes"] = (body(chunk(b"IHDR", bytes(12)), idat, iend), "IHDR: length 12")
    out["bad CRC on IHDR"] = (body(chunk(b"IHDR", struct.pack(">IIBBBBB", 17, 17, 8, 2, 0, 0, 0), crc=1), idat, iend),
                              "IHDR: bad CRC")
    out["bad CRC on PLTE"] = (body(ihdr(17, 17, 2), chunk(b"PLTE", bytes(6), crc=1), idat, iend), "PLTE: bad CRC")
    out["bad CRC on IDAT"] = (body(ihdr(17, 17, 2), chunk(b"IDAT", stream, crc=1), iend), "IDAT: bad CRC")
    out["bad CRC on IEND"] = (body(ihdr(17, 17, 2), idat, chunk(b"IEND", crc=1)), "IEND: bad CRC")
    out["missing PLTE"] = (body(ihdr(17, 17, 3), idat, iend), "without a PLTE")
    out["empty PLTE"] = (body(ihdr(17, 17, 3), chunk(b"PLTE"), idat, iend), "PLTE: length 0")
    out["PLTE of 7 bytes"] = (body(ihdr(17, 17, 3), chunk(b"PLTE", bytes(7)), idat, iend), "PLTE: length 7")
    out["PLTE of 771 bytes"] = (body(ihdr(17, 17, 3), chunk(b"PLTE", bytes(771)), idat, iend), "PLTE: length 771")
    out["missing IDAT"] = (body(ihdr(17, 17, 2), iend), "no IDAT")
    out["missing IEND"] = (body(ihdr(17, 17, 2), idat), "no IEND")
    out["IDAT run interrupted"] = (body(ihdr(17, 17, 2), chunk(b"IDAT", stream[:50]), chunk(b"tEXt", b"a\0b"),
                                        chunk(b"IDAT", stream[50:]), iend), "interrupted")
    out["truncated chunk"] = (good[:len(good) - 20], "IDAT: truncated")
    out["truncated chunk header"] = (good[:8 + 25 + 5], "truncated chunk header")
    out["length past the file"] = (body(ihdr(17, 17, 2), struct.pack(">I", 0x7FFFFFF0) + b"IDAT" + stream, iend),
                                   "length runs past the file")
    out["unknown critical chunk"] = (body(ihdr(17, 17, 2), chunk(b"ABCD", b"x"), idat, iend), "critical chunk ABCD")
    bad = lambda b0, b1: body(ihdr(17, 17, 2), chunk(b"IDAT", bytes([b0, b1]) + stream[2:]), iend)
    out["zlib CM 7"] = (bad(0x77, 0x09), "compression method 7")
    out["zlib CINFO 8"] = (bad(0x88, 0x1C), "CINFO 8")
    out["zlib FCHECK"] = (bad(0x78, 0x02), "FCHECK")
    out["zlib FDICT"] = (bad(0x78, 0x20), "FDICT")
    out["IDAT of 5 bytes"] = (body(ihdr(17, 17, 2), chunk(b"IDAT", stream[:5]), iend), "no zlib stream")
    return out


def device_errors():
    """{what: (file bytes 17 x 17, the reason's text)}: the header is fine, the device finds the error"""
    raw, stream, good = _base()
    S = R.STATUS
    out = {}

    def rgb(deflate, adler_of=raw):
        return png(17, 17, 2, zwrap(deflate, adler_of))

    def fixed(symbols):
        w = DeflateWriter()
        w.fixed(symbols, final=True)
        return w.finish()

    w = DeflateWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w._symbols([raw[0], 286], canonical(FIXED_LIT), canonical(FIXED_DIST))
    out["symbol 286"] = (rgb(w.finish()), S["bad_code"])
    lit = [0] * 258
    lit[0], lit[256], lit[257] = 1, 2, 2
    w = DeflateWriter()
    w.dynamic(None, lit, [1], final=True)
    w.code(canonical(lit)[0])
    w.code(canonical(lit)[257])
    w.bits(1, 1)                        # the distance code has one pattern, "0": this is the other one
    out["undefined distance pattern"] = (rgb(w.finish() + bytes(8)), S["bad_code"])
    w = DeflateWriter()
    w.dynamic(None, [1, 1, 1] + [0] * 253 + [2], [0], final=True)
    out["over-subscribed lengths"] = (rgb(w.finish()), S["over_subscribed"])
    w = DeflateWriter()
    w.dynamic(None, [2] + [0] * 255 + [2], [0], final=True)
    out["incomplete lengths"] = (rgb(w.finish()), S["incomplete"])
    w = DeflateWriter()
    w.dynamic(None, [1] + [0] * 255 + [1], [2, 2], final=True)
    out["incomplete distance lengths"] = (rgb(w.finish()), S["incomplete"])
    w = DeflateWriter()
    w.dynamic(None, [1] * 257, [0], final=True, ops=[(16, 0)])
    out["repeat without a previous length"] = (rgb(w.finish()), S["bad_dyn_header"])
    w = DeflateWriter()
    w.dynamic(None, [0] * 257, [0], final=True, ops=[(18, 127), (18, 110)])
    out["repeat past HLIT + HDIST"] = (rgb(w.finish()), S["bad_dyn_header"])
    w = DeflateWriter()
    w.dynamic(None, [1, 1] + [0] * 255, [0], final=True)
    out["no end-of-block code"] = (rgb(w.finish()), S["bad_dyn_header"])
    w = DeflateWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    out["BTYPE 3"] = (rgb(w.finish() + bytes(8)), S["bad_block_type"])
    w = DeflateWriter()
    w.stored(raw, final=True, nlen=len(raw))
    out["LEN != ~NLEN"] = (rgb(w.finish()), S["bad_stored_len"])
    out["distance behind the start"] = (rgb(fixed([raw[0], match(3, 2)] + list(raw[4:]))), S["dist_too_far"])
    out["stream cut in half"] = (rgb(fixed(list(raw))[:400]), S["ends_early"])
    w = DeflateWriter()
    w.stored(raw, final=True)
    out["stored block cut short"] = (rgb(w.finish()[:300]), S["ends_early"])
    out["six bytes short"] = (rgb(fixed(list(raw[:-6]))), S["too_short"])
    out["one byte long"] = (rgb(fixed(list(raw) + [0])), S["too_long"])
    w = DeflateWriter()
    w.fixed(list(raw), final=False)
    w.stored(b"surplus", final=True)
    out["a surplus block"] = (rgb(w.finish()), S["too_long"])
    bad = bytearray(raw)
    bad[5 * 52] = 5
    out["filter type 5"] = (rgb(fixed(list(bad)), bytes(bad)), S["bad_filter"])
    out["Adler-32 off by one"] = (png(17, 17, 2, stream[:-1] + bytes([stream[-1] ^ 1])), S["bad_adler"])
    rows = image("noise", 17, 17, 1, seed=12) % 2
    rows[9, 9] = 2
    praw = filter_rows(rows, 1, [0] * 17)
    out["palette index 2 of 2"] = (png(17, 17, 3, zwrap(fixed(list(praw)), praw), plte=palette(2)), S["bad_index"])
    return out


# ---- the committed files ------------------------------------------------------------------------------
def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".png"))


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".png")


def fixture_bytes(name):
    with open(fixture_path(name), "rb") as f:
        return f.read()


def fixture_pixels(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["gray"], z["bgr"]


def fixtures_by_size():
    """{(w, h): [names]}: one decoder call per entry"""
    out = {}
    for n in fixture_names():
        w, h = struct.unpack(">II", fixture_bytes(n)[16:24])
        out.setdefault((w, h), []).append(n)
    return out


def pillow_pixels(data):
    """-> (gray or None, bgr) as Pillow decodes the file; gray only for gray files (the rule for colour
    files is libpng's, not Pillow's)"""
    import io
    from PIL import Image, ImageFile
    before = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True      # (Pillow then skips an ancillary chunk's bad CRC, as the decoder does)
    try:
        im = Image.open(io.BytesIO(data))
        im.load()
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = before
    bgr = np.array(im.convert("RGB"))[:, :, ::-1]
    gray = np.array(im.convert("L")) if im.mode in ("L", "LA") else None
    return gray, bgr


def generate():
    os.makedirs(GOLDEN, exist_ok=True)
    total = R.Counters()
    files = _build_fixtures()
    for name, data in sorted(files.items()):
        d = R.decode(data)
        h = d.header
        # the real libraries: zlib for the scanlines, Pillow for the pixels
        assert zlib.decompress(h.stream) == d.raw, name
        gray, bgr = pillow_pixels(data)
        assert np.array_equal(bgr, d.bgr), name
        if gray is not None:
            assert np.array_equal(gray, d.gray), name
        total.add(d.counters)
        assert len(data) <= 100000, (name, len(data))
        with open(fixture_path(name), "wb") as f:
            f.write(data)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), gray=d.gray, bgr=d.bgr)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 100000, name
    check_coverage(total)
    print("wrote %d fixtures to %s" % (len(files), GOLDEN))


def check_coverage(c):
    assert all(c.blocks), c.blocks
    assert all(c.filters), c.filters
    assert c.length_codes == set(range(257, 286)), sorted(set(range(257, 286)) - c.length_codes)
    assert c.dist_codes == set(range(30)), sorted(set(range(30)) - c.dist_codes)
    assert c.ring_wraps >= 3
    assert c.max_code_length == 15 and c.long_codes > 0
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= c.repeats, sorted(c.repeats)
    assert c.repeat_crossed and c.single_dist_code and c.no_dist_code and c.overlapping
    assert c.paeth_picks == {"a", "b", "c", "a tie", "b tie"}, c.paeth_picks
    assert c.average_carry > 0


if __name__ == "__main__":
    generate()
