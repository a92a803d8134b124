"""The JPEG decoder's input lists: the fixtures of tests/golden/jpeg_decode/ (written by
tests/golden/make_jpeg_decode_golden.py through libjpeg-turbo, each with the pixels the library
decodes beside it), the files of tests/golden/jpeg/, files the host parser must refuse, and scans
the device must find corrupt.  Everything is derived from committed bytes: no Pillow in here."""
import glob
import os

import numpy as np

import jpeg_inputs as I

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_decode")

SIZES = [(1, 1), (3, 2), (4, 4), (5, 5), (7, 9), (17, 17), (33, 15), (129, 47)]
CONTENTS = ["noise", "checker"]
VARIANTS = ["444_q95", "422_q50", "420_q95_rst1", "420_q95_rst3", "420_q50_opt", "gray_q95_rst2"]


def fixture_names():
    return ["%s_%dx%d_%s" % (c, w, h, v) for (w, h) in SIZES for c in CONTENTS for v in VARIANTS]


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".jpg")


def fixture_bytes(name):
    with open(fixture_path(name), "rb") as f:
        return f.read()


def fixture_pixels(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["gray"], z["bgr"]


def fixtures_by_size():
    """{(w, h): [names]}: one decoder call per entry"""
    return {(w, h): ["%s_%dx%d_%s" % (c, w, h, v) for c in CONTENTS for v in VARIANTS] for (w, h) in SIZES}


def encoder_files_by_case():
    """[(case, [bytes at each quality of jpeg_inputs.QUALITIES])]: the 576 files of tests/golden/jpeg/,
    the four qualities of one input together (their scans differ by more than 10 x in length)"""
    out = []
    for case in I.cases():
        out.append((case, [open(I.golden_jpg(case, q), "rb").read() for q in I.QUALITIES]))
    return out


def all_encoder_files():
    return sorted(glob.glob(os.path.join(I.GOLDEN, "*.jpg")))


# ---------------------------------------------------------------------------
# files taken apart and put together again
# ---------------------------------------------------------------------------


def split(data):
    """-> [(marker, payload)] up to and including SOS, the entropy-coded bytes, the trailer (EOI)"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    p, segs = 2, []
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        segs.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9"
    return segs, data[p:-2], data[-2:]


def join(segs, scan, trailer=b"\xff\xd9", soi=b"\xff\xd8"):
    out = soi
    for m, pl in segs:
        n = len(pl) + 2
        out += bytes([0xFF, m, n >> 8, n & 255]) + bytes(pl)
    return out + bytes(scan) + trailer


def _edit(data, marker, fn, which=0):
    segs, scan, tr = split(data)
    k = [i for i, (m, _) in enumerate(segs) if m == marker][which]
    new = fn(segs[k][1])
    if new is None:
        del segs[k]
    else:
        segs[k] = new if isinstance(new, tuple) else (marker, new)
    return join(segs, scan, tr)


def refusals():
    """{what: (bytes, a word the refusal's text must contain)}: every file shape the issue lists"""
    colour = fixture_bytes("noise_17x17_420_q95_rst1")
    gray = fixture_bytes("noise_17x17_gray_q95_rst2")
    out = {}
    out["progressive"] = (_edit(colour, 0xC0, lambda pl: (0xC2, pl)), "SOF2")
    out["extended"] = (_edit(colour, 0xC0, lambda pl: (0xC1, pl)), "SOF1")
    out["arithmetic"] = (_edit(colour, 0xC0, lambda pl: (0xC9, pl)), "SOF9")
    out["lossless"] = (_edit(colour, 0xC0, lambda pl: (0xC3, pl)), "SOF3")
    out["12-bit"] = (_edit(colour, 0xC0, lambda pl: bytes([12]) + pl[1:]), "12-bit")
    out["4 components"] = (_edit(colour, 0xC0, lambda pl: pl[:5] + bytes([4]) + pl[6:] + bytes([4, 0x11, 1])),
                           "4 components")
    out["2 components"] = (_edit(colour, 0xC0, lambda pl: pl[:5] + bytes([2]) + pl[6:12]), "2 components")
    out["sampling 1x2"] = (_edit(colour, 0xC0, lambda pl: pl[:7] + bytes([0x12]) + pl[8:]), "sampling")
    out["sampling 4x1"] = (_edit(colour, 0xC0, lambda pl: pl[:7] + bytes([0x41]) + pl[8:]), "sampling")
    out["chroma 2x1"] = (_edit(colour, 0xC0, lambda pl: pl[:10] + bytes([0x21]) + pl[11:]), "sampling")
    out["16-bit DQT"] = (_edit(colour, 0xDB, lambda pl: bytes([0x10 | pl[0]]) + b"".join(
        bytes([0, v]) for v in pl[1:])), "16-bit")
    out["several scans"] = (_edit(colour, 0xDA, lambda pl: bytes([1]) + pl[1:3] + pl[-3:]), "several scans")
    out["spectral selection"] = (_edit(colour, 0xDA, lambda pl: pl[:-3] + bytes([0, 5, 0])), "sequential")
    adobe = b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])
    segs, scan, tr = split(colour)
    out["Adobe transform 0"] = (join(segs[:1] + [(0xEE, adobe)] + segs[1:], scan, tr), "Adobe")
    out["ids R G B"] = (_edit(_edit(colour, 0xC0, lambda pl: pl[:6] + b"R" + pl[7:9] + b"G" + pl[10:12] + b"B" + pl[13:]),
                              0xDA, lambda pl: pl[:1] + b"R" + pl[2:3] + b"G" + pl[4:5] + b"B" + pl[6:]), "R G B")
    out["missing DHT"] = (_edit(colour, 0xC4, lambda pl: None, which=1), "Huffman table")
    out["missing DQT"] = (_edit(colour, 0xDB, lambda pl: None, which=1), "quantisation table")
    out["missing DQT, gray"] = (_edit(gray, 0xDB, lambda pl: None), "quantisation table")
    out["no SOF0"] = (_edit(colour, 0xC0, lambda pl: None), "SOF0")
    out["no SOI"] = (colour[2:], "SOI")
    out["empty"] = (b"", "SOI")
    out["no SOS"] = (join(segs[:-1], b"", tr), "SOS")
    out["no EOI"] = (colour[:-2], "EOI")
    out["a second scan"] = (colour[:-2] + b"\xff\xda\x00\x02\xff\xd9", "behind the scan")
    out["no EOI, gray"] = (gray[:-1], "EOI")
    out["DNL height"] = (_edit(colour, 0xC0, lambda pl: pl[:1] + bytes([0, 0]) + pl[3:]), "height")
    out["DRI length"] = (_edit(colour, 0xDD, lambda pl: pl + b"\0"), "DRI")
    out["DHT table id 2"] = (_edit(colour, 0xC4, lambda pl: bytes([pl[0] | 2]) + pl[1:]), "DHT")
    out["DHT oversubscribed"] = (_edit(colour, 0xC4, lambda pl: pl[:1] + bytes([3]) + pl[2:]), "DHT")
    out["segment past the end"] = (colour[:40], "past the file")
    return out


def accepted_extras():
    """files with segments the parser must skip: -> {what: (bytes, same pixels as this fixture)}"""
    name = "noise_17x17_420_q95_rst1"
    segs, scan, tr = split(fixture_bytes(name))
    com = (0xFE, b"a comment \xff\xd9 with a marker in it")
    app1 = (0xE1, b"Exif\0\0" + bytes(range(64)))
    adobe1 = (0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1]))
    whole = fixture_bytes(name)
    return {"bytes behind EOI": (whole + b"\0\0padding \xff\xd9 \xff\xda \xff", name),
            "a second image behind EOI": (whole + fixture_bytes("noise_33x15_444_q95"), name),
            "COM and APP1": (join(segs[:1] + [com, app1] + segs[1:], scan, tr), name),
            "Adobe transform 1": (join(segs[:1] + [adobe1] + segs[1:], scan, tr), name)}


# ---------------------------------------------------------------------------
# scans the device must find corrupt (bounded code: each runs once)
# ---------------------------------------------------------------------------


# what tests/jpeg_decode_reference.py says of each (the device's texts: jpegd::status_text)
CORRUPT_REASONS = {"all-one bits": "undefined Huffman code", "scan cut in half": "the scan ends early",
                   "RST1 altered": "wrong or missing RST", "run past 63": "run past coefficient 63"}


def corrupt_scans():
    """{what: bytes}: files of 17 x 17 pixels the host parser accepts and the entropy walk must refuse"""
    out = {}
    # all-one bits: 0xFF 0x00 pairs are data bytes 0xFF; sixteen 1-bits are no code of the standard tables
    segs, scan, tr = split(fixture_bytes("noise_17x17_444_q95"))
    out["all-one bits"] = join(segs, b"\xff\x00" * (len(scan) // 2), tr)
    # half the scan, EOI re-appended (cut so that no 0xFF is left dangling in front of it)
    half = scan[:len(scan) // 2]
    while half.endswith(b"\xff"):
        half = half[:-1]
    out["scan cut in half"] = join(segs, half, tr)
    # a restart fixture with one RSTn index altered
    segs, scan, tr = split(fixture_bytes("noise_17x17_420_q95_rst1"))
    at = scan.index(b"\xff\xd1")
    out["RST1 altered"] = join(segs, scan[:at] + b"\xff\xd5" + scan[at + 2:], tr)
    return out


# ---------------------------------------------------------------------------
# the second fixture family, tests/golden/jpeg_decode/streams/: every legal stream shape, not only
# what one encoder writes.  Groups a to d are derived here from committed bytes (header and scan
# rewrites without re-encoding, hand-coded scans); group e is written by Pillow when the fixtures
# are made (tests/golden/make_jpeg_decode_golden.py).  Beside each .jpg an .npz holds the pixels
# libjpeg-turbo decodes from it.
# ---------------------------------------------------------------------------
STREAMS = os.path.join(GOLDEN, "streams")

# name -> base fixture: a 4:2:0 file with restart markers, a 4:4:4 file, a gray file with restart
# markers, and a 4:2:0 file without (for the rewrites that need a scan without RSTn)
HEADER_BASES = {"420rst": "noise_17x17_420_q95_rst1", "444": "noise_17x17_444_q95",
                "gray": "noise_17x17_gray_q95_rst2", "420": "noise_17x17_420_q50_opt"}
# the one stream whose file is larger than a committed fixture may be: its .jpg is built by the
# tests from stream_rewrites(), its .npz (libjpeg-turbo's pixels of those very bytes) is committed
BUILT_NOT_COMMITTED = ("a_app2_65533_444",)


def join_filled(segs, scan, trailer=b"\xff\xd9", fill=0):
    """join() with `fill` 0xFF fill bytes in front of every marker of the header (T.81 B.1.1.2)"""
    out = b"\xff\xd8"
    for m, pl in segs:
        n = len(pl) + 2
        out += b"\xff" * fill + bytes([0xFF, m, n >> 8, n & 255]) + bytes(pl)
    return out + bytes(scan) + trailer


def _dht_tables(pl):
    """one DHT payload -> [the payload of each table in it]"""
    out, q = [], 0
    while q < len(pl):
        n = 17 + sum(pl[q + 1:q + 17])
        out.append(bytes(pl[q:q + n]))
        q += n
    return out


def _map_segs(segs, marker, fn):
    return [(m, fn(pl)) if m == marker else (m, pl) for m, pl in segs]


def _sof_ids(pl, ids):
    pl = bytearray(pl)
    for c in range(pl[5]):
        pl[6 + 3 * c] = ids[c]
    return bytes(pl)


def _sos_ids(pl, ids):
    pl = bytearray(pl)
    for c in range(pl[0]):
        pl[1 + 2 * c] = ids[c]
    return bytes(pl)


def header_rewrites():
    """group a: {name: bytes}; the scan of the base fixture stays as it is"""
    out = {}
    for tag, base in HEADER_BASES.items():
        data = fixture_bytes(base)
        segs, scan, tr = split(data)
        gray = tag == "gray"
        has_rst = tag in ("420rst", "gray")
        if tag != "420":
            # all tables in one DHT and one DQT segment, as most cameras write them
            dht = b"".join(pl for m, pl in segs if m == 0xC4)
            dqt = b"".join(pl for m, pl in segs if m == 0xDB)
            merged, seen = [], set()
            for m, pl in segs:
                if m in (0xC4, 0xDB):
                    if m not in seen:
                        merged.append((m, dht if m == 0xC4 else dqt))
                        seen.add(m)
                else:
                    merged.append((m, pl))
            out["a_one_dht_one_dqt_" + tag] = join(merged, scan, tr)
            # DRI first, every table behind SOF0
            order = ([s for s in segs if s[0] == 0xE0] + [s for s in segs if s[0] == 0xDD] +
                     [s for s in segs if s[0] == 0xC0] + [s for s in segs if s[0] == 0xDB] +
                     [s for s in segs if s[0] == 0xC4] + [s for s in segs if s[0] == 0xDA])
            assert len(order) == len(segs)
            out["a_tables_behind_sof0_" + tag] = join(order, scan, tr)
            out["a_no_jfif_" + tag] = join([s for s in segs if s[0] != 0xE0], scan, tr)
            ids = [0, 1, 2]
            out["a_ids_012_" + tag] = join(_map_segs(_map_segs(segs, 0xC0, lambda pl: _sof_ids(pl, ids)),
                                                     0xDA, lambda pl: _sos_ids(pl, ids)), scan, tr)
            if not gray:
                ids = list(b"rgb")
                out["a_ids_rgb_lower_" + tag] = join(_map_segs(_map_segs(segs, 0xC0, lambda pl: _sof_ids(pl, ids)),
                                                               0xDA, lambda pl: _sos_ids(pl, ids)), scan, tr)
            # Huffman ids 0 <-> 1 in DHT and SOS

            def swap_dht(pl):
                return b"".join(bytes([t[0] ^ 1]) + t[1:] for t in _dht_tables(pl))

            def swap_sos(pl):
                pl = bytearray(pl)
                for c in range(pl[0]):
                    pl[2 + 2 * c] ^= 0x11
                return bytes(pl)
            out["a_huffman_ids_swapped_" + tag] = join(_map_segs(_map_segs(segs, 0xC4, swap_dht), 0xDA, swap_sos),
                                                       scan, tr)
            # quantisation tables 2 and 3

            def q23_dqt(pl):
                return b"".join(bytes([pl[q] + 2]) + pl[q + 1:q + 65] for q in range(0, len(pl), 65))

            def q23_sof(pl):
                pl = bytearray(pl)
                for c in range(pl[5]):
                    pl[8 + 3 * c] += 2
                return bytes(pl)
            out["a_quant_ids_2_3_" + tag] = join(_map_segs(_map_segs(segs, 0xDB, q23_dqt), 0xC0, q23_sof), scan, tr)
            # a DQT defined twice: the later definition holds
            first_q = [pl for m, pl in segs if m == 0xDB][0]
            decoy = (0xDB, first_q[:1] + bytes([1 + (k * 37) % 255 for k in range(64)]))
            out["a_dqt_twice_" + tag] = join(segs[:1] + [decoy] + segs[1:], scan, tr)
            # an APP1 that holds a whole JPEG file (a thumbnail), fill bytes between the segments
            out["a_app1_whole_jpeg_" + tag] = join(segs[:1] + [(0xE1, b"Exif\0\0" + fixture_bytes("noise_5x5_444_q95"))] +
                                                   segs[1:], scan, tr)
            out["a_fill_between_segments_" + tag] = join_filled(segs, scan, tr, fill=3)
        if tag == "444":
            out["a_app2_65533_444"] = join(segs[:1] + [(0xE2, bytes((k * 7 + (k >> 8)) & 255 for k in range(65533)))] +
                                           segs[1:], scan, tr)
        if not has_rst:
            # DRI larger than the MCU count, and DRI 0, on a scan without RSTn
            sos = [i for i, s in enumerate(segs) if s[0] == 0xDA][0]
            out["a_dri_60000_" + tag] = join(segs[:sos] + [(0xDD, bytes([60000 >> 8, 60000 & 255]))] + segs[sos:], scan, tr)
            out["a_dri_0_" + tag] = join(segs[:sos] + [(0xDD, b"\0\0")] + segs[sos:], scan, tr)
    return out


# header rewrites of one picture that must all decode to the same pixels: one call holds them all
def same_picture_variants(tag="420rst"):
    return [n for n in sorted(header_rewrites()) if n.endswith("_" + tag)]


def _rst_offsets(scan):
    return [k for k in range(len(scan) - 1) if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7]


def scan_rewrites():
    """group b: {name: bytes}; the header of the base fixture stays as it is"""
    out = {}
    segs, scan, tr = split(fixture_bytes("noise_33x15_420_q95_rst1"))
    rst = _rst_offsets(scan)
    assert len(rst) == 2
    for n in (1, 3):
        out["b_fill%d_before_one_rst" % n] = join(segs, scan[:rst[1]] + b"\xff" * n + scan[rst[1]:], tr)

    def fill_every(name, fill=1):
        s, sc, t = split(fixture_bytes(name))
        parts, at = [], 0
        for k in _rst_offsets(sc):
            parts.append(sc[at:k] + b"\xff" * fill)
            at = k
        return join(s, b"".join(parts) + sc[at:], t)
    out["b_fill1_before_every_rst_420"] = fill_every("noise_33x15_420_q95_rst1")
    out["b_fill2_before_every_rst_gray"] = fill_every("noise_129x47_gray_q95_rst2", 2)   # (50 markers: RST7 -> RST0)
    out["b_fill_before_eoi_420"] = join(segs, scan + b"\xff\xff", tr)
    s4, sc4, t4 = split(fixture_bytes("noise_33x15_444_q95"))
    out["b_fill_before_eoi_444"] = join(s4, sc4 + b"\xff", t4)
    # a fill byte in front of a stuffed 0xFF: 0xFF 0xFF 0x00 is the data byte 0xFF.  Here at the first
    # stuffed byte of the last 1536 bytes of the scan, where libjpeg-turbo decodes with
    # decode_mcu_slow (see ff_ff_00_at_619 below)
    sb, scb, tb = split(fixture_bytes("noise_129x47_444_q95"))
    at = scb.index(b"\xff\x00", len(scb) - 1536)
    assert at == 13659
    out["b_ff_ff_00_444"] = join(sb, scb[:at] + b"\xff" + scb[at:], tb)
    # ... and two in front of every stuffed 0xFF of a smaller file
    assert sc4.count(b"\xff\x00") >= 3
    out["b_ff_ff_ff_00_everywhere_444"] = join(s4, sc4.replace(b"\xff\x00", b"\xff\xff\xff\x00"), t4)
    # zero bytes between the last block and EOI: libjpeg skips them (8 and more lie beyond what a
    # refill reads ahead)
    for n in (1, 7, 8, 9, 20):
        out["b_trailing_%d_420" % n] = join(segs, scan + b"\0" * n, tr)
    # bytes between the end of an interval's data and its RSTn: libjpeg skips to the marker (more
    # than a refill reads ahead; with a stuffed 0xFF among them; in front of every RSTn)
    for n in (1, 9, 20):
        out["b_bytes_%d_before_one_rst" % n] = join(segs, scan[:rst[1]] + b"\0" * n + scan[rst[1]:], tr)
    out["b_bytes_with_ff_00_before_rst"] = join(segs, scan[:rst[0]] + b"\x55\xff\0\0" * 3 + b"\xff" + scan[rst[0]:], tr)
    sg, scg, tg = split(fixture_bytes("noise_33x15_gray_q95_rst2"))
    parts, at = [], 0
    for k in _rst_offsets(scg):
        parts.append(scg[at:k] + bytes([k & 127] * (9 + k % 5)))
        at = k
    out["b_bytes_before_every_rst_gray"] = join(sg, b"".join(parts) + scg[at:], tg)
    out["b_trailing_9_444"] = join(s4, sc4 + b"\0" * 9, t4)
    out["b_trailing_text_gray"] = join(*(split(fixture_bytes("noise_33x15_gray_q95_rst2"))[:2]) + (tr,)).replace(
        b"\xff\xd9", b"not a marker\xff\xd9")
    return out


def ff_ff_00_at_619():
    """-> (bytes, the fixture whose pixels it must give).  The same fill byte in front of the first
    stuffed 0xFF of noise_129x47_444_q95, at scan offset 619.  No .npz: libjpeg-turbo's pixels of
    this file are not libjpeg's rule.  Its decode_mcu_fast takes 0xFF 0xFF for a marker, gives the
    MCU up and decodes it again with decode_mcu_slow (jpeg_fill_bit_buffer: one data byte 0xFF)
    into coefficient blocks that the abandoned pass has already written to, so coefficients that
    are zero keep what that pass left: 55 of the 64 pixels of one block differ.  Within the last
    512 bytes per block of the MCU it uses decode_mcu_slow alone and gives the pixels of the file
    without the fill byte, as it does at 18 of the 42 stuffed bytes of this scan before that.  A
    fill byte carries no information (T.81 B.1.1.2), so the expected pixels are the base's."""
    name = "noise_129x47_444_q95"
    sb, scb, tb = split(fixture_bytes(name))
    at = scb.index(b"\xff\x00")
    assert at == 619
    return join(sb, scb[:at] + b"\xff" + scb[at:], tb), name


def flat_quant_rewrites():
    """group d: the quantisation tables replaced by all 8 and all 16: IDCT output up to +-1303, where
    libjpeg-turbo clamps and the C code's range table would wrap"""
    out = {}
    for tag, base in (("gray", "noise_33x15_gray_q95_rst2"), ("444", "noise_33x15_444_q95"),
                      ("420", "noise_33x15_420_q95_rst1")):
        segs, scan, tr = split(fixture_bytes(base))
        for q in (8, 16):
            out["d_quant_all_%d_%s" % (q, tag)] = join(_map_segs(
                segs, 0xDB, lambda pl: b"".join(pl[k:k + 1] + bytes([q]) * 64 for k in range(0, len(pl), 65))), scan, tr)
    return out


# ---------------------------------------------------------------------------
# hand-coded scans: a symbol-level writer
# ---------------------------------------------------------------------------


class ScanWriter(object):
    """Entropy-coded bytes from (table, symbol, extra bits): MSB first, a 0x00 stuffed behind every
    0xFF byte, the last byte padded with 1-bits (T.81 F.1.2.3).  A table is {symbol: (code, length)}."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, length):
        assert 0 <= value < (1 << length)
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def put(self, table, symbol, extra=0, nextra=0):
        code, length = table[symbol]
        self.bits(code, length)
        if nextra:
            self.bits(extra, nextra)

    def value(self, table, run, v):
        """the symbol run << 4 | size of v and v's bits (a negative v is coded as v - 1, low bits)"""
        size = int(abs(v)).bit_length()
        self.put(table, (run << 4) | size, v if v >= 0 else v + (1 << size) - 1, size)

    def bytes(self):
        if self.n:
            self.bits((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def table_codes(bits, vals):
    """canonical codes (T.81 annex C): {symbol: (code, length)}"""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# one code of each length 1..16 (0, 10, 110, ...): lengths 9..16 take the maxcode loop
LADDER_BITS = [1] * 16
# DC: the categories a baseline scan may use (0..11) at lengths 5..16; 12..15 are in the table, unused
LADDER_DC_VALS = [12, 13, 14, 15, 11, 10, 9, 8, 0, 1, 2, 3, 4, 5, 6, 7]
# AC: EOB 0x00, ZRL 0xF0, size 10 alone (0x0A) and behind a run of 14 (0xEA: zigzag 63 after three ZRL)
LADDER_AC_VALS = [0x01, 0x00, 0x02, 0x11, 0x03, 0x21, 0x12, 0x31, 0x04, 0x41, 0x13, 0xF0, 0x0A, 0xE1, 0xEA, 0x51]
HAND_W, HAND_H, HAND_Q = 96, 8, 2     # twelve blocks in a row, every quantiser 2


def hand_file(scan, width=HAND_W, height=HAND_H, q=HAND_Q):
    """a gray file around a hand-coded scan: DQT all q, the ladder tables as DC 0 and AC 0"""
    segs = [(0xDB, bytes([0]) + bytes([q]) * 64),
            (0xC0, bytes([8, height >> 8, height & 255, width >> 8, width & 255, 1, 1, 0x11, 0])),
            (0xC4, bytes([0x00] + LADDER_BITS + LADDER_DC_VALS)),
            (0xC4, bytes([0x10] + LADDER_BITS + LADDER_AC_VALS)),
            (0xDA, bytes([1, 1, 0x00, 0, 63, 0]))]
    return join(segs, scan)


def _hand_scan(blocks, nblocks=HAND_W // 8):
    """blocks: [fn(writer, dc, ac)]; the rest of the row is DC difference 0 and EOB"""
    dc, ac = table_codes(LADDER_BITS, LADDER_DC_VALS), table_codes(LADDER_BITS, LADDER_AC_VALS)
    w = ScanWriter()
    assert len(blocks) <= nblocks
    for k in range(nblocks):
        if k < len(blocks):
            blocks[k](w, dc, ac)
        else:
            w.value(dc, 0, 0)
            w.put(ac, 0x00)
    return w.bytes()


def hand_coded():
    """group c: {name: bytes}: blocks no encoder emits from pixels"""
    out = {}
    ZRL, EOB = 0xF0, 0x00

    # every code of both ladders: DC categories 0..11 (lengths 9..16 and 8..5) with the sign that
    # brings the predictor back towards 0, and the sixteen AC symbols in turn
    def ladder_block(i):
        def fn(w, dc, ac):
            mag = 0 if i == 0 else (1 << i) - 1 - (i % 3)
            w.value(dc, 0, mag if i % 2 else -mag)
            w.value(ac, 0, 1)                    # 0x01
            w.value(ac, 0, -3 if i % 2 else 2)   # 0x02
            w.value(ac, 1, -1)                   # 0x11
            w.value(ac, 0, 5 + (i % 3))          # 0x03
            w.value(ac, 2, 1)                    # 0x21
            w.value(ac, 1, -2)                   # 0x12
            w.value(ac, 3, -1)                   # 0x31
            w.value(ac, 0, -9 - (i % 7))         # 0x04
            w.value(ac, 4, 1)                    # 0x41
            w.value(ac, 1, 4 + (i % 4))          # 0x13
            w.put(ac, ZRL)
            w.value(ac, 0, 1023 - 40 * i if i % 2 else 40 * i - 1023)   # 0x0A
            w.value(ac, 5, -1)                   # 0x51
            w.value(ac, 14, 1 if i % 2 else -1)  # 0xE1
            w.put(ac, EOB)
        return fn
    out["c_ladder_every_length"] = hand_file(_hand_scan([ladder_block(i) for i in range(12)]))

    # DC category 11 with both signs: + 2047, - 2047, - 2047, + 2047 (the predictor: 2047, 0, -2047, 0)
    def dc11(v):
        def fn(w, dc, ac):
            w.value(dc, 0, v)
            w.put(ac, EOB)
        return fn
    out["c_dc_category_11"] = hand_file(_hand_scan([dc11(2047), dc11(-2047), dc11(-2047), dc11(2047),
                                                    dc11(1024), dc11(-1024)]))

    # AC size 10 with both signs at zigzag 63, behind three ZRL and a run of 14
    def ac10_at_63(v):
        def fn(w, dc, ac):
            w.value(dc, 0, 0)
            for _ in range(3):
                w.put(ac, ZRL)
            w.value(ac, 14, v)
        return fn
    out["c_ac_size_10_at_63"] = hand_file(_hand_scan([ac10_at_63(1023), ac10_at_63(-1023), ac10_at_63(512),
                                                      ac10_at_63(-512)]))

    # 63 AC coefficients and no EOB
    def full_block(sign):
        def fn(w, dc, ac):
            w.value(dc, 0, 3 * sign)
            for k in range(1, 64):
                v = 1 + (k % 3 == 0) + 2 * (k % 7 == 0)     # sizes 1, 2 and 3: 0x01, 0x02, 0x03
                w.value(ac, 0, v * sign if k % 2 else -v * sign)
        return fn
    out["c_63_coefficients_no_eob"] = hand_file(_hand_scan([full_block(1), full_block(-1), full_block(1)]))

    # three ZRL and then a coefficient at position 63 (size 1, both signs); a block in between
    def zrl3(v):
        def fn(w, dc, ac):
            w.value(dc, 0, 40 if v > 0 else -40)
            for _ in range(3):
                w.put(ac, ZRL)
            w.value(ac, 14, v)
        return fn
    out["c_three_zrl_then_63"] = hand_file(_hand_scan([zrl3(1), dc11(7), zrl3(-1)]))

    # a ZRL that carries the index past 63: libjpeg ends the block there (k = 49 + 16, and k = 60 + 16)
    def zrl_past(pre):
        def fn(w, dc, ac):
            w.value(dc, 0, 25)
            for _ in range(3):
                w.put(ac, ZRL)
            for _ in range(pre):
                w.value(ac, 4, -1)      # 53, 58: the index stands at 59 behind two of them
            w.put(ac, ZRL)
        return fn
    out["c_zrl_past_63"] = hand_file(_hand_scan([zrl_past(0), dc11(-50), zrl_past(2), dc11(9)]))
    return out


def run_past_63():
    """a refusal: a run with a non-zero size that ends past coefficient 63 (three ZRL: 49; run 4:
    53; run 4: 58; run 2: 61; run 2 from 62: 64).  Same size as the hand-coded fixtures."""
    def bad(w, dc, ac):
        w.value(dc, 0, 5)
        for _ in range(3):
            w.put(ac, 0xF0)
        w.value(ac, 4, 1)
        w.value(ac, 4, 1)
        w.value(ac, 2, 1)
        w.value(ac, 2, 1)
        w.put(ac, 0x00)
    return hand_file(_hand_scan([bad]))


def undefined_ladder_code():
    """a refusal: sixteen 1-bits, the one 16-bit pattern the ladder tables leave without a symbol"""
    def bad(w, dc, ac):
        w.value(dc, 0, -5)
        w.value(ac, 0, 1)
        w.bits(0xFFFF, 16)
    return hand_file(_hand_scan([bad]))


def wrong_rst_behind_stray_bytes():
    """a refusal: RST5 where RST1 is due, behind twelve stray bytes and two fill bytes (the search
    for the marker finds it; its index is wrong).  17 x 17, 4:2:0."""
    segs, scan, tr = split(fixture_bytes("noise_17x17_420_q95_rst1"))
    at = _rst_offsets(scan)[1]
    assert scan[at + 1] == 0xD1
    return join(segs, scan[:at] + b"\0\x55\xff\0" * 3 + b"\xff\xff\xff\xd5" + scan[at + 2:], tr)


# ---------------------------------------------------------------------------
# group e: Pillow-written files outside the shapes of VARIANTS x SIZES
# ---------------------------------------------------------------------------
E_WHOLE, E_THIN, E_LONG = [(8, 8), (16, 16), (16, 8), (32, 16)], [(2, 1), (1, 2), (3, 1), (4, 1), (5, 3)], [(2049, 1), (1, 2049)]
E_SAMPLINGS = {"444": 0, "422": 1, "420": 2, "gray": None}


def pillow_specs():
    """[(name, content, w, h, sampling, quality, restart, optimize)]; restart: None, ("blocks", n) or
    ("rows", n) (Pillow's restart_marker_blocks / restart_marker_rows: MCUs and MCU rows)"""
    out = []

    def add(content, size, samp, q, rst=None, opt=False):
        name = "e_%s_%dx%d_%s_q%d" % (content, size[0], size[1], samp, q)
        if rst:
            name += "_rst%s%d" % ("row" if rst[0] == "rows" else "", rst[1])
        if opt:
            name += "_opt"
        out.append((name, content, size[0], size[1], samp, q, rst, opt))
    # every size at every sampling, random content (the long sizes, whose pixels do not compress: two each)
    for size in E_WHOLE + E_THIN:
        for samp in ("444", "422", "420", "gray"):
            add("random", size, samp, 30)
    add("random", (2049, 1), "444", 30)
    add("random", (1, 2049), "422", 30)
    add("random", (1, 2049), "420", 30)
    # saturated 0 / 255 content at the two ends of the quality scale
    for size in ((16, 16), (5, 3)):
        for samp in ("444", "422", "gray"):
            for q in (1, 100):
                add("saturated", size, samp, q)
    for size in ((2, 1), (4, 1)):
        for samp in ("444", "422", "gray"):
            for q in (1, 100):
                add("saturated", size, samp, q)
    # restart intervals of 1, 7, one MCU row and more than the MCU count, where today's fixtures have none
    for size in ((32, 16), (5, 3)):
        for samp in ("444", "422"):
            for rst in (("blocks", 1), ("blocks", 7), ("rows", 1), ("blocks", 60000)):
                add("random", size, samp, 100, rst)
    for size in ((2, 1), (1, 2), (3, 1), (4, 1), (8, 8), (16, 8)):
        for samp in ("444", "422"):
            add("random", size, samp, 100, ("blocks", 1))
    for size in ((8, 8), (16, 8)):
        for samp in ("444", "422"):
            add("random", size, samp, 100, ("rows", 1))
    add("random", (2049, 1), "422", 30, ("blocks", 1))      # (129 MCUs: RST7 -> RST0 sixteen times)
    add("random", (1, 2049), "444", 30, ("blocks", 7))
    # a file's own Huffman tables
    for size in ((8, 8), (32, 16)):
        for samp in ("444", "422", "gray"):
            add("random", size, samp, 100, opt=True)
    add("random", (2049, 1), "gray", 30, opt=True)
    assert len(set(s[0] for s in out)) == len(out)
    return out


def stream_rewrites():
    """groups a to d: {name: bytes}, all derived from committed bytes"""
    out = {}
    for part in (header_rewrites(), scan_rewrites(), hand_coded(), flat_quant_rewrites()):
        assert not set(part) & set(out)
        out.update(part)
    return out


def stream_names():
    """the whole family, in the order the generator writes it"""
    return sorted(stream_rewrites()) + [s[0] for s in pillow_specs()]


def stream_path(name):
    return os.path.join(STREAMS, name + ".jpg")


_stream_bytes = {}


def stream_bytes(name):
    """the committed file; of BUILT_NOT_COMMITTED the bytes stream_rewrites() gives"""
    if name not in _stream_bytes:
        if name in BUILT_NOT_COMMITTED:
            _stream_bytes[name] = stream_rewrites()[name]
        else:
            with open(stream_path(name), "rb") as f:
                _stream_bytes[name] = f.read()
    return _stream_bytes[name]


def stream_pixels(name):
    z = np.load(os.path.join(STREAMS, name + ".npz"))
    return z["gray"], z["bgr"]


def sof0_size(data):
    """(width, height) of the file's own SOF0 (segment by segment: an APPn may hold another file)"""
    p = 2
    while True:
        assert data[p] == 0xFF
        if data[p + 1] == 0xFF:     # fill byte
            p += 1
            continue
        if data[p + 1] == 0xC0:
            return (data[p + 7] << 8) | data[p + 8], (data[p + 5] << 8) | data[p + 6]
        p += 2 + ((data[p + 2] << 8) | data[p + 3])


def streams_by_size():
    """{(w, h): [names]}: one decoder call per entry"""
    out = {}
    for name in stream_names():
        out.setdefault(sof0_size(stream_bytes(name)), []).append(name)
    return out
