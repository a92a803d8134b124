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
                   "RST1 altered": "wrong or missing RST"}


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
