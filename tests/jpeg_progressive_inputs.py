"""The progressive JPEG decoder's input lists (tests/golden/jpeg_progressive/, written by
tests/golden/make_jpeg_progressive_golden.py; beside each .jpg an .npz of libjpeg-turbo's pixels):

  A  files Pillow writes with libjpeg-turbo's default script (DC with Al = 1 interleaved, split Y
     bands, refinements): three contents, six sizes, seven variants
  B  files of the symbol-level ProgressiveWriter below: the coefficients of baseline fixtures under
     scripts no encoder picks.  Same coefficients, same pixels as the baseline fixture's .npz
  C  two large gray files: an AC scan of one EOB run of 32 767 and one of 1, and EOB runs of every
     category 0..13 in a first and in a refinement scan
  D  refusals(): one file per rule of the host parser
  E  corrupt_scans(): the five statuses of the device, each a 17 x 17 file the parser accepts

B to E are derived here from committed bytes: no Pillow in here."""
import os

import numpy as np

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
from jpeg_reference import ZIGZAG

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_progressive")

# ---------------------------------------------------------------------------
# A: Pillow-written
# ---------------------------------------------------------------------------
A_SIZES = [(1, 1), (3, 2), (7, 9), (17, 17), (33, 15), (129, 47)]
A_CONTENTS = {"noise": "noise", "checker": "checker", "gradient": "ramp"}     # name -> jpeg_inputs content
# name: channels, Pillow's subsampling, quality, restart keyword or None
A_VARIANTS = {
    "444_q95": (3, 0, 95, None),
    "422_q50": (3, 1, 50, None),
    "420_q95": (3, 2, 95, None),
    "420_q95_rst1": (3, 2, 95, ("restart_marker_blocks", 1)),
    "444_q50_rstrow1": (3, 0, 50, ("restart_marker_rows", 1)),
    "gray_q95_rst2": (1, None, 95, ("restart_marker_blocks", 2)),
    "gray_q20": (1, None, 20, None),
}


def a_names():
    return ["a_%s_%dx%d_%s" % (c, w, h, v) for (w, h) in A_SIZES for c in A_CONTENTS for v in A_VARIANTS]


# ---------------------------------------------------------------------------
# the writer: quantised coefficients + a scan script -> a file
# ---------------------------------------------------------------------------


def optimal_table(freq):
    """jpeg_gen_optimal_table (jchuff.c; T.81 K.2): {symbol: count} -> (bits[16], vals).  No code is
    all ones (the reserved symbol 256), none longer than 16 bits."""
    f = [0] * 257
    for s, n in freq.items():
        f[s] = n
    f[256] = 1
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 300
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(299, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for length in range(1, 300) for s in range(256) if codesize[s] == length]
    return bits[1:17], vals


def _seg(marker, payload):
    n = len(payload) + 2
    return bytes([0xFF, marker, n >> 8, n & 255]) + bytes(payload)


def dqt_payload(tq, table):
    """table: natural order"""
    return bytes([tq]) + bytes(int(table[int(ZIGZAG[z])]) for z in range(64))


class ProgressiveWriter(object):
    """comps: [(id, h, v, tq)]; qtables {tq: natural-order 64}; coefs: per component (blocks down,
    blocks across, 64), natural order, whole MCUs.  write(script) -> bytes.  A script is a list of
      ("scan", dict(comps=[indices], ss, se, ah, al, td=[DC table id per component], ta=AC table id,
                    eob="max" or "one", tokens=None or the scan's tokens by hand, sos=None or the
                    SOS payload to write in place of the true one, rst_fill=0xFF bytes in front of
                    every RSTn, tail=bytes behind the scan's last bit, dht=True))
      ("dri", n)  ("seg", marker, payload)  ("raw", bytes)
    A scan's Huffman tables are made for its own symbols (optimal_table) and written in a DHT in
    front of its SOS under the ids the scan names, so every scan redefines its tables.  Tokens are
    ("sym", class, slot, symbol, extra, nextra), ("bits", value, n) and ("rst",)."""

    def __init__(self, width, height, comps, qtables, coefs, jfif=True):
        self.width, self.height, self.comps, self.qtables, self.coefs = width, height, comps, qtables, coefs
        self.jfif = jfif
        self.hmax = max(c[1] for c in comps) if len(comps) > 1 else 1
        self.vmax = max(c[2] for c in comps) if len(comps) > 1 else 1

    def head(self, marker=0xC2):
        out = b"\xff\xd8"
        if self.jfif:
            out += _seg(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0")
        for tq in sorted(self.qtables):
            out += _seg(0xDB, dqt_payload(tq, self.qtables[tq]))
        sof = bytes([8, self.height >> 8, self.height & 255, self.width >> 8, self.width & 255, len(self.comps)])
        for (cid, h, v, tq) in self.comps:
            sof += bytes([cid, (h << 4) | v, tq])
        return out + _seg(marker, sof)

    # ---- the scan's blocks in the order it codes them ---------------------------------------------
    def mcus(self, comps):
        """-> [[(slot, block)] per MCU]"""
        if len(comps) == 1:
            c = comps[0]
            h, v = (self.comps[c][1], self.comps[c][2]) if len(self.comps) > 1 else (1, 1)
            nx = -(-(-(-self.width * h // self.hmax)) // 8)
            ny = -(-(-(-self.height * v // self.vmax)) // 8)
            return [[(0, self.coefs[c][y, x])] for y in range(ny) for x in range(nx)]
        mcux = -(-self.width // (8 * self.hmax))
        mcuy = -(-self.height // (8 * self.vmax))
        out = []
        for my in range(mcuy):
            for mx in range(mcux):
                m = []
                for slot, c in enumerate(comps):
                    h, v = self.comps[c][1], self.comps[c][2]
                    for by in range(v):
                        for bx in range(h):
                            m.append((slot, self.coefs[c][my * v + by, mx * h + bx]))
                out.append(m)
        return out

    # ---- jcphuff.c: encode_mcu_DC_first, _DC_refine, _AC_first, _AC_refine -> tokens -----------------
    def tokens(self, s, restart):
        zz = [int(v) for v in ZIGZAG]
        ss, se, ah, al = s["ss"], s["se"], s["ah"], s["al"]
        one = s.get("eob", "max") == "one"
        out = []
        st = dict(eobrun=0, be=[])

        def emit_eobrun():
            if st["eobrun"] > 0:
                nb = st["eobrun"].bit_length() - 1
                out.append(("sym", 1, 0, nb << 4, st["eobrun"] & ((1 << nb) - 1), nb))
                st["eobrun"] = 0
                for b in st["be"]:
                    out.append(("bits", b, 1))
                st["be"] = []

        pred = [0] * len(s["comps"])
        for i, mcu in enumerate(self.mcus(s["comps"])):
            if restart and i and i % restart == 0:
                emit_eobrun()
                out.append(("rst",))
                pred = [0] * len(s["comps"])
            for slot, blk in mcu:
                if ss == 0 and ah == 0:
                    v = int(blk[0]) >> al                      # (the point transform of DC: an arithmetic shift)
                    d = v - pred[slot]
                    pred[slot] = v
                    size = abs(d).bit_length()
                    out.append(("sym", 0, slot, size, d if d >= 0 else d + (1 << size) - 1, size))
                elif ss == 0:
                    out.append(("bits", (int(blk[0]) >> al) & 1, 1))
                elif ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        c = int(blk[zz[k]])
                        a = abs(c) >> al                       # (of AC: the magnitude, towards zero)
                        if a == 0:
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            out.append(("sym", 1, 0, 0xF0, 0, 0))
                            r -= 16
                        size = a.bit_length()
                        out.append(("sym", 1, 0, (r << 4) | size, a if c >= 0 else (~a) & ((1 << size) - 1), size))
                        r = 0
                    if r > 0:
                        st["eobrun"] += 1
                        if st["eobrun"] == 0x7FFF or one:
                            emit_eobrun()
                else:
                    av = [abs(int(blk[zz[k]])) >> al for k in range(64)]
                    eob = max([k for k in range(ss, se + 1) if av[k] == 1] or [0])
                    r, br = 0, []
                    for k in range(ss, se + 1):
                        a = av[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= eob:
                            emit_eobrun()
                            out.append(("sym", 1, 0, 0xF0, 0, 0))
                            r -= 16
                            out.extend(("bits", b, 1) for b in br)
                            br = []
                        if a > 1:
                            br.append(a & 1)
                            continue
                        emit_eobrun()
                        out.append(("sym", 1, 0, (r << 4) | 1, 0 if int(blk[zz[k]]) < 0 else 1, 1))
                        out.extend(("bits", b, 1) for b in br)
                        br, r = [], 0
                    if r > 0 or br:
                        st["eobrun"] += 1
                        st["be"] += br
                        if st["eobrun"] == 0x7FFF or len(st["be"]) > 937 or one:
                            emit_eobrun()
        emit_eobrun()
        return out

    def write(self, script, head=None, eoi=b"\xff\xd9"):
        out = self.head() if head is None else head
        restart = 0
        for item in script:
            if item[0] == "dri":
                restart = item[1]
                out += _seg(0xDD, bytes([restart >> 8, restart & 255]))
            elif item[0] == "seg":
                out += _seg(item[1], item[2])
            elif item[0] == "raw":
                out += item[1]
            else:
                out += self.scan(item[1], restart)
        return out + eoi

    def scan(self, s, restart):
        toks = s.get("tokens")
        if toks is None:
            toks = self.tokens(s, restart)
        # the scan's own tables, one per table id it names
        def tid(t):
            return s["ta"] if t[1] else s["td"][t[2]]
        freq = {}
        for t in toks:
            if t[0] == "sym":
                f = freq.setdefault((t[1], tid(t)), {})
                f[t[3]] = f.get(t[3], 0) + 1
        codes, out = {}, b""
        for (cls, th) in sorted(freq):
            bits, vals = optimal_table(freq[(cls, th)])
            codes[(cls, th)] = DI.table_codes(bits, vals)
            if s.get("dht", True):
                out += _seg(0xC4, bytes([(cls << 4) | th] + bits + vals))
        sos = bytes([len(s["comps"])])
        for slot, c in enumerate(s["comps"]):
            td = s["td"][slot] if s.get("td") else 0
            sos += bytes([self.comps[c][0], (td << 4) | s.get("ta", 0)])
        sos += bytes([s["ss"], s["se"], (s["ah"] << 4) | s["al"]])
        out += _seg(0xDA, s["sos"] if s.get("sos") is not None else sos)
        w, n_rst, data = DI.ScanWriter(), 0, b""
        for t in toks:
            if t[0] == "sym":
                w.put(codes[(t[1], tid(t))], t[3], t[4], t[5])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                data += w.bytes() + b"\xff" * s.get("rst_fill", 0) + bytes([0xFF, 0xD0 + (n_rst & 7)])
                n_rst += 1
                w = DI.ScanWriter()
        return out + data + w.bytes() + s.get("tail", b"")


def scan(comps, ss, se, ah, al, td=None, ta=0, **kw):
    d = dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, td=list(td) if td is not None else [0] * len(comps), ta=ta)
    d.update(kw)
    return ("scan", d)


def writer_of(name, flat=None):
    """the writer over the coefficients the baseline restatement decodes from a baseline fixture"""
    d = D.decode(DI.fixture_bytes(name))
    h = d.header
    comps = [(c["id"], c["h"] if len(h.comps) > 1 else 1, c["v"] if len(h.comps) > 1 else 1, c["tq"]) for c in h.comps]
    return ProgressiveWriter(h.width, h.height, comps, {c["tq"]: h.qtables[c["tq"]] for c in h.comps}, d.coefs)


# ---------------------------------------------------------------------------
# B: scripts no encoder picks, over the coefficients of baseline fixtures
# ---------------------------------------------------------------------------
B_BASES = {"420": "noise_%s_420_q95_rst1", "444": "noise_%s_444_q95", "gray": "noise_%s_gray_q95_rst2"}
B_SIZES = ["17x17", "33x15"]


def b_base(name):
    """the baseline fixture whose pixels a B file must give"""
    tag, size = name.split("_")[-2:]
    return B_BASES[tag] % size


def _all(n):
    return list(range(n))


def _spectral(n, **kw):
    """spectral selection only; DC not interleaved, one scan per component"""
    s = [scan([c], 0, 0, 0, 0, td=[c & 1], **kw) for c in range(n)]
    for c in range(n):
        s += [scan([c], 1, 5, 0, 0, ta=c & 1, **kw), scan([c], 6, 63, 0, 0, ta=c & 1, **kw)]
    return s


def _every_position(n):
    """every AC position of Y its own scan; the chroma components one band each"""
    s = [scan(_all(n), 0, 0, 0, 0, td=[0, 1, 1][:n])]
    s += [scan([0], k, k, 0, 0) for k in range(1, 64)]
    s += [scan([c], 1, 63, 0, 0, ta=1) for c in range(1, n)]
    return s


def _successive(n, **kw):
    """full successive approximation: DC from Al = 13 down, AC from Al = 3 down"""
    s = [scan(_all(n), 0, 0, 0, 13, td=[0, 1, 1][:n])]
    s += [scan(_all(n), 0, 0, a + 1, a) for a in range(12, -1, -1)]
    for c in range(n):
        s += [scan([c], 1, 63, 0, 3, ta=c & 1, **kw)]
        s += [scan([c], 1, 63, a + 1, a, ta=c & 1, **kw) for a in (2, 1, 0)]
    return s


def _dri_changes(n):
    """DRI 0 -> 2 -> 0 between scans; a fill byte in front of every RSTn of one scan"""
    s = [scan(_all(n), 0, 0, 0, 1, td=[0, 1, 1][:n]), ("dri", 2)]
    s += [scan([0], 1, 63, 0, 1, rst_fill=1), scan(_all(n), 0, 0, 1, 0), ("dri", 0)]
    s += [scan([c], 1, 63, 0, 1, ta=1) for c in range(1, n)]
    s += [("dri", 2)] + [scan([c], 1, 63, 1, 0, ta=c & 1) for c in range(n)]
    return s


def _table_ids_2_3(n):
    """table ids 2 and 3 in both classes; every scan redefines the table it names"""
    s = [scan(_all(n), 0, 0, 0, 0, td=[2, 3, 2][:n])]
    for c in range(n):
        s += [scan([c], 1, 63, 0, 1, ta=2 + (c & 1)), scan([c], 1, 63, 1, 0, ta=3 - (c & 1))]
    return s


def _dqt_redefined(n, w):
    """a DQT behind the component's first scan redefines its table: libjpeg has latched the first"""
    decoy = [("seg", 0xDB, dqt_payload(tq, [1 + (k * 37 + tq) % 255 for k in range(64)])) for tq in sorted(w.qtables)]
    s = [scan(_all(n), 0, 0, 0, 0, td=[0, 1, 1][:n])] + decoy
    for c in range(n):
        s += [scan([c], 1, 63, 0, 0, ta=c & 1)]
    return s


def _comments(n):
    """COM and fill bytes between scans, fill bytes in front of RSTn, bytes behind a scan's last block"""
    com = ("seg", 0xFE, b"a comment \xff\xda with markers \xff\xd9 in it")
    s = [("dri", 1), scan(_all(n), 0, 0, 0, 0, td=[0, 1, 1][:n], rst_fill=2), com, ("raw", b"\xff\xff\xff"), ("dri", 3)]
    for c in range(n):
        s += [scan([c], 1, 63, 0, 0, ta=c & 1, rst_fill=1, tail=b"\0\0\x55" if c == 0 else b""), com, ("raw", b"\xff")]
    return s


def b_files():
    """{name: bytes}"""
    out = {}
    for size in B_SIZES:
        for tag, base in B_BASES.items():
            w = writer_of(base % size)
            n = len(w.comps)
            end = "_%s_%s" % (tag, size)
            out["b_spectral" + end] = w.write(_spectral(n))
            out["b_successive" + end] = w.write(_successive(n))
            out["b_successive_eob1" + end] = w.write(_successive(n, eob="one"))
            out["b_spectral_eob1" + end] = w.write(_spectral(n, eob="one"))
            out["b_dri_changes" + end] = w.write(_dri_changes(n))
            out["b_table_ids_2_3" + end] = w.write(_table_ids_2_3(n))
            out["b_dqt_redefined" + end] = w.write(_dqt_redefined(n, w), )
            out["b_comments" + end] = w.write(_comments(n))
            if size == "17x17":
                out["b_every_position" + end] = w.write(_every_position(n))
    # interleaved against non-interleaved DC on planes with padding blocks (17 x 17 at 4:2:0: Y's
    # interleaved DC scan codes 4 x 4 blocks, the others 3 x 3)
    w = writer_of(B_BASES["420"] % "17x17")
    ac = [scan([c], 1, 63, 0, 0, ta=c & 1) for c in range(3)]
    out["b_dc_interleaved_420_17x17"] = w.write([scan([0, 1, 2], 0, 0, 0, 0, td=[0, 1, 1])] + ac)
    out["b_dc_not_interleaved_420_17x17"] = w.write([scan([c], 0, 0, 0, 0) for c in range(3)] + ac)
    out["b_dc_y_cbcr_420_17x17"] = w.write([scan([0], 0, 0, 0, 0), scan([1, 2], 0, 0, 0, 0, td=[1, 1])] + ac)
    return out


# ---------------------------------------------------------------------------
# C: large gray files written by hand
# ---------------------------------------------------------------------------
C_SIZES = {"c_eobrun_32767_gray_2048x1024": (2048, 1024), "c_eob_categories_gray_1024x1032": (1024, 1032)}


def c_files():
    out = {}
    # 32 768 blocks, DC 5 x 16 / 8 = 10 above 128, no AC: one EOB run of 32 767 (category 14, extra
    # bits all ones) and one of 1
    w, h = C_SIZES["c_eobrun_32767_gray_2048x1024"]
    coefs = np.zeros((h // 8, w // 8, 64), np.int64)
    coefs[..., 0] = 5
    pw = ProgressiveWriter(w, h, [(1, 1, 1, 0)], {0: [16] * 64}, [coefs])
    out["c_eobrun_32767_gray_2048x1024"] = pw.write([scan([0], 0, 0, 0, 0), scan([0], 1, 63, 0, 0)])
    # EOB runs of 2^r blocks, r = 0..13, between blocks that end at coefficient 63 (no EOB).  The
    # first scan is at Al = 1; the first block of every run gets a new coefficient at 63 in the
    # refinement scan, which so walks long runs of its own (categories 6..13 among them)
    w, h = C_SIZES["c_eob_categories_gray_1024x1032"]
    coefs = np.zeros((h // 8 * (w // 8), 64), np.int64)
    coefs[:, 0] = (np.arange(coefs.shape[0]) % 7) - 3
    at = 0
    for r in range(14):
        coefs[at, int(ZIGZAG[63])] = 2 if r & 1 else -3      # (non-zero at Al = 1: the run ends here)
        coefs[at, int(ZIGZAG[1 + r])] = 5 - r
        coefs[at + 1, int(ZIGZAG[63])] = 1 if r & 2 else -1  # (zero at Al = 1, new in the refinement)
        at += 1 + (1 << r)
    assert at <= coefs.shape[0]
    pw = ProgressiveWriter(w, h, [(1, 1, 1, 0)], {0: [2] * 64}, [coefs.reshape(h // 8, w // 8, 64)])
    out["c_eob_categories_gray_1024x1032"] = pw.write([scan([0], 0, 0, 0, 0), scan([0], 1, 63, 0, 1),
                                                       scan([0], 1, 63, 1, 0)])
    return out


# ---------------------------------------------------------------------------
# the family
# ---------------------------------------------------------------------------


def derived_files():
    """B and C: {name: bytes}"""
    out = b_files()
    out.update(c_files())
    return out


def names():
    return a_names() + sorted(b_files()) + sorted(C_SIZES)


def path(name):
    return os.path.join(GOLDEN, name + ".jpg")


_bytes = {}


def file_bytes(name):
    if name not in _bytes:
        with open(path(name), "rb") as f:
            _bytes[name] = f.read()
    return _bytes[name]


def pixels(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["gray"], z["bgr"]


def size_of(name):
    w, h = name.split("_")[-1 if name[0] != "a" else 2].split("x")
    return int(w), int(h)


def by_size():
    """{(w, h): [names]}: one decoder call per entry"""
    out = {}
    for n in names():
        out.setdefault(size_of(n), []).append(n)
    return out


# ---------------------------------------------------------------------------
# D: files the host parser must refuse
# ---------------------------------------------------------------------------


def refusals():
    """{what: (bytes, a word the refusal's text must contain)}; every text but those of the last
    three begins "SOF2 (progressive)" and names the scan"""
    w = writer_of(B_BASES["420"] % "17x17")
    g = writer_of(B_BASES["gray"] % "17x17")
    dc = scan([0, 1, 2], 0, 0, 0, 0, td=[0, 1, 1])
    ac = [scan([c], 1, 63, 0, 0, ta=c & 1) for c in range(3)]
    ok = w.write([dc] + ac)
    out = {}

    def sos(ns_ids, ss, se, ahal):
        return bytes([len(ns_ids)]) + b"".join(bytes([i, 0]) for i in ns_ids) + bytes([ss, se, ahal])
    out["Ss = 0 with Se = 5"] = (w.write([scan([0, 1, 2], 0, 0, 0, 0, td=[0, 1, 1], sos=sos([1, 2, 3], 0, 5, 0))] + ac),
                                 "scan 0: Ss = 0 with Se = 5")
    out["a baseline scan under SOF2"] = (DI.refusals()["progressive"][0], "SOF2")
    out["Ss > 0 with Ns = 2"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1, 2], 1, 63, 0))] + ac[1:]),
                                 "scan 1: Ss > 0 with Ns = 2")
    out["Se < Ss"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1], 9, 8, 0))] + ac[1:]), "scan 1: Se = 8 below Ss")
    out["Se > 63"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1], 1, 64, 0))] + ac[1:]), "scan 1: Se = 64")
    out["Al = 14"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1], 1, 63, 14))] + ac[1:]), "scan 1: Al = 14")
    out["Ah = 3 with Al = 1"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1], 1, 63, 0x31))] + ac[1:]),
                                 "scan 1: Ah = 3 with Al other than Ah - 1")
    out["first scan with Ah != 0"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([1], 1, 63, 0x10))] + ac[1:]),
                                      "scan 1: coefficient 1 refined before its first scan")
    out["refinement from another Al"] = (w.write([scan([0, 1, 2], 0, 0, 0, 2, td=[0, 1, 1]),
                                                  scan([0, 1, 2], 0, 0, 1, 0)] + ac),
                                         "scan 1: Ah = 1 is not the coefficient's current Al")
    out["sent first twice"] = (w.write([dc, ac[0], ac[0]] + ac[1:]), "scan 2: coefficient 1 sent first twice")
    out["AC before DC"] = (w.write([scan([0], 0, 0, 0, 0), ac[1], scan([1, 2], 0, 0, 0, 0, td=[1, 1]), ac[0], ac[2]]),
                           "scan 1: AC scan of component 1 before its DC scan")
    out["component the frame does not define"] = (w.write([dc, scan([0], 1, 63, 0, 0, sos=sos([7], 1, 63, 0))] + ac[1:]),
                                                  "scan 1: component id 7")
    out["component order"] = (w.write([scan([0, 1, 2], 0, 0, 0, 0, td=[0, 1, 1], sos=sos([2, 1, 3], 0, 0, 0))] + ac),
                              "scan 0: component order")
    out["table the file does not define"] = (w.write([dc, scan([0], 1, 63, 0, 0, ta=0, sos=bytes([1, 1, 0x03, 1, 63, 0]))] +
                                                     ac[1:]), "scan 1: Huffman table id 3")
    out["ends before bit 0"] = (w.write([scan([0, 1, 2], 0, 0, 0, 1, td=[0, 1, 1])] + ac),
                                "ends before coefficient 0 of component 0 has reached bit 0")
    out["ends before Cr's AC"] = (w.write([dc] + ac[:2]), "ends before coefficient 1 of component 2")
    out["ends before bit 0, gray"] = (g.write([scan([0], 0, 0, 0, 0), scan([0], 1, 63, 0, 1)]),
                                      "ends before coefficient 1 of component 0")
    out["SOF0 between scans"] = (w.write([dc, ("seg", 0xC0, w.head()[-15:])] + ac), "marker C0 between scans")
    out["DNL between scans"] = (w.write([dc, ("seg", 0xDC, b"\0\x11")] + ac), "marker DC between scans")
    out["no EOI"] = (ok[:-2], "no EOI")
    out["no EOI, cut inside a scan"] = (ok[:-8], "no EOI")
    out["no EOI, cut behind a scan"] = (w.write([dc] + ac, eoi=b""), "no EOI")
    out["SOF2 twice"] = (w.write([dc] + ac, head=w.head() + w.head()[-19:]), "second SOF2")
    return out


def accepted_extras():
    """{what: (bytes, the B file whose pixels it gives)}: bytes behind EOI are ignored"""
    name = "b_spectral_420_17x17"
    return {"bytes behind EOI": (b_files()[name] + b"\0\0padding \xff\xd9 \xff\xda \xff", name)}


# ---------------------------------------------------------------------------
# E: scans the device must find corrupt (bounded code: each runs once)
# ---------------------------------------------------------------------------

# the device's text (jpegd::status_text) and what tests/jpeg_progressive_reference.py says
CORRUPT_REASONS = {
    "all-one bits": ("an undefined Huffman code", "undefined Huffman code"),
    "scan cut in half": ("the scan ends before its last block", "the scan ends early"),
    "RST1 altered": ("a wrong or missing RSTn marker", "wrong or missing RST"),
    "run past the band": ("a run past the end of the scan's band", "run past the end of the band"),
    "refinement of size 2": ("a refinement coefficient of a size other than 1", "size other than 1"),
}


def corrupt_scans():
    """{what: bytes}: files of 17 x 17 pixels (4:2:0) the host parser accepts and the walk must refuse"""
    w = writer_of(B_BASES["420"] % "17x17")
    dc = scan([0, 1, 2], 0, 0, 0, 0, td=[0, 1, 1])
    ac = [scan([c], 1, 63, 0, 0, ta=c & 1) for c in range(3)]
    out = {}
    # Y's AC scan replaced by 0xFF 0x00 pairs: sixteen 1-bits are no code of an optimal table
    y = w.scan(ac[0][1], 0)
    body = len(y) - y.index(b"\xff\xda") - 10
    out["all-one bits"] = w.write([dc, ("raw", y[:len(y) - body] + b"\xff\x00" * (body // 2))] + ac[1:])
    half = y[:len(y) - body // 2]
    while half.endswith(b"\xff"):
        half = half[:-1]
    out["scan cut in half"] = w.write([dc, ("raw", half)] + ac[1:])
    good = w.write([("dri", 2), dc] + ac)
    at = good.index(b"\xff\xd1", good.index(b"\xff\xda"))
    out["RST1 altered"] = good[:at] + b"\xff\xd5" + good[at + 2:]
    # a first scan of the band 1..5 whose first symbol is run 7, size 1: k = 1 + 7 > Se; the rest of
    # the scan is one EOB run (Y's 3 x 3 blocks)
    toks = [("sym", 1, 0, 0x71, 1, 1), ("sym", 1, 0, 0x30, 0, 3)]
    out["run past the band"] = w.write([dc, scan([0], 1, 5, 0, 0, tokens=toks), scan([0], 6, 63, 0, 0)] + ac[1:])
    # a refinement scan whose first symbol has size 2
    toks = [("sym", 1, 0, 0x02, 3, 2), ("sym", 1, 0, 0x30, 0, 3)]
    out["refinement of size 2"] = w.write([dc, scan([0], 1, 63, 0, 1), scan([0], 1, 63, 1, 0, tokens=toks),
                                           scan([1], 1, 63, 0, 0, ta=1), scan([2], 1, 63, 0, 0)])
    return out
