"""NumPy restatement of libjpeg's progressive decoder (SOF2: jdmarker.c, jdinput.c, jdphuff.c) in
front of the baseline restatement's IDCT, upsampling and colour conversion
(tests/jpeg_decode_reference.py): what cv::imread / Pillow's Image.open give for a complete
progressive 8-bit Huffman file, gray or Y Cb Cr with Y sampled 1x1, 2x1 or 2x2.

The parser keeps the whole marker sequence up to EOI as a scan list and refuses, in the words of
the C++ parser (aerial_mapper_amd/csrc/amhip_jpeg_decode_host.h), what libjpeg refuses
(JERR_BAD_PROGRESSION, JERR_BAD_PROG_SCRIPT), what it only warns about (JWRN_BOGUS_PROGRESSION),
and a file whose scans leave a coefficient short of bit 0: libjpeg would decode such a file and
smooth its blocks (jdcoefct.c), which is not restated.  The four decode procedures follow
jdphuff.c rule by rule.  Deliberately stricter than libjpeg, which warns and goes on: a scan that
ends early, a wrong RSTn index, a refinement coefficient of a size other than 1.

Pinned: the .npz files of tests/golden/jpeg_progressive/ hold what libjpeg-turbo decodes, and
tests/test_jpeg_progressive_reference.py compares bit for bit.  This module is the yardstick of
k_jpegd_entropy_prog (aerial_mapper_amd/csrc/amhip_jpeg_decode.hip).
"""
import numpy as np

import jpeg_decode_reference as D
from jpeg_reference import ZIGZAG

Refused, Corrupt, HuffTable = D.Refused, D.Corrupt, D.HuffTable
PROG = "SOF2 (progressive): "
KINDS = ("dc_first", "dc_refine", "ac_first", "ac_refine")


class Scan(object):
    """index; begin, end: the byte range of the entropy-coded segment (end: the 0xFF of the marker
    behind it); comps: component indices, increasing; ss, se, ah, al; restart: the scan's MCUs per
    interval as DRI stood at this SOS; dc: [HuffTable or None per component of the scan]; ac:
    HuffTable or None; nx, ny: the scan's MCUs (per_scan_setup); kind: one of KINDS"""
    pass


class Header(object):
    """width, height, channels; comps: [dict(id, h, v, tq)], tq renumbered to the component's index;
    qtables {component index: natural-order 64}: the table in effect at the SOS of the first scan
    that contains the component (latch_quant_tables, jdinput.c); scans: [Scan]; progressive"""
    pass


def first_frame_marker(data):
    """the file's first SOFn (0xC0..0xCF but DHT, JPG, DAC), segment by segment; None: none found"""
    data = bytes(data)
    p, n = 2, len(data)
    while p + 4 <= n and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m
        if m in (0xD9, 0xDA):
            return None
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    return None


def parse(data):
    """-> Header of a progressive file; a file whose first frame marker is not SOF2 goes to the
    baseline restatement's parse_header (its Header gets progressive = False)"""
    data = bytes(data)
    if first_frame_marker(data) != 0xC2:
        h = D.parse_header(data)
        h.progressive = False
        return h
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    h = Header()
    h.progressive, h.comps, h.qtables, h.scans = True, None, {}, []
    q, huff = {}, {}
    restart, adobe_transform = 0, None
    bits = None     # coef_bits: per component, the Al each coefficient has reached; -1: not sent
    p = 2
    while True:
        between = len(h.scans) > 0
        if between:
            if p + 2 > n:
                raise Refused("no EOI")
        elif p + 4 > n:
            raise Refused("no SOS")
        if data[p] != 0xFF:
            raise Refused("marker expected at byte %d" % p)
        m = data[p + 1]
        if m == 0xFF:      # fill byte
            p += 1
            continue
        if m == 0xD9:
            if between:
                break
            raise Refused("no SOS")
        if p + 4 > n:
            raise Refused("no EOI")
        length = (data[p + 2] << 8) | data[p + 3]
        if length < 2 or p + 2 + length > n:
            raise Refused("segment %02X runs past the file" % m)
        pl = data[p + 4:p + 2 + length]
        if between and not (m in (0xC4, 0xDB, 0xDD, 0xDA, 0xFE) or 0xE0 <= m <= 0xEF):
            raise Refused(PROG + "marker %02X between scans" % m)
        if m in (0xC0, 0xC2):
            if h.comps is not None:
                raise Refused("second SOF0" if m == 0xC0 else "second SOF2 (progressive)")
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
                ids = [c["id"] for c in h.comps]
                if ids == [ord("R"), ord("G"), ord("B")]:
                    raise Refused("SOF0: component ids R G B")
                if len(set(ids)) != 3 and m == 0xC2:
                    raise Refused(PROG + "a component id twice")
            bits = [[-1] * 64 for _ in h.comps]
        elif m in D._SOF_NAMES:
            raise Refused("marker %s" % D._SOF_NAMES[m])
        elif m == 0xDB:
            at = 0
            while at < len(pl):
                if pl[at] >> 4:
                    raise Refused("DQT: 16-bit table")
                if (pl[at] & 15) > 3 or at + 65 > len(pl):
                    raise Refused("DQT: bad table id or length")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(pl[at + 1:at + 65], np.uint8)
                q[pl[at] & 15] = t
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(pl):
                # ids 0..3 in both classes under SOF2 (T.81 B.2.4.2)
                if at + 17 > len(pl) or (pl[at] >> 4) > 1 or (pl[at] & 15) > 3:
                    raise Refused("DHT: bad table class, id or length")
                b = list(pl[at + 1:at + 17])
                nv = sum(b)
                if nv > 256 or at + 17 + nv > len(pl):
                    raise Refused("DHT: bad symbol count")
                vals = list(pl[at + 17:at + 17 + nv])
                if (pl[at] >> 4) == 0 and any(v > 15 for v in vals):
                    raise Refused("DHT: DC symbol above 15")
                huff[(pl[at] >> 4, pl[at] & 15)] = HuffTable(b, vals)    # (a later DHT replaces it)
                at += 17 + nv
        elif m == 0xDD:
            if len(pl) != 2:
                raise Refused("DRI: bad length")
            restart = (pl[0] << 8) | pl[1]
        elif m == 0xEE and pl[:5] == b"Adobe" and len(pl) >= 12:
            adobe_transform = pl[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDA:
            if h.comps is None:
                raise Refused("SOS before SOF0")
            # get_sos (jdmarker.c), start_pass_phuff_decoder (jdphuff.c)
            si = len(h.scans)
            if len(pl) < 1 or len(pl) != 4 + 2 * pl[0]:
                raise Refused(PROG + "scan %d: bad SOS length" % si)
            s = Scan()
            s.index, ns = si, pl[0]
            if ns < 1 or ns > len(h.comps):
                raise Refused(PROG + "scan %d: Ns = %d, more components than the frame defines" % (si, ns))
            s.ss, s.se, s.ah, s.al = pl[-3], pl[-2], pl[-1] >> 4, pl[-1] & 15
            if s.ss == 0 and s.se == 63 and pl[-1] == 0:
                raise Refused("marker SOF2 (progressive)")     # (a sequential scan: the baseline's words)
            if s.ss == 0 and s.se != 0:
                raise Refused(PROG + "scan %d: Ss = 0 with Se = %d" % (si, s.se))
            if s.ss > 0 and ns != 1:
                raise Refused(PROG + "scan %d: Ss > 0 with Ns = %d" % (si, ns))
            if s.se < s.ss or s.se > 63:
                raise Refused(PROG + "scan %d: Se = %d below Ss or above 63" % (si, s.se))
            if s.al > 13:
                raise Refused(PROG + "scan %d: Al = %d above 13" % (si, s.al))
            if s.ah != 0 and s.al != s.ah - 1:
                raise Refused(PROG + "scan %d: Ah = %d with Al other than Ah - 1" % (si, s.ah))
            s.comps, s.dc, s.ac = [], [], None
            for k in range(ns):
                cid = pl[1 + 2 * k]
                found = [i for i, c in enumerate(h.comps) if c["id"] == cid]
                if not found:
                    raise Refused(PROG + "scan %d: component id %d the frame does not define" % (si, cid))
                c = found[0]
                if s.comps and c <= s.comps[-1]:
                    raise Refused(PROG + "scan %d: component order" % si)
                s.comps.append(c)
                if c not in h.qtables:
                    # latch_quant_tables: the table as it stands at the component's first scan
                    if h.comps[c]["tq"] not in q:
                        raise Refused("SOS: missing quantisation table")
                    h.qtables[c] = q[h.comps[c]["tq"]].copy()
                if s.ss > 0 and bits[c][0] < 0:
                    raise Refused(PROG + "scan %d: AC scan of component %d before its DC scan" % (si, c))
                for z in range(s.ss, s.se + 1):
                    if s.ah == 0 and bits[c][z] >= 0:
                        raise Refused(PROG + "scan %d: coefficient %d sent first twice (Ah = 0)" % (si, z))
                    if s.ah != 0 and bits[c][z] < 0:
                        raise Refused(PROG + "scan %d: coefficient %d refined before its first scan (Ah)" % (si, z))
                    if s.ah != 0 and bits[c][z] != s.ah:
                        raise Refused(PROG + "scan %d: Ah = %d is not the coefficient's current Al" % (si, s.ah))
                    bits[c][z] = s.al
                # a scan needs only the tables it uses: a DC refinement scan none
                cls = 0 if s.ss == 0 else 1
                th = (pl[2 + 2 * k] & 15) if cls else (pl[2 + 2 * k] >> 4)
                if cls == 0 and s.ah != 0:
                    s.dc.append(None)
                    continue
                if th > 3 or (cls, th) not in huff:
                    raise Refused(PROG + "scan %d: Huffman table id %d the file does not define" % (si, th))
                if cls:
                    s.ac = huff[(cls, th)]
                else:
                    s.dc.append(huff[(cls, th)])
            if adobe_transform == 0 and len(h.comps) == 3:
                raise Refused("Adobe transform 0 (RGB)")
            s.restart = restart
            s.kind = KINDS[(2 if s.ss else 0) + (1 if s.ah else 0)]
            hmax, vmax, mcux, mcuy, samp = D.layout(h)
            if ns > 1:
                s.nx, s.ny = mcux, mcuy
            else:
                # per_scan_setup: a scan of one component walks its real blocks only
                ch, cv = samp[s.comps[0]]
                s.nx = ((h.width * ch + hmax - 1) // hmax + 7) // 8
                s.ny = ((h.height * cv + vmax - 1) // vmax + 7) // 8
            # next_marker: the segment ends at the first marker that is neither 0xFF 0x00 nor RSTn
            s.begin = at = p + 2 + length
            while True:
                run = data.find(b"\xff", at)
                if run < 0:
                    raise Refused("no EOI")
                k = run + 1
                while k < n and data[k] == 0xFF:
                    k += 1
                if k >= n:
                    raise Refused("no EOI")
                if data[k] == 0 or 0xD0 <= data[k] <= 0xD7:
                    at = k + 1
                    continue
                s.end = run
                break
            h.scans.append(s)
            p = s.end
            continue
        else:
            raise Refused("marker %02X" % m)
        p += 2 + length
    for c in range(len(h.comps)):
        for z in range(64):
            if bits[c][z] != 0:
                raise Refused(PROG + "the file ends before coefficient %d of component %d has reached bit 0" % (z, c))
    for i, c in enumerate(h.comps):
        c["tq"] = i                      # (h.qtables is keyed by component: the latched tables)
    h.channels = len(h.comps)
    return h


# ---------------------------------------------------------------------------
# entropy decoding (jdphuff.c)
# ---------------------------------------------------------------------------


class Counters(object):
    def __init__(self):
        self.scans = {k: 0 for k in KINDS}
        # EOBRUN categories (the r of an EOBr symbol, 0..14) seen in first and in refinement scans
        self.eob_category = {"ac_first": np.zeros(15, np.int64), "ac_refine": np.zeros(15, np.int64)}
        self.corrected_positive = self.corrected_negative = 0   # correction bits that changed a coefficient
        self.correction_bits = 0                                 # ... all of them
        self.new_plus = self.new_minus = 0                       # new coefficients + p1 and - p1 of refinement scans
        self.zrl_passing_nonzero = 0     # ZRL in a refinement scan that passes non-zero coefficients
        self.eobrun_blocks_with_nonzero = 0   # refinement blocks entered with EOBRUN > 0 that hold non-zero coefficients
        self.restarts = 0
        self.restarts_clearing_predictor = 0   # restarts that set a non-zero DC predictor back to 0
        self.restarts_clearing_eobrun = 0
        self.non_interleaved_on_padded_plane = 0   # scans of one component whose plane has padding blocks
        self.interleaved_dc = 0
        self.zrl_past_band = 0           # ZRLs of first scans that carry k past Se
        self.fill_bytes = self.stuffed = self.before_rst = 0
        self.slow_codes = 0
        self.max_eobrun = 0
        self.max_al = 0
        self.trailing = 0                # bytes between a scan's last block and its end


class _Bits(object):
    """jpeg_fill_bit_buffer over one scan's segment [pos, end): as the baseline restatement's"""

    def __init__(self, data, begin, end, cnt):
        self.data, self.pos, self.end, self.cnt = data, begin, end, cnt
        self.acc = self.nbits = self.fake = 0

    def fill(self):
        data, end, cnt = self.data, self.end, self.cnt
        while self.nbits <= 56:
            pos, b = self.pos, 0
            if pos >= end:
                self.fake += 8
            else:
                b = data[pos]
                if b == 0xFF:
                    k = pos + 1
                    while k < end and data[k] == 0xFF:
                        k += 1
                    b2 = data[k] if k < end else 0xD9
                    if b2 == 0:
                        self.pos = k + 1
                        cnt.stuffed += 1
                        cnt.fill_bytes += k - pos - 1
                    else:
                        b = 0
                        self.fake += 8
                else:
                    self.pos = pos + 1
            self.acc = ((self.acc << 8) | b) & ((1 << 64) - 1)
            self.nbits += 8

    def peek(self, nb):
        return (self.acc >> (self.nbits - nb)) & ((1 << nb) - 1)

    def drop(self, nb):
        self.nbits -= nb
        if self.nbits < self.fake:
            raise Corrupt("the scan ends early")

    def get(self, nb):
        self.fill()
        v = self.peek(nb)
        self.drop(nb)
        return v

    def symbol(self, t):
        self.fill()
        e = t.look[self.peek(D.LOOKAHEAD)]
        if e:
            self.drop(e >> 8)
            return e & 255
        self.cnt.slow_codes += 1
        l = D.LOOKAHEAD + 1
        while l <= 16 and self.peek(l) > t.maxcode[l]:
            l += 1
        if l > 16:
            raise Corrupt("undefined Huffman code")
        code = self.peek(l)
        self.drop(l)
        return t.huffval[(code + t.valoffset[l]) & 255]

    def extend(self, s):
        """HUFF_EXTEND(receive(s), s)"""
        v = self.get(s)
        return v - ((1 << s) - 1) if v < (1 << (s - 1)) else v

    def restart(self, next_rst):
        """process_restart / read_restart_marker / next_marker, as the baseline restatement's: the
        partial byte is dropped, the next marker must be RST`next_rst`"""
        data, end, cnt = self.data, self.end, self.cnt
        self.acc = self.nbits = self.fake = 0
        pos, code, k = self.pos, None, self.pos
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
            cnt.before_rst += 1
            cnt.stuffed += 1
            cnt.fill_bytes += k - pos - 1
            pos = k + 1
        if code != 0xD0 + next_rst:
            raise Corrupt("wrong or missing RST%d" % next_rst)
        cnt.fill_bytes += k - pos - 1
        self.pos = k + 1


def _i16(v):
    """(JCOEF) of an int: what a corrupt file's shifts leave in a 16-bit coefficient"""
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def entropy_decode(data, h, counters=None):
    """-> [coefficients of component c: (blocks down, blocks across, 64) int64, natural order, whole
    MCUs; blocks no scan codes stay 0]"""
    cnt = counters if counters is not None else Counters()
    hmax, vmax, mcux, mcuy, samp = D.layout(h)
    planes = [np.zeros((mcuy * v, mcux * hh, 64), np.int64) for (hh, v) in samp]
    zz = [int(v) for v in ZIGZAG]
    for s in h.scans:
        cnt.scans[s.kind] += 1
        cnt.max_al = max(cnt.max_al, s.al)
        br = _Bits(data, s.begin, s.end, cnt)      # (the bit buffer is empty at every scan's start)
        ns = len(s.comps)
        if ns > 1:
            cnt.interleaved_dc += 1
        else:
            c = s.comps[0]
            if (s.nx, s.ny) != (planes[c].shape[1], planes[c].shape[0]):
                cnt.non_interleaved_on_padded_plane += 1
        pred = [0] * ns
        eobrun = 0
        todo, next_rst = s.restart, 0
        p1, m1 = 1 << s.al, -(1 << s.al)
        for my in range(s.ny):
            for mx in range(s.nx):
                if s.restart:
                    if todo == 0:
                        # process_restart: every s.restart MCUs of THIS scan (single blocks when Ns =
                        # 1); the RST index starts at 0 in every scan; predictors and EOBRUN to 0
                        br.restart(next_rst)
                        next_rst = (next_rst + 1) & 7
                        cnt.restarts += 1
                        cnt.restarts_clearing_predictor += any(pred)
                        cnt.restarts_clearing_eobrun += eobrun > 0
                        pred = [0] * ns
                        eobrun = 0
                        todo = s.restart
                    todo -= 1
                for j, c in enumerate(s.comps):
                    ch, cv = samp[c] if ns > 1 else (1, 1)
                    for by in range(cv):
                        for bx in range(ch):
                            blk = planes[c][my * cv + by, mx * ch + bx]
                            if s.kind == "dc_first":
                                # decode_mcu_DC_first
                                t = br.symbol(s.dc[j])
                                if t:
                                    pred[j] += br.extend(t)
                                blk[0] = _i16(pred[j] << s.al)
                            elif s.kind == "dc_refine":
                                # decode_mcu_DC_refine: one bit per block
                                if br.get(1):
                                    blk[0] = _i16(int(blk[0]) | p1)
                            elif s.kind == "ac_first":
                                eobrun = _ac_first(br, s, blk, zz, eobrun, cnt)
                            else:
                                eobrun = _ac_refine(br, s, blk, zz, eobrun, p1, m1, cnt)
        # what lies between the scan's last block and its end is skipped
        cnt.trailing += s.end - br.pos
    return planes


def _eobrun(br, r, cnt, kind):
    cnt.eob_category[kind][r] += 1
    run = 1 << r
    if r:
        run += br.get(r)
    cnt.max_eobrun = max(cnt.max_eobrun, run)
    return run


def _ac_first(br, s, blk, zz, eobrun, cnt):
    """decode_mcu_AC_first: one block; -> EOBRUN behind it"""
    if eobrun > 0:
        return eobrun - 1
    k = s.ss
    while k <= s.se:
        rs = br.symbol(s.ac)
        r, size = rs >> 4, rs & 15
        if size:
            k += r
            if k > s.se:
                raise Corrupt("run past the end of the band")
            blk[zz[k]] = _i16(br.extend(size) << s.al)
            k += 1
        elif r == 15:
            k += 16            # ZRL (past Se: the block ends there)
            cnt.zrl_past_band += k > s.se
        else:
            return _eobrun(br, r, cnt, "ac_first") - 1       # (this block is the run's first)
    return 0


def _correct(br, blk, pos, p1, m1, cnt):
    """a non-zero coefficient of a refinement scan: one bit; 1 and the bit not yet set: the
    magnitude grows by p1"""
    cnt.correction_bits += 1
    if br.get(1):
        v = int(blk[pos])
        if (v & p1) == 0:
            if v >= 0:
                blk[pos] = _i16(v + p1)
                cnt.corrected_positive += 1
            else:
                blk[pos] = _i16(v + m1)
                cnt.corrected_negative += 1


def _ac_refine(br, s, blk, zz, eobrun, p1, m1, cnt):
    """decode_mcu_AC_refine: one block; -> EOBRUN behind it"""
    k = s.ss
    if eobrun == 0:
        while k <= s.se:
            rs = br.symbol(s.ac)
            r, size = rs >> 4, rs & 15
            new = 0
            if size:
                if size != 1:
                    raise Corrupt("refinement coefficient of a size other than 1")    # (libjpeg: a warning)
                new = p1 if br.get(1) else m1
            elif r != 15:
                eobrun = _eobrun(br, r, cnt, "ac_refine")      # (no decrement here)
                break
            # a new value or ZRL: advance over r zero coefficients, correcting the non-zero ones
            # passed; stop at the (r + 1)-th zero, or behind Se
            passed = False
            while k <= s.se:
                pos = zz[k]
                if blk[pos] != 0:
                    _correct(br, blk, pos, p1, m1, cnt)
                    passed = True
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if not size and passed:
                cnt.zrl_passing_nonzero += 1
            if new:
                if k > s.se:
                    raise Corrupt("run past the end of the band")
                blk[zz[k]] = new
                if new > 0:
                    cnt.new_plus += 1
                else:
                    cnt.new_minus += 1
            k += 1
    elif any(blk[zz[z]] != 0 for z in range(k, s.se + 1)):
        cnt.eobrun_blocks_with_nonzero += 1
    if eobrun > 0:
        # inside an EOB run: every non-zero coefficient from k to Se is corrected
        while k <= s.se:
            if blk[zz[k]] != 0:
                _correct(br, blk, zz[k], p1, m1, cnt)
            k += 1
        eobrun -= 1
    return eobrun


# ---------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------


def decode(data, counters=None, pixels=True):
    """-> jpeg_decode_reference.Decoded (header, coefs, gray, bgr).  A file that is not progressive is
    decoded by the baseline restatement.  pixels = False: coefficients only."""
    data = bytes(data)
    h = parse(data)
    if not h.progressive:
        return D.decode(data)
    out = D.Decoded()
    out.header = h
    out.coefs = entropy_decode(data, h, counters)
    if not pixels:
        return out
    planes = D.component_planes(h, out.coefs)
    hmax, vmax = D.layout(h)[:2]
    y = planes[0][:h.height, :h.width]
    out.gray = y.astype(np.uint8)
    if len(planes) == 1:
        out.bgr = np.repeat(out.gray[..., None], 3, axis=-1)
    else:
        cb = D.upsample(planes[1], h.width, h.height, hmax, vmax)
        cr = D.upsample(planes[2], h.width, h.height, hmax, vmax)
        out.bgr = D.ycc_to_bgr(y, cb, cr).astype(np.uint8)
    return out


def decode_pixels(data, colored):
    d = decode(data)
    return d.bgr if colored else d.gray
