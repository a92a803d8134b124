"""The GeoTIFF pyramid the GPU writer has to produce and the reader's level rules, restated on the host.
DESIGN 4.18.  geotiff_reference (one IFD) and geotiff_read_reference (the accepted set) are imported
and left as they are.

  1 levels      level k >= 1 is ceil(w / 2) x ceil(h / 2) of level k - 1, computed from it
  2 reduction   pixel (r, c) from rows 2r, 2r + 1 and columns 2c, 2c + 1, clipped.  f32: NaN is nodata;
                the others added as float64 in the order (2r, 2c), (2r, 2c + 1), (2r + 1, 2c),
                (2r + 1, 2c + 1), divided by their number, rounded to float32 once; none: 0x7FC00000.
                u8 / rgb8: (sum + n // 2) // n per band
  3 count       overviews = n >= 0: levels 1..n; -1: until both sides are at most the tile's
  4 container   header, IFD 0 at 8 with its values (the tags of geotiff_reference), IFD 1, .. each with
                its own values, chained; an overview IFD: 254 = 1, no geo tags; tile data from the next
                multiple of 16, coarsest level first, level 0 last
  5 reading     level 0 = IFD 0; level k = the k-th later IFD with 254 bit 0 set and bit 2 clear; the
                geotransform scaled by W0 / Wk and H0 / Hk; nodata the base's
"""
import struct

import numpy as np

import geotiff_read_reference as R
import geotiff_reference as W
import png_encode_reference as PR

CANONICAL_NAN = np.uint32(0x7FC00000)


def reduce(level, kind=None):
    """rule 2: the next level of `level`"""
    a = np.asarray(level)
    kind = kind or W.kind_of(a)
    h, w = a.shape[:2]
    H, Wd = (h + 1) // 2, (w + 1) // 2
    if kind == "f32":
        s = np.zeros((H, Wd), np.float64)
        n = np.zeros((H, Wd), np.int64)
        for dr, dc in ((0, 0), (0, 1), (1, 0), (1, 1)):      # the fixed order
            part = a[dr::2, dc::2]
            ph, pw = part.shape
            ok = ~np.isnan(part)
            with np.errstate(invalid="ignore", over="ignore"):
                add = s[:ph, :pw] + part.astype(np.float64)
            s[:ph, :pw] = np.where(ok, add, s[:ph, :pw])
            n[:ph, :pw] += ok
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out = (s / n.astype(np.float64)).astype(np.float32)
        bits = out.view(np.uint32).copy()
        bits[(n == 0) | np.isnan(out)] = CANONICAL_NAN      # (+inf with -inf: the NaN's sign is the processor's)
        return bits.view(np.float32)
    s = np.zeros((H, Wd) + a.shape[2:], np.uint32)
    n = np.zeros((H, Wd) + (1,) * (a.ndim - 2), np.uint32)
    for dr, dc in ((0, 0), (0, 1), (1, 0), (1, 1)):
        part = a[dr::2, dc::2]
        ph, pw = part.shape[:2]
        s[:ph, :pw] += part
        n[:ph, :pw] += 1
    return ((s + n // 2) // n).astype(np.uint8)


def level_count(width, height, side, overviews):
    """rule 3; raises ValueError for what the writer refuses"""
    if overviews < -1 or overviews > 16:
        raise ValueError("overviews")
    w, h, k = width, height, 0
    while (w > side or h > side) if overviews < 0 else k < overviews:
        if w == 1 and h == 1:
            raise ValueError("overviews: a 1 x 1 level is not reduced")
        w, h, k = (w + 1) // 2, (h + 1) // 2, k + 1
    return k


def pyramid(raster, side, overviews):
    levels = [np.asarray(raster)]
    for _ in range(level_count(levels[0].shape[1], levels[0].shape[0], side, overviews)):
        levels.append(reduce(levels[-1]))
    return levels


def _ifd_tags(width, height, kind, side, n, overview):
    bands = 3 if kind == "rgb8" else 1
    short = lambda *v: (W.SHORT, len(v), struct.pack("<%dH" % len(v), *v))
    long_ = lambda *v: (W.LONG, len(v), struct.pack("<%dI" % len(v), *v))
    tags = {256: long_(width), 257: long_(height),
            258: short(*([8] * 3 if bands == 3 else [32 if kind == "f32" else 8])),
            259: short(8), 262: short(2 if bands == 3 else 1), 277: short(bands), 284: short(1),
            317: short(3 if kind == "f32" else 2), 322: long_(side), 323: long_(side),
            324: long_(*([0] * n)), 325: long_(*([0] * n)),
            339: short(*([1] * 3 if bands == 3 else [3 if kind == "f32" else 1]))}
    if overview:
        tags[254] = long_(1)
    if kind == "f32":
        tags[42113] = (W.ASCII, 4, b"nan\0")
    return tags


def container(sizes, kind, side, geotransform, utm_zone, northern, counts):
    """rule 4: sizes = [(width, height)] per level, counts = [[bytes per tile]] per level -> the file in
    front of the tile data, where every level's tiles start, the file's size"""
    long_ = lambda *v: (W.LONG, len(v), struct.pack("<%dI" % len(v), *v))
    ifds, at = [], 8
    for k, ((w, h), cnt) in enumerate(zip(sizes, counts)):
        tags = _ifd_tags(w, h, kind, side, len(cnt), k > 0)
        if k == 0:
            tags.update(W.geo_tags(geotransform, utm_zone, northern))
        order = sorted(tags)
        ifd_at = at
        at += 2 + 12 * len(order) + 4
        where = {}
        for tag in order:
            size = len(tags[tag][2])
            if size > 4:
                where[tag] = at
                at += size + (size & 1)
        ifds.append((ifd_at, tags, order, where))
    data_at = (at + 15) & ~15
    level_at, run = [0] * len(sizes), data_at
    for k in reversed(range(len(sizes))):
        level_at[k] = run
        run += sum(counts[k])
    if run > 0xFFFFFFFF:
        raise ValueError("the file would exceed 2^32 - 1 bytes")
    head = bytearray(data_at)
    head[:8] = b"II" + struct.pack("<HI", 42, 8)
    for k, (ifd_at, tags, order, where) in enumerate(ifds):
        offs, o = [], level_at[k]
        for c in counts[k]:
            offs.append(o)
            o += c
        tags[324], tags[325] = long_(*offs), long_(*counts[k])
        struct.pack_into("<H", head, ifd_at, len(order))
        for e, tag in enumerate(order):
            typ, count, payload = tags[tag]
            entry = ifd_at + 2 + 12 * e
            struct.pack_into("<HHI", head, entry, tag, typ, count)
            if tag in where:
                struct.pack_into("<I", head, entry + 8, where[tag])
                head[where[tag]:where[tag] + len(payload)] = payload
            else:
                head[entry + 8:entry + 8 + len(payload)] = payload
        nxt = ifds[k + 1][0] if k + 1 < len(ifds) else 0
        struct.pack_into("<I", head, ifd_at + 2 + 12 * len(order), nxt)
    return bytes(head), level_at, run


def encode(raster, geotransform, utm_zone=32, northern=True, tile=256, overviews=0, stream=PR.zlib_stream):
    """The file with `overviews` levels behind level 0."""
    raster = np.asarray(raster)
    kind = W.kind_of(raster)
    side = tile or 256
    levels = pyramid(raster, side, overviews)
    streams = [[stream(p) for p in W.tile_payloads(l, side)] for l in levels]
    head, level_at, total = container([(l.shape[1], l.shape[0]) for l in levels], kind, side, geotransform, utm_zone,
                                      northern, [[len(z) for z in s] for s in streams])
    out = head + b"".join(b"".join(s) for s in reversed(streams))
    assert len(out) == total
    return out


# ---- rule 5 ----------------------------------------------------------------------------------------

def ifd_chain(data):
    """[(offset, NewSubfileType or None)] of the chain; Refused for a chain the reader refuses"""
    if len(data) < 8 or data[:2] != b"II" or struct.unpack_from("<H", data, 2)[0] != 42:
        raise R.Refused("no classic little-endian TIFF")
    at, = struct.unpack_from("<I", data, 4)
    out = []
    while True:
        if len(out) == 64:
            raise R.Refused("more than 64 IFDs")
        if at in [o for o, _ in out]:
            raise R.Refused("the chain returns to an IFD")
        if at < 8 or at + 2 > len(data):
            raise R.Refused("IFD outside the file")
        n, = struct.unpack_from("<H", data, at)
        if at + 2 + 12 * n + 4 > len(data):
            raise R.Refused("IFD runs past the file")
        sub = None
        for k in range(n):
            tag, typ, count, value = struct.unpack_from("<HHII", data, at + 2 + 12 * k)
            if tag == 254 and typ in (3, 4) and count == 1:
                sub = value & 0xFFFF if typ == 3 else value
        out.append((at, sub))
        at, = struct.unpack_from("<I", data, at + 2 + 12 * n)
        if at == 0:
            return out


def level_ifds(data):
    chain = ifd_chain(data)
    return [chain[0][0]] + [o for o, sub in chain[1:] if sub is not None and sub & 1 and not sub & 4]


def _at_ifd(data, offset):
    """the file with `offset` as its first IFD: every other offset is absolute and stays"""
    return bytes(data[:4]) + struct.pack("<I", offset) + bytes(data[8:])


def level_info(data, level):
    """R.parse's dict of a level, with the geotransform and nodata of rule 5"""
    ifds = level_ifds(data)
    if not 0 <= level < len(ifds):
        raise R.Refused("level %d of %d" % (level, len(ifds)))
    base = R.parse(data)
    if level == 0:
        return base
    dims = [R.parse(_at_ifd(data, o)) for o in ifds[:level + 1]]
    for a, b in zip(dims, dims[1:]):
        if b["width"] > a["width"] or b["height"] > a["height"] or \
                (b["width"] == a["width"] and b["height"] == a["height"]):
            raise R.Refused("a level is not smaller than the one before it")
    p = dims[level]
    if p["kind"] != base["kind"]:
        raise R.Refused("a level of another kind")
    gt = [np.float64(v) for v in base["geotransform"]]
    gt[1] = gt[1] * np.float64(base["width"]) / np.float64(p["width"])
    gt[5] = gt[5] * np.float64(base["height"]) / np.float64(p["height"])
    p = dict(p)
    for key in ("has_geo", "epsg", "raster_type", "nodata"):
        p[key] = base[key]
    p["geotransform"] = tuple(float(v) for v in gt)
    return p


def levels(data):
    return [level_info(data, k) for k in range(len(level_ifds(data)))]


def decode(data, level):
    """-> (the level's raster, level_info(data, level))"""
    raster, _ = R.decode(_at_ifd(data, level_ifds(data)[level]))
    return raster, level_info(data, level)


def auto_level(data, res):
    """the coarsest level whose pixels are no larger than `res` in either direction, else 0"""
    infos = levels(data)
    for k in reversed(range(1, len(infos))):
        gt = infos[k]["geotransform"]
        if gt[1] <= res and -gt[5] <= res:
            return k
    return 0


# ---- foreign chains ---------------------------------------------------------------------------------

def chain(files):
    """Single-IFD files (R.write's) -> one file whose IFDs follow each other in that order: every later
    file is appended whole at an even offset, its offsets moved, and hooked to the one before it."""
    out = bytearray(files[0])
    last_ifd = 8
    for f in files[1:]:
        out += b"\0" * (len(out) & 1)
        base = len(out)
        f = bytearray(f)
        ifd, = struct.unpack_from("<I", f, 4)
        n, = struct.unpack_from("<H", f, ifd)
        for k in range(n):
            e = ifd + 2 + 12 * k
            tag, typ, count, value = struct.unpack_from("<HHII", f, e)
            size = R.TYPE_SIZE[typ] * count
            where = e + 8 if size <= 4 else value
            if tag in (273, 324):
                for q in range(count):
                    fmt = "<H" if typ == 3 else "<I"
                    v, = struct.unpack_from(fmt, f, where + q * R.TYPE_SIZE[typ])
                    struct.pack_into(fmt, f, where + q * R.TYPE_SIZE[typ], v + base)
            if size > 4:
                struct.pack_into("<I", f, e + 8, value + base)
        out += f
        n_last, = struct.unpack_from("<H", out, last_ifd)
        struct.pack_into("<I", out, last_ifd + 2 + 12 * n_last, base + ifd)
        last_ifd = base + ifd
    return bytes(out)


def subfile(value):
    """extra_tags for R.write: NewSubfileType = value"""
    return {254: (4, [value])}
