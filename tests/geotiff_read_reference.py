"""The GeoTIFF reader (amhip_tiff_decode.hip, amhip_tiff_decode_host.h) restated in numpy, and a
writer of every variant the reader accepts.  DESIGN 4.17.

  1 parse       classic little-endian TIFF, first IFD; tiles (322 / 323 / 324 / 325) or strips
                (273 / 278 / 279; RowsPerStrip absent or above the height: one strip); Compression 1, 8,
                32946; kinds f32, u8, u16, i16, rgb8; Predictor 1, 2, 3 (f32), ignored with Compression 1
                as libtiff ignores it; geo tags by pixel scale +
                tiepoint or by a transformation matrix, PixelIsPoint moves the origin by half a pixel;
                GDAL_NODATA as float() reads it
  2 chunks      a chunk is `rows * chunk width * bytes per pixel` bytes: zlib.decompress, or as it lies
  3 predictor   per chunk row.  2: an inclusive prefix sum of whole samples (bytes, 16-bit words, 32-bit
                words), stride = bands, modulo the sample's width.  3: an inclusive prefix sum modulo 256
                over the row's 4 w bytes, then float k = bytes [k], [w + k], [2 w + k], [3 w + k], most
                significant first.  w: the tile's width, or the image's for strips
  4 crop        the padding of edge tiles is dropped
  5 place       cell (i, j) of a map window takes the pixel its centre lies in: col = floor((x - GT0) /
                GT1), row = floor((y - GT3) / GT5) in IEEE double; floats keep their bits, integers become
                floats, rgb8 the packed colour value; a cell outside the raster, on a nodata pixel or on a
                NaN keeps what it holds
"""
import struct
import zlib

import numpy as np

KINDS = {"f32": 0, "u8": 1, "rgb8": 2, "u16": 3, "i16": 4}
DTYPES = {"f32": np.float32, "u8": np.uint8, "rgb8": np.uint8, "u16": np.uint16, "i16": np.int16}
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8, 17: 8, 18: 8}
FMT = {3: "H", 4: "I", 12: "d"}


class Refused(ValueError):
    pass


def kind_of(raster):
    raster = np.asarray(raster)
    if raster.ndim == 3:
        assert raster.dtype == np.uint8 and raster.shape[2] == 3
        return "rgb8"
    assert raster.ndim == 2
    return {np.dtype(np.float32): "f32", np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16",
            np.dtype(np.int16): "i16"}[raster.dtype]


def pixel_bytes(kind):
    return {"f32": 4, "u8": 1, "rgb8": 3, "u16": 2, "i16": 2}[kind]


# ---- rule 1 ----------------------------------------------------------------------------------------

def read_ifd(data):
    """{tag: (type, count, values)} of the first IFD, for the types the reader looks into"""
    if len(data) < 8 or data[:2] != b"II" or struct.unpack_from("<H", data, 2)[0] != 42:
        raise Refused("no classic little-endian TIFF")
    ifd, = struct.unpack_from("<I", data, 4)
    if ifd + 2 > len(data):
        raise Refused("IFD outside the file")
    n, = struct.unpack_from("<H", data, ifd)
    if ifd + 2 + 12 * n + 4 > len(data):
        raise Refused("IFD runs past the file")
    tags = {}
    for k in range(n):
        tag, typ, count, value = struct.unpack_from("<HHII", data, ifd + 2 + 12 * k)
        if typ not in TYPE_SIZE:
            continue
        size = TYPE_SIZE[typ] * count
        at = ifd + 2 + 12 * k + 8 if size <= 4 else value
        raw = data[at:at + size]
        if len(raw) != size:
            raise Refused("tag %d: values run past the file" % tag)
        if typ == 2:
            vals = raw
        elif typ in FMT:
            vals = struct.unpack("<%d%s" % (count, FMT[typ]), raw)
        else:
            vals = None
        tags[tag] = (typ, count, vals)
    return tags


def parse(data):
    """what amhip_geotiff_info reports, plus "chunks": [(offset, count, rows)] in row-major order"""
    tags = read_ifd(data)

    def scalar(tag, default):
        return tags[tag][2][0] if tag in tags else default

    def refuse(tag, what):
        raise Refused("tag %d: %s" % (tag, what))
    width, height = scalar(256, 0), scalar(257, 0)
    if not 1 <= width <= 1 << 20:
        refuse(256, width)
    if not 1 <= height <= 1 << 20:
        refuse(257, height)
    compression = scalar(259, 1)
    if compression not in (1, 8, 32946):
        refuse(259, compression)
    if scalar(262, 1) == 3 or 320 in tags:
        refuse(262, "palette")
    if scalar(266, 1) != 1:
        refuse(266, scalar(266, 1))
    if scalar(274, 1) != 1:
        refuse(274, scalar(274, 1))
    bands = scalar(277, 1)
    if bands not in (1, 3):
        refuse(277, bands)
    if 338 in tags and tags[338][1] > 0:
        refuse(338, "extra samples")
    bits = set(tags[258][2]) if 258 in tags else {1}
    fmts = set(tags[339][2]) if 339 in tags else {1}
    if len(bits) != 1 or (258 in tags and tags[258][1] not in (1, bands)):
        refuse(258, sorted(bits))
    if len(fmts) != 1 or (339 in tags and tags[339][1] not in (1, bands)):
        refuse(339, sorted(fmts))
    bits, fmt = bits.pop(), fmts.pop()
    if bands == 3:
        if bits != 8:
            refuse(258, bits)
        if fmt != 1:
            refuse(339, fmt)
        if scalar(284, 1) != 1:
            refuse(284, scalar(284, 1))
        kind = "rgb8"
    else:
        kind = {(32, 3): "f32", (8, 1): "u8", (16, 1): "u16", (16, 2): "i16"}.get((bits, fmt))
        if kind is None:
            refuse(258 if bits not in (8, 16, 32) else 339, (bits, fmt))
    predictor = scalar(317, 1)
    if predictor not in (1, 2, 3) or (predictor == 3 and kind != "f32"):
        refuse(317, predictor)
    if compression == 1:
        predictor = 1      # (libtiff's predictor belongs to its LZW and Deflate codecs: not acted on here)
    px = pixel_bytes(kind)
    if 322 in tags or 323 in tags or 324 in tags:
        tw, th = scalar(322, 0), scalar(323, 0)
        if tw < 16 or tw % 16:
            refuse(322, tw)
        if th < 16 or th % 16:
            refuse(323, th)
        tiled, cw, ch = 1, tw, th
        across, down = -(-width // tw), -(-height // th)
        off_tag, cnt_tag = 324, 325
    else:
        rps = scalar(278, 0xFFFFFFFF)
        if rps < 1:
            refuse(278, rps)
        rps = min(rps, height)
        tiled, cw, ch = 0, width, rps
        across, down = 1, -(-height // rps)
        off_tag, cnt_tag = 273, 279
    for t in (off_tag, cnt_tag):
        if t not in tags or tags[t][0] not in (3, 4):
            refuse(t, "missing")
        if tags[t][1] != across * down:
            refuse(t, "%d entries for %d chunks" % (tags[t][1], across * down))
    chunks = []
    for t, (off, cnt) in enumerate(zip(tags[off_tag][2], tags[cnt_tag][2])):
        rows = ch if tiled else min(ch, height - t * ch)
        if off + cnt > len(data):
            raise Refused("chunk %d runs past the file" % t)
        if compression == 1:
            if cnt != rows * cw * px:
                raise Refused("chunk %d: %d bytes uncompressed" % (t, cnt))
        else:
            if cnt < 6:
                raise Refused("chunk %d: no zlib stream" % t)
            cmf, flg = data[off], data[off + 1]
            if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 0x20:
                raise Refused("chunk %d: zlib header" % t)
        chunks.append((off, cnt, rows))
    gt, has_geo = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0], False
    if 33550 in tags or 33922 in tags:
        if 33550 not in tags:
            refuse(33550, "missing")
        if 33922 not in tags or tags[33922][1] != 6:
            refuse(33922, "one tiepoint is read")
        sx, sy = np.float64(tags[33550][2][0]), np.float64(tags[33550][2][1])
        tie = [np.float64(v) for v in tags[33922][2]]
        gt = [tie[3] - tie[0] * sx, sx, 0.0, tie[4] + tie[1] * sy, 0.0, -sy]
        has_geo = True
    elif 34264 in tags:
        m = [np.float64(v) for v in tags[34264][2]]
        if len(m) != 16 or m[1] != 0.0 or m[4] != 0.0:
            refuse(34264, "rotation")
        gt = [m[3], m[0], 0.0, m[7], 0.0, m[5]]
        has_geo = True
    raster_type, epsg = 1, 0
    if 34735 in tags:
        keys = tags[34735][2]
        if len(keys) < 4 or 4 + 4 * keys[3] > len(keys):
            refuse(34735, "directory")
        for k in range(1, keys[3] + 1):
            kid, loc, _, value = keys[4 * k:4 * k + 4]
            if loc == 0 and kid == 1025:
                if value not in (1, 2):
                    refuse(34735, "RasterType %d" % value)
                raster_type = value
            if loc == 0 and kid == 3072:
                epsg = value
    if has_geo:
        if not (gt[1] > 0.0 and gt[5] < 0.0):
            raise Refused("geo tags: not north-up")
        if raster_type == 2:
            gt[0] = gt[0] - np.float64(0.5) * gt[1]
            gt[3] = gt[3] - np.float64(0.5) * gt[5]
    nodata = None
    if 42113 in tags:
        text = bytes(tags[42113][2])[:63].split(b"\0")[0].decode("latin-1").strip()
        try:
            nodata = float(text)
        except ValueError:
            refuse(42113, text)
    return {"width": width, "height": height, "bands": bands, "kind": kind, "tiled": tiled,
            "tile_width": cw if tiled else 0, "tile_height": ch if tiled else 0,
            "rows_per_strip": 0 if tiled else ch, "compression": compression, "predictor": predictor,
            "has_geo": has_geo, "geotransform": tuple(float(v) for v in gt), "epsg": epsg,
            "raster_type": raster_type, "nodata": nodata,
            "chunks": chunks, "chunk_w": cw, "chunk_h": ch, "across": across, "down": down}


# ---- rules 2 - 4 -----------------------------------------------------------------------------------

def unpredict(coded, kind, predictor, w):
    """coded: (rows, w * bytes per pixel) uint8 of one chunk -> the same shape, the predictor undone"""
    px = pixel_bytes(kind)
    rows = coded.shape[0]
    if predictor == 1:
        return coded
    if predictor == 3:
        summed = np.cumsum(coded, axis=1, dtype=np.uint8)
        return np.ascontiguousarray(summed.reshape(rows, 4, w).transpose(0, 2, 1)[:, :, ::-1]).reshape(rows, 4 * w)
    bands = 3 if kind == "rgb8" else 1
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[px // bands]
    samples = np.ascontiguousarray(coded).view(word).reshape(rows, w, bands)
    return np.ascontiguousarray(np.cumsum(samples, axis=1, dtype=word)).view(np.uint8).reshape(rows, w * px)


def predict(plain, kind, predictor, w):
    """the writer's direction"""
    px = pixel_bytes(kind)
    rows = plain.shape[0]
    if predictor == 1:
        return plain
    if predictor == 3:
        planes = np.ascontiguousarray(plain.reshape(rows, w, 4)[:, :, ::-1].transpose(0, 2, 1)).reshape(rows, 4 * w)
        out = planes.copy()
        out[:, 1:] = planes[:, 1:] - planes[:, :-1]
        return out
    bands = 3 if kind == "rgb8" else 1
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[px // bands]
    samples = np.ascontiguousarray(plain).view(word).reshape(rows, w, bands)
    out = samples.copy()
    out[:, 1:] = samples[:, 1:] - samples[:, :-1]
    return np.ascontiguousarray(out).view(np.uint8).reshape(rows, w * px)


def decode(data):
    """-> (raster in the file's dtype, parse(data))"""
    p = parse(data)
    kind, px, cw, ch = p["kind"], pixel_bytes(p["kind"]), p["chunk_w"], p["chunk_h"]
    full = np.zeros((p["down"] * ch, p["across"] * cw * px), np.uint8)
    for t, (off, cnt, rows) in enumerate(p["chunks"]):
        z = bytes(data[off:off + cnt])
        raw = z if p["compression"] == 1 else zlib.decompress(z)
        if len(raw) != rows * cw * px:
            raise Refused("chunk %d: %d bytes behind the decompressor" % (t, len(raw)))
        coded = np.frombuffer(raw, np.uint8).reshape(rows, cw * px)
        ty, tx = divmod(t, p["across"])
        full[ty * ch:ty * ch + rows, tx * cw * px:(tx + 1) * cw * px] = unpredict(coded, kind, p["predictor"], cw)
    crop = np.ascontiguousarray(full[:p["height"], :p["width"] * px])
    raster = crop.view(DTYPES[kind])
    if kind == "rgb8":
        raster = raster.reshape(p["height"], p["width"], 3)
    return raster, p


# ---- rule 5 ----------------------------------------------------------------------------------------

def place(before, grid, window, info, raster):
    """before: the window's layer as AerialGridMap.get() gives it, shape (cols, rows), a[j, i] = cell
    (i, j); window = (i0, j0, rows, cols) of the map `grid` -> the layer after the call"""
    i0, j0, rows, cols = window
    res = np.float64(grid.resolution)
    base_x = np.float64(grid.pos_x) + (np.float64(0.5) * np.float64(grid.length_x) - np.float64(0.5) * res)
    base_y = np.float64(grid.pos_y) + (np.float64(0.5) * np.float64(grid.length_y) - np.float64(0.5) * res)
    x = base_x + res * (-(np.arange(rows) + i0).astype(np.float64))
    y = base_y + res * (-(np.arange(cols) + j0).astype(np.float64))
    gt = [np.float64(v) for v in info["geotransform"]]
    col = np.floor((x - gt[0]) / gt[1])
    row = np.floor((y - gt[3]) / gt[5])
    h, w = raster.shape[:2]
    ok = ((row >= 0) & (row < h))[:, None] & ((col >= 0) & (col < w))[None, :]
    r = np.clip(np.nan_to_num(row), 0, h - 1).astype(np.int64)
    c = np.clip(np.nan_to_num(col), 0, w - 1).astype(np.int64)
    pix = raster[r[:, None], c[None, :]]
    nodata = info["nodata"]
    kind = info["kind"]
    if kind == "f32":
        value = pix.view(np.uint32)
        ok &= ~np.isnan(pix)
        if nodata is not None:
            ok &= ~(pix == np.float32(nodata))
    elif kind == "rgb8":
        p32 = pix.astype(np.uint32)
        value = (p32[..., 0] << 16) | (p32[..., 1] << 8) | p32[..., 2]
        if nodata is not None:
            ok &= ~np.all(pix.astype(np.float64) == nodata, axis=-1)
    else:
        value = pix.astype(np.float32).view(np.uint32)
        if nodata is not None:
            ok &= ~(pix.astype(np.float64) == nodata)
    out = np.array(before, np.float32, copy=True).view(np.uint32)
    out[ok] = value[ok]
    return out.view(np.float32)


# ---- the writer of every accepted variant -----------------------------------------------------------

def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(raw) + c.flush()


def geo_entries(gt, form="scale", pixel_is_point=False, epsg=32632):
    """{tag: (type, values)}; gt describes pixel AREAS: a PixelIsPoint file's tiepoint is moved to the
    first pixel's centre, so that the reader finds gt again"""
    gt = [float(v) for v in gt]
    x0, y0 = (gt[0] + 0.5 * gt[1], gt[3] + 0.5 * gt[5]) if pixel_is_point else (gt[0], gt[3])
    keys = [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 2 if pixel_is_point else 1, 3072, 0, 1, epsg]
    out = {34735: (3, keys)}
    if form == "scale":
        out[33550] = (12, [gt[1], -gt[5], 0.0])
        out[33922] = (12, [0.0, 0.0, 0.0, x0, y0, 0.0])
    else:
        out[34264] = (12, [gt[1], 0.0, 0.0, x0, 0.0, gt[5], 0.0, y0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    return out


def write(raster, tile=None, rows_per_strip="absent", compression=8, predictor=1, level=6,
          strategy=zlib.Z_DEFAULT_STRATEGY, gt=None, geo_form="scale", pixel_is_point=False, epsg=32632,
          nodata=None, extra_tags=None, drop_tags=()):
    """The file.  tile = (tile width, tile length): tiles; else strips of rows_per_strip rows ("absent":
    no tag 278, one strip).  gt None: no geo tags.  nodata: the tag's text.  extra_tags: {tag: (type,
    values)} added or overriding (the refusal tests)."""
    raster = np.asarray(raster)
    kind = kind_of(raster)
    px = pixel_bytes(kind)
    bands = 3 if kind == "rgb8" else 1
    h, w = raster.shape[:2]
    rows_bytes = np.ascontiguousarray(raster).view(np.uint8).reshape(h, w * px)
    payloads = []
    tag_predictor = predictor
    if compression == 1:
        predictor = 1      # (the tag is written as asked for and, as by libtiff, not acted on)
    if tile is not None:
        tw, th = tile
        for ty in range(-(-h // th)):
            for tx in range(-(-w // tw)):
                full = np.zeros((th, tw * px), np.uint8)
                part = rows_bytes[ty * th:(ty + 1) * th, tx * tw * px:(tx + 1) * tw * px]
                full[:part.shape[0], :part.shape[1]] = part
                payloads.append(predict(full, kind, predictor, tw).tobytes())
    else:
        rps = h if rows_per_strip == "absent" else min(int(rows_per_strip), h)
        for r0 in range(0, h, rps):
            payloads.append(predict(rows_bytes[r0:r0 + rps], kind, predictor, w).tobytes())
    chunks = [p if compression == 1 else deflate(p, level, strategy) for p in payloads]
    bits = {"f32": 32, "u8": 8, "rgb8": 8, "u16": 16, "i16": 16}[kind]
    fmt = {"f32": 3, "i16": 2}.get(kind, 1)
    tags = {256: (4, [w]), 257: (4, [h]), 258: (3, [bits] * bands), 259: (3, [compression]),
            262: (3, [2 if bands == 3 else 1]), 277: (3, [bands]), 284: (3, [1]), 339: (3, [fmt] * bands)}
    if tag_predictor != 1:
        tags[317] = (3, [tag_predictor])
    if tile is not None:
        tags[322], tags[323] = (4, [tile[0]]), (4, [tile[1]])
        off_tag, cnt_tag = 324, 325
    else:
        if rows_per_strip != "absent":
            tags[278] = (4, [int(rows_per_strip)])
        off_tag, cnt_tag = 273, 279
    tags[off_tag] = (4, [0] * len(chunks))
    tags[cnt_tag] = (4, [len(c) for c in chunks])
    if gt is not None:
        tags.update(geo_entries(gt, geo_form, pixel_is_point, epsg))
    if nodata is not None:
        text = nodata if isinstance(nodata, bytes) else (str(nodata).encode() + b"\0")
        tags[42113] = (2, text)
    tags.update(extra_tags or {})
    for t in drop_tags:
        tags.pop(t, None)

    def payload(typ, values):
        if typ == 2:
            return bytes(values)
        return struct.pack("<%d%s" % (len(values), FMT[typ]), *values)
    order = sorted(tags)
    at = 8 + 2 + 12 * len(order) + 4
    where = {}
    for t in order:
        size = len(payload(*tags[t]))
        if size > 4:
            where[t] = at
            at += size + (size & 1)
    data_at = (at + 15) & ~15
    offs, run = [], data_at
    for c in chunks:
        offs.append(run)
        run += len(c) + (-len(c) & 1)    # (chunks at even offsets, otherwise as they come)
    if off_tag in tags and len(tags[off_tag][1]) == len(chunks):
        tags[off_tag] = (tags[off_tag][0], offs)
    head = bytearray(data_at)
    head[:8] = b"II" + struct.pack("<HI", 42, 8)
    struct.pack_into("<H", head, 8, len(order))
    for k, t in enumerate(order):
        typ, values = tags[t]
        raw = payload(typ, values)
        entry = 10 + 12 * k
        struct.pack_into("<HHI", head, entry, t, typ, len(raw) // TYPE_SIZE[typ])
        if t in where:
            struct.pack_into("<I", head, entry + 8, where[t])
            head[where[t]:where[t] + len(raw)] = raw
        else:
            head[entry + 8:entry + 8 + len(raw)] = raw
    out = bytearray(head)
    for c in chunks:
        out += c + b"\0" * (-len(c) & 1)
    return bytes(out)
