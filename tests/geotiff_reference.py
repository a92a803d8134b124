"""The tiled Deflate GeoTIFF the GPU encoder (amhip_tiff_encode.hip) has to write, restated on the
host, and its inverse.  DESIGN 4.16.

  1 raster kinds   f32: one band of 32-bit floats, Predictor 3, SampleFormat 3, GDAL_NODATA "nan"
                   u8: one band of bytes, Predictor 2, BlackIsZero
                   rgb8: three bands of bytes, pixel interleaved, Predictor 2, Photometric RGB
  2 tiles          square, side a multiple of 16 in 16..1024, row-major tile order, every tile full
                   size, zero bytes outside the raster before the predictor
  3 predictor      per tile row.  f32 (libtiff's fpDiff): four byte planes, most significant first,
                   then differenced with stride 1 across the whole row; u8 / rgb8: byte k minus
                   byte k - bands
  4 stream         one zlib stream per tile: level 1, Z_RLE, window 15, memLevel 8
                   (png_encode_reference.zlib_stream restates it, zlib_rle_stream is the library)
  5 container      classic little-endian TIFF, the IFD at offset 8, tags ascending, out-of-line
                   values behind it in tag order, word aligned, tile tables as LONG (inline for one
                   tile), tile data from the next multiple of 16, tightly packed
  6 geo tags       ModelPixelScale, ModelTiepoint, GeoKeyDirectory, GeoAsciiParams as
                   amhip_geotiff_write_u8 writes them
"""
import struct
import zlib

import numpy as np

import png_encode_reference as PR

KINDS = {"f32": 0, "u8": 1, "rgb8": 2}
SHORT, LONG, ASCII, DOUBLE = 3, 4, 2, 12
TYPE_SIZE = {SHORT: 2, LONG: 4, ASCII: 1, DOUBLE: 8}


def kind_of(raster):
    raster = np.asarray(raster)
    if raster.ndim == 3:
        assert raster.dtype == np.uint8 and raster.shape[2] == 3
        return "rgb8"
    assert raster.ndim == 2 and raster.dtype in (np.float32, np.uint8)
    return "f32" if raster.dtype == np.float32 else "u8"


def tile_rows(raster, kind, side, ty, tx):
    """rule 2: the (side, side * bytes per pixel) bytes of tile (ty, tx) before the predictor"""
    px = {"f32": 4, "u8": 1, "rgb8": 3}[kind]
    h, w = raster.shape[:2]
    full = np.zeros((side, side * px), np.uint8)
    r0, c0 = ty * side, tx * side
    part = np.ascontiguousarray(raster[r0:r0 + side, c0:c0 + side])
    nr, nc = part.shape[:2]
    full[:nr, :nc * px] = part.view(np.uint8).reshape(nr, nc * px)
    return full


def predict(rows, kind, side):
    """rule 3"""
    if kind == "f32":
        planes = rows.reshape(side, side, 4)[:, :, ::-1].transpose(0, 2, 1).reshape(side, 4 * side)
        stride = 1
    else:
        planes = rows
        stride = 1 if kind == "u8" else 3
    out = planes.copy()
    out[:, stride:] = planes[:, stride:] - planes[:, :-stride]
    return out


def unpredict(coded, kind, side):
    stride = 3 if kind == "rgb8" else 1
    rows = coded.copy()
    for s in range(stride):
        rows[:, s::stride] = np.cumsum(coded[:, s::stride], axis=1, dtype=np.uint8)
    if kind == "f32":
        rows = rows.reshape(side, 4, side).transpose(0, 2, 1)[:, :, ::-1].reshape(side, 4 * side)
    return np.ascontiguousarray(rows)


def tile_payloads(raster, side):
    """the predictor bytes of every tile, in row-major tile order"""
    raster = np.asarray(raster)
    kind = kind_of(raster)
    h, w = raster.shape[:2]
    return [predict(tile_rows(raster, kind, side, ty, tx), kind, side).tobytes()
            for ty in range((h + side - 1) // side) for tx in range((w + side - 1) // side)]


def geo_tags(geotransform, utm_zone, northern):
    """rule 6: {tag: (type, count, payload bytes)}"""
    gt = [float(v) for v in geotransform]
    citation = "UTM %d (WGS84) in %s hemisphere.|" % (utm_zone, "northern" if northern else "southern")
    ascii_ = (citation + "WGS 84|").encode() + b"\0"
    keys = [1, 1, 0, 7,
            1024, 0, 1, 1,
            1025, 0, 1, 1,
            1026, 34737, len(citation), 0,
            2048, 0, 1, 4326,
            2049, 34737, 7, len(citation),
            3072, 0, 1, (32600 if northern else 32700) + utm_zone,
            3076, 0, 1, 9001]
    return {33550: (DOUBLE, 3, struct.pack("<3d", gt[1], -gt[5], 0.0)),
            33922: (DOUBLE, 6, struct.pack("<6d", 0.0, 0.0, 0.0, gt[0], gt[3], 0.0)),
            34735: (SHORT, 32, struct.pack("<32H", *keys)),
            34737: (ASCII, len(ascii_), ascii_)}


def container(width, height, kind, side, geotransform, utm_zone, northern, counts):
    """rule 5: the file in front of the tile data, and the file's size"""
    bands = 3 if kind == "rgb8" else 1
    n = len(counts)
    short = lambda *v: (SHORT, len(v), struct.pack("<%dH" % len(v), *v))
    long_ = lambda *v: (LONG, len(v), struct.pack("<%dI" % len(v), *v))
    tags = {256: long_(width), 257: long_(height),
            258: short(*([8] * 3 if bands == 3 else [32 if kind == "f32" else 8])),
            259: short(8), 262: short(2 if bands == 3 else 1), 277: short(bands), 284: short(1),
            317: short(3 if kind == "f32" else 2), 322: long_(side), 323: long_(side),
            324: None, 325: None,
            339: short(*([1] * 3 if bands == 3 else [3 if kind == "f32" else 1]))}
    tags.update(geo_tags(geotransform, utm_zone, northern))
    if kind == "f32":
        tags[42113] = (ASCII, 4, b"nan\0")
    order = sorted(tags)
    at = 8 + 2 + 12 * len(order) + 4
    where = {}
    for tag in order:
        size = 4 * n if tags[tag] is None else len(tags[tag][2])
        if size > 4:
            where[tag] = at
            at += size + (size & 1)
    data_at = (at + 15) & ~15
    offsets, run = [], data_at
    for c in counts:
        offsets.append(run)
        run += c
    if run > 0xFFFFFFFF:
        raise ValueError("the file would exceed 2^32 - 1 bytes")
    tags[324] = long_(*offsets)
    tags[325] = long_(*counts)
    head = bytearray(data_at)
    head[:8] = b"II" + struct.pack("<HI", 42, 8)
    struct.pack_into("<H", head, 8, len(order))
    for k, tag in enumerate(order):
        typ, count, payload = tags[tag]
        entry = 10 + 12 * k
        struct.pack_into("<HHI", head, entry, tag, typ, count)
        if tag in where:
            struct.pack_into("<I", head, entry + 8, where[tag])
            head[where[tag]:where[tag] + len(payload)] = payload
        else:
            head[entry + 8:entry + 8 + len(payload)] = payload
    return bytes(head), run


def encode(raster, geotransform, utm_zone=32, northern=True, tile=256, stream=PR.zlib_stream):
    """The file.  stream: predictor bytes of a tile -> its zlib stream (the restatement by default;
    PR.zlib_rle_stream is the library itself)."""
    raster = np.asarray(raster)
    kind = kind_of(raster)
    side = tile or 256
    assert side % 16 == 0 and 16 <= side <= 1024
    streams = [stream(p) for p in tile_payloads(raster, side)]
    head, total = container(raster.shape[1], raster.shape[0], kind, side, geotransform, utm_zone, northern,
                            [len(z) for z in streams])
    out = head + b"".join(streams)
    assert len(out) == total
    return out


def parse_ifd(data):
    """{tag: (type, count, values)} of the first IFD; ASCII values as bytes"""
    assert data[:4] == b"II*\0"
    ifd, = struct.unpack_from("<I", data, 4)
    n, = struct.unpack_from("<H", data, ifd)
    tags = {}
    prev = -1
    for k in range(n):
        tag, typ, count, value = struct.unpack_from("<HHII", data, ifd + 2 + 12 * k)
        assert tag > prev, "tags ascend"
        prev = tag
        size = TYPE_SIZE[typ] * count
        at = ifd + 2 + 12 * k + 8 if size <= 4 else value
        if size > 4:
            assert value % 2 == 0, "values are word aligned"
        raw = data[at:at + size]
        assert len(raw) == size
        if typ == ASCII:
            vals = raw
        else:
            vals = struct.unpack("<%d%s" % (count, {SHORT: "H", LONG: "I", DOUBLE: "d"}[typ]), raw)
        tags[tag] = (typ, count, vals)
    assert struct.unpack_from("<I", data, ifd + 2 + 12 * n)[0] == 0
    return tags


def decode(data):
    """The inverse: {"raster", "kind", "tile", "geotransform", "epsg", "tags", "streams"}."""
    tags = parse_ifd(data)
    v = lambda t: tags[t][2]
    width, height = v(256)[0], v(257)[0]
    assert v(259) == (8,) and v(284) == (1,) and 273 not in tags and 278 not in tags and 279 not in tags
    side = v(322)[0]
    assert v(323)[0] == side
    bands = v(277)[0]
    if bands == 3:
        kind = "rgb8"
        assert v(258) == (8, 8, 8) and v(339) == (1, 1, 1) and v(262) == (2,) and v(317) == (2,)
    elif v(258) == (32,):
        kind = "f32"
        assert v(339) == (3,) and v(317) == (3,) and v(262) == (1,) and v(42113) == b"nan\0"
    else:
        kind = "u8"
        assert v(258) == (8,) and v(339) == (1,) and v(317) == (2,) and v(262) == (1,)
    px = {"f32": 4, "u8": 1, "rgb8": 3}[kind]
    across, down = (width + side - 1) // side, (height + side - 1) // side
    offs, cnts = v(324), v(325)
    assert len(offs) == len(cnts) == across * down
    full = np.zeros((down * side, across * side * px), np.uint8)
    streams = []
    at = offs[0]
    assert at % 16 == 0
    for t in range(across * down):
        assert offs[t] == at, "tiles are tightly packed in order"
        z = data[offs[t]:offs[t] + cnts[t]]
        assert len(z) == cnts[t]
        streams.append(z)
        at += cnts[t]
        coded = np.frombuffer(zlib.decompress(z), np.uint8)
        assert coded.size == side * side * px
        ty, tx = divmod(t, across)
        full[ty * side:(ty + 1) * side, tx * side * px:(tx + 1) * side * px] = \
            unpredict(coded.reshape(side, side * px), kind, side)
    assert at == len(data)
    crop = np.ascontiguousarray(full[:height, :width * px])
    if kind == "f32":
        raster = crop.view(np.float32)
    elif kind == "u8":
        raster = crop
    else:
        raster = crop.reshape(height, width, 3)
    scale, tie = v(33550), v(33922)
    keys = v(34735)
    epsg = [keys[4 * k + 3] for k in range(1, keys[3] + 1) if keys[4 * k] == 3072][0]
    return {"raster": raster, "kind": kind, "tile": side, "tags": tags, "streams": streams, "epsg": epsg,
            "geotransform": (tie[3], scale[0], 0.0, tie[4], 0.0, -scale[1])}


def layer_raster(layer, kind, lower=0.0, upper=255.0):
    """The north-up raster of a layer as AerialGridMap.get() gives it -- shape (cols, rows), a[j, i] =
    cell (i, j) -- by DESIGN 4.16: width = rows, height = cols, pixel (r, c) = cell (rows - 1 - c, r)."""
    a = np.asarray(layer, np.float32)
    north = np.ascontiguousarray(a[:, ::-1])
    if kind == "f32":
        return north
    if kind == "u8":
        # grid_map_cv's toImage: float arithmetic, truncating cast, non-finite -> 0
        lo, hi = np.float32(lower), np.float32(upper)
        with np.errstate(invalid="ignore"):
            v = np.minimum(np.maximum(north, lo), hi)
            t = ((v - lo) / (hi - lo)) * np.float32(255.0)
        out = np.zeros(north.shape, np.uint8)
        ok = np.isfinite(north)
        out[ok] = t[ok].astype(np.int32).astype(np.uint8)
        return out
    bits = north.view(np.uint32)
    bits = np.where(np.isnan(north), 0, bits)
    return np.stack([(bits >> 16) & 255, (bits >> 8) & 255, bits & 255], axis=-1).astype(np.uint8)


def layer_geotransform(grid, window):
    """{x0, res, 0, y0, 0, -res} of a context's window (i0, j0, rows, cols) of the map `grid`"""
    i0, j0, rows, _ = window
    res = grid.resolution
    return (grid.pos_x - grid.length_x / 2 + res * float(grid.rows - i0 - rows), res, 0.0,
            grid.pos_y + grid.length_y / 2 - res * float(j0), 0.0, -res)
