"""Inputs of the GeoTIFF pyramid tests: rasters of every kind at the sizes that reach an
edge, contents that separate the reduction rule from its neighbours, the files foreign writers leave,
and the committed fixtures."""
import glob
import os

import numpy as np

import geotiff_pyramid_reference as P
import geotiff_read_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "geotiff_pyramid")
GT = (464500.25, 0.5, 0.0, 5272800.75, 0.0, -0.5)

# (width, height, tile): the smallest that reach each edge
SIZES = [(2, 2, 16), (3, 5, 16), (1, 9, 16), (17, 33, 16), (31, 16, 16), (64, 48, 16), (100, 70, 32)]
KINDS = ("f32", "u8", "rgb8")


def raster(kind, w, h, seed=7):
    rng = np.random.default_rng(seed + 1000 * w + h)
    if kind == "f32":
        a = (rng.standard_normal((h, w)) * 30.0 + 400.0).astype(np.float32)
        a[rng.random((h, w)) < 0.2] = np.nan
        return a
    if kind == "u8":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def f32_hard():
    """13 x 12: blocks with 0..4 NaN in every position, a NaN column on the odd edge, a NaN with a payload,
    infinities, -0.0, denormals, 1e30 beside 1 in both orders, four values whose float64 sum rounds
    otherwise than their float32 sum"""
    f = np.float32
    nan = f(np.nan)
    a = np.full((12, 13), 1.5, np.float32)
    # rows 0..7, columns 0..7: the sixteen NaN patterns of a block, one block each
    for m in range(16):
        r, c = 2 * (m // 4), 2 * (m % 4)
        vals = np.array([3.25, -7.5, 100.125, 0.0625], np.float32) * f(m + 1)
        for k in range(4):
            a[r + (k >> 1), c + (k & 1)] = nan if m >> k & 1 else vals[k]
    a[:, 12] = nan                                                   # the odd edge: blocks of 2, all NaN
    a[0, 8:12] = np.array([0x7FA00123, 0xFFC00001, 0x7F800001, 0x7FC00000], np.uint32).view(np.float32)
    a[1, 8:12] = nan                                                  # payloads only: canonical NaN out
    a[2, 8:10], a[3, 8:10] = [np.inf, 1.0], [2.0, 3.0]
    a[2, 10:12], a[3, 10:12] = [np.inf, -np.inf], [1.0, 2.0]
    a[4, 8:10], a[5, 8:10] = [-0.0, -0.0], [-0.0, -0.0]
    a[4, 10:12], a[5, 10:12] = np.array([1, 2, 3, 0x007FFFFF], np.uint32).view(np.float32).reshape(2, 2)
    a[6, 8:10], a[7, 8:10] = [1e30, 1.0], [-1e30, 1.0]
    a[6, 10:12], a[7, 10:12] = [1.0, 1e30], [1.0, -1e30]
    a[8, 0:2], a[9, 0:2] = [16777216.0, 1.0], [1.0, 1.0]               # float32 sum loses the ones
    a[8, 2:4], a[9, 2:4] = [1.0000001, 1.0000002], [1.0000004, 3.4e38]
    a[8, 4:6], a[9, 4:6] = [3.4e38, 3.4e38], [3.4e38, 3.4e38]          # the sum exceeds float32, the mean does not
    a[10, 0:2], a[11, 0:2] = [-np.inf, nan], [nan, -np.inf]
    return a


def u8_hard():
    """7 x 5: sums with remainder 2 of 4, clipped blocks of 2 with an odd sum, and of 1"""
    a = np.array([[1, 1, 0, 0, 255, 255, 3],
                  [0, 0, 1, 0, 255, 254, 4],
                  [1, 2, 2, 2, 0, 1, 255],
                  [2, 2, 3, 4, 1, 1, 254],
                  [7, 8, 254, 255, 0, 1, 9]], np.uint8)
    return a


def rgb8_hard():
    """per-band independence: every band its own pattern"""
    a = u8_hard()
    return np.stack([a, a[::-1, ::-1], (a.astype(np.int32) * 7 % 256).astype(np.uint8)], axis=-1)


def foreign():
    """{name: (file, [the levels' rasters])}: what other writers leave"""
    out = {}
    base = raster("f32", 40, 36)
    l1, l2 = P.reduce(base), P.reduce(P.reduce(base))
    mask = (np.arange(36 * 40).reshape(36, 40) % 3 == 0).astype(np.uint8) * 255
    page = raster("u8", 20, 18)
    w = lambda a, sub=None, **kw: R.write(a, extra_tags=None if sub is None else P.subfile(sub), **kw)
    # tiled base, strip-based overviews with Predictor 3 and 2 strips
    out["strips"] = (P.chain([w(base, tile=(16, 16), predictor=3, gt=GT, nodata="nan"),
                              w(l1, 1, rows_per_strip=7, predictor=3),
                              w(l2, 1, predictor=1)]), [base, l1, l2])
    # a mask (254 = 4) and a mask of an overview (254 = 5) and a page (254 absent) between the levels
    out["mask_page"] = (P.chain([w(base, tile=(16, 16), predictor=3, gt=GT),
                                 w(mask, 4, tile=(16, 16)),
                                 w(l1, 1, tile=(32, 16), predictor=3),
                                 w(page, None, rows_per_strip=5),
                                 w(mask[::2, ::2], 5, tile=(16, 16)),
                                 w(page, 2, rows_per_strip=5),
                                 w(l2, 1, tile=(16, 16), predictor=2)]), [base, l1, l2])
    rgb = raster("rgb8", 33, 20)
    out["rgb_uncompressed"] = (P.chain([w(rgb, rows_per_strip=6, gt=GT, compression=1),
                                        w(P.reduce(rgb), 1, tile=(16, 16), predictor=2)]), [rgb, P.reduce(rgb)])
    return out


def refused_chains():
    """{name: (file, level asked, a word of the text)}"""
    base = raster("u8", 20, 18)
    l1 = P.reduce(base)
    w = lambda a, sub=None, **kw: R.write(a, extra_tags=None if sub is None else P.subfile(sub), **kw)
    out = {}
    good = P.chain([w(base, gt=GT), w(l1, 1)])
    chain = P.ifd_chain(good)
    import struct
    loop = bytearray(good)
    n, = struct.unpack_from("<H", loop, chain[1][0])
    struct.pack_into("<I", loop, chain[1][0] + 2 + 12 * n, chain[0][0])
    out["loop"] = (bytes(loop), 1, "returns")
    out["65_ifds"] = (P.chain([w(base, gt=GT)] + [w(raster("u8", 2, 2), None)] * 64), 0, "more than 64")
    out["larger"] = (P.chain([w(base, gt=GT), w(l1, 1), w(base[:10, :12], 1)]), 2, "not smaller")
    out["same_size"] = (P.chain([w(base, gt=GT), w(base, 1)]), 1, "not smaller")
    out["other_kind"] = (P.chain([w(base, gt=GT), w(raster("f32", 10, 9), 1)]), 1, "kind")
    out["no_such_level"] = (good, 2, "level 2")
    lzw = bytearray(good)
    # the overview's Compression becomes 5 (LZW): level 0 still reads
    n1, = struct.unpack_from("<H", lzw, chain[1][0])
    for k in range(n1):
        e = chain[1][0] + 2 + 12 * k
        if struct.unpack_from("<H", lzw, e)[0] == 259:
            struct.pack_into("<H", lzw, e + 8, 5)
    out["level_lzw"] = (bytes(lzw), 1, "level 1 (IFD 1")
    return out


def fixture_paths():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.tif")))


def fixtures():
    """{name: (raster, tile, overviews)}: the committed pyramid files, written by the reference"""
    return {"f32_hard_13x12_t16_o2": (f32_hard(), 16, 2),
            "f32_17x33_t16_auto": (raster("f32", 17, 33), 16, -1),
            "u8_hard_7x5_t16_o3": (u8_hard(), 16, 3),
            "u8_31x16_t16_o1": (raster("u8", 31, 16), 16, 1),
            "rgb8_hard_7x5_t16_o2": (rgb8_hard(), 16, 2),
            "rgb8_33x20_t16_auto": (raster("rgb8", 33, 20), 16, -1)}
