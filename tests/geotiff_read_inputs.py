"""Files for the GeoTIFF reader's tests: every accepted variant from the test writer
(geotiff_read_reference.write), the refusals, and the committed files libtiff wrote
(tests/golden/geotiff_read/, tests/golden/make_geotiff_read_golden.py).  Everything is a function of
its arguments and a fixed seed."""
import glob
import os
import struct
import zlib

import numpy as np

import geotiff_inputs as GI
import geotiff_read_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GT = GI.GT


def fixture_paths():
    """the committed files: libtiff's (through Pillow) and the GPU writer's own"""
    return sorted(glob.glob(os.path.join(HERE, "golden", "geotiff_read", "*.tif")) +
                  glob.glob(os.path.join(HERE, "golden", "geotiff", "*.tif")))


def words16(h, w, signed):
    """16-bit samples whose differences carry across the byte boundary; negative ones when signed"""
    a = (np.arange(w, dtype=np.int64)[None, :] * 251 + np.arange(h, dtype=np.int64)[:, None] * 4099)
    if signed:
        return ((a % 65536) - 32768).astype(np.int16)
    return (a % 65536).astype(np.uint16)


def far_match_tile():
    """128 x 128 floats, 64 KB: the lower half repeats the upper, so that with Predictor 1 every match of
    the second half lies 32768 bytes back"""
    top = GI.noise("f32", 128)[:64]
    return np.ascontiguousarray(np.concatenate([top, top]))


def variants():
    """name -> (file, raster): what decode_geotiff has to return, bit for bit"""
    out = {}

    def add(name, raster, **kw):
        kw.setdefault("gt", GT)
        out[name] = (R.write(raster, **kw), raster)
    # chunk geometry: the edge sizes at tile 16, a non-square tile, strips of every kind
    for h, w in GI.EDGE_SIZES:
        add("f32_p3_%dx%d_t16" % (h, w), GI.edge_raster("f32", h, w), tile=(16, 16), predictor=3)
    add("f32_p3_33x47_t32x16", GI.edge_raster("f32", 33, 47), tile=(32, 16), predictor=3)
    add("u8_p2_33x47_t16x32", GI.edge_raster("u8", 33, 47), tile=(16, 32), predictor=2)
    for rps in (1, 3, 17, 100, "absent"):
        add("f32_p3_17x16_rps_%s" % rps, GI.edge_raster("f32", 17, 16), rows_per_strip=rps, predictor=3)
    # row lengths for the scans
    for w in (1, 17, 70, 300):
        add("f32_p3_3x%d_strip" % w, GI.edge_raster("f32", 3, w), rows_per_strip=2, predictor=3)
        add("f32_p2_3x%d_strip" % w, GI.edge_raster("f32", 3, w), rows_per_strip=2, predictor=2)
    add("u8_p2_4x5_strip", GI.edge_raster("u8", 4, 5), predictor=2)
    add("rgb8_p2_4x7_strip", GI.edge_raster("rgb8", 4, 7), predictor=2)
    add("rgb8_p2_33x47_t16", GI.edge_raster("rgb8", 33, 47), tile=(16, 16), predictor=2)
    add("rgb8_p1_5x70_strip", GI.edge_raster("rgb8", 5, 70), rows_per_strip=2)
    add("u16_p2_5x70_strip", words16(5, 70, False), rows_per_strip=2, predictor=2)
    add("i16_p2_5x70_strip", words16(5, 70, True), rows_per_strip=2, predictor=2)
    add("i16_p2_33x47_t16", words16(33, 47, True), tile=(16, 16), predictor=2, nodata="-9999")
    add("u16_p1_33x47_t16", words16(33, 47, False), tile=(16, 16))
    add("f32_p1_33x47_t16", GI.edge_raster("f32", 33, 47), tile=(16, 16))
    # streams: every block type
    add("f32_p3_noise_128_t128_level0", GI.noise("f32", 128), tile=(128, 128), predictor=3, level=0)
    add("f32_p1_far_matches_128_t128_level9", far_match_tile(), tile=(128, 128), level=9)
    add("f32_p3_terrain_128_t128_level9", GI.terrain(128, 128), tile=(128, 128), predictor=3, level=9)
    add("f32_p3_33x47_t16_fixed", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, strategy=zlib.Z_FIXED)
    add("f32_p3_33x47_t16_none", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, compression=1)
    add("u8_p2_33x47_strip_none", GI.edge_raster("u8", 33, 47), rows_per_strip=8, predictor=2, compression=1)
    add("f32_p3_33x47_t16_32946", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, compression=32946)
    # georeferencing and nodata
    add("f32_p3_33x47_t16_matrix", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, geo_form="matrix")
    add("f32_p3_33x47_t16_point", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, pixel_is_point=True)
    add("f32_p3_33x47_t16_nogeo", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, gt=None)
    add("f32_p3_33x47_t16_nodata", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, nodata=b"-9999 \0")
    add("f32_p3_33x47_t16_nodata_nan", GI.edge_raster("f32", 33, 47), tile=(16, 16), predictor=3, nodata="nan")
    return out


def nine_tiles():
    """48 x 48 floats in 3 x 3 tiles of 16"""
    return GI.terrain(48, 48) + GI.noise("f32", 48).view(np.uint32).astype(np.float32) * np.float32(1e-12)


def refusals():
    """what -> (file, a word the refusal's text has to hold)"""
    a = GI.edge_raster("u8", 20, 20)
    f = GI.edge_raster("f32", 20, 20)
    good = R.write(a, tile=(16, 16), gt=GT)
    out = {}

    def tag(what, word, raster=a, **kw):
        kw.setdefault("tile", (16, 16))
        out[what] = (R.write(raster, **kw), word)
    out["big-endian"] = (b"MM\0*" + good[4:], "big-endian")
    out["BigTIFF"] = (good[:2] + struct.pack("<H", 43) + good[4:], "BigTIFF")
    out["no header"] = (b"II", "no TIFF header")
    out["IFD outside the file"] = (good[:4] + struct.pack("<I", len(good)) + good[8:], "IFD")
    for name, code in (("LZW", 5), ("PackBits", 32773), ("JPEG", 7), ("ZSTD", 50000), ("LERC", 34887)):
        tag(name, "tag 259 (Compression): %d" % code, extra_tags={259: (3, [code])})
    tag("64-bit samples", "tag 258 (BitsPerSample): 64", extra_tags={258: (3, [64])})
    tag("1-bit samples", "tag 258 (BitsPerSample): 1", extra_tags={258: (3, [1])})
    tag("4-bit samples", "tag 258 (BitsPerSample): 4", extra_tags={258: (3, [4])})
    tag("32-bit integers", "tag 339 (SampleFormat): 1 with 32 bits", extra_tags={258: (3, [32])})
    tag("8-bit signed", "tag 339 (SampleFormat): 2 with 8 bits", extra_tags={339: (3, [2])})
    tag("2 bands", "tag 277 (SamplesPerPixel): 2", extra_tags={277: (3, [2])})
    tag("4 bands", "tag 277 (SamplesPerPixel): 4", extra_tags={277: (3, [4])})
    tag("palette", "tag 262", extra_tags={262: (3, [3])})
    tag("colour map", "tag 262", extra_tags={320: (3, [0] * 768)})
    tag("extra samples", "tag 338 (ExtraSamples)", extra_tags={338: (3, [2])})
    tag("planar rgb", "tag 284 (PlanarConfiguration): 2", raster=GI.edge_raster("rgb8", 20, 20), extra_tags={284: (3, [2])})
    tag("16-bit rgb", "tag 258 (BitsPerSample): 16 with three bands", raster=GI.edge_raster("rgb8", 20, 20),
        extra_tags={258: (3, [16, 16, 16])})
    tag("predictor 3 on bytes", "tag 317 (Predictor): 3", extra_tags={317: (3, [3])})
    tag("predictor 4", "tag 317 (Predictor): 4", extra_tags={317: (3, [4])})
    tag("fill order", "tag 266 (FillOrder): 2", extra_tags={266: (3, [2])})
    tag("orientation", "tag 274 (Orientation): 3", extra_tags={274: (3, [3])})
    tag("tile width", "tag 322 (TileWidth): 24", extra_tags={322: (4, [24])})
    tag("tile length", "tag 323 (TileLength): 8", extra_tags={323: (4, [8])})
    tag("width 0", "tag 256 (ImageWidth): 0", extra_tags={256: (4, [0])})
    tag("height too large", "tag 257 (ImageLength)", extra_tags={257: (4, [(1 << 20) + 1])})
    tag("chunk count", "tag 324: 3 entries, the layout has 4 chunks", extra_tags={324: (4, [400, 400, 400])})
    tag("no byte counts", "tag 325", drop_tags=(325,))
    tag("rows per strip 0", "tag 278 (RowsPerStrip): 0", tile=None, rows_per_strip=5, extra_tags={278: (4, [0])})
    tag("rotated", "tag 34264 (ModelTransformation): rotation",
        extra_tags={34264: (12, [1.0, 0.5, 0, 0, 0.5, -1.0, 0, 0] + [0.0] * 8)})
    tag("south-up", "north-up", gt=(0.0, 1.0, 0.0, 0.0, 0.0, 1.0))
    tag("scale without tiepoint", "tag 33550 (ModelPixelScale) without", gt=GT, drop_tags=(33922,))
    tag("two tiepoints", "tag 33922 (ModelTiepoint)", gt=GT, extra_tags={33922: (12, [0.0] * 12)})
    tag("nodata without a number", "tag 42113 (GDAL_NODATA)", nodata="none")
    tag("floats of 16 bit", "tag 339 (SampleFormat): 3 with 16 bits", raster=words16(20, 20, False),
        extra_tags={339: (3, [3])})
    # chunks
    bad = bytearray(R.write(f, tile=(16, 16), predictor=3, gt=GT))
    p = R.parse(bytes(bad))
    off = p["chunks"][1][0]
    for what, patch, word in (("zlib method", b"\x79\x9c", "chunk 1: zlib header: compression method"),
                              ("zlib window", b"\x88\x1c", "chunk 1: zlib header: CINFO"),
                              ("zlib check", b"\x78\x9d", "chunk 1: zlib header: FCHECK"),
                              ("zlib dictionary", b"\x78\xbb", "chunk 1: zlib header: FDICT")):
        q = bytearray(bad)
        q[off:off + 2] = patch
        out[what] = (bytes(q), word)
    out["chunk past the file"] = (bytes(bad[:-3]), "chunk 3: its bytes")
    tag("short chunk", "chunk 0: 4 bytes are no zlib stream", extra_tags={325: (4, [4, 4, 4, 4])})
    tag("uncompressed length", "chunk 0: 255 bytes uncompressed, its rows take 256", compression=1,
        extra_tags={325: (4, [255, 256, 256, 256])})
    return out
