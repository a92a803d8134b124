"""Rasters for the GeoTIFF encoder's tests (geotiff_reference.py, test_gpu_geotiff.py) and for
tests/golden/make_geotiff_golden.py.  Everything is a function of its arguments and a fixed seed."""
import numpy as np

GT = (464499.25, 0.5, 0.0, 5272700.75, 0.0, -0.5)   # a north-up geotransform in UTM 32N
EDGE_SIZES = [(1, 1), (16, 16), (17, 16), (16, 17), (33, 47), (50, 70)]   # (height, width) at tile 16


def terrain(h, w, res=0.5):
    """SURVEY's 400 + 10 sin cos surface"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64) * res
    return (400.0 + 10.0 * np.sin(x / 7.0) * np.cos(y / 5.0)).astype(np.float32)


def edge_raster(kind, h, w, seed=0):
    """a small raster with structure and noise: runs, holes, negative values"""
    rng = np.random.default_rng(1000 * h + w + seed)
    if kind == "f32":
        a = terrain(h, w) - np.float32(405.0)          # both signs
        a[rng.random((h, w)) < 0.2] = np.nan            # holes
        if h * w > 4:
            a.reshape(-1)[1] = np.float32(np.uint32(0x7FC12345).view(np.float32))   # a NaN with a payload
        return a
    if kind == "u8":
        a = (np.arange(w)[None, :] // 5 * 9 + np.arange(h)[:, None] // 3 * 17).astype(np.uint8)
        noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
        return np.where(rng.random((h, w)) < 0.3, noise, a).astype(np.uint8)
    a = np.stack([edge_raster("u8", h, w, seed + k) for k in (1, 2, 3)], axis=-1)
    return np.ascontiguousarray(a)


def noise(kind, n=128, seed=7):
    rng = np.random.default_rng(seed)
    if kind == "f32":
        return rng.integers(0, 1 << 32, (n, n), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rng.integers(0, 256, (n, n, 3) if kind == "rgb8" else (n, n), dtype=np.uint8)


def golden_cases():
    """name -> (raster, tile): what tests/golden/geotiff/ pins with zlib 1.2.11's own bytes"""
    nan = np.full((33, 47), np.nan, np.float32)
    one = np.full((64, 64), np.float32(412.5))
    one[37, 21] = np.float32(-3.25)
    return {
        "f32_1x1_t16": (np.array([[np.float32(-7.5)]], np.float32), 16),
        "u8_16x16_t16": (edge_raster("u8", 16, 16), 16),
        "rgb8_17x16_t16": (edge_raster("rgb8", 17, 16), 16),
        "f32_16x17_t16": (edge_raster("f32", 16, 17), 16),
        "f32_33x47_t16": (edge_raster("f32", 33, 47), 16),
        "u8_33x47_t16": (edge_raster("u8", 33, 47), 16),
        "rgb8_50x70_t16": (edge_raster("rgb8", 50, 70), 16),
        "f32_allnan_33x47_t16": (nan, 16),
        "u8_all255_40x40_t32": (np.full((40, 40), 255, np.uint8), 32),
        "f32_one_sample_64x64_t64": (one, 64),
        "f32_terrain_100x90_t64": (terrain(100, 90), 64),
        "f32_noise_128_t128": (noise("f32"), 128),
        "rgb8_noise_128_t128": (noise("rgb8"), 128),
    }
