"""Writes tests/golden/geotiff_read/: files libtiff wrote (through Pillow) with the rasters they hold,
for the GeoTIFF reader's tests.  Needs Pillow; the tests that use the files do not.

    python tests/golden/make_geotiff_read_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import geotiff_inputs as GI  # noqa: E402

OUT = os.path.join(HERE, "geotiff_read")


def cases():
    rng = np.random.default_rng(11)
    u16 = (np.arange(70, dtype=np.uint32)[None, :] * 251 + np.arange(33, dtype=np.uint32)[:, None] * 4099) % 65536
    return {
        # name: (raster, Pillow mode, predictor, rows per strip or None)
        "pil_f32_p3_33x47": (GI.edge_raster("f32", 33, 47), "F", 3, None),
        "pil_f32_p2_50x70_rps7": (GI.edge_raster("f32", 50, 70), "F", 2, 7),
        "pil_f32_p3_terrain_200x300": (GI.terrain(200, 300), "F", 3, None),     # strips of about 64 KB
        "pil_u8_p2_33x47": (GI.edge_raster("u8", 33, 47), "L", 2, None),
        "pil_u16_p2_33x70_rps5": (u16.astype(np.uint16), "I;16", 2, 5),
        "pil_rgb8_p2_50x70": (GI.edge_raster("rgb8", 50, 70), "RGB", 2, None),
        "pil_u8_p1_noise_64x64": (rng.integers(0, 256, (64, 64), dtype=np.uint8), "L", 1, None),
    }


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (raster, mode, predictor, rps) in cases().items():
        im = Image.fromarray(raster)
        assert im.mode == mode, (name, im.mode)
        info = {317: predictor}
        if rps:
            info[278] = rps
        path = os.path.join(OUT, name + ".tif")
        im.save(path, format="TIFF", compression="tiff_adobe_deflate", tiffinfo=info)
        back = np.asarray(Image.open(path))
        assert back.tobytes() == raster.tobytes(), name
        np.save(os.path.join(OUT, name + ".npy"), raster)
        print(name, os.path.getsize(path))


if __name__ == "__main__":
    main()
