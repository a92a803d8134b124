"""Writes tests/golden/geotiff/: the inputs of geotiff_inputs.golden_cases() as .npy and, for each,
the file geotiff_reference.encode() builds with the tiles' streams from zlib itself.  Run where
zlib.ZLIB_RUNTIME_VERSION is 1.2.11: these files pin that version's bytes for machines whose zlib
differs.  Usage: python tests/golden/make_geotiff_golden.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import geotiff_inputs as GI   # noqa: E402
import geotiff_reference as GR   # noqa: E402
import png_encode_reference as PR   # noqa: E402


def main():
    assert zlib.ZLIB_RUNTIME_VERSION == "1.2.11", zlib.ZLIB_RUNTIME_VERSION
    out = os.path.join(HERE, "geotiff")
    os.makedirs(out, exist_ok=True)
    total = 0
    for name, (raster, tile) in sorted(GI.golden_cases().items()):
        np.save(os.path.join(out, name + ".npy"), raster)
        data = GR.encode(raster, GI.GT, 32, True, tile, stream=PR.zlib_rle_stream)
        with open(os.path.join(out, name + ".tif"), "wb") as fh:
            fh.write(data)
        total += len(data) + raster.nbytes
        print("%-28s %8d bytes raw, %8d in the file" % (name, raster.nbytes, len(data)))
    print("total", total)


if __name__ == "__main__":
    main()
