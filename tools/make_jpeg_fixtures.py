"""Writes tests/golden/jpeg/: every input of tests/jpeg_inputs.py as .npz and the file Pillow
(libjpeg-turbo) writes for it at every quality, quality=q, subsampling=2, optimize=False.
Needs Pillow; the tests do not.  Usage: python tools/make_jpeg_fixtures.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_inputs as I  # noqa: E402


def pillow_jpeg(image, quality):
    f = io.BytesIO()
    im = Image.fromarray(image if image.ndim == 2 else np.ascontiguousarray(image[..., ::-1]))
    im.save(f, "JPEG", quality=quality, subsampling=2, optimize=False)
    return f.getvalue()


if __name__ == "__main__":
    os.makedirs(I.GOLDEN, exist_ok=True)
    total = 0
    for case in I.cases():
        img = case.image()
        np.savez_compressed(I.golden_npz(case), image=img)
        total += os.path.getsize(I.golden_npz(case))
        for q in I.QUALITIES:
            data = pillow_jpeg(img, q)
            open(I.golden_jpg(case, q), "wb").write(data)
            total += len(data)
    print("%d cases, %d bytes" % (len(I.cases()), total))
