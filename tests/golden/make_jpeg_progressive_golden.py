"""Writes tests/golden/jpeg_progressive/: progressive JPEG files and beside each an .npz of what
libjpeg-turbo decodes from it through Pillow (libjpeg's defaults: JDCT_ISLOW, fancy upsampling).

    python tests/golden/make_jpeg_progressive_golden.py

  A  Pillow-written (progressive=True: libjpeg-turbo's default script), tests/jpeg_progressive_inputs.py:
     A_CONTENTS x A_SIZES x A_VARIANTS
  B  tests/jpeg_progressive_inputs.py's ProgressiveWriter over the coefficients of baseline fixtures,
     under scripts no encoder picks.  Asserted here: libjpeg-turbo decodes each to the very pixels of
     the baseline fixture's committed .npz
  C  the two large gray files

Needs Pillow; the tests read the committed files and do not.  A stream the library refuses, or
warns about, stops the run."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_inputs as DI  # noqa: E402
import jpeg_inputs as I  # noqa: E402
import jpeg_progressive_inputs as PI  # noqa: E402
from make_jpeg_decode_golden import libjpeg_pixels  # noqa: E402

MAX_FILE = 16 * 1024     # (the size the fixtures of tests/golden/jpeg_decode/ keep)


def pillow_files():
    from PIL import Image
    out = {}
    for (w, h) in PI.A_SIZES:
        for cname, content in PI.A_CONTENTS.items():
            for vname, (ch, sub, quality, rst) in PI.A_VARIANTS.items():
                img = I.make_image(content, w, h, ch)
                pil = Image.fromarray(img if ch == 1 else np.ascontiguousarray(img[..., ::-1]))
                kw = dict(quality=quality, progressive=True)
                if ch == 3:
                    kw["subsampling"] = sub
                if rst:
                    kw[rst[0]] = rst[1]
                buf = io.BytesIO()
                pil.save(buf, "JPEG", **kw)
                out["a_%s_%dx%d_%s" % (cname, w, h, vname)] = buf.getvalue()
    return out


def main():
    os.makedirs(PI.GOLDEN, exist_ok=True)
    files = pillow_files()
    assert list(files) == PI.a_names()
    derived = PI.derived_files()
    files.update(derived)
    assert sorted(files) == sorted(PI.names())
    total = 0
    for name in PI.names():
        data = files[name]
        w, h = PI.size_of(name)
        gray, bgr = libjpeg_pixels(data, w, h)
        if name.startswith("b_"):
            # same coefficients, same pixels: the baseline fixture's
            g0, b0 = DI.fixture_pixels(PI.b_base(name))
            assert np.array_equal(gray, g0) and np.array_equal(bgr, b0), name
        if name == "c_eobrun_32767_gray_2048x1024":
            assert (gray == 138).all() and (bgr == 138).all()
        assert len(data) < MAX_FILE, (name, len(data))
        with open(PI.path(name), "wb") as f:
            f.write(data)
        np.savez_compressed(os.path.join(PI.GOLDEN, name + ".npz"), gray=gray, bgr=bgr)
        total += len(data) + os.path.getsize(os.path.join(PI.GOLDEN, name + ".npz"))
    print("wrote %d files, %d bytes with their pixels" % (len(files), total))


if __name__ == "__main__":
    main()
