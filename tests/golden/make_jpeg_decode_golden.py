"""Writes tests/golden/jpeg_decode/: files libjpeg-turbo encodes through Pillow, and beside each an
.npz of what it decodes from them (libjpeg's defaults: JDCT_ISLOW, fancy upsampling).

    python tests/golden/make_jpeg_decode_golden.py            the 96 encoder-written fixtures
    python tests/golden/make_jpeg_decode_golden.py streams    tests/golden/jpeg_decode/streams/

streams/ is the second family (tests/jpeg_decode_inputs.py: stream_names()): header and scan
rewrites of the fixtures above, hand-coded scans and flat quantisation tables, whose bytes
jpeg_decode_inputs derives from committed files, and Pillow-written files of further shapes.  Each
gets the pixels libjpeg-turbo decodes from it; a stream the library refuses stops the run.

Needs Pillow; the tests read the committed files and do not.  Content: the seeded noise and the
checker of tests/jpeg_inputs.py.  Sizes and variants: see SIZES and VARIANTS below (dw = chroma
width: 2 is the last that libjpeg upsamples by replication, 3 the first that takes the fancy filter).
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_inputs as I  # noqa: E402

OUT = os.path.join(HERE, "jpeg_decode")

# 1x1; 3x2 and 4x4 (dw = 2); 5x5 (dw = 3, odd height); 7x9; 17x17 and 33x15 (partial MCUs);
# 129x47: more blocks than one IDCT workgroup holds, a partial last group, 26 restart markers
SIZES = [(1, 1), (3, 2), (4, 4), (5, 5), (7, 9), (17, 17), (33, 15), (129, 47)]
CONTENTS = ["noise", "checker"]
# name, channels, Pillow's subsampling, quality, restart_marker_blocks, optimize
VARIANTS = [
    ("444_q95", 3, 0, 95, 0, False),
    ("422_q50", 3, 1, 50, 0, False),
    ("420_q95_rst1", 3, 2, 95, 1, False),
    ("420_q95_rst3", 3, 2, 95, 3, False),
    ("420_q50_opt", 3, 2, 50, 0, True),
    ("gray_q95_rst2", 1, 2, 95, 2, False),
]


def names():
    return ["%s_%dx%d_%s" % (c, w, h, v[0]) for (w, h) in SIZES for c in CONTENTS for v in VARIANTS]


def libjpeg_pixels(data, w=None, h=None):
    """(gray, bgr) as libjpeg-turbo decodes them through Pillow: JCS_GRAYSCALE and JCS_RGB"""
    import warnings
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.draft("L", im.size)
        gray = np.asarray(im.convert("L") if im.mode != "L" else im)
        assert im.mode == "L" and (w is None or gray.shape == (h, w))
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return gray, np.ascontiguousarray(rgb[..., ::-1])


def stream_image(content, w, h, ch, name):
    """random: uniform bytes; saturated: every sample 0 or 255.  Seeded by the name."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    shape = (h, w) if ch == 1 else (h, w, 3)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    return img if content == "random" else np.where(img >= 128, 255, 0).astype(np.uint8)


def main_streams():
    from PIL import Image
    import jpeg_decode_inputs as DI
    out_dir = DI.STREAMS
    os.makedirs(out_dir, exist_ok=True)
    files = dict(DI.stream_rewrites())
    for (name, content, w, h, samp, quality, rst, opt) in DI.pillow_specs():
        ch = 1 if samp == "gray" else 3
        pil = Image.fromarray(stream_image(content, w, h, ch, name))      # (R, G, B as they come)
        kw = dict(quality=quality, optimize=opt)
        if ch == 3:
            kw["subsampling"] = DI.E_SAMPLINGS[samp]
        if rst:
            kw["restart_marker_" + rst[0]] = rst[1]
        buf = io.BytesIO()
        pil.save(buf, "JPEG", **kw)
        files[name] = buf.getvalue()
    assert list(files) and sorted(files) == sorted(DI.stream_names())
    total = 0
    for name in DI.stream_names():
        data = files[name]
        gray, bgr = libjpeg_pixels(data)
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), gray=gray, bgr=bgr)
        total += os.path.getsize(os.path.join(out_dir, name + ".npz"))
        if name in DI.BUILT_NOT_COMMITTED:
            continue
        assert len(data) < 16 * 1024, (name, len(data))
        with open(os.path.join(out_dir, name + ".jpg"), "wb") as f:
            f.write(data)
        total += len(data)
    print("wrote %d streams, %d bytes" % (len(files), total))


def main():
    from PIL import Image
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for (w, h) in SIZES:
        for content in CONTENTS:
            for (vname, ch, sub, quality, rst, opt) in VARIANTS:
                img = I.make_image(content, w, h, ch)
                pil = Image.fromarray(img if ch == 1 else np.ascontiguousarray(img[..., ::-1]))
                buf = io.BytesIO()
                kw = dict(quality=quality, subsampling=sub, optimize=opt)
                if rst:
                    kw["restart_marker_blocks"] = rst
                pil.save(buf, "JPEG", **kw)
                data = buf.getvalue()
                base = os.path.join(OUT, "%s_%dx%d_%s" % (content, w, h, vname))
                with open(base + ".jpg", "wb") as f:
                    f.write(data)
                im = Image.open(io.BytesIO(data))
                im.draft("L", im.size)
                gray = np.asarray(im.convert("L") if im.mode != "L" else im)
                assert gray.shape == (h, w) and (ch == 1 or im.mode == "L")
                rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                np.savez_compressed(base + ".npz", gray=gray, bgr=np.ascontiguousarray(rgb[..., ::-1]))
                total += len(data)
    print("wrote %d files, %d bytes of JPEG" % (len(names()), total))


if __name__ == "__main__":
    if sys.argv[1:] == ["streams"]:
        main_streams()
    else:
        main()
