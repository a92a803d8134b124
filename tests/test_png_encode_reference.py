"""CPU: the restatement of the PNG encoder's file (tests/png_encode_reference.py) against the
committed files whose streams zlib 1.2.11 wrote (tests/golden/png_encode/), those files against three
decoders, larger inputs generated here, and amhip_png_bound.  No GPU."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_decode_reference as D
import png_encode_inputs as I
import png_encode_reference as R

NAMES = I.fixture_names()


def test_the_family_is_there_and_reaches_what_the_generator_asserted():
    assert len(NAMES) == 21
    pixels = [I.fixture_pixels(n) for n in NAMES]
    stats = []
    for px in pixels:
        stats.append(R.Stats())
        R.encode(px, stats[-1])
    I.check_coverage(stats, pixels, [I.fixture_bytes(n) for n in NAMES])


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_equals_the_committed_file(name):
    assert R.encode(I.fixture_pixels(name)) == I.fixture_bytes(name)


def _unfilter(raw, h, w, c):
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * c)
    assert (rows[:, 0] == 1).all()
    px = np.cumsum(rows[:, 1:].reshape(h, w, c).astype(np.uint32), axis=1).astype(np.uint8)
    return px[:, :, 0] if c == 1 else px[:, :, ::-1]


@pytest.mark.parametrize("name", NAMES)
def test_the_committed_file_decodes_to_its_pixels(name):
    from PIL import Image
    data, px = I.fixture_bytes(name), I.fixture_pixels(name)
    h, w = px.shape[:2]
    c = 1 if px.ndim == 2 else 3
    # the container, by hand
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-12:] == R.chunk(b"IEND", b"")
    assert struct.unpack(">IIBBBBB", data[16:29]) == (w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    stream = I.zlib_stream_of(data)
    assert stream[:2] == b"\x78\x01" and len(data) == 33 + len(stream) + 12 * -(-len(stream) // 8192) + 12
    # Pillow
    im = Image.open(io.BytesIO(data))
    assert im.mode == ("L" if c == 1 else "RGB")
    got = np.array(im)
    assert np.array_equal(got if c == 1 else got[:, :, ::-1], px)
    # zlib's inflate and the filter undone
    assert np.array_equal(_unfilter(zlib.decompress(stream), h, w, c), px)
    # the project's restatement of its own decoder
    d = D.decode(data)
    assert np.array_equal(d.gray if c == 1 else d.bgr, px)


def _image_like(rng, h, w):
    """scanline-like content: smooth ramps, flat areas and noise, side by side"""
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    px = ((x // 3 + y // 5) % 256).astype(np.uint8)
    px[h // 4:h // 2] = 90
    px[h // 2:h // 2 + h // 8] = rng.integers(0, 256, (h // 8, w), dtype=np.uint8)
    px[h - h // 8:, :w // 2] = rng.integers(0, 3, (h // 8, w // 2), dtype=np.uint8) * 7
    return px


def test_larger_inputs_generated_here():
    """several slides of the 32 KiB window, hundreds of blocks, blocks of more than 32506 bytes.  Compared
    with the local zlib if that zlib reproduces every committed stream; otherwise only decoded (the test
    then says so in its output)."""
    trust_local = I.local_zlib_reproduces_the_fixtures()
    if not trust_local:
        print("the local zlib (%s) does not reproduce the committed streams: restatement checked by "
              "decoding alone" % zlib.ZLIB_RUNTIME_VERSION)
    rng = np.random.default_rng(4)
    inputs = [rng.integers(0, 256, 200 * 16383, dtype=np.uint8).tobytes(),               # 200 stored blocks
              _image_like(rng, 700, 1500).tobytes(),                                      # 1 MB, image-like
              R.scanlines(_image_like(rng, 400, 601)),
              (rng.integers(0, 256, 3000000, dtype=np.uint8) * (rng.random(3000000) < 0.01)).astype(np.uint8).tobytes(),
              bytes(5000000),                                                             # blocks of 4.2 MB
              np.repeat(rng.integers(0, 256, 200000, dtype=np.uint8), 2).tobytes()]       # 400 000 literals
    blocks = 0
    for raw in inputs:
        s = R.Stats()
        z = R.zlib_stream(raw, s)
        blocks += len(s.block_types)
        assert zlib.decompress(z) == raw
        if trust_local:
            assert z == R.zlib_rle_stream(raw)
    assert blocks > 250


def test_png_bound_holds_and_is_tight_on_noise(hip_built):
    """through the library, no device needed: at least every file's size.  On noise every block is stored
    and starts on a byte, so the zlib stream is raw + 5 per block + 6 bytes, where the bound counts raw + 5
    per possible block + 7: the slack is the one byte kept for a last block's padding, or 4 bytes when the
    symbol count is a multiple of 16383 and the last block is the empty fixed one (2 bytes, not 5)."""
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    for n in NAMES:
        px = I.fixture_pixels(n)
        assert lib.amhip_png_bound(px.shape[1], px.shape[0], 1 if px.ndim == 2 else 3) >= len(I.fixture_bytes(n)), n
    assert lib.amhip_png_bound(0, 5, 1) == 0 and lib.amhip_png_bound(5, 65536, 3) == 0 and lib.amhip_png_bound(5, 5, 2) == 0
    rng = np.random.default_rng(9)
    seen = set()
    for shape in [(61, 83), (200, 333, 3), (129, 126)]:
        c = 3 if len(shape) == 3 else 1
        px = I.pixels_of(I.no_neighbours_equal(shape[0] * shape[1] * c, rng, 0).reshape(shape[0], shape[1] * c), c)
        s = R.Stats()
        data = R.encode(px, s)
        raw = shape[0] * (1 + shape[1] * c)
        assert set(s.block_types[:-1]) <= {"stored"} and s.symbols == raw
        zbound = raw + 5 * (raw // 16383 + 1) + 7
        bound = lib.amhip_png_bound(shape[1], shape[0], c)
        assert bound == 33 + zbound + 12 * -(-zbound // 8192) + 12
        slack = zbound - len(I.zlib_stream_of(data))
        assert slack == (4 if s.block_types[-1] == "fixed" else 1), (shape, slack)
        assert 0 < bound - len(data) <= 4 + 12
        seen.add(s.block_types[-1])
    assert seen == {"stored", "fixed"}
