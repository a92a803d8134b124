"""CPU tests of the PNG decoder's exports of the C ABI: they exist with the stated signatures,
amhip_png_info agrees with the fixtures, and every argument and host error of
amhip_io_decode_png_frames is AMHIP_ERR_ARG with a text, reported before any device is touched."""
import ctypes as C
import os
import re

import pytest

import png_decode_inputs as PI
import png_decode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "amhip_png_info": "int amhip_png_info(const uint8_t* file, size_t len, int* width, int* height, "
                      "int* channels);",
    "amhip_io_decode_png_frames": "int amhip_io_decode_png_frames(int device, const uint8_t* const* files, "
                                  "const size_t* lens, size_t F, int colored, uint8_t** dev_frames, int* width, "
                                  "int* height, size_t* row_step, size_t* frame_stride);",
}


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports_exist_with_the_stated_signatures(L):
    lib = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "aerial_mapper_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name, sig in SIGNATURES.items():
        assert hasattr(lib, name), name        # (on a library without the decoder: fails here)
        assert name in L.EXPORTS
        assert sig in flat, name
    from aerial_mapper_amd import build
    assert "amhip_png_decode.hip" in build.HIP_SOURCES and "amhip_png_decode_host.h" in build.HIP_HEADERS
    # the budget of the raw scanlines is a tuning key, named in the header
    assert "pngd_raw_budget_mb" in hdr
    L.set_tuning("pngd_raw_budget_mb", 1.0)
    assert L.load().amhip_get_tuning(b"pngd_raw_budget_mb", 4096.0) == 1.0
    L.set_tuning("pngd_raw_budget_mb", None)
    assert L.load().amhip_get_tuning(b"pngd_raw_budget_mb", 4096.0) == 4096.0
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`amhip_io_decode_png_frames`" in doc and "`amhip_png_info`" in doc
    from aerial_mapper_amd import io as AIO
    assert callable(AIO.png_info) and callable(AIO.decode_png_frames) and callable(AIO.load_images_named)


def test_png_info_agrees_with_the_fixtures(L):
    from aerial_mapper_amd import io as AIO
    for name in PI.fixture_names():
        data = PI.fixture_bytes(name)
        h = R.parse(data)
        assert AIO.png_info(data) == (h.width, h.height, 1 if h.colour_type in (0, 4) else 3), name
    lib = L.load()
    w, h, ch = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    for what, (data, word) in PI.refusals().items():
        assert lib.amhip_png_info(data, len(data), C.byref(w), C.byref(h), C.byref(ch)) == L.ERR_ARG, what
        assert word.encode() in lib.amhip_last_error(), (what, lib.amhip_last_error())
        with pytest.raises(L.AmhipError):
            AIO.png_info(data)
    good = PI.good_17x17()
    assert lib.amhip_png_info(None, 10, C.byref(w), C.byref(h), C.byref(ch)) == L.ERR_ARG
    assert lib.amhip_png_info(good, len(good), None, C.byref(h), C.byref(ch)) == L.ERR_ARG
    assert lib.amhip_png_info(good, len(good), C.byref(w), None, C.byref(ch)) == L.ERR_ARG
    assert lib.amhip_png_info(good, len(good), C.byref(w), C.byref(h), None) == L.ERR_ARG
    assert lib.amhip_png_info(good, 7, C.byref(w), C.byref(h), C.byref(ch)) == L.ERR_ARG      # len too short


def test_argument_and_host_errors_are_reported_without_a_device(L):
    """A bad device index (1 << 20) rides along: an argument or host error must come first."""
    lib = L.load()
    dec = lib.amhip_io_decode_png_frames
    good = PI.good_17x17()
    other = PI.fixture_bytes("size_64x3_gray")
    no_device = 1 << 20

    def call(files, lens=None, F=None, nulls=(), colored=0):
        n = len(files)
        ptrs = (C.c_char_p * max(n, 1))(*files)
        ln = (C.c_size_t * max(n, 1))(*(lens if lens is not None else [len(f) for f in files]))
        out = C.c_void_p(0xDEAD)
        w, h = C.c_int(-1), C.c_int(-1)
        row, stride = C.c_size_t(), C.c_size_t()
        args = [no_device, ptrs, ln, n if F is None else F, colored, C.byref(out), C.byref(w), C.byref(h),
                C.byref(row), C.byref(stride)]
        for k in nulls:
            args[k] = None
        rc = dec(*args)
        assert rc == L.ERR_ARG, (rc, lib.amhip_last_error())
        text = lib.amhip_last_error().decode()
        assert len(text) > 10 and "amhip_io_decode_png_frames" in text
        if 5 not in nulls:
            assert out.value is None          # *dev_frames = NULL
        return text

    for k in (1, 2, 5, 6, 7, 8, 9):
        assert "null" in call([good], nulls=(k,))
    assert "F = 0" in call([good], F=0)
    assert "frame 1: null file" in call([good, None], lens=[len(good), 10])
    assert "frame 0: no PNG signature" in call([good], lens=[7])                # len too short
    assert "frame 0: chunk IEND: truncated" in call([good], lens=[len(good) - 1])
    for what, (data, word) in PI.refusals().items():
        text = call([good, good, data, good], colored=1)
        assert "frame 2: " in text and word in text, (what, text)
    text = call([good, good, good, other, good])
    assert "frame 3 is 64 x 3, frame 0 is 17 x 17" in text
