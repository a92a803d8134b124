"""CPU tests of the JPEG exports of the C ABI: they exist with the stated signatures, the size bound
holds on the whole input list, and every argument error is AMHIP_ERR_ARG with a text, reported
before the context is looked at (no device needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_inputs as I
import jpeg_reference as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "amhip_jpeg_bound": "size_t amhip_jpeg_bound(int width, int height, int channels);",
    "amhip_jpeg_encode_dev": "int amhip_jpeg_encode_dev(amhip_ctx* ctx, const uint8_t* dev_pixels, size_t step, "
                             "int width, int height, int channels, int quality, uint8_t* dev_out, size_t cap, "
                             "size_t* bytes);",
    "amhip_jpeg_write": "int amhip_jpeg_write(amhip_ctx* ctx, const char* filename, const uint8_t* pixels, "
                        "int on_device, size_t step, int width, int height, int channels, int quality);",
    "amhip_layer_write_jpeg": "int amhip_layer_write_jpeg(amhip_ctx* ctx, int layer, int bgr, float lower, "
                              "float upper, int quality, const char* filename);",
    "amhip_session_layer_write_jpeg": "int amhip_session_layer_write_jpeg(amhip_session* s, int layer, int bgr, "
                                      "float lower, float upper, int quality, const char* filename);",
    "amhip_mosaic_encode_jpeg_dev": "int amhip_mosaic_encode_jpeg_dev(amhip_mosaic* mosaic, int quality, "
                                    "uint8_t* dev_out, size_t cap, size_t* bytes);",
    "amhip_mosaic_write_jpeg": "int amhip_mosaic_write_jpeg(amhip_mosaic* mosaic, int quality, "
                               "const char* filename);",
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
        assert hasattr(lib, name), name        # (on a library without the encoder: fails here)
        assert name in L.EXPORTS
        assert sig in flat, name
    assert L.ABI_VERSION == 2 and L.load().amhip_abi_version() == 2
    assert "#define AMHIP_ABI_VERSION 2" in hdr
    # timed into AMHIP_K_MISC: no new kernel slot
    assert L.NUM_KERNELS == 8 and "AMHIP_NUM_KERNELS = 8" in hdr


def test_bound_is_monotone_and_covers_the_whole_input_list(L):
    lib = L.load()
    for ch in (1, 3):
        last = 0
        for n in (1, 7, 8, 9, 16, 17, 33, 129, 1000, 4097, 65535):
            b = lib.amhip_jpeg_bound(n, n, ch)
            assert b >= last      # (sizes inside one block / MCU share a bound)
            last = b
            assert lib.amhip_jpeg_bound(n + 1 if n < 65535 else n, n, ch) >= b
            assert lib.amhip_jpeg_bound(n, n + 1 if n < 65535 else n, ch) >= b
        assert lib.amhip_jpeg_bound(17, 16, ch) > lib.amhip_jpeg_bound(16, 16, ch)
        assert lib.amhip_jpeg_bound(16, 17, ch) > lib.amhip_jpeg_bound(16, 16, ch)
        assert lib.amhip_jpeg_bound(64, 64, 3) >= lib.amhip_jpeg_bound(64, 64, 1)
    for bad in ((0, 8, 1), (8, 0, 1), (65536, 8, 1), (8, 65536, 3), (8, 8, 2), (-1, 8, 1)):
        assert lib.amhip_jpeg_bound(*bad) == 0
    for case in I.cases():
        img = case.image()
        b = lib.amhip_jpeg_bound(case.width, case.height, case.channels)
        for q in I.QUALITIES:
            assert b >= len(J.encode(img, q)), (case, q)
    big = I.large_case()
    assert lib.amhip_jpeg_bound(big.width, big.height, 1) >= len(J.encode(big.image(), 95))


def test_argument_errors_are_reported_without_a_device(L, tmp_path):
    lib = L.load()
    n = C.c_size_t()
    px = np.zeros((8, 24), np.uint8)
    out = np.zeros(4096, np.uint8)
    p, o = C.c_void_p(px.ctypes.data), C.c_void_p(out.ctypes.data)
    # (a context that is never looked at: the argument checks come first)
    fake = C.c_void_p(px.ctypes.data)
    name = str(tmp_path / "never.jpg").encode()

    def refused(rc):
        assert rc == L.ERR_ARG
        assert len(lib.amhip_last_error()) > 10
        assert not out.any() and not os.path.exists(name.decode())

    enc = lib.amhip_jpeg_encode_dev
    refused(enc(None, p, 24, 8, 8, 3, 95, o, 4096, C.byref(n)))
    refused(enc(fake, None, 24, 8, 8, 3, 95, o, 4096, C.byref(n)))
    refused(enc(fake, p, 24, 8, 8, 3, 95, None, 4096, C.byref(n)))
    refused(enc(fake, p, 24, 8, 8, 3, 95, o, 4096, None))
    refused(enc(fake, p, 24, 8, 8, 2, 95, o, 4096, C.byref(n)))          # channels = 2
    refused(enc(fake, p, 24, 8, 8, 3, 101, o, 4096, C.byref(n)))         # quality
    refused(enc(fake, p, 24, 8, 8, 3, -1, o, 4096, C.byref(n)))
    refused(enc(fake, p, 24, 0, 8, 3, 95, o, 4096, C.byref(n)))          # width
    refused(enc(fake, p, 1 << 20, 65536, 8, 3, 95, o, 4096, C.byref(n)))
    refused(enc(fake, p, 24, 8, 0, 3, 95, o, 4096, C.byref(n)))          # height
    refused(enc(fake, p, 24, 8, 65536, 3, 95, o, 4096, C.byref(n)))
    refused(enc(fake, p, 23, 8, 8, 3, 95, o, 4096, C.byref(n)))          # step < width * channels
    refused(enc(fake, p, 7, 8, 8, 1, 95, o, 4096, C.byref(n)))
    wr = lib.amhip_jpeg_write
    refused(wr(None, name, p, 0, 24, 8, 8, 3, 95))
    refused(wr(fake, None, p, 0, 24, 8, 8, 3, 95))
    refused(wr(fake, name, None, 0, 24, 8, 8, 3, 95))
    refused(wr(fake, name, p, 0, 24, 8, 8, 2, 95))
    refused(wr(fake, name, p, 0, 24, 8, 8, 3, 101))
    refused(wr(fake, name, p, 0, 24, 8, 8, 3, -1))
    refused(wr(fake, name, p, 0, 24, 0, 8, 3, 95))
    refused(wr(fake, name, p, 0, 1 << 20, 65536, 8, 3, 95))
    refused(wr(fake, name, p, 0, 23, 8, 8, 3, 95))
    lw = lib.amhip_layer_write_jpeg
    refused(lw(None, 0, 0, 0.0, 255.0, 95, name))
    refused(lw(fake, 0, 0, 0.0, 255.0, 95, None))
    refused(lw(fake, -1, 0, 0.0, 255.0, 95, name))
    refused(lw(fake, L.NUM_LAYERS, 0, 0.0, 255.0, 95, name))
    refused(lw(fake, 0, 0, 0.0, 255.0, 101, name))
    refused(lw(fake, 0, 0, 0.0, 255.0, -1, name))
    refused(lw(fake, 0, 0, 5.0, 5.0, 95, name))                          # upper <= lower
    sw = lib.amhip_session_layer_write_jpeg
    refused(sw(None, 0, 0, 0.0, 255.0, 95, name))
    refused(sw(fake, 0, 0, 0.0, 255.0, 95, None))
    refused(sw(fake, 6, 0, 0.0, 255.0, 95, name))
    refused(sw(fake, 0, 0, 0.0, 255.0, 101, name))
    refused(sw(fake, 0, 0, 255.0, 0.0, 95, name))
    me = lib.amhip_mosaic_encode_jpeg_dev
    refused(me(None, 95, o, 4096, C.byref(n)))
    refused(me(fake, 95, None, 4096, C.byref(n)))
    refused(me(fake, 95, o, 4096, None))
    refused(me(fake, 101, o, 4096, C.byref(n)))
    refused(me(fake, -1, o, 4096, C.byref(n)))
    mw = lib.amhip_mosaic_write_jpeg
    refused(mw(None, 95, name))
    refused(mw(fake, 95, None))
    refused(mw(fake, 101, name))
    refused(mw(fake, -1, name))
