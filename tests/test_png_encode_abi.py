"""CPU tests of the PNG encoder's nine exports of the C ABI: they exist with the stated signatures,
hip_lib binds them, INTEGRATION.md carries their rows, the tuning key of the scratch round-trips, and
every argument error is AMHIP_ERR_ARG with a text that names the export and the field, reported before
any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "amhip_png_bound": "size_t amhip_png_bound(int width, int height, int channels);",
    "amhip_png_encode_dev": "int amhip_png_encode_dev(amhip_ctx* ctx, const uint8_t* dev_pixels, size_t step, int width, "
                            "int height, int channels, uint8_t* dev_out, size_t cap, size_t* bytes);",
    "amhip_png_write": "int amhip_png_write(amhip_ctx* ctx, const char* filename, const uint8_t* pixels, int on_device, "
                       "size_t step, int width, int height, int channels);",
    "amhip_layer_write_png": "int amhip_layer_write_png(amhip_ctx* ctx, int layer, int bgr, float lower, float upper, "
                             "const char* filename);",
    "amhip_session_layer_write_png": "int amhip_session_layer_write_png(amhip_session* s, int layer, int bgr, float lower, "
                                     "float upper, const char* filename);",
    "amhip_mosaic_encode_png_dev": "int amhip_mosaic_encode_png_dev(amhip_mosaic* mosaic, uint8_t* dev_out, size_t cap, "
                                   "size_t* bytes);",
    "amhip_mosaic_write_png": "int amhip_mosaic_write_png(amhip_mosaic* mosaic, const char* filename);",
    "amhip_io_encode_png_frames": "int amhip_io_encode_png_frames(int device, const uint8_t* dev_frames, size_t F, "
                                  "int width, int height, int channels, size_t row_step, size_t frame_stride, "
                                  "uint8_t** dev_files, size_t* offsets);",
    "amhip_io_write_png_frames": "int amhip_io_write_png_frames(int device, const uint8_t* frames, int on_device, "
                                 "size_t F, int width, int height, int channels, size_t row_step, "
                                 "size_t frame_stride, const char* const* filenames);",
}
ARGC = {"amhip_png_bound": 3, "amhip_png_encode_dev": 9, "amhip_png_write": 8, "amhip_layer_write_png": 6,
        "amhip_session_layer_write_png": 6, "amhip_mosaic_encode_png_dev": 4, "amhip_mosaic_write_png": 2,
        "amhip_io_encode_png_frames": 10, "amhip_io_write_png_frames": 10}

# (what is wrong, the arguments that differ from a good call, a word of the text)
REFUSALS = [
    ("F = 0", dict(F=0), "F = 0"),
    ("width 0", dict(width=0), "width"),
    ("width 65536", dict(width=65536), "width"),
    ("height 0", dict(height=0), "height"),
    ("height 65536", dict(height=65536), "height"),
    ("channels 2", dict(channels=2), "channels"),
    ("channels 4", dict(channels=4), "channels"),
    ("row_step short", dict(row_step=50), "row_step"),
    ("frame_stride short", dict(frame_stride=17 * 51 - 1), "frame_stride"),
]
GOOD = dict(F=3, width=17, height=17, channels=3, row_step=51, frame_stride=17 * 51)
NO_DEVICE = 1 << 20     # a bad device index rides along: an argument error must come first
FAKE = 0x1000           # a handle that is never looked into: the refusal comes first


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports_exist_with_the_stated_signatures(L):
    lib = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "aerial_mapper_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(SIGNATURES) == 9
    for name, sig in SIGNATURES.items():
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
        assert len(getattr(L.load(), name).argtypes) == ARGC[name], name
        assert sig in flat, name
        assert "`%s`" % name in doc, name
    assert L.load().amhip_png_bound.restype is C.c_size_t
    # additive only
    assert L.ABI_VERSION == 2 and L.load().amhip_abi_version() == 2


def test_python_mirrors_exist():
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E, io as AIO
    for name in ("encode_png", "write_png", "layer_to_png", "session_layer_to_png"):
        assert callable(getattr(E, name)) and getattr(A, name) is getattr(E, name)
    assert callable(AIO.encode_png_frames) and callable(AIO.write_png_frames)
    assert callable(A.OrthoForwardHomography.encode_png) and callable(A.OrthoForwardHomography.write_png)


def test_the_scratch_budget_is_a_tuning_key_named_in_the_header(L):
    hdr = open(os.path.join(ROOT, "include", "aerial_mapper_hip.h")).read()
    assert "pnge_scratch_budget_mb (4096)" in hdr
    L.set_tuning("pnge_scratch_budget_mb", 1.0)
    assert L.load().amhip_get_tuning(b"pnge_scratch_budget_mb", 4096.0) == 1.0
    L.set_tuning("pnge_scratch_budget_mb", None)
    assert L.load().amhip_get_tuning(b"pnge_scratch_budget_mb", 4096.0) == 4096.0


def _encode(lib, L, nulls=(), **changed):
    a = dict(GOOD, **changed)
    frames = (C.c_uint8 * 16)()        # never read: the refusal comes first
    out = C.c_void_p(0xDEAD)
    offsets = (C.c_size_t * 8)()
    args = [NO_DEVICE, C.cast(frames, C.c_void_p), a["F"], a["width"], a["height"], a["channels"], a["row_step"],
            a["frame_stride"], C.byref(out), offsets]
    for k in nulls:
        args[k] = None
    rc = lib.amhip_io_encode_png_frames(*args)
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG, (rc, text)
    assert len(text) > 10 and text.startswith("amhip_io_encode_png_frames: "), text
    if 8 not in nulls:
        assert out.value is None           # *dev_files = NULL
    return text


def _write(lib, L, nulls=(), names=None, **changed):
    a = dict(GOOD, **changed)
    frames = (C.c_uint8 * 16)()
    files = [b"/nonexistent-directory/a.png", b"/nonexistent-directory/b.png", b"/nonexistent-directory/c.png"]
    arr = (C.c_char_p * 3)(*(files if names is None else names))
    args = [NO_DEVICE, C.cast(frames, C.c_void_p), 0, a["F"], a["width"], a["height"], a["channels"], a["row_step"],
            a["frame_stride"], arr]
    for k in nulls:
        args[k] = None
    rc = lib.amhip_io_write_png_frames(*args)
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG, (rc, text)
    assert len(text) > 10 and text.startswith("amhip_io_write_png_frames: "), text
    return text


@pytest.mark.parametrize("what,changed,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_stack_argument_errors_name_the_export_and_the_field_without_a_device(L, what, changed, word):
    lib = L.load()
    assert word in _encode(lib, L, **changed)
    assert word in _write(lib, L, **changed)


def test_stack_null_pointers_are_refused_without_a_device(L):
    lib = L.load()
    for k in (1, 8, 9):
        assert "null" in _encode(lib, L, nulls=(k,))
    for k in (1, 9):
        assert "null" in _write(lib, L, nulls=(k,))
    text = _write(lib, L, names=[b"/tmp/a.png", None, b"/tmp/c.png"])
    assert "filenames[1]" in text and "null" in text


def test_a_single_frame_needs_no_frame_stride(L):
    """F = 1: frame_stride is not looked at, so the call gets as far as the device index"""
    lib = L.load()
    out = C.c_void_p(0xDEAD)
    offsets = (C.c_size_t * 2)()
    frames = (C.c_uint8 * 16)()
    rc = lib.amhip_io_encode_png_frames(NO_DEVICE, C.cast(frames, C.c_void_p), 1, 17, 17, 3, 51, 0, C.byref(out), offsets)
    text = lib.amhip_last_error().decode()
    assert rc in (L.ERR_ARG, L.ERR_NO_DEVICE) and "frame_stride" not in text, (rc, text)
    assert ("device" in text) and out.value is None


IMAGE_REFUSALS = [(dict(channels=2), "channels"), (dict(width=0), "width and height"),
                  (dict(width=65536), "width and height"), (dict(height=0), "width and height"),
                  (dict(height=65536), "width and height"), (dict(step=50), "step")]


@pytest.mark.parametrize("changed,word", IMAGE_REFUSALS, ids=[str(r[0]) for r in IMAGE_REFUSALS])
def test_single_image_argument_errors_come_before_the_context_is_looked_at(L, changed, word):
    lib = L.load()
    a = dict(dict(step=51, width=17, height=17, channels=3), **changed)
    px = (C.c_uint8 * 16)()
    n = C.c_size_t(77)
    rc = lib.amhip_png_encode_dev(C.c_void_p(FAKE), C.cast(px, C.c_void_p), a["step"], a["width"], a["height"],
                                  a["channels"], C.cast(px, C.c_void_p), 16, C.byref(n))
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG and text.startswith("amhip_png_encode_dev: ") and word in text, text
    assert n.value == 77
    rc = lib.amhip_png_write(C.c_void_p(FAKE), b"/nonexistent-directory/a.png", C.cast(px, C.c_void_p), 0, a["step"],
                             a["width"], a["height"], a["channels"])
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG and text.startswith("amhip_png_write: ") and word in text, text


def test_single_image_null_and_range_errors(L):
    lib = L.load()
    px = (C.c_uint8 * 16)()
    p = C.cast(px, C.c_void_p)
    n = C.c_size_t()
    calls = [("amhip_png_encode_dev", lambda: lib.amhip_png_encode_dev(None, p, 51, 17, 17, 3, p, 16, C.byref(n))),
             ("amhip_png_encode_dev", lambda: lib.amhip_png_encode_dev(C.c_void_p(FAKE), None, 51, 17, 17, 3, p, 16, C.byref(n))),
             ("amhip_png_encode_dev", lambda: lib.amhip_png_encode_dev(C.c_void_p(FAKE), p, 51, 17, 17, 3, None, 16, C.byref(n))),
             ("amhip_png_encode_dev", lambda: lib.amhip_png_encode_dev(C.c_void_p(FAKE), p, 51, 17, 17, 3, p, 16, None)),
             ("amhip_png_write", lambda: lib.amhip_png_write(None, b"/tmp/a.png", p, 0, 51, 17, 17, 3)),
             ("amhip_png_write", lambda: lib.amhip_png_write(C.c_void_p(FAKE), None, p, 0, 51, 17, 17, 3)),
             ("amhip_png_write", lambda: lib.amhip_png_write(C.c_void_p(FAKE), b"/tmp/a.png", None, 0, 51, 17, 17, 3)),
             ("amhip_layer_write_png", lambda: lib.amhip_layer_write_png(None, 0, 0, 0.0, 255.0, b"/tmp/a.png")),
             ("amhip_layer_write_png", lambda: lib.amhip_layer_write_png(C.c_void_p(FAKE), 0, 0, 0.0, 255.0, None)),
             ("amhip_layer_write_png", lambda: lib.amhip_layer_write_png(C.c_void_p(FAKE), -1, 0, 0.0, 255.0, b"/tmp/a.png")),
             ("amhip_layer_write_png", lambda: lib.amhip_layer_write_png(C.c_void_p(FAKE), 99, 0, 0.0, 255.0, b"/tmp/a.png")),
             ("amhip_layer_write_png", lambda: lib.amhip_layer_write_png(C.c_void_p(FAKE), 0, 0, 5.0, 5.0, b"/tmp/a.png")),
             ("amhip_session_layer_write_png", lambda: lib.amhip_session_layer_write_png(None, 0, 0, 0.0, 255.0, b"/tmp/a.png")),
             ("amhip_session_layer_write_png", lambda: lib.amhip_session_layer_write_png(C.c_void_p(FAKE), 0, 0, 0.0, 255.0, None)),
             ("amhip_session_layer_write_png", lambda: lib.amhip_session_layer_write_png(C.c_void_p(FAKE), 99, 0, 0.0, 255.0, b"/tmp/a.png")),
             ("amhip_session_layer_write_png", lambda: lib.amhip_session_layer_write_png(C.c_void_p(FAKE), 0, 0, 5.0, 1.0, b"/tmp/a.png")),
             ("amhip_mosaic_encode_png_dev", lambda: lib.amhip_mosaic_encode_png_dev(None, p, 16, C.byref(n))),
             ("amhip_mosaic_encode_png_dev", lambda: lib.amhip_mosaic_encode_png_dev(C.c_void_p(FAKE), None, 16, C.byref(n))),
             ("amhip_mosaic_encode_png_dev", lambda: lib.amhip_mosaic_encode_png_dev(C.c_void_p(FAKE), p, 16, None)),
             ("amhip_mosaic_write_png", lambda: lib.amhip_mosaic_write_png(None, b"/tmp/a.png")),
             ("amhip_mosaic_write_png", lambda: lib.amhip_mosaic_write_png(C.c_void_p(FAKE), None))]
    for who, call in calls:
        rc = call()
        text = lib.amhip_last_error().decode()
        assert rc == L.ERR_ARG and text.startswith(who + ": "), (who, rc, text)
