"""CPU tests of the batched JPEG encoder's exports of the C ABI (amhip_io_encode_jpeg_frames,
amhip_io_write_jpeg_frames): they exist with the stated signatures, hip_lib binds them, the tuning key
of their scratch round-trips, and every argument error is AMHIP_ERR_ARG with a text that names the
export and the field, reported before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "amhip_io_encode_jpeg_frames": "int amhip_io_encode_jpeg_frames(int device, const uint8_t* dev_frames, size_t F, "
                                   "int width, int height, int channels, size_t row_step, size_t frame_stride, "
                                   "int quality, uint8_t** dev_files, size_t* offsets);",
    "amhip_io_write_jpeg_frames": "int amhip_io_write_jpeg_frames(int device, const uint8_t* frames, int on_device, "
                                  "size_t F, int width, int height, int channels, size_t row_step, "
                                  "size_t frame_stride, int quality, const char* const* filenames);",
}

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
    ("quality -1", dict(quality=-1), "quality"),
    ("quality 101", dict(quality=101), "quality"),
]
GOOD = dict(F=3, width=17, height=17, channels=3, row_step=51, frame_stride=17 * 51, quality=95)
NO_DEVICE = 1 << 20     # a bad device index rides along: an argument error must come first


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
        assert hasattr(lib, name), name
        assert name in L.EXPORTS
        assert getattr(L.load(), name).argtypes is not None, name
        assert sig in flat, name
    assert len(L.load().amhip_io_encode_jpeg_frames.argtypes) == 11
    assert len(L.load().amhip_io_write_jpeg_frames.argtypes) == 11
    # additive only
    assert L.ABI_VERSION == 2 and L.load().amhip_abi_version() == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`amhip_io_encode_jpeg_frames`" in doc and "`amhip_io_write_jpeg_frames`" in doc


def test_the_scratch_budget_is_a_tuning_key_named_in_the_header(L):
    hdr = open(os.path.join(ROOT, "include", "aerial_mapper_hip.h")).read()
    assert "jpege_scratch_budget_mb (4096)" in hdr
    assert hdr.index("jpegd_coef_budget_mb (4096)") < hdr.index("jpege_scratch_budget_mb (4096)")
    L.set_tuning("jpege_scratch_budget_mb", 1.0)
    assert L.load().amhip_get_tuning(b"jpege_scratch_budget_mb", 4096.0) == 1.0
    L.set_tuning("jpege_scratch_budget_mb", None)
    assert L.load().amhip_get_tuning(b"jpege_scratch_budget_mb", 4096.0) == 4096.0


def _encode(lib, L, nulls=(), **changed):
    a = dict(GOOD, **changed)
    frames = (C.c_uint8 * 16)()        # never read: the refusal comes first
    out = C.c_void_p(0xDEAD)
    offsets = (C.c_size_t * 8)()
    args = [NO_DEVICE, C.cast(frames, C.c_void_p), a["F"], a["width"], a["height"], a["channels"], a["row_step"],
            a["frame_stride"], a["quality"], C.byref(out), offsets]
    for k in nulls:
        args[k] = None
    rc = lib.amhip_io_encode_jpeg_frames(*args)
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG, (rc, text)
    assert len(text) > 10 and text.startswith("amhip_io_encode_jpeg_frames: "), text
    if 9 not in nulls:
        assert out.value is None           # *dev_files = NULL
    return text


def _write(lib, L, nulls=(), names=None, **changed):
    a = dict(GOOD, **changed)
    frames = (C.c_uint8 * 16)()
    files = [b"/nonexistent-directory/a.jpg", b"/nonexistent-directory/b.jpg", b"/nonexistent-directory/c.jpg"]
    arr = (C.c_char_p * 3)(*(files if names is None else names))
    args = [NO_DEVICE, C.cast(frames, C.c_void_p), 0, a["F"], a["width"], a["height"], a["channels"], a["row_step"],
            a["frame_stride"], a["quality"], arr]
    for k in nulls:
        args[k] = None
    rc = lib.amhip_io_write_jpeg_frames(*args)
    text = lib.amhip_last_error().decode()
    assert rc == L.ERR_ARG, (rc, text)
    assert len(text) > 10 and text.startswith("amhip_io_write_jpeg_frames: "), text
    return text


@pytest.mark.parametrize("what,changed,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_argument_errors_name_the_export_and_the_field_without_a_device(L, what, changed, word):
    lib = L.load()
    assert word in _encode(lib, L, **changed)
    assert word in _write(lib, L, **changed)


def test_null_pointers_are_refused_without_a_device(L):
    lib = L.load()
    for k in (1, 9, 10):
        assert "null" in _encode(lib, L, nulls=(k,))
    for k in (1, 10):
        assert "null" in _write(lib, L, nulls=(k,))
    text = _write(lib, L, names=[b"/tmp/a.jpg", None, b"/tmp/c.jpg"])
    assert "filenames[1]" in text and "null" in text


def test_a_single_frame_needs_no_frame_stride(L):
    """F = 1: frame_stride is not looked at, so the call gets as far as the device index"""
    lib = L.load()
    out = C.c_void_p(0xDEAD)
    offsets = (C.c_size_t * 2)()
    frames = (C.c_uint8 * 16)()
    rc = lib.amhip_io_encode_jpeg_frames(NO_DEVICE, C.cast(frames, C.c_void_p), 1, 17, 17, 3, 51, 0, 95,
                                         C.byref(out), offsets)
    text = lib.amhip_last_error().decode()
    assert rc in (L.ERR_ARG, L.ERR_NO_DEVICE) and "frame_stride" not in text, (rc, text)
    assert ("device" in text) and out.value is None
