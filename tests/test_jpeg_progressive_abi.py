"""CPU tests of the JPEG decoder's exports of the C ABI on progressive files: amhip_jpeg_info agrees
with every fixture, and every refusal of the host parser is AMHIP_ERR_ARG with its text and the
frame's index, from amhip_jpeg_info and from amhip_io_decode_jpeg_frames before any device is
touched."""
import ctypes as C
import os

import pytest

import jpeg_decode_inputs as DI
import jpeg_progressive_inputs as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_jpeg_info_agrees_with_every_progressive_fixture(L):
    from aerial_mapper_amd import io as AIO
    for name in PI.names():
        w, h = PI.size_of(name)
        assert AIO.jpeg_info(PI.file_bytes(name)) == (w, h, 1 if "gray" in name else 3), name
    for what, data in PI.corrupt_scans().items():
        assert AIO.jpeg_info(data) == (17, 17, 3), what        # (only the device finds these)
    for what, (data, _) in PI.accepted_extras().items():
        assert AIO.jpeg_info(data) == (17, 17, 3), what


def test_refusals_are_reported_by_jpeg_info(L):
    from aerial_mapper_amd import io as AIO
    lib = L.load()
    w, h, ch = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    for what, (data, word) in PI.refusals().items():
        assert lib.amhip_jpeg_info(data, len(data), C.byref(w), C.byref(h), C.byref(ch)) == L.ERR_ARG, what
        text = lib.amhip_last_error().decode()
        assert text.startswith("amhip_jpeg_info: ") and word in text, (what, text)
        with pytest.raises(L.AmhipError):
            AIO.jpeg_info(data)


def test_refusals_are_reported_without_a_device_and_name_the_frame(L):
    """A bad device index (1 << 20) rides along: a header or script error must come first.  The good
    frames around the refused one are a progressive and a baseline file."""
    lib = L.load()
    good = PI.file_bytes("b_spectral_420_17x17")
    base = DI.fixture_bytes("noise_17x17_444_q95")

    def call(files, colored, want=None):
        n = len(files)
        ptrs = (C.c_char_p * n)(*files)
        lens = (C.c_size_t * n)(*[len(f) for f in files])
        out = C.c_void_p(0xDEAD)
        w, h = C.c_int(-1), C.c_int(-1)
        row, stride = C.c_size_t(), C.c_size_t()
        rc = lib.amhip_io_decode_jpeg_frames(1 << 20, ptrs, lens, n, colored, C.byref(out), C.byref(w), C.byref(h),
                                             C.byref(row), C.byref(stride))
        assert rc in (want or (L.ERR_ARG,)) and out.value is None, (rc, out.value)
        return lib.amhip_last_error().decode()

    for what, (data, word) in PI.refusals().items():
        for colored in (0, 1):
            text = call([good, base, data, good], colored)
            assert text.startswith("amhip_io_decode_jpeg_frames: frame 2: ") and word in text, (what, text)
    # a progressive frame of another size than frame 0
    text = call([good, base, PI.file_bytes("b_spectral_420_33x15")], 0)
    assert "frame 2 is 33 x 15, frame 0 is 17 x 17" in text
    # accepted files get as far as the device index
    text = call([good, base, good], 1, want=(L.ERR_ARG, L.ERR_NO_DEVICE))
    assert "bad device index" in text or "no HIP device" in text, text


def test_the_documents_name_the_progressive_shapes():
    for rel in ("include/aerial_mapper_hip.h", "README.md", "INTEGRATION.md", "DESIGN.md", "aerial_mapper_amd/io.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "progressive" in text and "SOF2" in text, rel
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_jpegd_entropy_prog" in design and "block smoothing" in design
