"""GPU: progressive JPEG frames (SOF2) through the batched decoder (amhip_io_decode_jpeg_frames,
aerial_mapper_amd.io), bit for bit against libjpeg-turbo's pixels (tests/golden/jpeg_progressive/)
and against tests/jpeg_progressive_reference.py, gray and coloured: every file of the family in
stacks grouped by size, stacks that mix baseline and progressive frames, the same stacks split into
groups, and the errors only the device can find."""
import ctypes as C

import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_progressive_inputs as PI
import jpeg_progressive_reference as P

pytestmark = pytest.mark.gpu


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


_ref = {}


def ref(data, colored):
    """the restatement's pixels (baseline files: the baseline restatement's), computed once per file"""
    if data not in _ref:
        d = P.decode(data)
        _ref[data] = (d.gray, d.bgr)
    return _ref[data][1 if colored else 0]


def decode(files, colored):
    fr = _io().decode_jpeg_frames(files, colored=colored)
    try:
        assert fr.num_frames == len(files) and fr.channels == (3 if colored else 1)
        out = fr.to_host()
    finally:
        fr.close()
    return out


# ---- 1. every file of A, B and C --------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("size", sorted(PI.by_size()), ids=lambda s: "%dx%d" % s)
def test_every_file_equals_libjpeg_and_the_restatement(size, colored):
    """one call per size: Pillow's default script at every sampling with and without restart markers,
    and at 17 x 17 and 33 x 15 the hand-written scripts beside them"""
    names = PI.by_size()[size]
    got = decode([PI.file_bytes(n) for n in names], colored)
    assert got.dtype == np.uint8 and got.shape[:3] == (len(names), size[1], size[0])
    for k, n in enumerate(names):
        want = PI.pixels(n)[1 if colored else 0]
        assert np.array_equal(got[k], want), (n, int((got[k] != want).sum()))
        assert np.array_equal(got[k], ref(PI.file_bytes(n), colored)), n


def test_the_family_is_whole():
    by = PI.by_size()
    assert sum(len(v) for v in by.values()) == len(PI.names()) == 182
    assert len(by[(17, 17)]) >= 21 + 27 and len(by[(2048, 1024)]) == 1 and len(by[(1024, 1032)]) == 1


# ---- 2. baseline and progressive frames in one call -------------------------------------------------
def _mixed_17():
    base = [DI.fixture_bytes(n) for n in DI.fixtures_by_size()[(17, 17)]]
    prog = [PI.file_bytes(n) for n in PI.by_size()[(17, 17)]]
    # baseline runs of one, two and three frames between progressive frames, either kind first and last
    order = [prog[0], base[0], prog[1], prog[2], base[1], base[2], prog[3], base[3], base[4], base[5], prog[4]]
    order += [x for pair in zip(base[6:], prog[5:]) for x in pair] + prog[5 + len(base[6:]):] + [base[0]]
    return order


@pytest.mark.parametrize("colored", [False, True])
def test_a_mixed_stack_equals_its_frames_one_by_one(colored):
    files = _mixed_17()
    assert 20 < len(files) < 80
    got = decode(files, colored)
    for k, data in enumerate(files):
        assert np.array_equal(decode([data], colored)[0], got[k]), k
        assert np.array_equal(got[k], ref(data, colored)), k


@pytest.mark.parametrize("budget_mb", [0.0, 0.01])
@pytest.mark.parametrize("colored", [False, True])
def test_groups_of_a_mixed_stack_equal_one_group(colored, budget_mb, tuning):
    """0: one frame per group; 10 KB: three frames of 17 x 17 at 4:4:4 (27 blocks of 128 bytes) or at
    4:2:0 (24 blocks), nine gray ones: groups that begin and end inside runs of either kind"""
    files = _mixed_17()
    whole = decode(files, colored)
    tuning(jpegd_coef_budget_mb=budget_mb)
    got = decode(files, colored)
    assert np.array_equal(got, whole)


# ---- 3. errors only the device can find (bounded code; each runs once) ------------------------------
def _raw_call(files, colored=0):
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    n = len(files)
    ptrs = (C.c_char_p * n)(*files)
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = C.c_void_p(0xDEAD)
    w, h = C.c_int(), C.c_int()
    row, stride = C.c_size_t(), C.c_size_t()
    rc = lib.amhip_io_decode_jpeg_frames(0, ptrs, lens, n, colored, C.byref(out), C.byref(w), C.byref(h),
                                         C.byref(row), C.byref(stride))
    return rc, out.value, lib.amhip_last_error().decode()


@pytest.mark.parametrize("what", sorted(PI.CORRUPT_REASONS))
def test_a_corrupt_scan_is_an_error_return_naming_the_frame(what):
    from aerial_mapper_amd import hip_lib as L
    good = PI.file_bytes("b_spectral_420_17x17")
    base = DI.fixture_bytes("noise_17x17_420_q95_rst1")
    bad = PI.corrupt_scans()[what]
    assert _io().jpeg_info(bad) == (17, 17, 3)          # the header and the script are fine
    rc, out, text = _raw_call([good, base, bad, good])
    assert rc == L.ERR_ARG and out is None, (rc, out, text)
    assert text.endswith("frame 2: " + PI.CORRUPT_REASONS[what][0]), text
    # (the restatement stops at the same rule)
    with pytest.raises(P.Corrupt) as ei:
        P.decode(bad)
    assert PI.CORRUPT_REASONS[what][1] in str(ei.value)
    # a following good call still succeeds
    got = decode([good, base, good], True)
    assert np.array_equal(got[0], ref(good, True)) and np.array_equal(got[1], ref(base, True))
