"""tests/png_decode_reference.py, the PNG decoder restated rule by rule, against the committed
fixtures of tests/golden/png_decode/ and against the real libraries: zlib.decompress for the
scanlines, Pillow (where it is importable) for raw pixels and B, G, R.  The gray of a colour file is
checked against its stated formula only, (9797 R + 19234 G + 3737 B) >> 15: libpng's rgb_to_gray as
cv::imread sets it up cannot be pinned here (adopted, unpinned)."""
import zlib

import numpy as np
import pytest

import png_decode_inputs as PI
import png_decode_reference as R

_decoded = {}


def decoded(name):
    if name not in _decoded:
        _decoded[name] = R.decode(PI.fixture_bytes(name))
    return _decoded[name]


def test_every_fixture_equals_its_committed_pixels_and_zlib():
    names = PI.fixture_names()
    assert len(names) == 56
    for n in names:
        d = decoded(n)
        gray, bgr = PI.fixture_pixels(n)
        assert np.array_equal(d.gray, gray) and np.array_equal(d.bgr, bgr), n
        assert zlib.decompress(d.header.stream) == d.raw, n


def test_every_fixture_equals_pillow():
    pytest.importorskip("PIL")
    for n in PI.fixture_names():
        d = decoded(n)
        gray, bgr = PI.pillow_pixels(PI.fixture_bytes(n))
        assert np.array_equal(d.bgr, bgr), n
        if gray is not None:
            assert np.array_equal(d.gray, gray), n


def test_gray_of_a_colour_file_is_the_stated_formula():
    """against the formula only: truncating, and exact when R = G = B"""
    seen = 0
    for n in PI.fixture_names():
        d = decoded(n)
        if d.header.colour_type in (0, 4):
            assert np.array_equal(d.bgr[:, :, 0], d.gray) and np.array_equal(d.bgr[:, :, 2], d.gray), n
            continue
        B, G, R_ = (d.bgr[:, :, k].astype(np.int64) for k in range(3))
        assert np.array_equal(d.gray, (9797 * R_ + 19234 * G + 3737 * B) >> 15), n
        seen += 1
    assert seen > 20
    assert 9797 + 19234 + 3737 == 32768


def test_the_family_reaches_every_rule():
    total = R.Counters()
    for n in PI.fixture_names():
        total.add(decoded(n).counters)
    PI.check_coverage(total)
    # python's zlib: stored at level 0, fixed codes under Z_FIXED, dynamic otherwise
    assert decoded("z_level0_129x47_rgb").counters.blocks[1:] == [0, 0]
    c = decoded("z_fixed_129x47_rgb").counters.blocks
    assert c[0] == 0 and c[1] > 0 and c[2] == 0
    for v in ("level1", "level6", "level9", "rle", "huffman_only", "filtered", "wbits9"):
        assert decoded("z_%s_129x47_rgb" % v).counters.blocks[2] > 0, v
    # zlib's matcher never reaches distance 32768: only the hand-coded stream does
    assert 29 in decoded("hand_len258_dist32768_200x190_gray").counters.dist_codes
    b = decoded("hand_blocks_256x256_gray").counters.blocks      # empty + 65535 + 8 offsets; fixed ones between; one dynamic
    assert b[0] == 10 and b[1] >= 3 and b[2] == 1, b


def test_refusals_and_device_errors_stop_at_their_rule():
    for what, (data, word) in PI.refusals().items():
        with pytest.raises(R.Refused) as ei:
            R.parse(data)
        assert word in str(ei.value), what
    errors = PI.device_errors()
    assert set(text for _, text in errors.values()) == set(R.STATUS.values())
    for what, (data, text) in errors.items():
        with pytest.raises(R.Corrupt) as ei:
            R.decode(data)
        assert str(ei.value) == text, what
