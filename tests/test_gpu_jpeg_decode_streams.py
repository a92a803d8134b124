"""GPU: the batched JPEG decoder on every legal stream shape, not only on what one encoder family
writes: the second fixture family tests/golden/jpeg_decode/streams/ (header rewrites, fill bytes
and stray bytes in the scan, hand-coded scans, flat quantisation tables, Pillow's further shapes),
each with libjpeg-turbo's own pixels beside it.  Bit for bit against those pixels and against
tests/jpeg_decode_reference.py, gray and coloured, one call per frame size; no stream is left out.
And the scans the walk refuses on purpose, among good frames."""
import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
from test_gpu_jpeg_decode import _io, _raw_call, check_batch, decode

pytestmark = pytest.mark.gpu

BY_SIZE = DI.streams_by_size()
N_STREAMS = 170


def test_the_sizes_hold_every_stream_of_the_generators_list():
    names = [n for size in sorted(BY_SIZE) for n in BY_SIZE[size]]
    assert sorted(names) == sorted(DI.stream_names()) and len(names) == len(set(names)) == N_STREAMS
    assert len(BY_SIZE) == 15 and max(max(s) for s in BY_SIZE) == 2049


# ---- 1. the family, one call per frame size ------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("size", sorted(BY_SIZE), ids=lambda s: "%dx%d" % s)
def test_streams_equal_libjpeg_and_the_restatement(size, colored):
    names = BY_SIZE[size]
    files = [DI.stream_bytes(n) for n in names]
    got = decode(files, colored)
    assert got.dtype == np.uint8 and got.shape[:3] == (len(names), size[1], size[0])
    bad = []
    for k, n in enumerate(names):
        want = DI.stream_pixels(n)[1 if colored else 0]
        assert got[k].shape == want.shape, n
        if not np.array_equal(got[k], want):
            bad.append((n, int((got[k] != want).sum())))
    assert not bad, bad
    check_batch(files, colored, size)


# ---- 2. header variants of one picture side by side -----------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("tag", sorted(DI.HEADER_BASES))
def test_header_variants_of_one_picture_decode_to_equal_frames(tag, colored):
    """tables merged, moved, renumbered, defined twice; ids 0 1 2 and r g b; no JFIF; a file inside
    an APP1; fill bytes between segments; DRI without RSTn: one call, every frame the same"""
    names = DI.same_picture_variants(tag)
    assert len(names) == {"420rst": 10, "444": 13, "gray": 9, "420": 2}[tag]
    files = [DI.fixture_bytes(DI.HEADER_BASES[tag])] + [DI.stream_bytes(n) for n in names]
    got = decode(files, colored)
    want = DI.fixture_pixels(DI.HEADER_BASES[tag])[1 if colored else 0]
    assert np.array_equal(got[0], want)
    for k, n in enumerate(names):
        assert np.array_equal(got[k + 1], got[0]), n


# ---- 3. segments and bytes the parser skips, decoded ----------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
def test_accepted_extras_decode_to_the_pixels_of_their_fixture(colored):
    extras = DI.accepted_extras()
    assert len(extras) == 4
    files = [data for data, _ in extras.values()]
    got = decode(files, colored)
    for k, (what, (data, same_as)) in enumerate(extras.items()):
        assert np.array_equal(got[k], DI.fixture_pixels(same_as)[1 if colored else 0]), what
    check_batch(files, colored, "extras")


@pytest.mark.parametrize("colored", [False, True])
def test_a_fill_byte_where_libjpeg_turbo_strays_gives_the_pixels_without_it(colored):
    """0xFF 0xFF 0x00 at scan offset 619 (jpeg_decode_inputs.ff_ff_00_at_619): libjpeg's rule, one
    data byte 0xFF, so the frame equals the fixture's without the fill byte"""
    data, base = DI.ff_ff_00_at_619()
    got = decode([data, DI.fixture_bytes(base)], colored)
    assert np.array_equal(got[0], DI.fixture_pixels(base)[1 if colored else 0])
    assert np.array_equal(got[0], got[1])
    check_batch([data], colored, "0xFF 0xFF 0x00 at 619")


# ---- 4. the refusals that stay (bounded code; each runs once) -------------------------------------
@pytest.mark.parametrize("what,make,good,reason", [
    ("run past 63", DI.run_past_63, "c_zrl_past_63", "a run past coefficient 63"),
    ("undefined ladder code", DI.undefined_ladder_code, "c_ladder_every_length", "an undefined Huffman code"),
    ("wrong RSTn", DI.wrong_rst_behind_stray_bytes, "a_fill_between_segments_420rst", "a wrong or missing RSTn marker"),
], ids=["run-past-63", "undefined-code", "wrong-rst-behind-stray-bytes"])
def test_a_refused_scan_among_good_frames_is_an_error_return_naming_the_frame(what, make, good, reason):
    from aerial_mapper_amd import hip_lib as L
    bad = make()
    good_bytes = DI.stream_bytes(good)      # (of the refusal's size)
    assert _io().jpeg_info(bad)[:2] == _io().jpeg_info(good_bytes)[:2]      # the header is fine
    rc, out, text = _raw_call([good_bytes, good_bytes, bad, good_bytes])
    assert rc == L.ERR_ARG and out is None, (rc, out, text)
    assert text.endswith("frame 2: " + reason), text
    # (the restatement stops at the same rule)
    with pytest.raises(D.Corrupt) as ei:
        D.decode(bad)
    word = {"run past 63": "run past coefficient 63", "undefined ladder code": "undefined Huffman code",
            "wrong RSTn": "wrong or missing RST"}[what]
    assert word in str(ei.value)
    # a following good call still succeeds
    check_batch([good_bytes] * 4, True, "after " + what)
