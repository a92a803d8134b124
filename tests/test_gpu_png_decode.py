"""GPU: the batched PNG decoder (amhip_io_decode_png_frames, aerial_mapper_amd.io) bit for bit against
the committed pixels of tests/golden/png_decode/ (zlib's scanlines, Pillow's pixels) and against
tests/png_decode_reference.py: every fixture, gray and coloured, in one call per size; colour types
mixed in one call; groups of frames under pngd_raw_budget_mb; every error the device finds, each as
one frame among good ones; a size mismatch; and the decoded stack handed unchanged to the mosaic.

The gray of a colour file is held to the stated formula only, (9797 R + 19234 G + 3737 B) >> 15
(libpng's rgb_to_gray as cv::imread sets it up: adopted, unpinned)."""
import ctypes as C

import numpy as np
import pytest

import png_decode_inputs as PI
import png_decode_reference as R

pytestmark = pytest.mark.gpu


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


_ref = {}


def ref(data, colored):
    """the restatement's pixels, computed once per file"""
    if data not in _ref:
        d = R.decode(data)
        _ref[data] = (d.gray, d.bgr)
    return _ref[data][1 if colored else 0]


def decode(files, colored):
    fr = _io().decode_png_frames(files, colored=colored)
    try:
        assert fr.num_frames == len(files) and fr.channels == (3 if colored else 1)
        assert fr.row_step == fr.width * fr.channels and fr.frame_stride == fr.height * fr.row_step
        out = fr.to_host()
    finally:
        fr.close()
    return out


SIZES = sorted(PI.fixtures_by_size())


def test_the_family_is_whole():
    """no fixture left out: the committed family is the one the generator asserts its coverage on"""
    names = PI.fixture_names()
    assert len(names) == 56 and sum(len(v) for v in PI.fixtures_by_size().values()) == 56
    for want in ("hand_len258_dist32768_200x190_gray", "hand_all_codes_200x190_gray", "hand_blocks_256x256_gray",
                 "hand_repeats_17x17_gray", "hand_len15_codes_17x17_gray", "idat_bytes_64x3_rgb",
                 "chunks_ancillary_17x17_p", "z_level0_129x47_rgb", "z_fixed_129x47_rgb", "ct6_1x1"):
        assert want in names


@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_fixture_equals_the_committed_pixels_and_the_restatement(size, colored):
    """one call per size: whatever colour types, filters, block types and IDAT splits share it"""
    names = PI.fixtures_by_size()[size]
    files = [PI.fixture_bytes(n) for n in names]
    got = decode(files, colored)
    assert got.dtype == np.uint8 and got.shape[0] == len(files)
    for k, n in enumerate(names):
        want = PI.fixture_pixels(n)[1 if colored else 0]
        assert got[k].shape == want.shape, n
        assert np.array_equal(got[k], want), (n, int((got[k] != want).sum()))
        assert np.array_equal(got[k], ref(files[k], colored)), n


@pytest.mark.parametrize("colored", [False, True])
def test_mixed_colour_types_in_one_call(colored):
    names = ["ct%d_129x47" % ct for ct in (6, 0, 3, 2, 4)] + ["z_level6_129x47_rgb", "size_129x47_gray"]
    files = [PI.fixture_bytes(n) for n in names]
    assert sorted(set(R.parse(f).colour_type for f in files)) == [0, 2, 3, 4, 6]
    got = decode(files, colored)
    for k, n in enumerate(names):
        assert np.array_equal(got[k], PI.fixture_pixels(n)[1 if colored else 0]), n


def _files_17():
    names = PI.fixtures_by_size()[(17, 17)]
    return [PI.fixture_bytes(names[k % len(names)]) for k in range(70)]


@pytest.mark.parametrize("budget_mb", [0.002, 0.0])
@pytest.mark.parametrize("colored", [False, True])
def test_groups_of_frames_equal_one_group(colored, budget_mb, tuning):
    """70 frames, more than one round of waves holds per CU; 2 KB of raw scanlines hold 1 to 6 of these
    frames (306 to 1173 bytes each), 0 one frame per group"""
    files = _files_17()
    whole = decode(files, colored)
    for k, data in enumerate(files):
        assert np.array_equal(whole[k], ref(data, colored)), k
    tuning(pngd_raw_budget_mb=budget_mb)
    assert np.array_equal(decode(files, colored), whole)


def _raw_call(files, colored=0):
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    n = len(files)
    ptrs = (C.c_char_p * n)(*files)
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    out = C.c_void_p(0xDEAD)
    w, h = C.c_int(), C.c_int()
    row, stride = C.c_size_t(), C.c_size_t()
    rc = lib.amhip_io_decode_png_frames(0, ptrs, lens, n, colored, C.byref(out), C.byref(w), C.byref(h),
                                        C.byref(row), C.byref(stride))
    return rc, out.value, lib.amhip_last_error().decode()


@pytest.mark.parametrize("what", sorted(PI.device_errors()))
def test_a_stream_the_device_refuses_is_an_error_return_naming_the_frame(what):
    """malformed streams are inputs with a status, bounded like any other; each runs once"""
    from aerial_mapper_amd import hip_lib as L
    bad, reason = PI.device_errors()[what]
    good = PI.good_17x17()
    assert _io().png_info(bad)[:2] == (17, 17)          # the header is fine
    # (the restatement stops at the same rule)
    with pytest.raises(R.Corrupt) as ei:
        R.decode(bad)
    assert str(ei.value) == reason
    rc, out, text = _raw_call([good, good, bad, good], colored=1)
    assert rc == L.ERR_ARG and out is None, (rc, out, text)
    assert text == "amhip_io_decode_png_frames: frame 2: " + reason, text
    # a following good call on the same device still decodes
    got = decode([good, good], True)
    assert np.array_equal(got[0], ref(good, True)) and np.array_equal(got[1], got[0])


def test_a_size_mismatch_names_the_frame():
    from aerial_mapper_amd import hip_lib as L
    a, b = PI.fixture_bytes("size_17x17_gray"), PI.fixture_bytes("size_64x3_gray")
    rc, out, text = _raw_call([a, a, a, b, a])
    assert rc == L.ERR_ARG and out is None
    assert "frame 3 is 64 x 3, frame 0 is 17 x 17" in text


def test_decoded_stack_feeds_ortho_backward_grid():
    """one small gray mosaic from a PNG stack in HBM and from the same pixels uploaded: identical layers"""
    import aerial_mapper_amd as A
    import scenarios as S
    sc = S.Scene(60.0, 44.0, 0.5, 100, seed=71, num_frames=5, altitude=300.0)
    cam = sc.cam
    files = []
    for f in sc.frames:
        rows = np.ascontiguousarray(f).reshape(f.shape[0], -1)
        stream = PI.zdeflate(PI.filter_rows(rows, 1, [y % 5 for y in range(rows.shape[0])]))
        files.append(PI.png(f.shape[1], f.shape[0], 0, stream))
    names = ["ortho", "num_observations", "observation_index", "elevation_angle"]
    outs = []
    fr = _io().decode_png_frames(files)
    try:
        assert np.array_equal(fr.to_host(), np.stack([np.asarray(f) for f in sc.frames]))
        for images in (fr.frames, [np.ascontiguousarray(f) for f in sc.frames]):
            g = sc.grid
            with A.AerialGridMap(A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)) as m:
                m.set("elevation", np.zeros((m.cols, m.rows), np.float32))
                nc = A.NCamera(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height, cam.distortion,
                               tuple(cam.dist), sc.T_C_B)
                A.OrthoBackwardGrid(nc, A.OrthoSettings(), m).process(sc.poses, images, m)
                outs.append({n: m.get(n) for n in names})
    finally:
        fr.close()
    assert (~np.isnan(outs[1]["observation_index"])).mean() > 0.3
    S.assert_layers_equal(outs[0], outs[1], names)
