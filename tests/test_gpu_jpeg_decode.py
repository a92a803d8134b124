"""GPU: the batched JPEG decoder (amhip_io_decode_jpeg_frames, aerial_mapper_amd.io) against
tests/jpeg_decode_reference.py, bit for bit: every fixture of tests/golden/jpeg_decode/ and every
file of tests/golden/jpeg/, gray and coloured, in batches grouped by size; more frames than one
scheduling round holds; a round trip through the GPU encoder; the errors the device finds; and the
decoded stack handed unchanged to the mosaic and to Stereo."""
import ctypes as C

import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
import jpeg_inputs as I

pytestmark = pytest.mark.gpu


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


_ref = {}


def ref(data, colored):
    """the restatement's pixels, computed once per file"""
    if data not in _ref:
        d = D.decode(data)
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


def check_batch(files, colored, what):
    got = decode(files, colored)
    assert got.dtype == np.uint8 and got.shape[0] == len(files)
    for k, data in enumerate(files):
        want = ref(data, colored)
        assert got[k].shape == want.shape, (what, k)
        assert np.array_equal(got[k], want), (what, k, int((got[k] != want).sum()))


# ---- 1. the fixtures libjpeg-turbo wrote and decoded ----------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("size", DI.SIZES, ids=lambda s: "%dx%d" % s)
def test_new_fixtures_equal_the_restatement_and_libjpeg(size, colored):
    """one call per size: 4:4:4, 4:2:2, 4:2:0 with two restart intervals, a file's own Huffman
    tables and gray, of two contents, side by side"""
    names = DI.fixtures_by_size()[size]
    files = [DI.fixture_bytes(n) for n in names]
    check_batch(files, colored, size)
    got = decode(files, colored)
    for k, n in enumerate(names):
        assert np.array_equal(got[k], DI.fixture_pixels(n)[1 if colored else 0]), n


# ---- 2. the files the encoder is held to ---------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("size", I.SIZES, ids=lambda s: "%dx%d" % s)
def test_encoder_fixtures_equal_the_restatement(size, colored):
    """the four qualities of one input make one call: their scans differ by more than 10 x in length"""
    n = 0
    for case, files in DI.encoder_files_by_case():
        if (case.width, case.height) != size:
            continue
        if case.content == "noise" and case.width * case.height > 4000:
            scans = [h.scan_end - h.scan_begin for h in (D.parse_header(f) for f in files)]
            assert max(scans) > 10 * min(scans), (case, scans)
        check_batch(files, colored, case)
        n += len(files)
    assert n >= 7 * 2 * 4


# ---- 3. more frames than one round of waves ------------------------------------------------------
def _files_17():
    files = [DI.fixture_bytes(n) for n in DI.fixtures_by_size()[(17, 17)]]
    for case, fs in DI.encoder_files_by_case():
        if (case.width, case.height) == (17, 17):
            files += fs
    return [files[k % len(files)] for k in range(130)]


@pytest.mark.parametrize("colored", [False, True])
def test_130_frames_in_one_call_equal_130_calls(colored):
    files = _files_17()
    assert len(files) == 130 and len(set(files)) > 70
    fr = _io().decode_jpeg_frames(files, colored=colored)
    try:
        t = fr.frames
        tail = (3, 1) if colored else (1,)
        assert tuple(t.shape) == (130, 17, 17) + ((3,) if colored else ())
        assert fr.row_step >= 17 * len(tail) * 1 and fr.frame_stride >= 17 * fr.row_step
        assert tuple(t.stride()) == (fr.frame_stride, fr.row_step) + tail
        got = t.cpu().numpy()
        # a cropped view walks the same strides
        crop = t[5:120:7, 3:11, 2:15]
        assert tuple(crop.stride())[:2] == (7 * fr.frame_stride, fr.row_step)
        assert np.array_equal(crop.cpu().numpy(), got[5:120:7, 3:11, 2:15])
    finally:
        fr.close()
    for k, data in enumerate(files):
        one = decode([data], colored)
        assert np.array_equal(one[0], got[k]), k
        assert np.array_equal(got[k], ref(data, colored)), k


@pytest.mark.parametrize("budget_mb", [0.01, 0.0])
@pytest.mark.parametrize("colored", [False, True])
def test_groups_of_frames_equal_one_group(colored, budget_mb, tuning):
    """the coefficient budget splits a call into groups that run one after another and reuse the
    scratch: 10 KB holds 3 to 9 of these frames (their samplings differ), 0 one frame per group"""
    files = _files_17()
    whole = decode(files, colored)
    tuning(jpegd_coef_budget_mb=budget_mb)
    got = decode(files, colored)
    assert np.array_equal(got, whole)
    for k, data in enumerate(files):
        assert np.array_equal(got[k], ref(data, colored)), k


# ---- 4. what the GPU encoder writes --------------------------------------------------------------
@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def test_round_trip_through_the_gpu_encoder(gmap):
    from aerial_mapper_amd import export
    for (w, h, ch) in ((513, 24, 1), (129, 47, 3)):
        files = [export.encode_jpeg(gmap, I.make_image(c, w, h, ch), q)
                 for c, q in (("noise", 95), ("ramp", 95), ("checker", 50))]
        assert _io().jpeg_info(files[0]) == (w, h, ch)
        for colored in (False, True):
            check_batch(files, colored, (w, h, ch))


# ---- 5. errors only the device can find (bounded code; each runs once) ---------------------------
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


@pytest.mark.parametrize("what,reason", [("all-one bits", "an undefined Huffman code"),
                                         ("scan cut in half", "the scan ends before its last block"),
                                         ("RST1 altered", "a wrong or missing RSTn marker")])
def test_a_corrupt_scan_is_an_error_return_naming_the_frame(what, reason):
    from aerial_mapper_amd import hip_lib as L
    good = DI.fixture_bytes("noise_17x17_420_q95_rst1")
    bad = DI.corrupt_scans()[what]
    assert _io().jpeg_info(bad) == (17, 17, 3)          # the header is fine
    rc, out, text = _raw_call([good, good, bad, good])
    assert rc == L.ERR_ARG and out is None, (rc, out, text)
    assert text.endswith("frame 2: " + reason), text
    # (the restatement stops at the same rule)
    with pytest.raises(D.Corrupt) as ei:
        D.decode(bad)
    assert DI.CORRUPT_REASONS[what] in str(ei.value)
    # a following good call still succeeds
    check_batch([good, good, good, good], True, "after " + what)


# ---- 6. the decoded stack goes unchanged into the mosaic and into Stereo ----------------------------
def test_decoded_stack_feeds_ortho_backward_grid(gmap):
    import aerial_mapper_amd as A
    import scenarios as S
    from aerial_mapper_amd import export
    sc = S.Scene(60.0, 44.0, 0.5, 100, seed=71, num_frames=5, altitude=300.0)
    cam = sc.cam
    files = [export.encode_jpeg(gmap, f, 95) for f in sc.frames]
    names = ["ortho", "num_observations", "observation_index", "elevation_angle"]
    outs = []
    fr = _io().decode_jpeg_frames(files)
    try:
        for images in (fr.frames, [ref(f, False) for f in files]):
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


def test_decoded_stack_feeds_stereo(gmap):
    import aerial_mapper_amd as A
    import stereo_sequence as SS
    from aerial_mapper_amd import export
    seq = SS.Sequence(3, 240, 160)
    files = [export.encode_jpeg(gmap, np.ascontiguousarray(f), 95) for f in seq.frames]
    K = seq.K
    nc = A.NCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], seq.W, seq.H, 0, (0.0, 0.0, 0.0, 0.0), seq.T_C_B)
    clouds = []
    fr = _io().decode_jpeg_frames(files)
    try:
        for images in (fr.frames, [ref(f, False) for f in files]):
            with A.Stereo(nc, A.StereoSettings(use_every_nth_image=1, images_need_undistortion=False), A.BlockMatchingParameters(use_BM=True), gmap) as st:
                xyz, inten = st.add_frames(seq.T_G_B, images)[:2]
                clouds.append((xyz.cpu().numpy().copy(), inten.cpu().numpy().copy()))
    finally:
        fr.close()
    assert clouds[1][0].shape[0] > 1000
    assert np.array_equal(clouds[0][0].view(np.uint64), clouds[1][0].view(np.uint64))
    assert np.array_equal(clouds[0][1], clouds[1][1])
