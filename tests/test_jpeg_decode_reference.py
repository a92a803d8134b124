"""CPU: tests/jpeg_decode_reference.py (the yardstick of the GPU JPEG decoder) against libjpeg's own
pixels: the .npz beside every fixture of tests/golden/jpeg_decode/ (what libjpeg-turbo decoded when
the fixtures were written), Pillow directly on the 576 files of tests/golden/jpeg/ where Pillow is
present, and tests/jpeg_reference.py's coefficients.  And that the fixtures reach every branch.
The same for the second family, tests/golden/jpeg_decode/streams/: stream shapes no encoder of
ours writes (jpeg_decode_inputs.stream_names())."""
import glob
import os


import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
import jpeg_inputs as I
import jpeg_reference as J


@pytest.fixture(scope="module")
def decoded():
    """every fixture decoded once, with the branch counters of the whole list"""
    counters = D.AllCounters()
    per_file = {}
    out = {}
    for name in DI.fixture_names():
        c = D.AllCounters()
        out[name] = D.decode(DI.fixture_bytes(name), c)
        per_file[name] = c
        for part in ("entropy", "idct", "sample"):
            a, b = getattr(counters, part), getattr(c, part)
            for k, v in vars(b).items():
                setattr(a, k, getattr(a, k, 0) + v)
    return out, counters, per_file


def test_fixture_list_is_the_committed_one():
    import glob
    import os
    have = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(DI.GOLDEN, "*.jpg")))
    assert have == sorted(DI.fixture_names()) and len(have) == 96
    for name in have:
        assert os.path.getsize(DI.fixture_path(name)) < 16 * 1024


def test_restatement_equals_libjpeg_on_every_fixture(decoded):
    out = decoded[0]
    for name, d in out.items():
        gray, bgr = DI.fixture_pixels(name)
        assert d.gray.dtype == np.uint8 and d.gray.shape == gray.shape, name
        assert np.array_equal(d.gray, gray), name
        assert np.array_equal(d.bgr, bgr), name


def test_headers_of_the_fixtures_are_what_the_variants_say(decoded):
    out = decoded[0]
    for (w, h) in DI.SIZES:
        for c in DI.CONTENTS:
            want = {"444_q95": (3, (1, 1), 0), "422_q50": (3, (2, 1), 0), "420_q95_rst1": (3, (2, 2), 1),
                    "420_q95_rst3": (3, (2, 2), 3), "420_q50_opt": (3, (2, 2), 0), "gray_q95_rst2": (1, None, 2)}
            for v, (ch, samp, rst) in want.items():
                hd = out["%s_%dx%d_%s" % (c, w, h, v)].header
                assert (hd.width, hd.height, hd.channels) == (w, h, ch)
                if samp:
                    assert (hd.comps[0]["h"], hd.comps[0]["v"]) == samp
                # restart_marker_blocks counts MCUs
                assert hd.restart == rst, (c, w, h, v)
    # optimize=True: the tables differ from file to file and from the standard ones
    tabs = set()
    for (w, h) in DI.SIZES:
        hd = out["noise_%dx%d_420_q50_opt" % (w, h)].header
        tabs.add(tuple(hd.huff[(1, 0)].bits))
        assert hd.huff[(1, 0)].bits != J.AC_LUM_BITS
    assert len(tabs) > 4


def test_fixtures_reach_every_branch(decoded):
    _, c, per_file = decoded
    # upsampling: replication at dw <= 2, both fancy filters, 4:4:4
    assert c.sample.replicated and c.sample.h2v1_fancy and c.sample.h2v2_fancy and c.sample.fullsize
    for v, attr in (("422_q50", "h2v1_fancy"), ("420_q95_rst1", "h2v2_fancy")):
        # dw = 2 is the last size that replicates, dw = 3 the first that filters
        assert per_file["noise_4x4_" + v].sample.replicated == 2 and not getattr(per_file["noise_4x4_" + v].sample, attr)
        assert per_file["noise_3x2_" + v].sample.replicated == 2
        assert getattr(per_file["noise_5x5_" + v].sample, attr) == 2 and not per_file["noise_5x5_" + v].sample.replicated
    # a code longer than the lookahead: the maxcode loop
    assert c.entropy.slow_codes > 100
    assert per_file["noise_129x47_420_q50_opt"].entropy.slow_codes > 0    # ... with a file's own tables too
    # RSTn: n wraps past 7; an interval that does not divide the MCU count
    assert c.entropy.rst_wraps > 0
    e = per_file["noise_129x47_420_q95_rst1"].entropy
    assert e.restarts == 26 and e.rst_wraps == 3
    # (129 x 47 at 4:2:0 is 9 x 3 MCUs: intervals of 3 divide them, 8 markers ...)
    assert per_file["noise_129x47_420_q95_rst3"].entropy.restarts == 8
    # (... 17 x 17 is 2 x 2 MCUs: the last interval of 3 is cut short)
    hd = decoded[0]["noise_17x17_420_q95_rst3"].header
    assert (2 * 2) % hd.restart != 0 and per_file["noise_17x17_420_q95_rst3"].entropy.restarts == 1
    # 0xFF 0x00 in the data
    assert c.entropy.stuffed > 0
    # clamping at 0 and at 255
    assert c.idct.clamped_low > 0 and c.idct.clamped_high > 0


def _scan_order(hd, coefs):
    """plane-ordered natural coefficients -> (N, 64) zigzag in the order the scan codes the blocks"""
    hmax, vmax, mcux, mcuy, samp = D.layout(hd)
    rows = []
    for my in range(mcuy):
        for mx in range(mcux):
            for ci, (hh, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(hh):
                        rows.append(coefs[ci][my * v + by, mx * hh + bx][J.ZIGZAG])
    return np.array(rows)


def test_coefficients_equal_the_encoder_restatements_decoder():
    n = 0
    for case in I.cases():
        for q in I.QUALITIES:
            n += 1
            data = open(I.golden_jpg(case, q), "rb").read()
            want = J.decode(data)
            hd = D.parse_header(data)
            got = _scan_order(hd, D.entropy_decode(data, hd))
            assert np.array_equal(got, want.coef), (case, q)
    assert n == 576


def test_restatement_equals_pillow_on_the_encoder_fixtures():
    PIL_Image = pytest.importorskip("PIL.Image")
    import io
    files = DI.all_encoder_files()
    assert len(files) == 576
    for f in files:
        data = open(f, "rb").read()
        d = D.decode(data)
        im = PIL_Image.open(io.BytesIO(data))
        im.draft("L", im.size)
        assert np.array_equal(d.gray, np.asarray(im)), f
        rgb = np.asarray(PIL_Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(d.bgr, rgb[..., ::-1]), f


def test_refused_files_are_refused_with_a_text_and_extras_are_skipped():
    for what, (data, word) in DI.refusals().items():
        with pytest.raises(D.Refused) as ei:
            D.parse_header(data)
        assert word in str(ei.value), (what, str(ei.value))
    for what, (data, same_as) in DI.accepted_extras().items():
        gray, bgr = DI.fixture_pixels(same_as)
        d = D.decode(data)
        assert np.array_equal(d.gray, gray) and np.array_equal(d.bgr, bgr), what


def test_corrupt_scans_are_found():
    for what, data in DI.corrupt_scans().items():
        D.parse_header(data)
        with pytest.raises(D.Corrupt):
            D.decode(data)


# ---------------------------------------------------------------------------
# the second family: every legal stream shape (tests/golden/jpeg_decode/streams/)
# ---------------------------------------------------------------------------


def _merge(total, one):
    """counters of one file into the family's: max_* / highest by max, lowest by min, the rest summed"""
    for part in ("entropy", "idct", "sample"):
        a, b = getattr(total, part), getattr(one, part)
        for k, v in vars(b).items():
            if k.startswith("max_") or k == "highest":
                setattr(a, k, max(getattr(a, k, 0), v))
            elif k == "lowest":
                setattr(a, k, min(getattr(a, k, 0), v))
            else:
                setattr(a, k, getattr(a, k, 0) + v)


@pytest.fixture(scope="module")
def streams():
    """every stream decoded once: {name: Decoded}, the family's counters, {name: counters}"""
    total, per_file, out = D.AllCounters(), {}, {}
    for name in DI.stream_names():
        c = D.AllCounters()
        out[name] = D.decode(DI.stream_bytes(name), c)
        per_file[name] = c
        _merge(total, c)
    return out, total, per_file


def test_stream_list_is_the_committed_one_and_small():
    names = DI.stream_names()
    assert len(names) == len(set(names)) == 170
    assert len(DI.stream_rewrites()) == 66 and len(DI.pillow_specs()) == 104
    jpg = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(DI.STREAMS, "*.jpg")))
    npz = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(DI.STREAMS, "*.npz")))
    assert npz == sorted(names)
    assert jpg == sorted(n for n in names if n not in DI.BUILT_NOT_COMMITTED)
    sizes = [os.path.getsize(f) for f in glob.glob(os.path.join(DI.STREAMS, "*"))]
    assert max(sizes) < 25 * 1024 and sum(sizes) < 512 * 1024
    for n in jpg:
        assert os.path.getsize(DI.stream_path(n)) < 16 * 1024, n


def test_rewrites_and_hand_coded_scans_are_the_committed_bytes():
    """groups a to d are derived from committed fixtures without an encoder: the derivation gives
    the very bytes libjpeg-turbo decoded when the .npz files were written"""
    for name, data in DI.stream_rewrites().items():
        if name not in DI.BUILT_NOT_COMMITTED:
            with open(DI.stream_path(name), "rb") as f:
                assert f.read() == data, name


def test_restatement_equals_libjpeg_on_every_stream(streams):
    out = streams[0]
    assert len(out) == 170
    for name, d in out.items():
        gray, bgr = DI.stream_pixels(name)
        assert d.gray.dtype == np.uint8 and d.gray.shape == gray.shape and d.bgr.shape == bgr.shape, name
        assert np.array_equal(d.gray, gray), (name, int((d.gray != gray).sum()))
        assert np.array_equal(d.bgr, bgr), (name, int((d.bgr != bgr).sum()))


def test_header_rewrites_give_the_pixels_of_their_base(streams):
    out = streams[0]
    n = 0
    for tag, base in DI.HEADER_BASES.items():
        gray, bgr = DI.fixture_pixels(base)
        for name in DI.same_picture_variants(tag):
            n += 1
            assert np.array_equal(out[name].gray, gray) and np.array_equal(out[name].bgr, bgr), name
    assert n == len(DI.header_rewrites()) == 34
    # ... and so does a fill byte where libjpeg-turbo's fast path strays from libjpeg's rule
    data, base = DI.ff_ff_00_at_619()
    d = D.decode(data)
    gray, bgr = DI.fixture_pixels(base)
    assert np.array_equal(d.gray, gray) and np.array_equal(d.bgr, bgr)


def test_streams_reach_what_the_encoder_fixtures_do_not(streams):
    out, c, per_file = streams
    e = c.entropy
    # a slow code of every length 9..16 (the ladder tables), in one file and on the whole
    assert all(per_file["c_ladder_every_length"].entropy.slow_by_length[9:17] > 0)
    assert all(e.slow_by_length[9:17] > 0) and e.slow_by_length[:9].sum() == 0
    assert e.slow_by_length.sum() == e.slow_codes
    # the largest sizes a baseline scan may hold, both signs of each
    assert e.max_dc_size == 11 and e.max_ac_size == 10
    dc = out["c_dc_category_11"].coefs[0][0, :, 0]
    assert list(dc[:4]) == [2047, 0, -2047, 0]
    at63 = out["c_ac_size_10_at_63"].coefs[0][0, :, 63]
    assert list(at63[:4]) == [1023, -1023, 512, -512]
    # 63 coefficients and no EOB; three ZRL and a coefficient at 63; a ZRL past 63 ends the block
    full = out["c_63_coefficients_no_eob"].coefs[0][0]
    assert all((full[k][1:] != 0).all() for k in range(3)) and per_file["c_63_coefficients_no_eob"].entropy.at_63 == 3
    pe = per_file["c_three_zrl_then_63"].entropy
    assert pe.at_63 == 2 and pe.zrls == 6
    assert list(out["c_three_zrl_then_63"].coefs[0][0, :3, 63]) == [1, 0, -1]
    pe = per_file["c_zrl_past_63"].entropy
    assert pe.zrl_past_63 == 2 and pe.zrls == 8 and pe.at_63 == 0
    # (the blocks behind them are where they belong: the predictor goes 25, -25, 0, 9)
    assert list(out["c_zrl_past_63"].coefs[0][0, :5, 0]) == [25, -25, 0, 9, 9]
    # fill bytes in front of RSTn and of a stuffed byte, stuffed bytes, bytes in front of EOI
    assert e.stuffed > 0 and e.fill_bytes > 0 and e.trailing > 0
    assert per_file["b_fill3_before_one_rst"].entropy.fill_bytes == 3
    pe = per_file["b_fill2_before_every_rst_gray"].entropy
    assert pe.restarts == 50 and pe.fill_bytes == 100 and pe.rst_wraps == 6
    assert per_file["b_ff_ff_00_444"].entropy.fill_bytes == 1
    pe = per_file["b_ff_ff_ff_00_everywhere_444"].entropy
    assert pe.fill_bytes == 2 * pe.stuffed > 0
    # bytes between an interval's data and its RSTn, beyond what a refill has read ahead
    assert [per_file["b_bytes_%d_before_one_rst" % n].entropy.before_rst for n in (1, 9, 20)] == [0, 2, 13]
    assert per_file["b_bytes_before_every_rst_gray"].entropy.before_rst >= 4 * 2
    pe = per_file["b_bytes_with_ff_00_before_rst"].entropy
    assert pe.before_rst > 0 and pe.fill_bytes == 1
    # (a refill reads up to 7 bytes ahead: of 8, 9 and 20 bytes 1, 2 and 13 are left unread)
    assert [per_file["b_trailing_%d_420" % n].entropy.trailing for n in (1, 7, 8, 9, 20)] == [0, 0, 1, 2, 13]
    # a restart counter that wraps past RST7 in a Pillow-written file of one row of MCUs
    pe = per_file["e_random_2049x1_422_q30_rst1"].entropy
    assert pe.restarts == 128 and pe.rst_wraps == 16
    # DRI without RSTn: an interval longer than the scan
    for name in ("a_dri_60000_444", "a_dri_60000_420", "e_random_32x16_444_q100_rst60000"):
        assert out[name].header.restart == 60000 and per_file[name].entropy.restarts == 0, name
    assert out["a_dri_0_444"].header.restart == 0
    # clamping on both sides, and IDCT output up to the edge of the contract (+-1303) and not beyond
    assert c.idct.clamped_low > 0 and c.idct.clamped_high > 0
    assert c.idct.lowest == -1303 and 1100 < c.idct.highest <= 1303
    for q, lo in ((8, -652), (16, -1303)):
        assert per_file["d_quant_all_%d_gray" % q].idct.lowest == lo
    # every upsampling rule; replication at dw <= 2 for both subsamplings
    s = c.sample
    assert s.replicated and s.h2v1_fancy and s.h2v2_fancy and s.fullsize
    for size in ("2x1", "1x2", "3x1", "4x1"):
        for samp in ("422", "420"):
            ps = per_file["e_random_%s_%s_q30" % (size, samp)].sample
            assert ps.replicated == 2 and not ps.h2v1_fancy and not ps.h2v2_fancy, (size, samp)
    assert per_file["e_random_5x3_422_q30"].sample.h2v1_fancy == 2
    assert per_file["e_random_5x3_420_q30"].sample.h2v2_fancy == 2
    assert per_file["e_random_2049x1_444_q30"].sample.fullsize == 2
    # a file's own Huffman tables
    assert out["e_random_32x16_444_q100_opt"].header.huff[(1, 0)].bits != J.AC_LUM_BITS


def test_a_run_past_coefficient_63_is_corrupt():
    data = DI.run_past_63()
    assert DI.sof0_size(data) == (DI.HAND_W, DI.HAND_H)
    D.parse_header(data)
    with pytest.raises(D.Corrupt) as ei:
        D.decode(data)
    assert DI.CORRUPT_REASONS["run past 63"] in str(ei.value)
