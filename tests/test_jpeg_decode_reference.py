"""CPU: tests/jpeg_decode_reference.py (the yardstick of the GPU JPEG decoder) against libjpeg's own
pixels: the .npz beside every fixture of tests/golden/jpeg_decode/ (what libjpeg-turbo decoded when
the fixtures were written), Pillow directly on the 576 files of tests/golden/jpeg/ where Pillow is
present, and tests/jpeg_reference.py's coefficients.  And that the fixtures reach every branch."""
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
