"""tests/jpeg_progressive_reference.py against libjpeg-turbo's pixels of every progressive fixture
(tests/golden/jpeg_progressive/), bit for bit; its counters show which rules of jdphuff.c the family
reaches; the files the parser refuses and the scans that do not decode."""
import os

import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
import jpeg_progressive_inputs as PI
import jpeg_progressive_reference as P


@pytest.fixture(scope="module")
def family():
    """every file decoded once: {name: Decoded}, and the counters of them all"""
    cnt = P.Counters()
    return {n: P.decode(PI.file_bytes(n), cnt) for n in PI.names()}, cnt


def test_the_committed_files_are_the_family_and_within_the_size_the_fixtures_keep():
    names = PI.names()
    assert len(names) == len(set(names)) == 182
    on_disk = sorted(os.listdir(PI.GOLDEN))
    assert on_disk == sorted([n + ".jpg" for n in names] + [n + ".npz" for n in names])
    for f in on_disk:
        assert os.path.getsize(os.path.join(PI.GOLDEN, f)) < 32 * 1024, f
    # B and C are what the writer makes of committed bytes today
    for n, data in PI.derived_files().items():
        assert data == PI.file_bytes(n), n


def test_every_fixture_equals_libjpeg(family):
    decoded, _ = family
    for n in PI.names():                       # (no file left out)
        gray, bgr = PI.pixels(n)
        w, h = PI.size_of(n)
        assert gray.shape == (h, w) and bgr.shape == (h, w, 3), n
        assert np.array_equal(decoded[n].gray, gray), n
        assert np.array_equal(decoded[n].bgr, bgr), n


def test_same_coefficients_under_another_script(family):
    """B: the coefficients are the baseline fixture's, but for the padding blocks that a scan of one
    component does not code"""
    decoded, _ = family
    for n in PI.names():
        if not n.startswith("b_"):
            continue
        base = D.decode(DI.fixture_bytes(PI.b_base(n)))
        h = decoded[n].header
        assert h.progressive and (h.width, h.height) == (base.header.width, base.header.height)
        hmax, vmax = D.layout(h)[:2]
        for c, (got, want) in enumerate(zip(decoded[n].coefs, base.coefs)):
            ch, cv = (h.comps[c]["h"], h.comps[c]["v"]) if len(h.comps) > 1 else (1, 1)
            nx = -(-(-(-h.width * ch // hmax)) // 8)
            ny = -(-(-(-h.height * cv // vmax)) // 8)
            assert np.array_equal(got[:ny, :nx], want[:ny, :nx]), (n, c)
        assert np.array_equal(decoded[n].gray, base.gray) and np.array_equal(decoded[n].bgr, base.bgr), n


def test_the_large_files_coefficients(family):
    decoded, _ = family
    c = decoded["c_eobrun_32767_gray_2048x1024"].coefs[0]
    assert c.shape == (128, 256, 64) and (c[..., 0] == 5).all() and not c[..., 1:].any()
    c = decoded["c_eob_categories_gray_1024x1032"].coefs[0].reshape(-1, 64)
    assert (c[:, 0] == (np.arange(c.shape[0]) % 7) - 3).all()
    assert int((c[:, 1:] != 0).sum()) == 14 * 3 - 1


def test_the_family_reaches_every_rule(family):
    _, c = family
    assert all(c.scans[k] > 100 for k in P.KINDS), c.scans
    first, refine = c.eob_category["ac_first"], c.eob_category["ac_refine"]
    assert (first > 0).all(), first                       # categories 0..14 in first scans
    assert refine[0] > 0 and refine[1] > 0 and refine[5:].sum() > 0, refine
    assert c.max_eobrun == 32767
    assert c.corrected_positive > 1000 and c.corrected_negative > 1000
    assert c.correction_bits > c.corrected_positive + c.corrected_negative
    assert c.new_plus > 1000 and c.new_minus > 1000
    assert c.zrl_passing_nonzero > 10
    assert c.eobrun_blocks_with_nonzero > 10
    assert c.restarts > 1000 and c.restarts_clearing_predictor > 10
    assert c.non_interleaved_on_padded_plane > 10 and c.interleaved_dc > 10
    assert c.fill_bytes > 10 and c.stuffed > 10 and c.slow_codes > 10
    assert c.max_al == 13


def test_counters_of_single_files():
    """the rules one fixture each is there for"""
    c = P.Counters()
    d = P.decode(PI.file_bytes("c_eobrun_32767_gray_2048x1024"), c, pixels=False)
    assert [s.kind for s in d.header.scans] == ["dc_first", "ac_first"]
    assert list(np.nonzero(c.eob_category["ac_first"])[0]) == [0, 14] and c.max_eobrun == 32767
    c = P.Counters()
    P.decode(PI.file_bytes("c_eob_categories_gray_1024x1032"), c, pixels=False)
    assert (c.eob_category["ac_first"][:14] == 1).all() and (c.eob_category["ac_refine"][6:14] > 0).all()
    # 17 x 17 at 4:2:0: Y's interleaved DC scan codes 4 x 4 blocks, its AC scans 3 x 3
    h = P.parse(PI.file_bytes("b_dc_interleaved_420_17x17"))
    assert [(s.nx, s.ny) for s in h.scans] == [(2, 2), (3, 3), (2, 2), (2, 2)]
    h = P.parse(PI.file_bytes("b_dc_not_interleaved_420_17x17"))
    assert [(s.nx, s.ny) for s in h.scans[:3]] == [(3, 3), (2, 2), (2, 2)]
    # DRI 0 -> 2 -> 0 -> 2 between scans
    h = P.parse(PI.file_bytes("b_dri_changes_420_17x17"))
    assert [s.restart for s in h.scans] == [0, 2, 2, 0, 0, 2, 2, 2]
    # table ids 2 and 3, redefined between scans: the scans of one id hold different tables
    h = P.parse(PI.file_bytes("b_table_ids_2_3_444_17x17"))
    acs = [s.ac for s in h.scans if s.ac is not None]
    assert len(set(id(t) for t in acs)) == len(acs) == 6
    # a DQT behind the first scan is not the component's table
    h = P.parse(PI.file_bytes("b_dqt_redefined_420_17x17"))
    base = D.parse_header(DI.fixture_bytes(PI.b_base("b_dqt_redefined_420_17x17")))
    for ci, c0 in enumerate(base.comps):
        assert np.array_equal(h.qtables[ci], base.qtables[c0["tq"]])
    # Pillow's files: libjpeg-turbo's default script
    h = P.parse(PI.file_bytes("a_noise_17x17_420_q95"))
    assert [(len(s.comps), s.ss, s.se, s.ah, s.al) for s in h.scans] == [
        (3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1),
        (3, 0, 0, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]


def test_refusals_are_refused_with_their_word():
    for what, (data, word) in PI.refusals().items():
        with pytest.raises(P.Refused) as ei:
            P.parse(data)
        assert word in str(ei.value), (what, str(ei.value))
    # what the baseline restatement refuses, this one refuses in the same words
    for what, (data, word) in DI.refusals().items():
        with pytest.raises(P.Refused) as ei:
            P.parse(data)
        with pytest.raises(D.Refused) as e0:
            D.parse_header(data)
        assert str(ei.value) == str(e0.value), what
    for what, (data, same_as) in PI.accepted_extras().items():
        d = P.decode(data)
        assert np.array_equal(d.bgr, PI.pixels(same_as)[1]), what


@pytest.mark.parametrize("what", sorted(PI.CORRUPT_REASONS))
def test_corrupt_scans_are_accepted_by_the_parser_and_stop_the_walk(what):
    data = PI.corrupt_scans()[what]
    h = P.parse(data)
    assert (h.width, h.height, h.channels) == (17, 17, 3)
    with pytest.raises(P.Corrupt) as ei:
        P.decode(data)
    assert PI.CORRUPT_REASONS[what][1] in str(ei.value)
