"""tests/jpeg_reference.py against libjpeg: the restatement's bytes equal every committed file
Pillow (libjpeg-turbo) wrote for tests/jpeg_inputs.py -- every case, both colour modes, all four
qualities -- its decoder reads every file back, and every input reaches the branch it was made for.
No GPU, no library of the project."""
import io
import os

import numpy as np
import pytest

import jpeg_inputs as I
import jpeg_reference as J

CASES = I.cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def encoded():
    """(case name, quality) -> Encoded, computed once"""
    cache = {}

    def get(case, q):
        key = (case.name, q)
        if key not in cache:
            cache[key] = J.encode_full(case.image(), q)
        return cache[key]
    return get


def test_the_list_covers_every_size_mode_and_content():
    seen = {(c.width, c.height, c.channels) for c in CASES}
    assert seen == {(w, h, ch) for (w, h) in I.SIZES for ch in (1, 3)}
    for size in I.CONTENT_SIZES:
        for ch in (1, 3):
            assert {c.content for c in CASES if (c.width, c.height) == size and c.channels == ch} == set(I.CONTENTS)
    assert len(set(IDS)) == len(IDS)
    # nothing under golden/jpeg that the list does not name, nothing missing
    want = {os.path.basename(I.golden_npz(c)) for c in CASES} | \
        {os.path.basename(I.golden_jpg(c, q)) for c in CASES for q in I.QUALITIES}
    assert set(os.listdir(I.GOLDEN)) == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_equal_their_fixtures(case):
    img = np.load(I.golden_npz(case))["image"]
    assert img.dtype == np.uint8 and np.array_equal(img, case.image())
    assert os.path.getsize(I.golden_npz(case)) < 64 * 1024


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_libjpeg_bytes(case, encoded):
    for q in I.QUALITIES:
        want = open(I.golden_jpg(case, q), "rb").read()
        assert len(want) < 64 * 1024
        got = encoded(case, q).data
        if got != want:
            # locate it: by segment, then by block and coefficient
            d = J.decode(want)
            mine = encoded(case, q).blocks.coef
            bad = np.argwhere(d.coef != mine)
            raise AssertionError("%s q%d: %d vs %d bytes, first byte %s, first (block, coefficient) %s"
                                 % (case, q, len(got), len(want),
                                    next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None),
                                    bad[0].tolist() if len(bad) else None))


def _pillow_jpeg(image, quality):
    from PIL import Image
    f = io.BytesIO()
    im = Image.fromarray(image if image.ndim == 2 else np.ascontiguousarray(image[..., ::-1]))
    im.save(f, "JPEG", quality=quality, subsampling=2, optimize=False)
    return f.getvalue()


def test_fixtures_are_what_pillow_writes_here_and_the_large_scan_case():
    pytest.importorskip("PIL.Image")
    for case in CASES:
        img = case.image()
        for q in I.QUALITIES:
            assert _pillow_jpeg(img, q) == open(I.golden_jpg(case, q), "rb").read(), (case, q)
    big = I.large_case()
    img = big.image()
    assert (big.width + 7) // 8 * ((big.height + 7) // 8) > 64 * 256
    assert J.encode(img, 95) == _pillow_jpeg(img, 95)


def _error_bound(qtable):
    """|decoded sample - input sample| <= sum over the 64 basis functions of |basis| times the
    coefficient's error: half a quantisation step, plus 0.5 for the integer DCT (jfdctint keeps 3
    extra bits and rounds twice: well under half a unit of the unscaled coefficient), plus the
    decoder's own clamp-free float arithmetic (nothing)."""
    m = np.abs(J._idct_matrix())                       # (frequency, sample)
    step = qtable.reshape(8, 8) / 2.0 + 0.5
    return np.einsum("ur,uv,vc->rc", m, step, m)       # per position in the block


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decoder_reads_every_file_back(case):
    img = case.image()
    planes = J.component_planes(img)
    for q in I.QUALITIES:
        d = J.decode(open(I.golden_jpg(case, q), "rb").read())
        assert (d.width, d.height, len(d.comps)) == (case.width, case.height, case.channels)
        ref = J.blocks_of(img, q)
        assert np.array_equal(d.coef, ref.coef) and np.array_equal(d.comp, ref.comp)
        tables = J.quant_tables(q)
        for ci, (plane, t) in enumerate(planes):
            assert np.array_equal(d.qtables[d.comps[ci]["tq"]], tables[t])
            got = d.planes[ci][:plane.shape[0], :plane.shape[1]]
            bound = np.tile(_error_bound(tables[t]), (plane.shape[0] // 8, plane.shape[1] // 8))
            err = np.abs(got - plane)
            assert np.all(err <= bound), (case, q, ci, float((err - bound).max()))
        if case.channels == 1:
            assert d.pixels.shape == img.shape


def test_every_input_reaches_its_branch(encoded):
    by = {c.name: c for c in CASES}
    for ch in ("gray", "bgr"):
        for size in ("17x17", "129x47"):
            for content in ("zero", "full", "mid"):     # all-EOB blocks, DC difference 0 after the first
                for q in I.QUALITIES:
                    e = encoded(by["%s_%s_%s" % (content, size, ch)], q)
                    assert e.tokens.eob == e.blocks.coef.shape[0] and e.tokens.max_dc_cat <= 11
                    assert not e.blocks.coef[:, 1:].any()
                    comp0 = e.blocks.coef[e.blocks.comp == 0, 0]
                    assert np.all(np.diff(comp0) == 0)
            # category 11
            assert encoded(by["checker_%s_%s" % (size, ch)], 100).tokens.max_dc_cat == 11
            # ZRL: a zero run >= 16
            for q in (50, 1):
                assert encoded(by["lone_hf_%s_%s" % (size, ch)], q).tokens.zrl > 0
            # long codes: a value has at most 10 bits, so 25 bits need a 15- or 16-bit code
            e = encoded(by["noise_%s_%s" % (size, ch)], 100)
            assert e.tokens.length[:, 1:64].max() >= 25
            # stuffing: adjacent 0xFF bytes, one at the end of a lane's bytes, one at the end of a chunk
            raw = encoded(by["stuffed_%s_%s" % (size, ch)], 100).raw_scan
            ff = np.nonzero(raw == 0xFF)[0]
            assert len(ff) >= 1 and np.any(np.diff(ff) == 1)
            assert np.any(ff % I.STUFF_LANE_BYTES == I.STUFF_LANE_BYTES - 1)
            if size == "129x47":
                assert len(raw) > I.STUFF_CHUNK_BYTES
                assert np.any(ff % I.STUFF_CHUNK_BYTES == I.STUFF_CHUNK_BYTES - 1)
        # dummy blocks: in both directions at 17 x 17 (colour only: a gray scan has none)
        e = encoded(by["noise_17x17_%s" % ch], 95)
        assert int(e.blocks.dummy.sum()) == (7 if ch == "bgr" else 0)
        if ch == "bgr":
            d = e.blocks.dummy.reshape(2, 2, 6)
            assert d[0, 1, 1] and d[0, 1, 3] and d[1, 0, 2] and d[1, 0, 3] and d[1, 1, 1:4].all()
    # the 255 clamp of the tables at quality 1, and only there
    assert J.quant_clamped_entries(1) > 0 and J.quant_tables(1)[0].max() == 255
    assert all(J.quant_clamped_entries(q) == 0 for q in (95, 100, 50))
    assert J.quant_tables(100)[0].max() == 1    # (and the clamp to 1 at quality 100)
