"""CPU: hand-computed known answers for tests/bm_reference.py, one per rule of its reading of
OpenCV's StereoBM (the yardstick the GPU block matcher is held to)."""
import numpy as np
import pytest

import bm_reference as B
from sgbm_reference import tdiv


def P(**kw):
    return B.Params().replace(**kw)


def test_effective_parameters_are_the_wrappers_setters():
    e = B.effective(P(pre_filter_cap=31, pre_filter_size=9, disp_12_max_diff=3))
    assert e["preFilterCap"] == 9 and e["disp12MaxDiff"] == -1 and e["preFilterSize"] == 9
    assert e["preFilterType"] == "XSOBEL"
    assert B.effective(P(pre_filter_size=40))["preFilterCap"] == 40
    # pre_filter_cap and disp_12_max_diff change nothing
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (40, 120)).astype(np.uint8)
    b = np.roll(a, -5, axis=1)
    base = B.restate(a, b, P(num_disparities=16, block_size=5))[1]
    assert np.array_equal(base, B.restate(a, b, P(num_disparities=16, block_size=5, pre_filter_cap=63,
                                                   disp_12_max_diff=2))[1])


def test_xsobel_table_and_border_columns():
    img = np.zeros((4, 5), np.uint8)
    img[:, 3:] = 2      # x-gradient 2 at columns 2, 3 in each row: 2 + 2 * 2 + 2 = 8
    out = B.prefilter_xsobel(img, 3)
    assert (out[:, 0] == 3).all() and (out[:, -1] == 3).all()
    assert out[0].tolist() == [3, 3, 6, 6, 3]     # clamp(8, -3, 3) + 3 = 6; clamp(0) + 3 = 3
    img[:, 3:] = 0
    img[:, :2] = 1      # a falling edge: -(1 + 2 + 1) = -4 -> clamp to -3 -> 0
    assert B.prefilter_xsobel(img, 3)[1].tolist() == [3, 0, 0, 3, 3]
    img2 = np.zeros((2, 4), np.uint8)
    img2[:, 2:] = 1     # sum 4 <= cap 10 -> 14
    assert B.prefilter_xsobel(img2, 10)[0].tolist() == [10, 14, 14, 10]


def test_row_zero_reflected_and_odd_last_row_is_cap():
    img = np.zeros((3, 3), np.uint8)
    img[1, 2] = 10      # only row 1 has a gradient at column 1: d = 10
    out = B.prefilter_xsobel(img, 63)
    assert out[0, 1] == 63 + 10 + 2 * 0 + 10   # row 0: upper neighbour = row 1 (reflected) + lower row 1
    assert out[1, 1] == 63 + 2 * 10             # row 1: its own row, twice
    assert (out[2] == 63).all()                 # odd H: the pair loop stops short, the row is cap
    img4 = np.zeros((4, 3), np.uint8)
    img4[2, 2] = 10
    out4 = B.prefilter_xsobel(img4, 63)
    assert out4[3, 1] == 63 + 10 + 0 + 10       # even H: row 3's lower neighbour is row 2
    assert (B.prefilter_xsobel(np.full((1, 8), 7, np.uint8), 5) == 5).all()


def test_left_and_right_columns_clamp_independently():
    # minD = -8, D = 16: lofs = 7, rofs = 0, width1 = W - 15; the right base column clamps to
    # [0, W - D] before + d while the left column stays unclamped inside the region
    p = P(min_disparity=-8, num_disparities=16, block_size=5)
    W, H = 40, 9
    lofs, rofs, width1, reg = B.geometry(p, W, H)
    assert (lofs, rofs, width1) == (7, 0, 25)
    assert reg == (9, 32, 2, 7)     # xa = maxD + SW2 = 9, xb = min(W - SW2, W + minD) = 32
    rng = np.random.default_rng(3)
    lf = rng.integers(0, 19, (H, W)).astype(np.int64)
    rf = rng.integers(0, 19, (H, W)).astype(np.int64)
    sad, _ = B.sad_volume(lf, rf, p)
    X, y, d = 31, 4, 3
    want = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            lc = min(max(X + dx, 0), W - 1)
            rc = min(max(X + dx - lofs + rofs, 0), W - 16) + d
            want += abs(lf[y + dy, lc] - rf[y + dy, rc])
    assert sad[y - 2, X - 9, d] == want
    # the clamp binds here: X + dx - lofs reaches 26 > W - D = 24
    unclamped = sum(abs(lf[y + dy, X + dx] - rf[y + dy, X + dx - lofs + d])
                    for dy in range(-2, 3) for dx in range(-2, 3))
    assert unclamped != want


def _sel(sads, **kw):
    """select() on a single pixel with these SADs."""
    p = P(num_disparities=len(sads), **kw)
    sad = np.asarray(sads, np.int64)[None, None, :]
    tex = np.full((1, 1), kw.get("texture_threshold", 20), np.int64)
    return int(B.select(sad, tex, p)[0, 0])


def test_texture_comes_before_uniqueness():
    p = P(num_disparities=16, texture_threshold=50, uniqueness_ratio=0)
    sad = np.arange(16, dtype=np.int64)[::-1].copy()[None, None, :]
    assert B.select(sad, np.array([[49]]), p)[0, 0] == B.filtered_value(p)
    assert B.select(sad, np.array([[50]]), p)[0, 0] != B.filtered_value(p)
    # a pixel both textureless and ambiguous is filtered either way (the texture test short-cuts)
    flat = np.full((1, 1, 16), 7, np.int64)
    assert B.select(flat, np.array([[0]]), P(num_disparities=16, texture_threshold=1))[0, 0] == 0


def test_uniqueness_ignores_neighbours_uses_le_and_zero_disables():
    s = [100] * 16
    s[5], s[4], s[3] = 10, 10, 11       # mind = 4 (first of the minimum); d = 5, 3 are neighbours
    assert _sel(s, uniqueness_ratio=80) != 0
    s2 = list(s)
    s2[12] = 18                          # thresh = 10 + 10 * 80 / 100 = 18: <= filters
    assert _sel(s2, uniqueness_ratio=80) == 0
    s2[12] = 19
    assert _sel(s2, uniqueness_ratio=80) != 0
    s3 = list(s)
    s3[12] = 10                          # an equal far minimum: filtered with any ratio > 0 ...
    assert _sel(s3, uniqueness_ratio=1) == 0
    assert _sel(s3, uniqueness_ratio=0) != 0   # ... and ratio 0 turns the test off
    assert tdiv(-7, 2) == -3


def test_subpixel_formula():
    D, minD = 16, 1
    s = [200] * D
    s[6], s[5], s[7] = 10, 40, 20        # mind 6: p = sad[7] = 20, n = sad[5] = 40
    den = 20 + 40 - 20 + 20
    sub = -((20 * 256) // den)           # (p - n) * 256 / den = -5120 / 60 -> -85 (truncated)
    assert sub == -86 + 1
    want = ((D - 6 - 1 + minD) * 256 + sub + 15) >> 4
    assert _sel(s, uniqueness_ratio=0) == want == (10 * 256 - 85 + 15) >> 4 == 155
    # mind at 0: sad[-1] := sad[1], p = n -> no subpixel shift, disparity D - 1 + minD
    s0 = [200] * D
    s0[0], s0[1] = 3, 9
    assert _sel(s0, uniqueness_ratio=0) == ((D - 1 + minD) * 256 + 15) >> 4 == 16 * 16
    # mind at D - 1: sad[D] := sad[D-2], disparity minD
    s1 = [200] * D
    s1[D - 1], s1[D - 2] = 3, 9
    assert _sel(s1, uniqueness_ratio=0) == (minD * 256 + 15) >> 4 == 16
    # arithmetic shift of a negative value (minD = -3, mind = D - 1, p > n -> negative sub)
    s2 = [200] * D
    s2[D - 1], s2[D - 2] = 0, 1
    p2 = P(num_disparities=D, min_disparity=-3, uniqueness_ratio=0)
    got = int(B.select(np.asarray(s2, np.int64)[None, None, :], np.array([[99]]), p2)[0, 0])
    assert got == (-3 * 256 + 15) >> 4 == -48
    s4 = [200] * D
    s4[D - 3], s4[D - 2], s4[D - 4] = 0, 3, 1   # mind = D-3, p = 3, n = 1: den = 4 + 2 = 6
    got = int(B.select(np.asarray(s4, np.int64)[None, None, :], np.array([[99]]), p2)[0, 0])
    assert got == ((2 - 3) * 256 + 85 + 15) >> 4 == -10   # -156 >> 4 floors to -10
    # within half a pixel of the integer disparity for any SADs
    rng = np.random.default_rng(1)
    for _ in range(200):
        sr = rng.integers(0, 1000, D).tolist()
        mind = int(np.argmin(sr))
        v = _sel(sr, uniqueness_ratio=0)
        assert abs(v - (D - mind - 1 + minD) * 16) <= 8


def test_ties_go_to_the_largest_disparity():
    s = [50] * 16
    s[3] = s[9] = 5
    # the first index of the minimum is 3, i.e. disparity D - 1 - 3 + minD = 13 (not 7)
    assert _sel(s, uniqueness_ratio=0) >> 4 == 13


def test_valid_rectangle_borders_and_degenerate_widths():
    p = P()                          # minD 1, D 80, block 15
    assert B.geometry(p, 200, 100)[3] == (87, 193, 7, 93)
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (30, 120)).astype(np.uint8)
    raw = B.raw_map(a, np.roll(a, -10, 1), P(block_size=5, uniqueness_ratio=0, texture_threshold=0))
    assert (raw[:, :82] == 0).all() and (raw[:, 118:] == 0).all()
    assert (raw[:2] == 0).all() and (raw[28:] == 0).all()
    assert (raw[2:28, 82:118] != 0).all()
    # width1 < 1 / lofs >= W, and an empty valid rectangle: all FILTERED
    assert B.geometry(p, 60, 40)[3] is None       # width1 = 60 - 80 + 1 < 1
    assert B.geometry(p, 80, 40)[3] is None       # lofs = 80 >= W
    assert B.geometry(p, 94, 40)[3] is None       # xa = 87 = xb = 94 - 7
    assert B.geometry(p, 95, 40)[3] == (87, 88, 7, 33)
    assert B.geometry(p, 200, 14)[3] is None      # rows: ya = 7 = yb = 14 - 7
    b = rng.integers(0, 256, (40, 94)).astype(np.uint8)
    assert (B.restate(b, b)[1] == 0).all()
    q = P(min_disparity=-100, num_disparities=16)  # rofs = 85 >= W = 60
    assert B.geometry(q, 60, 40)[3] is None
    assert (B.restate(b[:, :60], b[:, :60], q)[1] == (-101 * 16)).all()


def test_speckle_range_unscaled_and_switches():
    a = np.zeros((6, 8), np.int64)
    a[1:4, 1:4] = 100                  # a 9-pixel region of 100
    a[2, 2] = 104                      # differs by 4 (1/16 pixel units) from its neighbours
    from sgbm_reference import filter_speckles
    out = filter_speckles(a, 0, 5, 4)  # range 4 unscaled: one 9-pixel region, kept (> 5)
    assert (out == a).all()
    out = filter_speckles(a, 0, 5, 3)  # range 3: the 104 pixel is its own speckle
    assert out[2, 2] == 0 and out[1, 1] == 100
    rng = np.random.default_rng(5)
    L = rng.integers(0, 256, (40, 140)).astype(np.uint8)
    R = np.roll(L, -6, 1)
    kw = dict(num_disparities=16, block_size=5, uniqueness_ratio=0, texture_threshold=0)
    raw_nof = B.raw_map(L, R, P(**kw)).astype(np.int16)
    for off in (dict(speckle_range=-1), dict(speckle_window_size=0)):
        assert np.array_equal(B.restate(L, R, P(**kw, **off))[1], raw_nof)
    # range r is compared with the 1/16-pixel values as is (SGBM would use 16 r)
    got = B.restate(L, R, P(**kw, speckle_range=3, speckle_window_size=100))[1]
    want = filter_speckles(raw_nof.astype(np.int64), 0, 100, 3).astype(np.int16)
    assert np.array_equal(got, want)



def test_restate_passes_speckle_range_unscaled(monkeypatch):
    crafted = np.zeros((6, 8), np.int64)
    crafted[1:4, 1:4] = 100
    crafted[2, 2] = 104
    monkeypatch.setattr(B, "raw_map", lambda l, r, p: crafted.copy())
    img = np.zeros((6, 8), np.uint8)
    kw = dict(speckle_window_size=5, num_disparities=16, block_size=5)
    assert B.restate(img, img, P(speckle_range=4, **kw))[1][2, 2] == 104   # one region of 9: kept
    assert B.restate(img, img, P(speckle_range=3, **kw))[1][2, 2] == 0     # (16 * 3 would keep it)
    assert B.restate(img, img, P(speckle_range=-1, **kw))[1][2, 2] == 104  # off


def test_mask_gives_max_invalid_disparity():
    rng = np.random.default_rng(6)
    L = rng.integers(0, 256, (30, 120)).astype(np.uint8)
    mask = np.full(L.shape, 255, np.uint8)
    mask[:, 90:] = 0
    f, raw = B.restate(L, np.roll(L, -4, 1), P(num_disparities=16, block_size=5), mask)
    assert (f[mask == 0] == 1.0).all()
    assert np.array_equal(f[mask != 0], raw[mask != 0].astype(np.float32) / np.float32(16))


@pytest.mark.parametrize("k", [3, 11])
def test_shifted_texture_gives_the_shift(k):
    rng = np.random.default_rng(7)
    W, H = 160, 60
    tex = rng.integers(0, 256, (H, W + k)).astype(np.uint8)
    f, raw = B.restate(tex[:, :W], tex[:, k:], P(num_disparities=16, block_size=9))
    reg = B.geometry(P(num_disparities=16, block_size=9), W, H)[3]
    xa, xb, ya, yb = reg
    inner = raw[ya:yb, xa:xb]
    assert (inner != 0).mean() > 0.9
    assert (np.abs(inner[inner != 0] - 16 * k) <= 8).all()
