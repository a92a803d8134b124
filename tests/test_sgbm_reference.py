"""CPU: hand-computed known-answer tests of tests/sgbm_reference.py (the yardstick of the GPU
matcher), one per rule, and one property: a texture and its copy shifted by k pixels."""
import numpy as np

import sgbm_reference as R


def test_truncating_division():
    assert R.tdiv(-48, 32) == -1 and R.tdiv(48, 32) == 1 and R.tdiv(-3, 2) == -1 and R.tdiv(3, -2) == -1


def test_derived_parameters():
    q = R.derived(R.Params(), 640)
    assert (q["P1"], q["P2"], q["ftzero"], q["disp12"]) == (120, 250, 35, 1)
    assert (q["minX1"], q["maxX1"], q["invalid"]) == (81, 640, 0)
    q = R.derived(R.Params(p1=0, p2=0, pre_filter_cap=4, disp_12_max_diff=-1, min_disparity=-3), 100)
    assert (q["P1"], q["P2"], q["ftzero"], q["disp12"]) == (2, 5, 15, 1)
    assert (q["minX1"], q["maxX1"], q["invalid"]) == (77, 97, -64)


def test_recurrence_subtracts_minlr_plus_p2_from_c_plus_p2():
    # one row (one chain), four disparities, P1 = 3, P2 = 10; previous Lr = [4, 1, 9, 30], minLr = 1
    C = np.array([[10, 3, 7, 20]])
    Lp = np.array([[4, 1, 9, 30]])
    L, m = R.lr_step(C, Lp, np.array([1]), 3, 10)
    # stored C + P2 = [20, 13, 17, 30], delta = minLr + P2 = 11
    # d0: min(4, inf, 1+3, 11) = 4  -> 20 + 4 - 11 = 13
    # d1: min(1, 4+3, 9+3, 11) = 1  -> 13 + 1 - 11 = 3
    # d2: min(9, 1+3, 30+3, 11) = 4 -> 17 + 4 - 11 = 10
    # d3: min(30, 9+3, inf, 11) = 11 -> 30 + 11 - 11 = 30  (= C + P2, the top of [C, C + P2])
    assert L.tolist() == [[13, 3, 10, 30]] and m.tolist() == [3]
    # from the zeroed border: Lr = C
    L0, m0 = R.lr_step(C, np.zeros((1, 4), np.int64), np.zeros(1, np.int64), 3, 10)
    assert L0.tolist() == C.tolist() and m0.tolist() == [3]


def _one_pixel(S16, minD=1, uniq=10):
    """select() on a single matchable column: D = 16, width = minX1 + 1."""
    p = R.Params(min_disparity=minD, num_disparities=16, uniqueness_ratio=uniq)
    W = max(minD + 16, 0) + 1
    S = np.array(S16, np.int64).reshape(1, 1, 16)
    return R.select(S, p, W)[0, W - 1]


def _costs(**at):
    s = [1000] * 16
    for k, v in at.items():
        s[int(k[1:])] = v
    return s


def test_subpixel_truncates_toward_zero():
    # best d = 5 (S = 90); den = S4 + S6 - 2 S5 = 16
    # (100 - 96) * 16 + 16 = 80, / 32 = 2.5 -> 2: 5 * 16 + 2, plus 16 * minD
    assert _one_pixel(_costs(d4=100, d5=90, d6=96)) == 82 + 16
    # (96 - 100) * 16 + 16 = -48, / 32 = -1.5 -> -1 (floor would give -2): 5 * 16 - 1
    assert _one_pixel(_costs(d4=96, d5=90, d6=100)) == 79 + 16
    assert _one_pixel(_costs(d4=96, d5=90, d6=100), minD=0) == 79
    # d = 0 and d = D-1: no interpolation
    assert _one_pixel(_costs(d0=50), minD=2) == 0 * 16 + 32
    assert _one_pixel(_costs(d15=50)) == 15 * 16 + 16


def test_uniqueness_rejects_only_beyond_the_neighbours():
    # S[d] * (100 - 10) < minS * 100  with |d - best| > 1  rejects
    # |d - best| = 1 never rejects: 91 * 90 < 9000, yet kept (den 911, (909*16 + 911) / 1822 = 8)
    assert _one_pixel(_costs(d5=90, d6=91)) == 5 * 16 + 8 + 16
    assert _one_pixel(_costs(d5=90, d8=99)) == 0              # 99 * 90 = 8910 < 9000: invalid (minD 1 -> 0)
    assert _one_pixel(_costs(d5=90, d3=99)) == 0              # (on either side)
    assert _one_pixel(_costs(d5=90, d8=100)) == 96            # 9000 < 9000 is false: kept
    assert _one_pixel(_costs(d5=90, d8=99), uniq=0) == 96     # uniqueness 0: never rejects
    # every S saturated (int16): bestDisp stays -1 in OpenCV -> invalid, also with uniqueness 0
    assert _one_pixel([40000] * 16) == 0 and _one_pixel([32767] * 16, uniq=0) == 0


def test_left_right_check_and_the_disp2_start_value():
    W = 12
    d1 = np.full((1, W), 0, np.int64)
    d1[0, 10] = 5 * 16                      # integer disparity 5: both roundings look at x = 5
    # min_disparity = 1: disp2 starts at (1 - 1) * 16 = 0, which fails disp2 >= minD -> kept
    d2 = np.zeros((1, W), np.int64)
    assert R.lr_check(d1, d2, 1, 1, 0)[0, 10] == 80
    # min_disparity = 2: the start value 16 passes >= 2 and differs from 5 by 11 > 1 -> invalid
    d1b = d1.copy()
    d1b[0, :10] = 16
    assert R.lr_check(d1b, np.full((1, W), 16, np.int64), 2, 1, 16)[0, 10] == 16
    # a written, consistent entry keeps it; an inconsistent one removes it
    d2[0, 5] = 6
    assert R.lr_check(d1, d2, 1, 1, 0)[0, 10] == 80       # |6 - 5| = 1 <= 1
    d2[0, 5] = 7
    assert R.lr_check(d1, d2, 1, 1, 0)[0, 10] == 0        # |7 - 5| = 2 > 1
    # fractional 5.1875: floor 5 (x = 5) and ceil 6 (x = 4); one consistent neighbour suffices
    d1[0, 10] = 83
    d2[0, 4] = 6
    assert R.lr_check(d1, d2, 1, 1, 0)[0, 10] == 83
    d2[0, 4] = 9
    assert R.lr_check(d1, d2, 1, 1, 0)[0, 10] == 0


def test_speckle_window_size_is_inclusive():
    a = np.zeros((8, 8), np.int64)
    a[1, 1:5] = 100                         # 4 pixels
    a[5, 1:6] = 300                         # 5 pixels
    a[6, 1] = 317                           # joins the 5 (|317 - 300| <= 17) -> 6
    out = R.filter_speckles(a, 0, 4, 16)
    assert (out[1, 1:5] == 0).all()          # exactly speckle_window_size: removed
    assert (out[5, 1:6] == 300).all()        # beyond it: kept
    assert out[6, 1] == 0                    # |317 - 300| = 17 > 16: its own region of 1
    out = R.filter_speckles(a, 0, 3, 16)
    assert (out[1, 1:5] == 100).all()        # window + 1 pixels: kept


def test_box_sum_borders():
    p = R.Params(block_size=3)               # SW2 = SH2 = 1
    pix = np.zeros((6, 5, 1), np.int64)
    pix[0, 0, 0] = 1
    C = R.block_cost(pix, p, 5)[..., 0]
    assert C[0, 0] == 4 and C[0, 1] == 2 and C[1, 0] == 2 and C[1, 1] == 1 and C[2, 2] == 0
    pix[:] = 0
    pix[2, 4, 0] = 1                         # right border: replicated
    C = R.block_cost(pix, p, 5)[..., 0]
    assert C[2, 4] == 2 and C[2, 3] == 1 and C[2, 2] == 0
    pix[:] = 0
    pix[5, 2, 0] = 1                         # bottom: row 5 keeps row 4's block cost (hold = H-1-SH2)
    C = R.block_cost(pix, p, 5)[..., 0]
    assert C[4, 2] == 1 and C[5, 2] == 1     # (a replicated box would give 2 in row 5)


def test_median_replicates_borders():
    a = np.arange(12).reshape(3, 4) * 10
    m = R.median3(a)
    assert m[0, 0] == 10 and m[1, 1] == 50 and m[2, 3] == 100


def test_shifted_texture_gives_the_shift():
    rng = np.random.default_rng(3)
    H, W, k = 48, 112, 13
    tex = rng.integers(0, 256, (H, W + k)).astype(np.uint8)
    disp, raw = R.restate(tex[:, :W], tex[:, k:W + k], R.Params(num_disparities=32))
    inner = raw[5:-5, 40:-5].astype(np.int64)
    assert np.abs(inner - 16 * k).max() <= 8
    assert disp.dtype == np.float32 and disp[20, 60] == raw[20, 60] / 16.0


def test_mask_sets_max_invalid_disparity():
    rng = np.random.default_rng(4)
    tex = rng.integers(0, 256, (30, 80)).astype(np.uint8)
    mask = np.zeros((30, 60), np.uint8)
    mask[:, 45:] = 255
    disp, raw = R.restate(tex[:, :60], tex[:, 7:67], R.Params(num_disparities=16), mask)
    assert (disp[:, :45] == 1.0).all() and (disp[:, 45:] == raw[:, 45:] / np.float32(16)).all()
