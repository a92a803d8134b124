"""CPU: the input families of tests/stereo_inputs.py reach what they claim.  For every family the
restatement ALONE (tests/sgbm_reference.py, tests/bm_reference.py) must show the condition the
family exists for -- ties, saturation, speckle removals, left-right failures -- and every case of
the CASES table must run through its restatement and leave more than its floor of pixels valid (or
be marked all-invalid and be exactly that), so that the GPU comparison of
tests/test_gpu_stereo_inputs.py is never one of empty or trivial maps.  These are conditions, not
measurements; the measured values are in the comments and leave room."""
import numpy as np
import pytest

import bm_reference as B
import sgbm_reference as R
import stereo_inputs as SI

BY_ID = {c.id: c for c in SI.CASES}


def sgbm_S(case):
    """OpenCV's int16 S of a case: pixel_cost -> block_cost -> aggregate, saturated."""
    left, right = case.images()
    p = case.params()
    q = R.derived(p, left.shape[1])
    C = R.block_cost(R.pixel_cost(left, right, p), p, left.shape[1])
    return np.minimum(R.aggregate(C, q["P1"], q["P2"]), R.SHRT_MAX)


def bm_sad(case):
    left, right = case.images()
    p = case.params()
    cap = p.pre_filter_size
    return B.sad_volume(B.prefilter_xsobel(left, cap), B.prefilter_xsobel(right, cap), p)[0]


def tie_share(vol):
    """share of pixels whose minimum over d is attained at more than one d"""
    return ((vol == vol.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean()


def valid_share(case, raw):
    return (raw != case.invalid()).mean()


# ---- ties ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat0", "flat128", "flat255"])
def test_flat_ties_at_nearly_every_pixel(name):
    assert tie_share(sgbm_S(BY_ID["sgbm-%s-defaults" % name])) >= 0.9      # measured 1.0
    assert tie_share(bm_sad(BY_ID["bm-%s-provoking" % name])) >= 0.9        # measured 1.0


@pytest.mark.parametrize("name", ["stripes8", "stripes16", "checker1"])
def test_periodic_patterns_tie_a_period_apart(name):
    S = sgbm_S(BY_ID["sgbm-%s-defaults" % name])
    assert tie_share(S) >= 0.9                                              # measured 1.0
    sad = bm_sad(BY_ID["bm-%s-provoking" % name])
    assert tie_share(sad) >= 0.9                                            # measured 1.0
    if name == "checker1":
        return   # (one-pixel squares have no x-Sobel response at all: every d ties, as on flat)
    period = dict(stripes8=8, stripes16=16)[name]
    # the tied minima lie `period` apart: the first two indices of the minimum differ by it
    m = sad == sad.min(axis=2, keepdims=True)
    first = m.argmax(axis=2)
    m2 = m.copy()
    np.put_along_axis(m2, first[..., None], False, 2)
    assert (np.median(m2.argmax(axis=2) - first) == period)


# ---- saturation --------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["sgbm-noise-provoking", "sgbm-noise_binary-provoking",
                                 "sgbm-half-provoking", "sgbm-noise-saturated_uniq0",
                                 "sgbm-noise_binary-saturated_uniq0"])
def test_large_p2_saturates_S_and_leaves_valid_pixels(cid):
    case = BY_ID[cid]
    sat = sgbm_S(case) >= R.SHRT_MAX
    # measured: 86 % / 88 % / 90 % of S at the ceiling; 46 / 235 / 22 pixels with every S there;
    # 25 % / 27 % / 52 % of the map valid
    assert sat.mean() >= 0.3
    assert sat.all(axis=2).sum() >= 10
    assert valid_share(case, case.restate()[1]) >= 0.1


@pytest.mark.parametrize("cid", ["sgbm-noise-saturated_uniq0", "sgbm-noise_binary-saturated_uniq0"])
def test_only_the_ceiling_rule_rejects_a_fully_saturated_pixel_at_ratio_0(cid):
    """With uniqueness_ratio = 0 the uniqueness loop rejects nothing, so `minS >= SHRT_MAX` alone makes
    these pixels invalid: select() without that rule would leave them valid at d = 0."""
    case = BY_ID[cid]
    p = case.params()
    assert R.derived(p, case.W)["uniq"] == 0
    S = sgbm_S(case)
    allsat = (S >= R.SHRT_MAX).all(axis=2)
    assert allsat.sum() >= 10                                  # measured 46 / 235
    bad = (S * 100 < S.min(axis=2, keepdims=True) * 100).any(axis=2)
    assert not bad[allsat].any()


def test_default_penalties_do_not_saturate():
    """(what the provoking sets add: under the defaults no S of these inputs reaches the ceiling)"""
    assert not (sgbm_S(BY_ID["sgbm-half-defaults"]) >= R.SHRT_MAX).any()


# ---- the speckle filter ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["sgbm-patches-provoking", "bm-patches-provoking",
                                 "bm-patches_flat-provoking"])
def test_patches_lose_some_regions_to_the_speckle_filter_and_keep_others(cid):
    case = BY_ID[cid]
    M = R if case.matcher == "sgbm" else B
    left, right = case.images()
    p = case.params()
    assert p.speckle_window_size == 100   # the default
    off = M.restate(left, right, p.replace(speckle_window_size=0))[1]
    on = M.restate(left, right, p)[1]
    assert (off != on).sum() >= 50         # measured 248 / 664 / 79
    inv = case.invalid()
    removed = survived = 0
    for y, x, h, w, d in SI.patch_layout(case.H, case.W, case.fkw.get("sizes", SI.PATCH_SIZES)):
        cy, cx = y + h // 2, x + w // 2
        if off[cy, cx] != inv:
            removed += on[cy, cx] == inv
            survived += on[cy, cx] != inv
    assert removed >= 1 and survived >= 1, (removed, survived)


# ---- the left-right check ------------------------------------------------------------------------
def test_occluder_fails_the_left_right_check():
    case = BY_ID["sgbm-occluder-defaults"]
    left, right = case.images()
    p = case.params()
    a = R.restate(left, right, p.replace(disp_12_max_diff=1))[1]
    b = R.restate(left, right, p.replace(disp_12_max_diff=1000))[1]
    assert (a != b).sum() >= 20            # measured 921
    # every value <= 0 is OpenCV's 1: there is no "disabled"
    for v in (0, -1):
        assert np.array_equal(R.restate(left, right, p.replace(disp_12_max_diff=v))[1], a)


# ---- BM's defaults filter zero texture; the tie cases run without the two filters ----------------
@pytest.mark.parametrize("name", ["flat0", "flat128", "flat255", "stripes8", "stripes16"])
def test_bm_defaults_filter_flat_and_stripes_and_the_tie_set_does_not(name):
    d = BY_ID["bm-%s-defaults" % name]
    assert d.params().texture_threshold == 20 and d.params().uniqueness_ratio == 80
    assert (d.restate()[1] == d.invalid()).all()                           # measured 0 % valid
    t = BY_ID["bm-%s-provoking" % name]
    assert t.params().texture_threshold == 0 and t.params().uniqueness_ratio == 0
    assert valid_share(t, t.restate()[1]) >= 0.3                            # measured 57 - 66 %


def test_binary_shift_matches_at_zero_cost_and_clips_the_sobel():
    case = BY_ID["sgbm-binary-defaults"]
    left, right = case.images()
    p = case.params()
    ftz = R.derived(p, left.shape[1])["ftzero"]
    f, _ = R._channels(left, ftz)
    assert np.isin(f[:, 1:-1], (0, 2 * ftz)).mean() >= 0.3   # clipped at +-ftzero
    assert (R.pixel_cost(left, right, p).min(axis=2) == 0).mean() >= 0.9


# ---- the table ---------------------------------------------------------------------------------
def test_the_table_names_every_family_and_few_degenerate_cases():
    fams = set(c.family for c in SI.CASES)
    assert fams >= set(SI.FAMILIES) - {"shifted_texture"}
    for m in ("sgbm", "bm"):
        assert set(c.family for c in SI.CASES if c.matcher == m) >= fams - {"half_correlated", "binary_shift"}
    marked = [c.id for c in SI.CASES if c.expect_all_invalid]
    assert len(marked) <= len(SI.CASES) // 6, marked
    assert all(c.floor > 0 for c in SI.CASES if not c.expect_all_invalid)


@pytest.mark.parametrize("case", SI.CASES, ids=lambda c: c.id)
def test_every_case_runs_and_is_not_empty(case):
    disp, raw = case.restate()            # (must finish: no accepted parameter set may raise)
    assert raw.dtype == np.int16 and disp.dtype == np.float32 and raw.shape == (case.H, case.W)
    share = valid_share(case, raw)
    if case.expect_all_invalid:
        assert share == 0.0
    else:
        assert share > case.floor, share
    # nothing wraps: every stored value lies between the marker and 16 * the largest disparity
    p = case.params()
    assert raw.min() >= (p.min_disparity - 1) * 16
    assert raw.max() <= (p.min_disparity + p.num_disparities) * 16
