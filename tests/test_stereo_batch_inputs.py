"""CPU: the seam inputs of tests/stereo_batch_inputs.py can catch a batch kernel that reads or joins
across the seam between two images of a stack.  With the restatements alone: the stack matched as ONE
tall image differs from the per-image results in the rows next to the seams -- for the cost sums, the
SGBM chains and BM's window sums (different noise per image), and for the speckle filter alone (two
small regions that touch a seam from both sides and together exceed speckle_window_size).  Without
these assertions the bit-for-bit GPU tests on the same stacks would prove nothing."""
import numpy as np
import pytest

import sgbm_reference as R
import stereo_batch_inputs as SB

# (BM on pure noise with the speckle filter on keeps nothing at these sizes: `half` serves there)
NOISE_CASES = [(m, kind, win) for m in ("sgbm", "bm") for kind in ("half", "noise") for win in (0, 100)
               if not (m == "bm" and kind == "noise" and win == 100)]


@pytest.mark.parametrize("W,H,D", SB.SHAPES)
@pytest.mark.parametrize("matcher,kind,win", NOISE_CASES)
def test_noise_stack_differs_at_the_seams_when_matched_as_one_image(W, H, D, matcher, kind, win):
    p = SB.params(matcher, D, win)
    lefts, rights = SB.noise_stack(W, H, kind)
    assert not np.array_equal(lefts[0], lefts[1]) and not np.array_equal(lefts[1], lefts[2])
    each_f, each_raw = SB.restate_each(matcher, lefts, rights, p)
    tall_f, tall_raw = SB.restate_tall(matcher, lefts, rights, p)
    invalid = (p.min_disparity - 1) * 16
    assert (each_raw != invalid).mean() > 0.1            # no comparison of empty maps
    rows = SB.seam_rows(H, SB.NB, 4)                     # (nb, H): the four rows either side of a seam
    differs = (each_raw != tall_raw).any(axis=2)         # per row
    # at least 7 of the 8 rows around each of the two seams come out different
    assert (differs & rows).sum() >= 14, (differs & rows).sum()
    assert (each_f.view(np.uint32) != tall_f.view(np.uint32))[rows].any()


@pytest.mark.parametrize("W,H,D", SB.SHAPES)
def test_speckle_stack_joins_regions_across_a_seam_when_filtered_as_one_image(W, H, D):
    p = SB.params("sgbm", D, 100).replace(speckle_range=2)
    lefts, rights = SB.speckle_stack(W, H)
    invalid = (p.min_disparity - 1) * 16
    # the maps in front of the speckle filter, per image (so that nothing but the filter differs)
    pre = SB.restate_each("sgbm", lefts, rights, p.replace(speckle_window_size=0))[1]
    each = SB.restate_each("sgbm", lefts, rights, p)[1]
    high = pre >= (SB.SPECKLE_D0 + SB.SPECKLE_STEP - 2) * 16       # the patches' disparity
    for b in range(SB.NB - 1):
        below, above = high[b, H - 10:].sum(), high[b + 1, :10].sum()
        assert 0 < below <= 100 and 0 < above <= 100 and below + above > 100, (b, below, above)
        assert high[b, H - 1].any() and high[b + 1, 0].any()       # both touch the seam
    assert not (each >= (SB.SPECKLE_D0 + SB.SPECKLE_STEP - 2) * 16).any()   # per image: all removed
    tall = R.filter_speckles(pre.reshape(SB.NB * H, W).copy(), invalid, p.speckle_window_size,
                             16 * p.speckle_range).reshape(SB.NB, H, W)
    rows = SB.seam_rows(H, SB.NB, 8)
    diff = tall != each
    assert diff[rows].sum() > 200 and not diff[~rows].any(), (diff[rows].sum(), diff[~rows].sum())
    # and the whole restatement on the tall image differs there too
    assert (SB.restate_tall("sgbm", lefts, rights, p)[1] != each)[rows].sum() > 200
    # BM cannot take this input's role: it never labels the rows next to a seam
    import bm_reference as B
    raw = B.restate(lefts[0], rights[0], SB.params("bm", D, 0))[1]
    f = B.filtered_value(SB.params("bm", D, 0))
    assert (raw[:3] == f).all() and (raw[-3:] == f).all()
