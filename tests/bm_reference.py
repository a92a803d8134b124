"""NumPy restatement of OpenCV's block matcher, as the reference's dense point-cloud pipeline runs it
when BlockMatchingParameters::use_BM is set (stereo::BlockMatchingBM: cv::StereoBM::create(0, 0)
plus the wrapper's setters, PREFILTER_XSOBEL on 8UC1 images), followed by the wrapper's
convertTo(CV_32F) / 16 and the rectification mask.

What it restates: OpenCV 3.2 - 4.x calib3d/src/stereobm.cpp (StereoBMImpl::compute,
prefilterXSobel, findStereoCorrespondenceBM, FindStereoCorrespInvoker), calib3d's
getValidDisparityROI and filterSpeckles.  Parity against OpenCV itself is UNPINNED: OpenCV is not
part of this project's build, so these rules are a reading of that source, not a comparison with it
(the status tests/sgbm_reference.py has for StereoSGBM).  Every rule below names the OpenCV function
it comes from.  This module is the yardstick of the GPU matcher
(aerial_mapper_amd/csrc/amhip_stereo.hip, k_bm_*), which must reproduce it bit for bit.

Readings that differ from a plain statement of the algorithm:
  * The wrapper (block-matching-bm.h) calls setPreFilterCap(pre_filter_cap) and then
    setPreFilterCap(pre_filter_size): the second call wins, so the effective preFilterCap is
    pre_filter_size (9 with the reference's defaults, not 31).  disp_12_max_diff is never passed:
    disp12MaxDiff keeps StereoBM::create's -1 and validateDisparity never runs.  effective().
  * prefilterXSobel walks the rows in pairs and stops one row short of an odd height: that last row
    is all cap; row 0's upper neighbour is row 1 and, for an even height, the last row's lower
    neighbour is row H-2 (the pair's srow3 falls back to srow1).
  * The left and right columns of the SAD window are clamped independently, as
    findStereoCorrespondenceBM's pointer arithmetic does: the left one to [0, W-1], the right base
    column to [0, W-D] before + d.  Inside the valid rectangle only the right clamp can bind (for a
    negative min_disparity).
  * FindStereoCorrespInvoker leaves the map unwritten when the valid rectangle
    (getValidDisparityROI) is empty; this restatement (and the GPU) writes FILTERED there.
  * StereoBM passes speckleRange to filterSpeckles as is, in 1/16 pixel (SGBM multiplies by 16).
  * Only the scalar findStereoCorrespondenceBM is restated; OpenCV's SIMD variants
    (findStereoCorrespondenceBM_SIMD / _SSE2, taken for preFilterCap <= 31 and blockSize <= 21 on
    some builds) are not, and may break ties or round the uniqueness threshold differently.
  * The CV_16S value is ((D - mind - 1 + minD) * 256 + sub + 15) >> 4, stored through a (short)
    cast; FILTERED = (minD - 1) * 16 likewise.  Both wrap as int16 for |minD| near 4096 (restated).

Integer arithmetic only (int32 / int64); C's truncating division is written out
(sgbm_reference.tdiv), never //.
"""
import numpy as np

from sgbm_reference import K_MAX_INVALID_DISPARITY, filter_speckles, tdiv

DISP_SHIFT = 4


class Params(object):
    """BlockMatchingParameters::BM (common.h), field for field, same defaults."""
    FIELDS = ("min_disparity", "num_disparities", "pre_filter_cap", "pre_filter_size",
              "uniqueness_ratio", "texture_threshold", "speckle_window_size", "speckle_range",
              "disp_12_max_diff", "block_size")

    def __init__(self, min_disparity=1, num_disparities=80, pre_filter_cap=31, pre_filter_size=9,
                 uniqueness_ratio=80, texture_threshold=20, speckle_window_size=100, speckle_range=5,
                 disp_12_max_diff=0, block_size=15):
        self.min_disparity = min_disparity
        self.num_disparities = num_disparities
        self.pre_filter_cap = pre_filter_cap
        self.pre_filter_size = pre_filter_size
        self.uniqueness_ratio = uniqueness_ratio
        self.texture_threshold = texture_threshold
        self.speckle_window_size = speckle_window_size
        self.speckle_range = speckle_range
        self.disp_12_max_diff = disp_12_max_diff
        self.block_size = block_size

    def replace(self, **kw):
        q = Params(**{f: getattr(self, f) for f in self.FIELDS})
        for k, v in kw.items():
            assert k in self.FIELDS, k
            setattr(q, k, v)
        return q


def effective(p):
    """StereoBMParams after BlockMatchingBM's constructor (block-matching-bm.h): StereoBM::create(0, 0),
    then the setters as written."""
    return dict(minDisparity=p.min_disparity, numDisparities=p.num_disparities,
                preFilterCap=p.pre_filter_size,     # setPreFilterCap(pre_filter_size) overwrites
                preFilterSize=9,                    # OpenCV's default, unused by PREFILTER_XSOBEL
                preFilterType="XSOBEL", uniquenessRatio=p.uniqueness_ratio,
                textureThreshold=p.texture_threshold, speckleWindowSize=p.speckle_window_size,
                speckleRange=p.speckle_range, disp12MaxDiff=-1, SADWindowSize=p.block_size)


def _int16(v):
    """C's (short) cast: wraps."""
    return np.asarray(v, np.int64).astype(np.int16).astype(np.int64)


def filtered_value(p):
    """FILTERED = (minDisparity - 1) << DISPARITY_SHIFT_16S, as a short."""
    return int(_int16((p.min_disparity - 1) * (1 << DISP_SHIFT)))


# ---- prefilterXSobel ---------------------------------------------------------------------------
def prefilter_xsobel(img, cap):
    """prefilterXSobel: tab[v] = clamp(v, -cap, cap) + cap of the 3x3 x-Sobel response; columns 0
    and W-1 = cap; rows in pairs (row 0's upper neighbour row 1, an even H's last row's lower
    neighbour row H-2), an odd H's last row all cap."""
    I = np.asarray(img, np.int64)
    H, W = I.shape
    out = np.full((H, W), cap, np.int64)
    n = H & ~1                       # rows the pair loop reaches
    if n == 0 or W < 3:
        return out
    ys = np.arange(n)
    up = np.where(ys > 0, ys - 1, 1)
    dn = np.where(ys < H - 1, ys + 1, H - 2)
    dx = lambda r: I[r, 2:] - I[r, :-2]
    sob = dx(up) + 2 * dx(ys) + dx(dn)
    out[:n, 1:-1] = np.clip(sob, -cap, cap) + cap
    return out


# ---- the matched region (FindStereoCorrespInvoker, getValidDisparityROI, compute) --------------
def geometry(p, W, H):
    """findStereoCorrespondenceBM's preamble and the matched region: (lofs, rofs, width1, region)
    with region = (xa, xb, ya, yb), the valid rectangle of getValidDisparityROI (empty ROIs: the
    whole image) within [lofs, lofs + width1); None when nothing is matched (StereoBMImpl::compute's
    `lofs >= width || rofs >= width || width1 < 1`, or an empty rectangle)."""
    D, minD, SW2 = p.num_disparities, p.min_disparity, p.block_size // 2
    lofs = max(D - 1 + minD, 0)
    rofs = -min(D - 1 + minD, 0)
    width1 = W - rofs - D + 1
    maxD = minD + D - 1
    xa, xb = max(maxD, 0) + SW2, min(W - SW2, lofs + width1)
    ya, yb = SW2, H - SW2
    if lofs >= W or rofs >= W or width1 < 1 or xb <= xa or yb <= ya:
        return lofs, rofs, width1, None
    return lofs, rofs, width1, (xa, xb, ya, yb)


def _box(a, SW2, axis):
    """Sums of a over windows of 2 SW2 + 1 along axis (output shrinks by 2 SW2)."""
    c = np.cumsum(a, axis=axis, dtype=np.int64)
    z = np.zeros_like(np.take(c, [0], axis=axis))
    c = np.concatenate([z, c], axis=axis)
    n = a.shape[axis] - 2 * SW2
    return np.take(c, np.arange(2 * SW2 + 1, 2 * SW2 + 1 + n), axis=axis) - \
        np.take(c, np.arange(n), axis=axis)


def sad_volume(lf, rf, p):
    """findStereoCorrespondenceBM's running sums: for the matched region (ny, nx) and index
    d in [0, D), the SAD over the block of |L'[y+dy][clamp(X+dx, 0, W-1)] -
    R'[y+dy][clamp(X+dx-lofs+rofs, 0, W-D) + d]|, and the texture sum of |L' - cap| over the block.
    Index d means disparity D-1-d+minD."""
    H, W = lf.shape
    D, cap, SW2 = p.num_disparities, p.pre_filter_size, p.block_size // 2
    lofs, rofs, _, reg = geometry(p, W, H)
    xa, xb, ya, yb = reg
    cols = np.arange(xa - SW2, xb + SW2)
    rows = slice(ya - SW2, yb + SW2)
    lc = lf[rows][:, np.clip(cols, 0, W - 1)]
    rbase = np.clip(cols - lofs + rofs, 0, W - D)
    sad = np.empty((yb - ya, xb - xa, D), np.int64)
    for d in range(D):
        e = np.abs(lc - rf[rows][:, rbase + d])
        sad[:, :, d] = _box(_box(e, SW2, 0), SW2, 1)
    tex = _box(_box(np.abs(lc - cap), SW2, 0), SW2, 1)
    return sad, tex


def select(sad, tex, p):
    """findStereoCorrespondenceBM's per-pixel tail: texture first, then the winner (the first index
    of the minimum: ties go to the largest disparity), uniqueness (only for a ratio > 0: any d with
    |d - mind| > 1 and SAD <= minsad + minsad * ratio / 100 filters), then the subpixel step of
    dispDescale with sad[-1] := sad[1], sad[D] := sad[D-2]."""
    D, minD = p.num_disparities, p.min_disparity
    FILTERED = filtered_value(p)
    mind = sad.argmin(axis=2)
    minsad = sad.min(axis=2)
    out = np.full(mind.shape, FILTERED, np.int64)
    ok = ~(tex < p.texture_threshold)
    if p.uniqueness_ratio > 0:
        thresh = minsad + tdiv(minsad * p.uniqueness_ratio, 100)
        dd = np.arange(D)[None, None, :]
        far = np.abs(dd - mind[..., None]) > 1
        ok &= ~(far & (sad <= thresh[..., None])).any(axis=2)
    pi = np.where(mind + 1 < D, mind + 1, D - 2)
    ni = np.where(mind > 0, mind - 1, 1)
    pv = np.take_along_axis(sad, pi[..., None], 2)[..., 0]
    nv = np.take_along_axis(sad, ni[..., None], 2)[..., 0]
    den = pv + nv - 2 * minsad + np.abs(pv - nv)
    sub = np.where(den != 0, tdiv((pv - nv) * 256, np.where(den != 0, den, 1)), 0)
    val = ((D - mind - 1 + minD) * 256 + sub + 15) >> DISP_SHIFT   # arithmetic shift
    out[ok] = _int16(val[ok])
    return out


def raw_map(left, right, p):
    """StereoBM::compute's CV_16S map, before filterSpeckles."""
    H, W = left.shape
    cap = p.pre_filter_size
    raw = np.full((H, W), filtered_value(p), np.int64)
    reg = geometry(p, W, H)[3]
    if reg is None:
        return raw
    lf, rf = prefilter_xsobel(left, cap), prefilter_xsobel(right, cap)
    sad, tex = sad_volume(lf, rf, p)
    xa, xb, ya, yb = reg
    raw[ya:yb, xa:xb] = select(sad, tex, p)
    return raw


def restate(left, right, p=None, mask=None):
    """(float32 disparity as BlockMatchingBM::computeDisparityMap leaves it, int16 raw map of
    StereoBM::compute) for 8UC1 images left / right (H, W) and an optional rectification mask."""
    p = p or Params()
    left = np.asarray(left, np.uint8)
    right = np.asarray(right, np.uint8)
    raw = raw_map(left, right, p)
    if p.speckle_range >= 0 and p.speckle_window_size > 0:   # StereoBMImpl::compute
        raw = filter_speckles(raw, filtered_value(p), p.speckle_window_size, p.speckle_range)
    raw = raw.astype(np.int16)
    disp = raw.astype(np.float32) / np.float32(16.0)   # convertTo(CV_32F), / 16.0
    if mask is not None:
        disp = np.where(np.asarray(mask) != 0, disp, np.float32(K_MAX_INVALID_DISPARITY)).astype(np.float32)
    return disp, raw
