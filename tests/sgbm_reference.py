"""NumPy restatement of OpenCV's semi-global block matcher, as the reference's dense point-cloud
pipeline runs it (stereo::BlockMatchingSGBM: cv::StereoSGBM::create(0, 0, 0) plus the ten setters of
BlockMatchingParameters::SGBM, i.e. MODE_SGBM on 8UC1 images), followed by the wrapper's
convertTo(CV_32F) / 16 and the rectification mask.

What it restates: OpenCV 3.2 - 4.x calib3d/src/stereosgbm.cpp (computeDisparitySGBM,
calcPixelCostBT, StereoSGBMImpl::compute, filterSpecklesImpl) and imgproc's 3x3 medianBlur, the
OpenCV of a ROS Melodic workspace.  Parity against OpenCV itself is UNPINNED: OpenCV is not part of
this project's build, so these rules are a reading of that source, not a comparison with it (the
same status oracle/amo_cvlike.h has for the forward mosaic).  Every rule below names the OpenCV
function it comes from, so that a real workspace can diff it.  This module is the yardstick of the
GPU matcher (aerial_mapper_amd/csrc/amhip_stereo.hip), which must reproduce it bit for bit.

Readings that differ from a plain statement of the algorithm:
  * computeDisparitySGBM stores C + P2 ("add P2 to every C(x,y). it saves a few operations in the
    inner loops") and subtracts minLr + P2 in the recurrence, so the stored Lr equals the textbook
    C + min(...) - minLr and lies in [C, C + P2].  Both forms are written out below.
  * The vertical running sum of the block cost is only updated while row y + SH2 is inside the
    image (the `if( k < height )` around the hsum / C update): the last SH2 rows keep the block
    cost of row H-1-SH2 instead of a replicated-border box.  Restated as such.
  * The left-right check tests disp2 >= minD (not >= 0).  disp2 starts at INVALID_DISP_SCALED =
    (minD-1)*16; with the reference's min_disparity = 1 that start value is 0, which FAILS the test
    (an unwritten disp2 entry never invalidates a pixel), while for min_disparity >= 2 it is
    (minD-1)*16 >= minD and an unwritten entry does take part.  Both are encoded.
  * Some OpenCV versions leave column minX1 of the running block cost at its row-0 value; the
    restatement uses the replicated box there (the later versions' behaviour).

Limits of the comparison: OpenCV keeps S in int16 with saturating adds.  Every Lr is >= 0, so the
saturated S is min(S, 32767) whatever the order of the adds; both this module and the GPU (which
sums in 32 bits) apply exactly that.  A pixel whose every S saturates keeps OpenCV's bestDisp = -1
and ends invalid without writing disp2 (restated).  C + P2 and Lr fit
int16 for every accepted parameter set (block_size <= 11, P2 <= 4096).  restate() also needs
width1 = maxX1 - minX1 > block_size // 2 (OpenCV's first hsum reads past the row otherwise).

Integer arithmetic only (int32 / int64); C's truncating division is written out (tdiv), never //.
"""
import numpy as np

SHRT_MAX = 32767
DISP_SHIFT = 4
DISP_SCALE = 1 << DISP_SHIFT
K_MAX_INVALID_DISPARITY = 1.0  # stereo::kMaxInvalidDisparity (common.h)


class Params(object):
    """BlockMatchingParameters::SGBM (common.h), field for field, same defaults."""
    FIELDS = ("min_disparity", "num_disparities", "pre_filter_cap", "uniqueness_ratio",
              "speckle_window_size", "speckle_range", "disp_12_max_diff", "p1", "p2", "block_size")

    def __init__(self, min_disparity=1, num_disparities=80, pre_filter_cap=35, uniqueness_ratio=10,
                 speckle_window_size=100, speckle_range=20, disp_12_max_diff=0, p1=120, p2=250,
                 block_size=9):
        self.min_disparity = min_disparity
        self.num_disparities = num_disparities
        self.pre_filter_cap = pre_filter_cap
        self.uniqueness_ratio = uniqueness_ratio
        self.speckle_window_size = speckle_window_size
        self.speckle_range = speckle_range
        self.disp_12_max_diff = disp_12_max_diff
        self.p1 = p1
        self.p2 = p2
        self.block_size = block_size

    def replace(self, **kw):
        q = Params(**{f: getattr(self, f) for f in self.FIELDS})
        for k, v in kw.items():
            assert k in self.FIELDS, k
            setattr(q, k, v)
        return q


def tdiv(a, b):
    """C's integer division: truncates toward zero (numpy's // floors)."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def derived(p, width):
    """computeDisparitySGBM's preamble."""
    minD = p.min_disparity
    maxD = minD + p.num_disparities
    D = maxD - minD
    assert D > 0 and D % 16 == 0, "CV_Assert( D % 16 == 0 )"
    P1 = p.p1 if p.p1 > 0 else 2
    P2 = max(p.p2 if p.p2 > 0 else 5, P1 + 1)
    ftzero = max(p.pre_filter_cap, 15) | 1
    uniq = p.uniqueness_ratio if p.uniqueness_ratio >= 0 else 10
    disp12 = p.disp_12_max_diff if p.disp_12_max_diff > 0 else 1
    win = p.block_size if p.block_size > 0 else 5
    minX1 = max(maxD, 0)
    maxX1 = width + min(minD, 0)
    return dict(minD=minD, maxD=maxD, D=D, P1=P1, P2=P2, ftzero=ftzero, uniq=uniq, disp12=disp12,
                SW2=win // 2, SH2=win // 2, minX1=minX1, maxX1=maxX1,
                invalid=(minD - 1) * DISP_SCALE)


# ---- calcPixelCostBT ---------------------------------------------------------------------
def _channels(img, ftzero):
    """calcPixelCostBT: the prefiltered channel (x-Sobel through clipTab) and the raw channel;
    rows above / below replicated at the image edge (n1 / s1 = 0); the first and last column of
    BOTH channels are tab[0] = ftzero."""
    I = img.astype(np.int32)
    up = np.vstack([I[:1], I[:-1]])
    dn = np.vstack([I[1:], I[-1:]])
    f = np.full(I.shape, ftzero, np.int32)
    sob = (I[:, 2:] - I[:, :-2]) * 2 + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
    f[:, 1:-1] = np.clip(sob, -ftzero, ftzero) + ftzero          # clipTab
    r = I.copy()
    r[:, 0] = ftzero
    r[:, -1] = ftzero
    return f, r


def _half_minmax(v):
    """calcPixelCostBT: min / max of v and its half-pixel neighbours (v + v[x-1]) / 2,
    (v + v[x+1]) / 2 (v itself at the row's ends)."""
    W = v.shape[1]
    vl = v.copy()
    vr = v.copy()
    vl[:, 1:] = tdiv(v[:, 1:] + v[:, :-1], 2)
    vr[:, :W - 1] = tdiv(v[:, :W - 1] + v[:, 1:], 2)
    return np.minimum(np.minimum(vl, vr), v), np.maximum(np.maximum(vl, vr), v)


def pixel_cost(left, right, p):
    """calcPixelCostBT for every row: (H, width1, D) int32, the Birchfield-Tomasi cost of the
    prefiltered channel plus that of the raw channel >> 2 (diff_scale)."""
    H, W = left.shape
    q = derived(p, W)
    minD, D, minX1, maxX1, ftz = q["minD"], q["D"], q["minX1"], q["maxX1"], q["ftzero"]
    w1 = maxX1 - minX1
    cost = np.zeros((H, w1, D), np.int32)
    for ch, (a, b) in enumerate(zip(_channels(left, ftz), _channels(right, ftz))):
        scale = 0 if ch == 0 else 2
        u = a[:, minX1:maxX1]
        u0, u1 = (m[:, minX1:maxX1] for m in _half_minmax(a))
        b0, b1 = _half_minmax(b)
        for d in range(D):
            s = d + minD                        # right column x - s
            v = b[:, minX1 - s:maxX1 - s]
            v0 = b0[:, minX1 - s:maxX1 - s]
            v1 = b1[:, minX1 - s:maxX1 - s]
            c0 = np.maximum(np.maximum(0, u - v1), v0 - u)
            c1 = np.maximum(np.maximum(0, v - u1), u0 - v)
            cost[:, :, d] += np.minimum(c0, c1) >> scale
    return cost


# ---- the block cost (computeDisparitySGBM: hsumAdd / C running sums) -----------------------
def block_cost(pix, p, width):
    """C(x, y, d) = sum of pix over |dx| <= SW2, |dy| <= SH2, columns clamped to [0, width1-1]
    (the hsumAdd initialisation with weight SW2+1 and the running min / max indices), rows clamped
    to [0, H-1] -- except that rows y > H-1-SH2 keep the block cost of row max(H-1-SH2, 0): the
    running update `C = Cprev + hsumAdd - hsumSub` only runs while row y+SH2 < height."""
    H, w1, D = pix.shape
    q = derived(p, width)
    SW2, SH2 = q["SW2"], q["SH2"]
    assert w1 > SW2, "width1 must exceed block_size // 2"
    hsum = np.zeros((H, w1, D), np.int64)
    for dx in range(-SW2, SW2 + 1):
        hsum += pix[:, np.clip(np.arange(w1) + dx, 0, w1 - 1), :]
    ye = np.array([0 if y == 0 else min(y, max(H - 1 - SH2, 0)) for y in range(H)])
    C = np.zeros((H, w1, D), np.int64)
    for dy in range(-SH2, SH2 + 1):
        C += hsum[np.clip(ye + dy, 0, H - 1)]
    return C


# ---- the path costs (computeDisparitySGBM, MODE_SGBM: NR = 5 directions) -------------------
def lr_step(Cp, Lp, mLp, P1, P2):
    """One step of the recurrence for a batch of chains: Cp, Lp (N, D), mLp (N,).
    computeDisparitySGBM: L = (C + P2) + min(Lr_p[d], Lr_p[d-1] + P1, Lr_p[d+1] + P1, delta) - delta,
    delta = minLr_p + P2; Lr_p[-1] = Lr_p[D] = MAX_COST."""
    N, D = Lp.shape
    big = np.full((N, 1), SHRT_MAX, np.int64)
    pad = np.hstack([big, Lp, big])
    delta = (mLp + P2)[:, None]
    Cstored = Cp + P2                                           # "add P2 to every C(x,y)"
    L = Cstored + np.minimum(np.minimum(Lp, pad[:, :-2] + P1),
                             np.minimum(pad[:, 2:] + P1, delta)) - delta
    return L, L.min(axis=1)


def aggregate(C, P1, P2):
    """S = sum of Lr over the five MODE_SGBM directions: left->right (r = (-1, 0)), top-left
    (-1, -1), top (0, -1), top-right (1, -1) in the forward sweep, right->left (1, 0) in the
    second loop over the row.  Outside the image and outside [minX1, maxX1) the previous Lr and
    minLr are 0 (the zeroed borders of the Lr / minLr buffers)."""
    H, w1, D = C.shape
    C = C.astype(np.int64)
    S = np.zeros((H, w1, D), np.int64)
    z = lambda *s: np.zeros(s, np.int64)
    # left -> right and right -> left: chains are rows
    for xs in (range(w1), range(w1 - 1, -1, -1)):
        Lp, mLp = z(H, D), z(H)
        for x in xs:
            Lp, mLp = lr_step(C[:, x], Lp, mLp, P1, P2)
            S[:, x] += Lp
    # top, top-left, top-right: the previous row's Lr of x, x-1, x+1
    for shift in (0, 1, -1):
        Lp, mLp = z(w1, D), z(w1)
        for y in range(H):
            Ls, ms = z(w1, D), z(w1)
            if shift == 0:
                Ls, ms = Lp, mLp
            elif shift == 1:
                Ls[1:], ms[1:] = Lp[:-1], mLp[:-1]
            else:
                Ls[:-1], ms[:-1] = Lp[1:], mLp[1:]
            Lp, mLp = lr_step(C[y], Ls, ms, P1, P2)
            S[y] += Lp
    return S


# ---- winner, uniqueness, subpixel, disp2, left-right check (computeDisparitySGBM) ----------
def select(S, p, width):
    """Raw CV_16S map of computeDisparitySGBM (before medianBlur / filterSpeckles)."""
    H, w1, D = S.shape
    q = derived(p, width)
    minD, minX1, inv, uniq, disp12 = q["minD"], q["minX1"], q["invalid"], q["uniq"], q["disp12"]
    # S is int16 with saturating adds (saturate_cast<CostType>); every Lr >= 0
    S = np.minimum(S, SHRT_MAX)
    best = S.argmin(axis=2)                  # `if( Sval < minS )`: the lowest d of the minimum
    minS = S.min(axis=2)
    dd = np.arange(D)[None, None, :]
    bad = (S * (100 - uniq) < minS[..., None] * 100) & (np.abs(best[..., None] - dd) > 1)
    # every S saturated: `Sval < minS` never holds, bestDisp stays -1, and the pixel ends invalid
    # either way (rejected by the uniqueness loop, or d = -1 -> (minD - 1) * 16) without a disp2 write
    ok = ~bad.any(axis=2) & (minS < SHRT_MAX)
    # disp2: x descending, `if( disp2cost[_x2] > minS )` -> of equal costs the largest x wins
    X = np.arange(w1)[None, :] + minX1
    x2 = X - best - minD
    key = np.full((H, width), np.iinfo(np.int64).max, np.int64)
    ys, xs = np.nonzero(ok)
    np.minimum.at(key, (ys, x2[ys, xs]), minS[ys, xs] * 65536 + (0xFFFF - X[0, xs]))
    disp2 = np.where(key == np.iinfo(np.int64).max, inv,
                     (0xFFFF - (key & 0xFFFF)) - np.arange(width)[None, :])
    # subpixel: d*16 + ((S[d-1] - S[d+1])*16 + den) / (den*2), C division, only for 0 < d < D-1
    bi = np.clip(best, 1, max(D - 2, 1))
    Sm = np.take_along_axis(S, (bi - 1)[..., None], 2)[..., 0]
    Sc = np.take_along_axis(S, bi[..., None], 2)[..., 0]
    Sp = np.take_along_axis(S, np.minimum(bi + 1, D - 1)[..., None], 2)[..., 0]
    den = np.maximum(Sm + Sp - 2 * Sc, 1)
    sub = best * DISP_SCALE + tdiv((Sm - Sp) * DISP_SCALE + den, den * 2)
    d16 = np.where((best > 0) & (best < D - 1), sub, best * DISP_SCALE)
    disp1 = np.full((H, width), inv, np.int64)
    disp1[:, minX1:minX1 + w1] = np.where(ok, d16 + minD * DISP_SCALE, inv)
    return lr_check(disp1, disp2, minD, disp12, inv)


def lr_check(disp1, disp2, minD, disp12, inv):
    """computeDisparitySGBM's last loop: round d1 down (d1 >> 4) and up ((d1 + 15) >> 4); the
    pixel is invalidated only if BOTH columns exist, hold disp2 >= minD and differ by more than
    disp12MaxDiff."""
    H, W = disp1.shape
    X = np.arange(W)[None, :].repeat(H, 0)
    lo = disp1 >> DISP_SHIFT                 # arithmetic shift: floor
    hi = (disp1 + DISP_SCALE - 1) >> DISP_SHIFT

    def fails(d):
        x = X - d
        inside = (x >= 0) & (x < W)
        v = np.take_along_axis(disp2, np.clip(x, 0, W - 1), 1)
        return inside & (v >= minD) & (np.abs(v - d) > disp12)
    out = disp1.copy()
    out[(disp1 != inv) & fails(lo) & fails(hi)] = inv
    return out


# ---- StereoSGBMImpl::compute: medianBlur(disp, disp, 3), filterSpeckles ---------------------
def median3(a):
    """medianBlur, 3x3, BORDER_REPLICATE."""
    H, W = a.shape
    pad = np.pad(a, 1, mode="edge")
    st = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return np.sort(st, axis=0)[4]


def filter_speckles(a, new_val, max_speckle_size, max_diff):
    """filterSpecklesImpl: 4-connected regions of pixels != newVal whose neighbours differ by at
    most maxDiff; a region of <= maxSpeckleSize pixels becomes newVal.  The regions are the
    connected components of a symmetric relation, so the scan order does not matter."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    H, W = a.shape
    v = a != new_val
    idx = np.arange(H * W).reshape(H, W)
    e_r = v[:, :-1] & v[:, 1:] & (np.abs(a[:, :-1] - a[:, 1:]) <= max_diff)
    e_d = v[:-1, :] & v[1:, :] & (np.abs(a[:-1, :] - a[1:, :]) <= max_diff)
    src = np.concatenate([idx[:, :-1][e_r], idx[:-1, :][e_d]])
    dst = np.concatenate([idx[:, 1:][e_r], idx[1:, :][e_d]])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(H * W, H * W))
    _, lab = connected_components(g, directed=False)
    size = np.bincount(lab, minlength=H * W)
    small = (size[lab] <= max_speckle_size).reshape(H, W) & v
    out = a.copy()
    out[small] = new_val
    return out


def restate(left, right, p=None, mask=None):
    """(float32 disparity as BlockMatchingSGBM::computeDisparityMap leaves it, int16 raw map of
    StereoSGBM::compute) for 8UC1 images left / right (H, W) and an optional rectification mask."""
    p = p or Params()
    left = np.asarray(left, np.uint8)
    right = np.asarray(right, np.uint8)
    H, W = left.shape
    q = derived(p, W)
    inv = q["invalid"]
    if q["minX1"] >= q["maxX1"]:
        raw = np.full((H, W), inv, np.int64)   # disp1 = Scalar::all(INVALID_DISP_SCALED)
    else:
        C = block_cost(pixel_cost(left, right, p), p, W)
        raw = select(aggregate(C, q["P1"], q["P2"]), p, W)
    raw = median3(raw)
    if p.speckle_window_size > 0:
        raw = filter_speckles(raw, inv, p.speckle_window_size, DISP_SCALE * p.speckle_range)
    raw = raw.astype(np.int16)
    disp = raw.astype(np.float32) / np.float32(16.0)   # convertTo(CV_32F), / 16.0
    if mask is not None:
        disp = np.where(np.asarray(mask) != 0, disp, np.float32(K_MAX_INVALID_DISPARITY)).astype(np.float32)
    return disp, raw
