"""Named input families for the stereo matchers (plain NumPy, no GPU) and the one table of cases
(CASES) that tests/test_stereo_inputs.py (CPU: the restatements alone show what each family is for)
and tests/test_gpu_stereo_inputs.py (GPU: bit for bit against the restatements) both walk.

pair() of tests/test_gpu_sgbm.py (a smooth texture under a tilted-plane disparity) stays where it is
and is one family here ("pair"); on it almost nothing that makes a block matcher go wrong happens.
Each family below returns (left, right), uint8 (H, W), from a seed.  A shift k means
right(x) = left(x + k): the left pixel x is seen at x - k in the right image, disparity k.
"""
import numpy as np

import bm_reference as B
import sgbm_reference as R


def _shifted(tex, W, k):
    """(left, right) of width W cut from tex, (H, W + |k|): right(x) = left(x + k), k of either sign."""
    o = max(-k, 0)
    return np.ascontiguousarray(tex[:, o:o + W]), np.ascontiguousarray(tex[:, o + k:o + k + W])


def flat(H, W, seed=0, v=128):
    """Ties at every d, zero texture, the clip table's centre."""
    a = np.full((H, W), v, np.uint8)
    return a, a.copy()


def uncorrelated_noise(H, W, seed=0, binary=False):
    """High costs everywhere: S saturation under a large P2, uniqueness rejections.  binary: 0 / 255
    only, the highest contrast (more pixels whose every S saturates)."""
    rng = np.random.default_rng(seed)
    if binary:
        return ((rng.integers(0, 2, (H, W)) * 255).astype(np.uint8),
                (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8))
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def half_correlated(H, W, seed=0, k=7):
    """The left half of the right image is a shifted copy, its right half is noise: saturated and
    unsaturated pixels in one image."""
    rng = np.random.default_rng(seed)
    left, right = _shifted(rng.integers(0, 256, (H, W + abs(k)), dtype=np.uint8), W, k)
    right[:, W // 2:] = rng.integers(0, 256, (H, W - W // 2), dtype=np.uint8)
    return left, right


def binary_shift(H, W, seed=0, k=5):
    """0 / 255 at random under an integer shift: the Sobel response clips at +-ftzero, and the true
    disparity matches at exactly zero cost."""
    rng = np.random.default_rng(seed)
    return _shifted((rng.integers(0, 2, (H, W + abs(k))) * 255).astype(np.uint8), W, k)


def vertical_stripes(H, W, seed=0, period=8, k=3):
    """Stripes whose period divides D: equal costs `period` apart (uniqueness, disp2 ties)."""
    x = np.arange(W + k)
    row = np.where(x % period < period // 2, 40, 220).astype(np.uint8)
    return _shifted(np.repeat(row[None, :], H, 0), W, k)


def checkerboard(H, W, seed=0, n=1, k=3):
    """Squares of n pixels: the half-pixel interpolation of the BT cost at its extremes."""
    yy, xx = np.mgrid[0:H, 0:W + k]
    return _shifted((((xx // n + yy // n) % 2) * 255).astype(np.uint8), W, k)


PATCH_SIZES = ((8, 12), (10, 10), (10, 11), (12, 12), (6, 9), (14, 15), (9, 11), (11, 10))
PATCH_SIZES_SMALL = ((4, 6), (6, 6), (6, 7), (8, 8), (3, 5), (10, 11), (5, 7), (7, 6))   # + a block's halo


def patch_layout(H, W, sizes=PATCH_SIZES, steps=(1, 2, 3, 4, 6, 9, 14, 20), x0=44, pitch=26):
    """[(y, x, h, w, d)]: where patches() puts its rectangles in the LEFT image, and their shifts
    relative to the ground's."""
    out = []
    x, y = x0, 8
    for i, (h, w) in enumerate(sizes):
        if x + w + 4 > W:
            x, y = x0, y + 28
        assert y + h + 2 <= H, "patches: image too small for the layout"
        out.append((y, x, h, w, steps[i % len(steps)]))
        x += pitch
    return out


def patches(H, W, seed=0, sizes=PATCH_SIZES, ground=128, ground_shift=None):
    """Shifted-noise rectangles of different integer disparities on a ground; the areas straddle
    speckle_window_size = 100 (96, 100, 110, 144, ...) and the disparity steps the speckle ranges:
    many small regions at the speckle threshold.  The ground is flat (value `ground`: BM filters it,
    so every patch is a region of its own) or, with ground_shift = d0, noise at disparity d0 with the
    patches at d0 + step (SGBM spreads a patch's disparity over a flat ground, where every d ties; on
    a textured ground a patch stays a region of about its own size)."""
    rng = np.random.default_rng(seed)
    if ground_shift is None:
        left = np.full((H, W), ground, np.uint8)
        right = left.copy()
        d0 = 0
    else:
        left, right = _shifted(rng.integers(0, 256, (H, W + ground_shift), dtype=np.uint8), W, ground_shift)
        d0 = ground_shift
    for y, x, h, w, d in patch_layout(H, W, sizes):
        tex = rng.integers(0, 256, (h, w), dtype=np.uint8)
        left[y:y + h, x:x + w] = tex
        right[y:y + h, x - d - d0:x - d - d0 + w] = tex
    return left, right


def ramp(H, W, seed=0, k=4):
    """A horizontal gradient that saturates at both ends: constant Sobel, long plateaus of equal cost."""
    x = np.arange(W + k, dtype=np.float64)
    row = np.clip((x - W / 4.0) * 255.0 / (W / 2.0), 0, 255).astype(np.uint8)
    return _shifted(np.repeat(row[None, :], H, 0), W, k)


def occluder(H, W, seed=0, d_bg=3, d_fg=20):
    """A foreground strip at a large disparity over a background at a small one: left-right check
    failures and several left pixels claiming one right pixel."""
    rng = np.random.default_rng(seed)
    left, right = _shifted(rng.integers(0, 256, (H, W + d_bg), dtype=np.uint8), W, d_bg)
    a, b = W // 2, W // 2 + W // 5
    fg = rng.integers(0, 256, (H, b - a), dtype=np.uint8)
    left[:, a:b] = fg
    right[:, a - d_fg:b - d_fg] = fg
    return left, right


def shifted_texture(H, W, seed=9, k=37):
    """The full-HD tests' texture: one large smooth region at disparity k."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W + k]
    tex = (np.sin(xx * 0.31) * 40 + np.cos(yy * 0.23) * 30 + 128 +
           rng.integers(-50, 50, (H, W + k))).clip(0, 255).astype(np.uint8)
    return _shifted(tex, W, k)


def pair_family(H, W, seed=0, disp=(6, 30)):
    from test_gpu_sgbm import pair
    return pair(seed, W, H, disp)


FAMILIES = dict(flat=flat, uncorrelated_noise=uncorrelated_noise, half_correlated=half_correlated,
                binary_shift=binary_shift, vertical_stripes=vertical_stripes, checkerboard=checkerboard,
                patches=patches, ramp=ramp, occluder=occluder, pair=pair_family,
                shifted_texture=shifted_texture)


class Case(object):
    """One restatement call: matcher ("sgbm" / "bm"), the family with its arguments, the size, the
    parameters that differ from the base set, and `floor`: the share of pixels the restatement must
    leave valid (strictly above), so that no GPU comparison is one of empty maps.  A case that is
    all-invalid by design says so (expect_all_invalid) and is then asserted to be exactly that."""

    def __init__(self, name, matcher, family, H, W, params, floor=0.0, expect_all_invalid=False,
                 seed=1, **fkw):
        self.name, self.matcher, self.family, self.H, self.W = name, matcher, family, H, W
        self.kw, self.floor, self.expect_all_invalid = dict(params), floor, expect_all_invalid
        self.seed, self.fkw = seed, fkw

    @property
    def id(self):
        return "%s-%s" % (self.matcher, self.name)

    def images(self):
        return FAMILIES[self.family](self.H, self.W, seed=self.seed, **self.fkw)

    def params(self):
        return (SGBM_BASE if self.matcher == "sgbm" else BM_BASE).replace(**self.kw)

    def invalid(self):
        p = self.params()
        return (p.min_disparity - 1) * 16 if self.matcher == "sgbm" else B.filtered_value(p)

    def restate(self, mask=None):
        return (R if self.matcher == "sgbm" else B).restate(*self.images(), self.params(), mask)


# The reference's defaults with D = 32: a restatement call at these sizes takes 0.02 - 0.2 s.
SGBM_BASE = R.Params(num_disparities=32)
BM_BASE = B.Params(num_disparities=32)

# the parameter sets that provoke what a family exists for
SGBM_SAT = dict(p1=1000, p2=4096, block_size=11, pre_filter_cap=63)    # S at its int16 ceiling
SGBM_SAT_EQ = dict(p1=4096, p2=4096, block_size=11, pre_filter_cap=63)
BM_TIES = dict(texture_threshold=0, uniqueness_ratio=0)                 # (the defaults filter flat / stripes)

BM_PATCHES = dict(block_size=5, uniqueness_ratio=15, speckle_range=16)   # regions of about a patch's size

H0, W0 = 96, 200


def _family_cases():
    """Section 3: every family x both matchers, the defaults and the family's provoking set.
    (name, family, its arguments, SGBM's provoking set, BM's, the floors of SGBM and of BM's
    provoking set, the floor of BM's defaults -- None: the defaults filter every pixel)"""
    textured = dict(ground_shift=2)
    fams = [
        ("flat0", "flat", dict(v=0), dict(uniqueness_ratio=0, speckle_window_size=0), BM_TIES, .5, .3, None),
        ("flat128", "flat", dict(v=128), dict(uniqueness_ratio=100), BM_TIES, .5, .3, None),
        ("flat255", "flat", dict(v=255), dict(min_disparity=0, block_size=1), BM_TIES, .5, .3, None),
        ("noise", "uncorrelated_noise", {}, SGBM_SAT_EQ, dict(uniqueness_ratio=5, texture_threshold=0),
         .02, .01, None),
        ("noise_binary", "uncorrelated_noise", dict(binary=True), SGBM_SAT,
         dict(uniqueness_ratio=1, texture_threshold=0, speckle_window_size=0), .02, .01, None),
        ("half", "half_correlated", {}, SGBM_SAT_EQ, dict(uniqueness_ratio=15), .2, .1, .1),
        ("binary", "binary_shift", {}, dict(pre_filter_cap=0, p1=8, p2=32),
         dict(pre_filter_size=1, uniqueness_ratio=15), .5, .3, .3),
        ("stripes8", "vertical_stripes", dict(period=8), dict(uniqueness_ratio=0, disp_12_max_diff=1000),
         BM_TIES, .5, .3, None),
        ("stripes16", "vertical_stripes", dict(period=16), dict(uniqueness_ratio=0, min_disparity=0),
         dict(BM_TIES, block_size=5), .5, .3, None),
        ("checker1", "checkerboard", dict(n=1), dict(uniqueness_ratio=0, block_size=3), BM_TIES, .5, .3, None),
        ("checker4", "checkerboard", dict(n=4), dict(uniqueness_ratio=0, pre_filter_cap=63), BM_TIES,
         .5, .3, None),
        ("patches", "patches", textured, dict(speckle_range=2), BM_PATCHES, .5, .3, .3),
        ("patches_flat", "patches", dict(sizes=PATCH_SIZES_SMALL), dict(speckle_range=2), BM_PATCHES,
         .2, .01, .01),
        ("ramp", "ramp", {}, dict(uniqueness_ratio=0, block_size=3), BM_TIES, .5, .2, .05),
        ("occluder", "occluder", {}, dict(disp_12_max_diff=1, uniqueness_ratio=0), dict(uniqueness_ratio=15),
         .5, .3, .3),
    ]
    out = []
    # with uniqueness_ratio = 0 nothing but `minS >= 32767` rejects a pixel whose every S is saturated
    # (with a ratio > 0 the uniqueness rule rejects it as well, all S being equal)
    for name, fkw, sat in (("noise_binary", dict(binary=True), SGBM_SAT), ("noise", {}, SGBM_SAT_EQ)):
        out.append(Case(name + "-saturated_uniq0", "sgbm", "uncorrelated_noise", H0, W0,
                        dict(sat, uniqueness_ratio=0, speckle_window_size=0), floor=.3, **fkw))
    for name, fam, fkw, sg, bm, fs, fb, fbd in fams:
        H, W = (120, 260) if fam == "patches" else (H0, W0)
        out.append(Case(name + "-defaults", "sgbm", fam, H, W, {}, floor=fs, **fkw))
        out.append(Case(name + "-provoking", "sgbm", fam, H, W, sg, floor=fs, **fkw))
        # (BM's defaults, texture_threshold 20 and uniqueness_ratio 80, filter every pixel of some)
        out.append(Case(name + "-defaults", "bm", fam, H, W, {}, floor=fbd or 0.0,
                        expect_all_invalid=fbd is None, **fkw))
        out.append(Case(name + "-provoking", "bm", fam, H, W, bm, floor=fb, **fkw))
    return out


def _edge_cases():
    """Section 4: every accepted parameter edge, on two inputs each.  A case whose disparity range
    misses the family's own shift moves the shift into the range (fkw)."""
    out = []

    def sg(name, kw, W=W0, pair_all_invalid=False, fkw=None, **ckw):
        out.append(Case("half_correlated-" + name, "sgbm", "half_correlated", H0, W, kw, floor=.05,
                        **dict(ckw, **(fkw or {}))))
        out.append(Case("pair-" + name, "sgbm", "pair", H0, W, kw, floor=.1,
                        **dict(ckw, expect_all_invalid=pair_all_invalid or ckw.get("expect_all_invalid", False))))

    # BM's default uniqueness_ratio = 80 leaves pair() nearly empty at this size (the family cases
    # above run the defaults); the edges run at 15 unless the ratio itself is the edge
    def bm(name, kw, H=H0, W=W0, pair_all_invalid=False, fkw=None, floor=.1, pair_floor=.01, **ckw):
        kw = dict(dict(uniqueness_ratio=15), **kw)
        out.append(Case("binary_shift-" + name, "bm", "binary_shift", H, W, kw, floor=floor,
                        **dict(ckw, **(fkw or {}))))
        out.append(Case("pair-" + name, "bm", "pair", H, W, kw, floor=pair_floor,
                        **dict(ckw, expect_all_invalid=pair_all_invalid or ckw.get("expect_all_invalid", False))))

    for p1, p2 in ((0, 0), (1, 1), (8, 32), (1000, 4096), (4096, 4096), (4096, 1)):
        sg("p1_%d_p2_%d" % (p1, p2), dict(p1=p1, p2=p2))
    for v in (0, 1, 15, 16, 63):
        sg("cap_%d" % v, dict(pre_filter_cap=v))
    # (at 99 / 100 only a pixel whose minimum of S is 0 survives: none on pair()'s noise)
    for v in (-1, 0, 1, 50, 99, 100):
        sg("uniq_%d" % v, dict(uniqueness_ratio=v), pair_all_invalid=v >= 99)
    for v in (-1, 0, 1, 5, 1000):
        sg("disp12_%d" % v, dict(disp_12_max_diff=v))
    for v in (0, 1, 200, 4096):             # (4096: the last accepted value)
        sg("speckle_range_%d" % v, dict(speckle_range=v))
    for v in (-1, 0, 1, 100000):            # (100000: no region is larger, everything goes)
        sg("speckle_window_%d" % v, dict(speckle_window_size=v), expect_all_invalid=(v == 100000))
    for v in (0, 1, 3, 11):
        sg("block_%d" % v, dict(block_size=v))
    # (w1 = W - 1 - D >= 64, and half_correlated's copied half reaches past column maxD)
    for v in (16, 64, 80, 128, 192, 256):
        sg("D_%d" % v, dict(num_disparities=v), W=max(W0, 2 * v + 100))
    # (-64: maxD = -32 <= 0, every disparity negative)
    for v, k in ((-64, -50), (-17, -5), (-1, 7), (0, 7), (1, 7), (17, 30)):
        sg("minD_%d" % v, dict(min_disparity=v), fkw=dict(k=k))

    for v in (0, 1, 100, 101, 1000):        # (from 100 on: only an exact match, minsad = 0, passes)
        bm("uniq_%d" % v, dict(uniqueness_ratio=v), pair_all_invalid=v >= 100)
    for v in (0, 1, 10 ** 6, 2 ** 31 - 1):  # (the window's texture sum is at most 31 * 31 * 63)
        bm("texture_%d" % v, dict(texture_threshold=v), expect_all_invalid=(v >= 10 ** 6))
    for v in (1, 2, 62, 63):
        bm("prefilter_%d" % v, dict(pre_filter_size=v))
    for v in (0, 1000):                     # (overridden by pre_filter_size: the output ignores it)
        bm("cap_%d" % v, dict(pre_filter_cap=v))
    bm("block_5", dict(block_size=5))
    bm("block_31", dict(block_size=31))
    # (one matched row, at most 1 / 21 of the image; no speckle filter: a row holds no 100-pixel region)
    bm("block_eq_H", dict(block_size=21, speckle_window_size=0), H=21, floor=.01, pair_floor=.001)
    # (block_size = W: the valid rectangle is empty whatever the rest)
    bm("block_eq_minWH", dict(block_size=31, num_disparities=16), H=40, W=31, expect_all_invalid=True)
    for v in (16, 48, 240, 256):
        bm("D_%d" % v, dict(num_disparities=v), W=max(W0, v + 1 + 14 + 72))
    for v, k in ((-64, -50), (-17, -5), (-1, 5), (0, 5), (1, 5), (17, 30)):
        bm("minD_%d" % v, dict(min_disparity=v), fkw=dict(k=k))
    return out


def _range_cases():
    """Section 5: the last accepted min_disparity on each side for D = 16 and D = 256 (the CV_16S
    map holds (min_disparity - 1) * 16 >= -32768 and (min_disparity + D) * 16 <= 32767), on a wide,
    short image whose shift lies inside the range.  Nothing wraps there (asserted on the CPU)."""
    out = []
    for D in (16, 256):
        for minD in (-2047, 2047 - D):
            k = minD + D // 2
            for m, fam, kw in (("sgbm", "half_correlated", {}), ("bm", "binary_shift", dict(uniqueness_ratio=15, block_size=5))):
                # (half_correlated copies the left half of the right image: 2 * 2400 columns reach past maxD)
                W = 4800 if m == "sgbm" and minD > 0 else 2400
                out.append(Case("range_D_%d_minD_%d" % (D, minD), m, fam, 8, W,
                                dict(kw, num_disparities=D, min_disparity=minD, speckle_window_size=20),
                                floor=.01, k=k))
    return out


# Tile edges (D = 16, binary_shift).  SGBM: w1 = W - 17 on, one below and one above its 64-column
# tiles, heights around the 32-row chunks of the vertical sum and below block_size / 2 (where the
# last updated row is row 0).  BM: the matched width W - 30 around its 32-column tiles, heights from
# one matched row to three 64-row bands.  (No speckle filter: at H = 1 a row holds no 100-pixel region.)
TILE_SGBM = [Case("tile_w1_%d_H_%d" % (w1, H), "sgbm", "binary_shift", H, w1 + 17,
                  dict(num_disparities=16, speckle_window_size=0), floor=.1)
             for w1 in (63, 64, 65, 127, 128, 129) for H in (1, 2, 3, 4, 31, 32, 33, 65)]
TILE_BM = [Case("tile_w_%d_H_%d" % (w, H), "bm", "binary_shift", H, w + 30,
                dict(num_disparities=16, uniqueness_ratio=15, speckle_window_size=0), floor=.005)
           for w in (31, 32, 33, 64, 65) for H in (15, 16, 63, 64, 65, 78, 79, 129)]

CASES = _family_cases() + _edge_cases() + _range_cases() + TILE_SGBM + TILE_BM
assert len(set(c.id for c in CASES)) == len(CASES)
