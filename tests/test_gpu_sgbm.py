"""GPU: amhip_sgbm_disparity_dev (stereo::BlockMatchingSGBM::computeDisparityMap) bit for bit
against tests/sgbm_reference.py -- the CV_16S map and the float map, on several sizes, seeds,
parameter sets and row steps wider than the width -- plus the mask, the degenerate width, determinism,
full HD accuracy on a shifted texture, and rectify -> SGBM -> densify -> DSM on the device."""
import numpy as np
import pytest

import sgbm_reference as R
from test_oracle_rectify import rig

pytestmark = pytest.mark.gpu


def pair(seed, W, H, disp=(6, 30), noise=40):
    """A textured left image and a right image that sees it shifted by a disparity that varies
    smoothly across the image (a tilted plane), plus a little noise."""
    rng = np.random.default_rng(seed)
    lo, hi = disp
    Wt = W + hi + 2
    yy, xx = np.mgrid[0:H, 0:Wt]
    tex = (np.sin(xx * 0.37) * 40 + np.cos(yy * 0.29 + xx * 0.05) * 30 + 128 +
           rng.integers(-noise, noise, (H, Wt))).clip(0, 255).astype(np.uint8)
    left = tex[:, :W]
    xr = np.arange(W)[None, :]
    dmap = lo + (hi - lo) * (np.arange(H)[:, None] / max(H - 1, 1) * 0.5 + xr / max(W - 1, 1) * 0.5)
    src = np.clip(np.round(xr + dmap).astype(np.int64), 0, Wt - 1)   # right(x) = left(x + d)
    right = np.take_along_axis(tex, src, 1)
    right = (right.astype(np.int32) + rng.integers(-3, 4, (H, W))).clip(0, 255).astype(np.uint8)
    return left, right


def to_dev(a, pad):
    import torch
    H, W = a.shape
    wide = torch.zeros((H, W + pad), dtype=torch.uint8, device="cuda")
    wide[:, :W] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return wide[:, :W]


def run(m, left, right, params, mask=None, pads=(24, 8, 40)):
    import aerial_mapper_amd as A
    sp = A.SgbmParameters(**{f: getattr(params, f) for f in R.Params.FIELDS})
    dm = to_dev(mask, pads[2]) if mask is not None else None
    disp, raw = A.compute_disparity_sgbm(m, to_dev(left, pads[0]), to_dev(right, pads[1]), sp,
                                         mask=dm, raw=True)
    return disp.cpu().numpy(), raw.cpu().numpy()


@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def check(m, left, right, params, mask=None):
    want_f, want_raw = R.restate(left, right, params, mask)
    got_f, got_raw = run(m, left, right, params, mask)
    assert np.array_equal(got_raw, want_raw), (np.argwhere(got_raw != want_raw)[:5],
                                               (got_raw != want_raw).sum())
    assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32))
    return want_raw


@pytest.mark.parametrize("seed,W,H", [(1, 160, 120), (2, 333, 211), (3, 640, 480)])
def test_default_parameters_bit_identical(gmap, seed, W, H):
    raw = check(gmap, *pair(seed, W, H), R.Params())
    assert (raw > 0).mean() > 0.3   # (the comparison is not of empty maps)


@pytest.mark.parametrize("kw", [
    dict(min_disparity=0), dict(num_disparities=16), dict(num_disparities=64),
    dict(num_disparities=128), dict(block_size=3), dict(block_size=5), dict(block_size=11),
    dict(speckle_window_size=0), dict(uniqueness_ratio=0), dict(min_disparity=3, disp_12_max_diff=2),
    dict(min_disparity=-4, num_disparities=48),
])
def test_parameter_sets_bit_identical(gmap, kw):
    disp = (2, 12) if kw.get("num_disparities") == 16 else (6, 30)
    check(gmap, *pair(7, 200, 150, disp), R.Params().replace(**kw))


def test_mask_is_honoured(gmap):
    left, right = pair(4, 160, 120)
    mask = np.full((120, 160), 255, np.uint8)
    mask[:, :50] = 0
    mask[90:, :] = 0
    check(gmap, left, right, R.Params(), mask)
    got_f, _ = run(gmap, left, right, R.Params(), mask)
    assert (got_f[mask == 0] == 1.0).all()


def test_width_not_above_max_disparity_is_all_invalid(gmap):
    left, right = pair(5, 81, 40)
    raw = check(gmap, left, right, R.Params())
    assert (raw == 0).all()   # INVALID_DISP_SCALED = (1 - 1) * 16


def test_two_calls_give_the_same_bits(gmap):
    left, right = pair(6, 333, 211)
    a = run(gmap, left, right, R.Params())
    b = run(gmap, left, right, R.Params())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_full_hd_shifted_texture_within_half_a_pixel(gmap):
    import aerial_mapper_amd as A
    rng = np.random.default_rng(9)
    W, H, k = 1920, 1080, 37
    yy, xx = np.mgrid[0:H, 0:W + k]
    tex = (np.sin(xx * 0.31) * 40 + np.cos(yy * 0.23) * 30 + 128 +
           rng.integers(-50, 50, (H, W + k))).clip(0, 255).astype(np.uint8)
    disp = A.compute_disparity_sgbm(gmap, to_dev(tex[:, :W], 0), to_dev(tex[:, k:], 0))
    inner = disp.cpu().numpy()[8:-8, 90:-8]
    assert np.abs(inner - k).max() <= 0.5


def test_dense_cloud_from_stereo_pair_equals_the_steps():
    import torch
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = rig(14, W=320, H=240)
    settings = A.GridMapSettings(12.0, -4.0, 160.0, 120.0, 0.5)
    with A.AerialGridMap(settings) as m:
        lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        pts, inten = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt)
        A.Dsm(A.DsmSettings(1), m).process(pts, m)
        elev_a = m.get("elevation")
        # step by step: GPU rectify, the restatement on the rectified images, GPU densify
        r = A.rectify_stereo_pair(m, K, R1, R2, t1, t2, lt, rt)
        want, _ = R.restate(r["image_left"].cpu().numpy(), r["image_right"].cpu().numpy(), R.Params(),
                            r["mask"].cpu().numpy())
        pts_b, inten_b = A.densify(m, torch.from_numpy(want).cuda(), r["image_left"], K, r["baseline"],
                                   r["R_G_C"], t1)
        assert pts.shape[0] > 1000
        assert torch.equal(pts, pts_b) and torch.equal(inten, inten_b)
        m.reset()
        A.Dsm(A.DsmSettings(1), m).process(pts_b, m)
        elev_b = m.get("elevation")
    assert np.array_equal(elev_a.view(np.uint32), elev_b.view(np.uint32))
    assert (~np.isnan(elev_a)).sum() > 100


def test_timing_slot_counts_the_matcher(gmap):
    left, right = pair(8, 160, 120)
    gmap.enable_timing(True)
    gmap.timing_reset()
    run(gmap, left, right, R.Params())
    ms, n = gmap.kernel_times()["k_stereo"]
    gmap.enable_timing(False)
    assert n == 1 and ms > 0.0
