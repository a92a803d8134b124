"""GPU: amhip_bm_disparity_dev (stereo::BlockMatchingBM::computeDisparityMap) bit for bit against
tests/bm_reference.py -- the CV_16S map and the float map, on several sizes (odd and even heights,
widths off the tile), parameter sets, row steps wider than the width and the mask -- plus the
degenerate widths, determinism, the scratch it shares with SGBM, full HD accuracy on a shifted
texture, the k_stereo timing slot and rectify -> BM -> densify -> DSM on the device."""
import numpy as np
import pytest

import bm_reference as B
import sgbm_reference as R
from test_gpu_sgbm import pair, to_dev
from test_oracle_rectify import rig

pytestmark = pytest.mark.gpu


def run(m, left, right, params, mask=None, pads=(24, 8, 40)):
    import aerial_mapper_amd as A
    bp = A.BmParameters(**{f: getattr(params, f) for f in B.Params.FIELDS})
    dm = to_dev(mask, pads[2]) if mask is not None else None
    disp, raw = A.compute_disparity_bm(m, to_dev(left, pads[0]), to_dev(right, pads[1]), bp,
                                       mask=dm, raw=True)
    return disp.cpu().numpy(), raw.cpu().numpy()


@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def check(m, left, right, params, mask=None):
    want_f, want_raw = B.restate(left, right, params, mask)
    got_f, got_raw = run(m, left, right, params, mask)
    assert np.array_equal(got_raw, want_raw), (np.argwhere(got_raw != want_raw)[:5],
                                               (got_raw != want_raw).sum())
    assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32))
    return want_raw


@pytest.mark.parametrize("seed,W,H", [(1, 160, 120), (2, 333, 211), (3, 640, 480), (4, 641, 479)])
def test_default_parameters_bit_identical(gmap, seed, W, H):
    raw = check(gmap, *pair(seed, W, H), B.Params())
    # (uniqueness 80 makes the map sparse; 160 x 120 leaves a narrow matched region at D = 80.  The
    # restatement's own output on these inputs: 2.8 %, 55 %, 76 %, 76 % valid)
    assert (raw != B.filtered_value(B.Params())).mean() > (0.02 if W < 200 else 0.4)


@pytest.mark.parametrize("kw", [
    dict(num_disparities=16), dict(num_disparities=64), dict(num_disparities=128),
    dict(num_disparities=256, min_disparity=0), dict(block_size=5), dict(block_size=9),
    dict(block_size=21), dict(block_size=31, uniqueness_ratio=10), dict(min_disparity=0), dict(min_disparity=-8),
    dict(min_disparity=20, num_disparities=32), dict(uniqueness_ratio=0), dict(uniqueness_ratio=15),
    dict(texture_threshold=0), dict(texture_threshold=200), dict(speckle_window_size=0),
    dict(speckle_range=-1), dict(speckle_range=0), dict(speckle_range=40), dict(pre_filter_size=31),
    dict(pre_filter_size=63), dict(min_disparity=-8, num_disparities=48, block_size=7),
])
def test_parameter_sets_bit_identical(gmap, kw):
    disp = (2, 12) if kw.get("num_disparities") == 16 else (6, 30)
    W = 400 if kw.get("num_disparities") == 256 or kw.get("block_size", 0) > 15 else 200
    check(gmap, *pair(7, W, 150, disp), B.Params().replace(**kw))


def test_mask_is_honoured(gmap):
    left, right = pair(4, 160, 120)
    mask = np.full((120, 160), 255, np.uint8)
    mask[:, :50] = 0
    mask[90:, :] = 0
    check(gmap, left, right, B.Params(), mask)
    got_f, _ = run(gmap, left, right, B.Params(), mask)
    assert (got_f[mask == 0] == 1.0).all()


@pytest.mark.parametrize("W", [60, 80, 94])
def test_degenerate_widths_are_all_filtered(gmap, W):
    # D = 80, minD = 1, block 15: W = 60 leaves width1 < 1, W = 80 lofs >= W, and W = 94 an empty
    # valid rectangle (xa = 80 + 7 = xb = 94 - 7)
    left, right = pair(5, W, 40)
    raw = check(gmap, left, right, B.Params())
    assert (raw == 0).all()   # FILTERED = (1 - 1) * 16


def test_two_calls_give_the_same_bits(gmap):
    left, right = pair(6, 333, 211)
    a = run(gmap, left, right, B.Params())
    b = run(gmap, left, right, B.Params())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_sgbm_after_bm_on_the_same_context(gmap):
    import aerial_mapper_amd as A
    left, right = pair(8, 333, 211)
    run(gmap, *pair(9, 641, 479), B.Params())   # (grows and fills the shared scratch)
    want_f, want_raw = R.restate(left, right, R.Params())
    disp, raw = A.compute_disparity_sgbm(gmap, to_dev(left, 0), to_dev(right, 0), raw=True)
    assert np.array_equal(raw.cpu().numpy(), want_raw)
    assert np.array_equal(disp.cpu().numpy().view(np.uint32), want_f.view(np.uint32))


def test_full_hd_shifted_texture_within_half_a_pixel(gmap):
    import aerial_mapper_amd as A
    rng = np.random.default_rng(9)
    W, H, k = 1920, 1080, 37
    yy, xx = np.mgrid[0:H, 0:W + k]
    tex = (np.sin(xx * 0.31) * 40 + np.cos(yy * 0.23) * 30 + 128 +
           rng.integers(-50, 50, (H, W + k))).clip(0, 255).astype(np.uint8)
    disp, raw = A.compute_disparity_bm(gmap, to_dev(tex[:, :W], 0), to_dev(tex[:, k:], 0), raw=True)
    d, r = disp.cpu().numpy()[8:-8, 95:-8], raw.cpu().numpy()[8:-8, 95:-8]
    valid = r != 0
    assert valid.mean() > 0.5
    assert np.abs(d[valid] - k).max() <= 0.5


def test_timing_slot_counts_the_matcher(gmap):
    left, right = pair(8, 160, 120)
    gmap.enable_timing(True)
    gmap.timing_reset()
    run(gmap, left, right, B.Params())
    ms, n = gmap.kernel_times()["k_stereo"]
    gmap.enable_timing(False)
    assert n == 1 and ms > 0.0


def test_dense_cloud_from_stereo_pair_with_use_bm_equals_the_steps():
    import torch
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = rig(14, W=320, H=240)
    settings = A.GridMapSettings(12.0, -4.0, 160.0, 120.0, 0.5)
    with A.AerialGridMap(settings) as m:
        lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        pts, inten = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt,
                                                    A.BlockMatchingParameters(use_BM=True))
        A.Dsm(A.DsmSettings(1), m).process(pts, m)
        elev_a = m.get("elevation")
        # step by step: GPU rectify, the restatement on the rectified images, GPU densify
        r = A.rectify_stereo_pair(m, K, R1, R2, t1, t2, lt, rt)
        want, _ = B.restate(r["image_left"].cpu().numpy(), r["image_right"].cpu().numpy(), B.Params(),
                            r["mask"].cpu().numpy())
        pts_b, inten_b = A.densify(m, torch.from_numpy(want).cuda(), r["image_left"], K, r["baseline"],
                                   r["R_G_C"], t1)
        assert pts.shape[0] > 100
        assert torch.equal(pts, pts_b) and torch.equal(inten, inten_b)
        # a BmParameters alone selects BM too
        pts_c, _ = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt, A.BmParameters())
        assert torch.equal(pts, pts_c)
        m.reset()
        A.Dsm(A.DsmSettings(1), m).process(pts_b, m)
        elev_b = m.get("elevation")
    assert np.array_equal(elev_a.view(np.uint32), elev_b.view(np.uint32))
    assert (~np.isnan(elev_a)).sum() > 100


def test_dense_cloud_default_is_still_sgbm():
    import torch
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = rig(14, W=320, H=240)
    with A.AerialGridMap(A.GridMapSettings(12.0, -4.0, 160.0, 120.0, 0.5)) as m:
        lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        a = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt)
        b = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt, A.SgbmParameters())
        c = A.dense_cloud_from_stereo_pair(m, K, R1, R2, t1, t2, lt, rt, A.BlockMatchingParameters())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
