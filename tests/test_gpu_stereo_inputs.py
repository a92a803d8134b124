"""GPU: both stereo matchers bit for bit against their restatements (tests/sgbm_reference.py,
tests/bm_reference.py) on the hard inputs and at every accepted parameter edge of
tests/stereo_inputs.py: every family x both matchers (ties, saturation, speckle-sized regions,
occlusions), the parameter edges, tile edges and degenerate heights, the last accepted disparity
ranges, one large single region, masks of other values than 0 / 255, row steps of the inputs and of
the outputs, and the state a context carries from one call to the next.
tests/test_stereo_inputs.py (CPU) shows that these inputs reach what they claim."""
import ctypes as C

import numpy as np
import pytest

import bm_reference as B
import sgbm_reference as R
import stereo_inputs as SI
import test_gpu_bm as TB
import test_gpu_sgbm as TS

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in SI.CASES}


@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def mod(case):
    return TS if case.matcher == "sgbm" else TB


def same(got, want):
    got_f, got_raw = got
    want_f, want_raw = want
    assert np.array_equal(got_raw, want_raw), (np.argwhere(got_raw != want_raw)[:5],
                                               (got_raw != want_raw).sum())
    assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32))


@pytest.mark.parametrize("case", SI.CASES, ids=lambda c: c.id)
def test_case_bit_identical(gmap, case):
    mod(case).check(gmap, *case.images(), case.params())


def test_bm_output_does_not_depend_on_pre_filter_cap(gmap):
    left, right = BY_ID["bm-pair-cap_0"].images()
    outs = [TB.run(gmap, left, right, BY_ID["bm-pair-cap_0"].params().replace(pre_filter_cap=v))
            for v in (0, 31, 1000, -5)]
    for o in outs[1:]:
        same(o, outs[0])


# One large single region: the union-find at its longest chains, both matchers, the default speckle
# filter, bit for bit.  1600 x 900 at D = 64 is the largest 16:9 size whose SGBM restatement stays
# under a minute and 4 GB on the CPU (measured: 1280 x 720 14 s, 2.3 GB; 1600 x 900 23 s, 3.6 GB;
# 1920 x 1080 would need about 5 GB).  BM's restatement of the same pair: 7 s.
LARGE = (1600, 900)


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_one_large_region_bit_identical(gmap, matcher):
    W, H = LARGE
    left, right = SI.shifted_texture(H, W)
    M, T = (R, TS) if matcher == "sgbm" else (B, TB)
    p = M.Params(num_disparities=64)
    assert p.speckle_window_size == 100
    raw = T.check(gmap, left, right, p)
    assert (raw != 0).mean() > 0.8   # (one region: nearly all of the matched area at disparity 37)


# ---- masks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_mask_values_other_than_0_and_255(gmap, matcher):
    case = BY_ID["%s-occluder-provoking" % matcher]
    left, right = case.images()
    rng = np.random.default_rng(5)
    mask = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), (case.H, case.W))
    mod(case).check(gmap, left, right, case.params(), mask)
    got_f, _ = mod(case).run(gmap, left, right, case.params(), mask)
    assert (got_f[mask == 0] == 1.0).all() and (mask == 0).sum() > 100
    want_f, _ = case.restate()
    assert np.array_equal(got_f[mask != 0].view(np.uint32), want_f[mask != 0].view(np.uint32))


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_mask_all_zero(gmap, matcher):
    case = BY_ID["%s-binary-defaults" % matcher]
    left, right = case.images()
    mask = np.zeros((case.H, case.W), np.uint8)
    mod(case).check(gmap, left, right, case.params(), mask)
    got_f, got_raw = mod(case).run(gmap, left, right, case.params(), mask)
    assert (got_f == 1.0).all()
    assert np.array_equal(got_raw, case.restate()[1])   # (the CV_16S map is not masked)


# ---- row steps -------------------------------------------------------------------------------------
FIRST_OF_FAMILY = []
for _c in SI.CASES:
    if (_c.matcher, _c.family) not in [(c.matcher, c.family) for c in FIRST_OF_FAMILY] and \
            not _c.expect_all_invalid:
        FIRST_OF_FAMILY.append(_c)


@pytest.mark.parametrize("pads", [(0, 0, 0), (1, 63, 7), (200, 0, 3)])
@pytest.mark.parametrize("case", FIRST_OF_FAMILY, ids=lambda c: c.id)
def test_input_row_steps(gmap, case, pads):
    left, right = case.images()
    mask = np.full((case.H, case.W), 255, np.uint8)
    mask[::3, ::5] = 0
    want = case.restate(mask)
    same(mod(case).run(gmap, left, right, case.params(), mask, pads=pads), want)


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_outputs_into_views_of_wider_tensors(gmap, matcher):
    """compute_disparity_sgbm / _bm allocate their outputs themselves (contiguous), so the output
    row steps are only reachable through the C ABI: the float map and the CV_16S map go into column
    ranges of wider tensors, and the columns around them must stay untouched."""
    import torch
    from aerial_mapper_amd import hip_lib as L
    case = BY_ID["%s-occluder-defaults" % matcher]
    left, right = case.images()
    H, W = case.H, case.W
    want_f, want_raw = case.restate()
    lt, rt = TS.to_dev(left, 5), TS.to_dev(right, 0)
    dwide = torch.full((H, W + 9), -7.0, dtype=torch.float32, device="cuda")
    rwide = torch.full((H, W + 34), -77, dtype=torch.int16, device="cuda")
    dv, rv = dwide[:, 4:4 + W], rwide[:, 21:21 + W]
    if matcher == "sgbm":
        p = L.SgbmParams(*(int(getattr(case.params(), n)) for n, _ in L.SgbmParams._fields_))
        fn = L.load().amhip_sgbm_disparity_dev
    else:
        p = L.BmParams(*(int(getattr(case.params(), n)) for n, _ in L.BmParams._fields_))
        fn = L.load().amhip_bm_disparity_dev
    gmap.wait_for_torch(lt)
    L.check(fn(gmap.handle, C.byref(p), W, H, C.c_void_p(lt.data_ptr()), lt.stride(0),
               C.c_void_p(rt.data_ptr()), rt.stride(0), None, 0,
               C.c_void_p(dv.data_ptr()), dv.stride(0) * 4, C.c_void_p(rv.data_ptr()), rv.stride(0) * 2))
    gmap.synchronize()
    d, r = dwide.cpu().numpy(), rwide.cpu().numpy()
    assert np.array_equal(r[:, 21:21 + W], want_raw)
    assert np.array_equal(d[:, 4:4 + W].view(np.uint32), want_f.view(np.uint32))
    assert (d[:, :4] == -7.0).all() and (d[:, 4 + W:] == -7.0).all()
    assert (r[:, :21] == -77).all() and (r[:, 21 + W:] == -77).all()


# ---- state carried between calls -------------------------------------------------------------------
def test_calls_of_different_kinds_and_sizes_on_one_context():
    """The scratch, the disp2 keys and the union-find arrays are reused from call to call and must be
    re-initialised by each: a large BM call, a small SGBM call on flat, a small BM call, then SGBM
    with another D, all on one fresh context, each equal to its restatement."""
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        TB.check(m, *TS.pair(9, 641, 479), B.Params())
        for cid in ("sgbm-flat128-defaults", "bm-patches-provoking", "sgbm-half_correlated-D_128",
                    "sgbm-patches-provoking", "bm-flat0-provoking", "sgbm-occluder-provoking"):
            c = BY_ID[cid]
            mod(c).check(m, *c.images(), c.params())
