"""GPU: amhip_rectify_stereo_pair_dev (stereo::Rectifier::rectifyStereoPair + computeMask,
rectifier.cpp:34-128) bit for bit against the oracle -- maps (float), both remapped images,
mask, rectified rotation, baseline; and, where it was built, against the reference's own
rectifier.cpp compiled over oracle/refkit.  Then the whole front of the dense pipeline stays on
the GPU: rectify -> (a synthetic disparity) -> densify -> Dsm."""
import numpy as np
import pytest

import oracle_ffi as O
import stereo_front_inputs as FI
import stereo_front_reference as FR
from test_oracle_rectify import rig

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,W,H", [(11, 160, 120), (12, 752, 480), (13, 333, 211)])
def test_gpu_rectifier_is_bit_exact(seed, W, H):
    import torch
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = rig(seed, W=W, H=H)
    which = "loops" if O.have_loops() else "port"
    rc, want = O.rectify_stereo_pair(K, R1, R2, t1, t2, left, right, which=which)
    assert rc == O.OK
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        # (row steps larger than the width: views of wider rasters)
        wide_l = torch.zeros((H, W + 24), dtype=torch.uint8, device="cuda")
        wide_r = torch.zeros((H, W + 8), dtype=torch.uint8, device="cuda")
        wide_l[:, :W] = torch.from_numpy(left).cuda()
        wide_r[:, :W] = torch.from_numpy(right).cuda()
        got = A.rectify_stereo_pair(m, K, R1, R2, t1, t2, wide_l[:, :W], wide_r[:, :W], want_maps=True)
    assert got["baseline"] == want["baseline"]
    assert np.array_equal(got["R_G_C"], want["R_G_C"])
    assert np.array_equal(got["maps"].cpu().numpy().view(np.uint32), want["maps"].view(np.uint32))
    assert np.array_equal(got["image_left"].cpu().numpy(), want["left"])
    assert np.array_equal(got["image_right"].cpu().numpy(), want["right"])
    assert np.array_equal(got["mask"].cpu().numpy(), want["mask"])
    assert 0.2 < (want["mask"] == 255).mean() < 1.0


def test_rectify_densify_dsm_stays_on_the_gpu():
    import torch
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = rig(14, W=320, H=240)
    with A.AerialGridMap(A.GridMapSettings(12.0, -4.0, 160.0, 120.0, 0.5)) as m:
        r = A.rectify_stereo_pair(m, K, R1, R2, t1, t2, torch.from_numpy(left).cuda(),
                                  torch.from_numpy(right).cuda())
        # the block matcher (OpenCV) is outside the path: a plane of constant disparity stands in
        disp = torch.full((240, 320), 11.0, dtype=torch.float32, device="cuda")
        disp[r["mask"] == 0] = -1.0
        pts, inten = A.densify(m, disp, r["image_left"], K, r["baseline"], r["R_G_C"], t1)
        assert pts.shape[0] > 1000 and pts.is_cuda
        A.Dsm(A.DsmSettings(1), m).process(pts, m)
        elev = m.get("elevation")
    assert (~np.isnan(elev)).sum() > 100


# ---- the edges: tests/stereo_front_inputs.py, against the numpy restatement and the oracle --------
@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def wide_pair(left, right):
    """Views of wider rasters with different row steps; the padding holds 255."""
    import torch
    H, W = left.shape
    wide_l = torch.full((H, W + 24), 255, dtype=torch.uint8, device="cuda")
    wide_r = torch.full((H, W + 8), 255, dtype=torch.uint8, device="cuda")
    wide_l[:, :W] = torch.from_numpy(left).cuda()
    wide_r[:, :W] = torch.from_numpy(right).cuda()
    return wide_l[:, :W], wide_r[:, :W]


def assert_equals(got, want, what):
    assert got["baseline"] == want["baseline"], what
    assert np.array_equal(got["R_G_C"].view(np.uint64), np.ascontiguousarray(want["R_G_C"]).view(np.uint64)), what
    assert np.array_equal(got["maps"].cpu().numpy().view(np.uint32), want["maps"].view(np.uint32)), what
    assert np.array_equal(got["image_left"].cpu().numpy(), want["left"]), what
    assert np.array_equal(got["image_right"].cpu().numpy(), want["right"]), what
    assert np.array_equal(got["mask"].cpu().numpy(), want["mask"]), what


def check_gpu(gmap, args):
    import aerial_mapper_amd as A
    K, R1, R2, t1, t2, left, right = args
    ref = FR.rectify_ref(*args)
    rc, port = O.rectify_stereo_pair(*args)
    assert rc == O.OK and not ref["zero_w"]
    l, r = wide_pair(left, right)
    got = A.rectify_stereo_pair(gmap, K, R1, R2, t1, t2, l, r, want_maps=True)
    assert_equals(got, ref, "numpy restatement")
    assert_equals(got, port, "oracle")
    return ref


_rigs = FI.rectify_rigs()


@pytest.mark.parametrize("name", sorted(_rigs))
def test_gpu_rectifier_at_the_edges(gmap, name):
    args = _rigs[name]
    ref = check_gpu(gmap, args)
    H, W = args[5].shape
    if name == "identity":       # the maps are (u, v), both images come back, the mask is full
        v, u = np.mgrid[0:H, 0:W].astype(np.float32)
        assert np.array_equal(ref["maps"], np.stack([u, v, u, v]))
        assert np.array_equal(ref["left"], args[5]) and np.array_equal(ref["right"], args[6])
        assert (ref["mask"] == 255).all()
    if name.startswith("axis"):
        assert ref["neg_decided"] > 0
    if name == "axis far":
        assert ref["wide_edges"] > 0
    if name == "2^26":
        assert ref["clamp_2_31"] > 0 and ref["clamp_short"] > 0


def _direct(gmap, args, l, r, maps, out_l, out_r, mask):
    import ctypes as C
    from aerial_mapper_amd import hip_lib as L
    K, R1, R2, t1, t2 = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in args[:5])
    H, W = args[5].shape
    f64p = C.POINTER(C.c_double)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    R, b = np.zeros(9), C.c_double()
    gmap.wait_for_torch(next(t for t in (l, out_l, mask) if t is not None))
    L.check(L.load().amhip_rectify_stereo_pair_dev(
        gmap.handle, K.ctypes.data_as(f64p), R1.ctypes.data_as(f64p), R2.ctypes.data_as(f64p),
        t1.ctypes.data_as(f64p), t2.ctypes.data_as(f64p), W, H, p(l), l.stride(0) if l is not None else 0,
        p(r), r.stride(0) if r is not None else 0, R.ctypes.data_as(f64p), C.byref(b), p(maps), p(out_l),
        p(out_r), p(mask)))
    gmap.synchronize()
    return R.reshape(3, 3), b.value


def test_optional_outputs(gmap):
    import torch
    args = _rigs["yaw +0.6"]
    ref = FR.rectify_ref(*args)
    H, W = args[5].shape
    l, r = wide_pair(args[5], args[6])
    new = lambda: torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    # maps, the right image and the mask not asked for
    out_l = new()
    R, b = _direct(gmap, args, l, r, None, out_l, None, None)
    assert b == ref["baseline"] and np.array_equal(R, ref["R_G_C"])
    assert np.array_equal(out_l.cpu().numpy(), ref["left"])
    # only the mask (no input image is needed for it)
    mask = new()
    R, b = _direct(gmap, args, None, None, None, None, None, mask)
    assert b == ref["baseline"] and np.array_equal(R, ref["R_G_C"])
    assert np.array_equal(mask.cpu().numpy(), ref["mask"])


def test_zero_w_is_reported_and_cleared(gmap):
    """w2 == 0.0f along row 60: CHECK_NE(xyw(2), 0.0) of rectifier.cpp:93,99.  The call that reports
    it clears the error word: the next pair on the same map is served, bit for bit."""
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib as L
    args = FI.zero_w_rig()
    assert FR.rectify_ref(*args)["zero_w"] and O.rectify_stereo_pair(*args)[0] == O.ERR_EXACT_HIT
    l, r = wide_pair(args[5], args[6])
    with pytest.raises(A.AmhipError) as ei:
        A.rectify_stereo_pair(gmap, *args[:5], l, r, want_maps=True)
    assert ei.value.status == L.ERR_ARG
    assert "rectifier.cpp:93,99" in str(ei.value) and "w == 0" in str(ei.value)
    check_gpu(gmap, _rigs["base -x"])
