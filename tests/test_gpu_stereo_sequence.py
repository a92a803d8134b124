"""GPU: stereo::Stereo as a sequence object (amhip_stereo_*, aerial_mapper_amd.Stereo): body poses +
frames in, one dense cloud out.  Every comparison is bit for bit: GPU rectify, both matchers and
densify are bit-exact against the CPU pieces the expected clouds are made of
(tests/stereo_sequence.py: oracle rectifier -> bm_reference / sgbm_reference -> oracle densifier),
and the sequence object adds no arithmetic of its own."""
import ctypes as C

import numpy as np
import pytest

import forward_undistort_cases as UC
import oracle_ffi as O
import stereo_front_inputs as FI
import stereo_front_reference as FR
import stereo_sequence as SS

pytestmark = pytest.mark.gpu


def _A():
    import aerial_mapper_amd as A
    return A


@pytest.fixture(scope="module")
def gmap():
    A = _A()
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


_seqs = {}


def seq_of(F, W, H):
    if (F, W, H) not in _seqs:
        _seqs[(F, W, H)] = SS.Sequence(F, W, H)
    return _seqs[(F, W, H)]


def ncam(seq, distortion=0, dist=(0.0, 0.0, 0.0, 0.0)):
    K = seq.K
    return _A().NCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], seq.W, seq.H, distortion, dist, seq.T_C_B)


def make(gmap, seq, use_bm, nth=1, undistort=False, distortion=0, dist=(0.0, 0.0, 0.0, 0.0)):
    A = _A()
    return A.Stereo(ncam(seq, distortion, dist),
                    A.StereoSettings(use_every_nth_image=nth, images_need_undistortion=undistort),
                    A.BlockMatchingParameters(use_BM=use_bm), gmap)


def host(t):
    return t.cpu().numpy()


def assert_cloud(got, want_xyz, want_i, what=""):
    xyz, inten = host(got[0]), host(got[1])
    assert xyz.shape == want_xyz.shape, (what, xyz.shape, want_xyz.shape)
    assert xyz.dtype == np.float64 and inten.dtype == np.int32
    assert np.array_equal(xyz.view(np.uint64), np.ascontiguousarray(want_xyz).view(np.uint64)), what
    assert np.array_equal(inten, want_i), what


def expected(seq, nth, use_bm):
    return SS.cpu_chain(seq, SS.pairs_of(seq.F, nth), use_bm, key=(seq.F, seq.W, seq.H, nth, use_bm))


# ---- 1. the whole sequence against the CPU chain ------------------------------------------------
@pytest.mark.parametrize("use_bm", [True, False])
def test_add_frames_equals_the_cpu_chain(gmap, use_bm):
    seq = seq_of(5, 240, 160)
    want_xyz, want_i, ns, _ = expected(seq, 1, use_bm)
    with make(gmap, seq, use_bm) as st:
        got = st.add_frames(seq.T_G_B, [f for f in seq.frames])
        assert st.pairs == 4 == len(ns)
        assert got[0].shape[0] == sum(ns)
        assert_cloud(got, want_xyz, want_i)


# ---- 2. use_every_nth_image -------------------------------------------------------------------
@pytest.mark.parametrize("nth,pairs", [(2, [(1, 3), (3, 5)]), (3, [(2, 5)])])
def test_use_every_nth_image(gmap, nth, pairs):
    seq = seq_of(7, 240, 160)
    assert SS.pairs_of(7, nth) == pairs
    want_xyz, want_i, ns, _ = expected(seq, nth, True)
    with make(gmap, seq, True, nth=nth) as st:
        got = st.add_frames(seq.T_G_B, [f for f in seq.frames])
        assert st.pairs == len(pairs)
        assert_cloud(got, want_xyz, want_i)
        # fewer than 2 n frames: one used frame at most, no pair
        st.reset()
        few = 2 * nth - 1
        got = st.add_frames(seq.T_G_B[:few], [f for f in seq.frames[:few]])
        assert st.pairs == 0 and got[0].shape == (0, 3) and got[1].shape == (0,)


# ---- 3. frame by frame, reset, determinism ------------------------------------------------------
def test_add_frame_one_by_one_reset_and_determinism(gmap):
    seq = seq_of(5, 240, 160)
    runs = []
    with make(gmap, seq, True) as st:
        for run in range(2):
            clouds = []
            for k in range(4):
                got = st.add_frame(seq.T_G_B[k], seq.frames[k])
                if k == 0:
                    assert got[0].shape == (0, 3) and got[1].shape == (0,) and st.pairs == 0
                    continue
                assert st.pairs == 1
                x, i, _ = SS.cpu_pair(seq, k - 1, k, True)
                assert x.shape[0] > 0.4 * seq.W * seq.H
                assert_cloud(got, x, i, "pair %d" % (k - 1))
                clouds.append((host(got[0]).copy(), host(got[1]).copy()))
            runs.append(clouds)
            st.reset()
            assert st.pairs == 0
        # the same sequence through add_frames, twice
        a = st.add_frames(seq.T_G_B, [f for f in seq.frames])
        a = (host(a[0]).copy(), host(a[1]).copy())
        st.reset()
        b = st.add_frames(seq.T_G_B, [f for f in seq.frames])
        assert np.array_equal(a[0].view(np.uint64), host(b[0]).view(np.uint64))
        assert np.array_equal(a[1], host(b[1]))
    for (xa, ia), (xb, ib) in zip(*runs):
        assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(ia, ib)


# ---- 4. against a loop of dense_cloud_from_stereo_pair (GPU against GPU) ------------------------
def pair_loop(gmap, seq, pairs, params, dev):
    import torch
    A = _A()
    Rs, ts = seq.camera_poses()
    xs, is_ = [], []
    for (i, j) in pairs:
        x, it = A.dense_cloud_from_stereo_pair(gmap, seq.K, Rs[i], Rs[j], ts[i], ts[j], dev[i], dev[j], params)
        xs.append(x.clone())
        is_.append(it.clone())
    return torch.cat(xs), torch.cat(is_)


@pytest.mark.parametrize("F,W,H,use_bm", [(4, 320, 240, True), (4, 320, 240, False), (3, 1920, 1080, True)])
def test_sequence_equals_a_loop_of_pair_calls(gmap, F, W, H, use_bm):
    import torch
    A = _A()
    seq = seq_of(F, W, H)
    dev = torch.from_numpy(seq.frames).cuda()
    bmp = A.BlockMatchingParameters(use_BM=use_bm)
    want = pair_loop(gmap, seq, SS.pairs_of(F, 1), bmp, dev)
    assert want[0].shape[0] > 0.4 * W * H * (F - 1)
    with make(gmap, seq, use_bm) as st:
        got = st.add_frames(seq.T_G_B, dev)
        assert st.pairs == F - 1
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 5. the PointCloud2 payload of the last pair ------------------------------------------------
def pc2_restated(r, K, W, H):
    """densifier.cpp:53-106 on the CPU chain's last pair: the payload as (H * W, 4) uint32."""
    disp, left = r["disparity"], r["left"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Q03, Q11, Q13, Q23, Q32 = -cx, fx / fy, -cy * (fx / fy), fx, 1.0 / r["baseline"]
    vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
    d = disp.astype(np.float64)
    with np.errstate(all="ignore"):
        w = Q32 * d
        p = np.stack([(uu + Q03) / w, (Q11 * vv + Q13) / w, Q23 / w], -1)
        Rm, t = r["R_G_C"], r["t_G_C1"]
        g = np.stack([((Rm[k, 0] * p[..., 0] + Rm[k, 1] * p[..., 1]) + Rm[k, 2] * p[..., 2]) + t[k]
                      for k in range(3)], -1)
        gf = g.astype(np.float32)                                   # (float)point_G
    valid = (disp > np.float32(1.0)) & ~np.isinf(gf[..., 2])        # :60, :77
    gray = left.astype(np.uint32)
    rec = np.full((H * W, 4), 0x7FC00000, np.uint32)                # kInvalidPoint in all four fields
    v = valid.reshape(-1)
    rec[v, :3] = gf.reshape(-1, 3).view(np.uint32)[v]
    rec[v, 3] = ((gray << 16) | (gray << 8) | gray).reshape(-1)[v]
    out = np.zeros((H * W, 4), np.uint32)                           # data.resize(): zeros
    out[1:] = rec[:-1]               # point_offset advances BEFORE the write (:58): pixel k -> slot k + 1
    return out, valid


@pytest.mark.parametrize("use_bm", [True, False])
def test_point_cloud2_payload_of_the_last_pair(gmap, use_bm):
    seq = seq_of(5, 240, 160)
    _, _, ns, last = expected(seq, 1, use_bm)
    want, valid = pc2_restated(last, seq.K, seq.W, seq.H)
    assert valid.sum() == ns[-1]
    # a second opinion: the payload of tests/stereo_front_reference.py
    second = FR.densify_full(last["disparity"], last["left"], seq.K, last["baseline"], last["R_G_C"], last["t_G_C1"])
    assert np.array_equal(second["pc2"], want) and np.array_equal(second["keep"], valid)
    with make(gmap, seq, use_bm) as st:
        before = host(st.point_cloud2())
        assert before.shape == (seq.H, seq.W, 16) and not before.any()
        st.add_frames(seq.T_G_B, [f for f in seq.frames])
        got = host(st.point_cloud2()).reshape(-1, 16).view(np.uint32)
    assert not got[0].any()                                  # slot 0 keeps the zeros
    assert (want[1:, 0] == 0x7FC00000).sum() > 0.2 * seq.W * seq.H > 0   # both kinds of slots occur
    assert np.array_equal(got, want)
    assert np.array_equal(got, second["pc2"])


# ---- 6. row steps and device stacks ----------------------------------------------------------
def test_wide_host_rows_and_device_stack(gmap):
    import torch
    seq = seq_of(5, 240, 160)
    want_xyz, want_i, _, _ = expected(seq, 1, True)
    wide = np.full((seq.F, seq.H, seq.W + 37), 201, np.uint8)
    wide[:, :, :seq.W] = seq.frames
    with make(gmap, seq, True) as st:
        assert_cloud(st.add_frames(seq.T_G_B, [w[:, :seq.W] for w in wide]), want_xyz, want_i, "wide host rows")
        st.reset()
        assert_cloud(st.add_frames(seq.T_G_B, torch.from_numpy(seq.frames).cuda()), want_xyz, want_i, "device stack")
        st.reset()
        dwide = torch.from_numpy(wide).cuda()
        assert_cloud(st.add_frames(seq.T_G_B, dwide[:, :, :seq.W]), want_xyz, want_i, "wide device rows")
        st.reset()
        for k in range(seq.F):
            got = st.add_frame(seq.T_G_B[k], dwide[k, :, :seq.W])
        x, i, _ = SS.cpu_pair(seq, seq.F - 2, seq.F - 1, True)
        assert_cloud(got, x, i, "add_frame, device rows")


# ---- 7. undistortion ---------------------------------------------------------------------------
def oracle_undistort(cam, frames):
    lib = O.lib()
    lib.amo_cv_undistort_image.argtypes = [C.POINTER(O.Camera), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = np.empty_like(frames)
    for k in range(frames.shape[0]):
        src = np.ascontiguousarray(frames[k])
        assert lib.amo_cv_undistort_image(C.byref(cam), src.ctypes.data, src.strides[0], 1,
                                          out[k].ctypes.data) == O.OK
    return out


@pytest.mark.parametrize("kind", ["radtan", "equidistant", "pincushion"])
def test_undistortion_before_rectification(gmap, kind):
    """The frames go through the mapped undistorter the forward mosaic uses, and like
    tests/test_gpu_forward.py this holds it to bit equality: radtan calls no libm function, and the
    map coordinate is rounded to float32 before it is scaled by 32, so a last-bit difference of a
    double atan reaches the float only once in ~2^29 pixels (tests/forward_undistort_cases.py
    checks that for the cameras it is asked of).  The two barrel lenses pull every coordinate
    inward; the pincushion one, 272 columns wide, takes BORDER_CONSTANT on all four sides and has
    live lanes in the second workgroup in x.  (The clouds see a wrong border rule at the top, the
    bottom and the right; the leftmost columns carry no disparity, so the left side is held by the
    forward mosaic's tests alone.)"""
    W, H = 240, 160
    if kind == "radtan":
        distortion, dist = O.DIST_RADTAN, (-0.25, 0.06, 3e-4, -2e-4)
    elif kind == "equidistant":
        distortion, dist = O.DIST_EQUIDISTANT, (-0.02, 0.004, -0.001, 0.0002)
    else:
        distortion, dist, W, H = O.DIST_RADTAN, (0.12, -0.02, -8e-4, 6e-4), 272, 96
    seq = SS.Sequence(4, W, H, distortion=(distortion, dist))     # rendered through that lens
    cam = O.Camera()
    cam.fu, cam.fv, cam.cu, cam.cv = seq.K[0, 0], seq.K[1, 1], seq.K[0, 2], seq.K[1, 2]
    cam.width, cam.height, cam.distortion = seq.W, seq.H, distortion
    for k in range(4):
        cam.dist[k] = dist[k]
    if kind == "pincushion":
        UC.assert_reaches_border(cam, second_workgroup=True)
    else:
        assert not UC.border_reach(cam)["outside"].any()
    if distortion == O.DIST_EQUIDISTANT:
        UC.assert_atan_robust(cam)
    und = oracle_undistort(cam, seq.frames)
    assert (und != seq.frames).mean() > 0.3          # the step does something
    want_xyz, want_i, _, _ = SS.cpu_chain(seq, SS.pairs_of(4, 1), True, frames=und)
    with make(gmap, seq, True, undistort=True, distortion=distortion, dist=dist) as st:
        assert_cloud(st.add_frames(seq.T_G_B, [f for f in seq.frames]), want_xyz, want_i, kind)
        st.reset()
        import torch
        assert_cloud(st.add_frames(seq.T_G_B, torch.from_numpy(seq.frames).cuda()), want_xyz, want_i,
                     kind + ", device frames")


def test_undistortion_of_a_distortion_free_camera_is_the_identity(gmap):
    seq = seq_of(4, 240, 160)
    with make(gmap, seq, True, undistort=False) as a, make(gmap, seq, True, undistort=True) as b:
        ga = a.add_frames(seq.T_G_B, [f for f in seq.frames])
        gb = b.add_frames(seq.T_G_B, [f for f in seq.frames])
        assert ga[0].shape[0] > 0.4 * seq.W * seq.H * 3
        assert_cloud(gb, host(ga[0]), host(ga[1]))


# ---- 8. sequence -> DSM -> OrthoFromPcl without a host copy ------------------------------------------
def test_sequence_feeds_dsm_and_ortho_from_pcl_on_the_device():
    import torch
    A = _A()
    seq = seq_of(5, 240, 160)
    want_xyz, want_i, _, _ = expected(seq, 1, True)
    settings = A.GridMapSettings(22.0, -4.0, 120.0, 90.0, 0.5)
    layers = []
    with A.AerialGridMap(settings) as m:
        with make(m, seq, True) as st:
            xyz, inten = st.add_frames(seq.T_G_B, [f for f in seq.frames])
            assert xyz.is_cuda and inten.is_cuda
            A.Dsm(A.DsmSettings(1), m).process(xyz, m)
            A.OrthoFromPcl(A.OrthoFromPclSettings(interpolation_radius=2)).process(xyz, inten, m)
            layers.append((m.get("elevation").copy(), m.get("ortho").copy()))
        m.reset()
        xyz, inten = torch.from_numpy(want_xyz).cuda(), torch.from_numpy(want_i).cuda()
        A.Dsm(A.DsmSettings(1), m).process(xyz, m)
        A.OrthoFromPcl(A.OrthoFromPclSettings(interpolation_radius=2)).process(xyz, inten, m)
        layers.append((m.get("elevation").copy(), m.get("ortho").copy()))
    (ea, oa), (eb, ob) = layers
    assert (~np.isnan(ea)).mean() > 0.2
    assert np.array_equal(ea.view(np.uint32), eb.view(np.uint32))
    assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32))


# ---- 9. refusals that need an object --------------------------------------------------------------
def test_refusals_on_a_live_object(gmap):
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    seq = seq_of(5, 240, 160)
    with make(gmap, seq, True) as st:
        for bad in (np.zeros((seq.H, seq.W, 3), np.uint8), np.zeros((seq.H, seq.W + 1), np.uint8),
                    np.zeros((seq.H - 1, seq.W), np.uint8), np.zeros((seq.H, seq.W), np.uint16)):
            with pytest.raises(A.AmhipError) as ei:
                st.add_frame(seq.T_G_B[0], bad)
            assert ei.value.status == L.ERR_ARG
        # two frames at the same position: CHECK_NE(baseline, 0.0); the pairs before it are kept
        T = seq.T_G_B.copy()
        T[3] = T[2]
        with pytest.raises(A.AmhipError) as ei:
            st.add_frames(T, [f for f in seq.frames])
        assert ei.value.status == L.ERR_ARG and "baseline" in str(ei.value)
        n, pairs = C.c_size_t(), C.c_size_t()
        assert L.load().amhip_stereo_cloud(st._h, None, None, C.byref(n), C.byref(pairs)) == L.OK
        want_xyz, _, ns, _ = expected(seq, 1, True)
        assert pairs.value == 2 and n.value == ns[0] + ns[1]
        st.reset()
        assert_cloud(st.add_frames(seq.T_G_B, [f for f in seq.frames]), want_xyz, expected(seq, 1, True)[1])
    with pytest.raises(A.AmhipError):
        A.Stereo(ncam(seq), A.StereoSettings(use_every_nth_image=0), None, gmap)
    with pytest.raises(A.AmhipError):
        A.Stereo(None, None, None, gmap)


def test_timing_goes_to_the_existing_slots(gmap):
    seq = seq_of(5, 240, 160)
    with make(gmap, seq, True) as st:
        gmap.enable_timing(True)
        gmap.timing_reset()
        st.add_frames(seq.T_G_B[:3], [f for f in seq.frames[:3]])
        times = gmap.kernel_times()
        gmap.enable_timing(False)
    assert times["k_stereo"][1] == 2 and times["k_stereo"][0] > 0.0      # one matcher call per pair
    assert times["memset/fill"][1] == 4                                   # (the misc slot) rectify + append per pair


# ---- 10. a zero w of the rectification in the middle of a sequence -----------------------------------
def chain_of(seq, pairs, use_bm):
    """cpu_chain for 160 x 120 frames: with 80 disparities the matchers leave the left 80 columns
    invalid, so a pair gives about (160 - 80 - a window) / 160 of its pixels, not cpu_chain's 40 %."""
    xs, is_, last = [], [], None
    for (i, j) in pairs:
        x, it, last = SS.cpu_pair(seq, i, j, use_bm)
        assert x.shape[0] > 0.3 * seq.W * seq.H
        xs.append(x)
        is_.append(it)
    return np.concatenate(xs), np.concatenate(is_), last


def raw_cloud(st):
    """amhip_stereo_cloud itself -> (status, xyz, intensities, pairs) on the host."""
    from aerial_mapper_amd import hip_lib as L
    from aerial_mapper_amd.mapper import _device_view
    xyz, inten, n, pairs = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    rc = L.load().amhip_stereo_cloud(st._h, C.byref(xyz), C.byref(inten), C.byref(n), C.byref(pairs))
    if n.value == 0:
        return rc, np.zeros((0, 3)), np.zeros(0, np.int32), pairs.value
    dev = st.map.device
    return (rc, host(_device_view(xyz.value, (n.value, 3), "<f8", dev, st)).copy(),
            host(_device_view(inten.value, (n.value,), "<i4", dev, st)).copy(), pairs.value)


@pytest.mark.parametrize("use_bm", [True, False])
def test_zero_w_in_the_third_pair(gmap, use_bm):
    """What the header promises (amhip_stereo_add_frame, amhip_stereo_set_pairs_in_flight): the zero w
    is found on the device; that pair and every later one add nothing; amhip_stereo_cloud -- the call
    that reads the status -- reports AMHIP_ERR_ARG with the rectifier's text and hands out the pairs
    before it; all of it bit for bit the same for every pairs_in_flight; amhip_stereo_reset recovers.
    The fourth pair is a GOOD pair (tests/stereo_front_inputs.py): only the sticky error word keeps it
    out -- in its own group of one (n = 1, 3), in the zero-w pair's group (n = 2), in one group (n = 8)."""
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    seq, good = FI.ZeroWSequence(), FI.ZeroWSequence(turned=False)
    want_xyz, want_i, last = chain_of(seq, [(0, 1), (1, 2)], use_bm)
    want_pc2 = FR.densify_full(last["disparity"], last["left"], seq.K, last["baseline"], last["R_G_C"],
                               last["t_G_C1"])["pc2"]
    good_xyz, good_i, _ = chain_of(good, SS.pairs_of(5, 1), use_bm)
    frames = [f for f in seq.frames]
    with make(gmap, seq, use_bm) as st:
        for n in (1, 2, 3, 8):
            what = "pairs_in_flight = %d" % n
            st.set_pairs_in_flight(n)
            with pytest.raises(A.AmhipError) as ei:
                st.add_frames(seq.T_G_B, frames)
            assert ei.value.status == L.ERR_ARG, what
            assert "rectifier.cpp:93,99" in str(ei.value) and "w == 0" in str(ei.value), what
            # (the failing call read and cleared the error word: the cloud is there to be had)
            rc, xyz, inten, pairs = raw_cloud(st)
            assert rc == L.OK and pairs == 2, what
            assert xyz.shape == want_xyz.shape, (what, xyz.shape, want_xyz.shape)
            assert np.array_equal(xyz.view(np.uint64), want_xyz.view(np.uint64)), what
            assert np.array_equal(inten, want_i), what
            # the payload is still the second pair's
            got_pc2 = host(st.point_cloud2()).reshape(-1, 16).view(np.uint32)
            assert np.array_equal(got_pc2, want_pc2), what
            # the documented recovery
            st.reset()
            assert_cloud(st.add_frames(good.T_G_B, [f for f in good.frames]), good_xyz, good_i, what + ", after reset")
            assert st.pairs == 4
            st.reset()
