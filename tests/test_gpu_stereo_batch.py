"""GPU: several stereo pairs per launch.  The batched matchers (compute_disparity_sgbm / _bm on
(B, H, W) stacks, amhip_*_disparity_batch_dev) give, pair by pair, the bits of the restatements
(tests/sgbm_reference.py, tests/bm_reference.py) and of B one-pair calls -- on different pairs, on
the seam inputs of tests/stereo_batch_inputs.py (shown on the CPU to catch a leak across a seam:
tests/test_stereo_batch_inputs.py), with masks, through padded layouts, and mixed with one-pair calls
on one context.  Stereo.add_frames with n pairs in flight gives the bits of n = 1 and of the CPU chain
(tests/stereo_sequence.py).  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import bm_reference as B
import sgbm_reference as R
import stereo_batch_inputs as SB
import stereo_sequence as SS
import test_gpu_sgbm as TS

pytestmark = pytest.mark.gpu


def _A():
    import aerial_mapper_amd as A
    return A


@pytest.fixture(scope="module")
def gmap():
    A = _A()
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        yield m


def gpu_params(matcher, p):
    A = _A()
    if matcher == "sgbm":
        return A.SgbmParameters(**{f: getattr(p, f) for f in R.Params.FIELDS})
    return A.BmParameters(**{f: getattr(p, f) for f in B.Params.FIELDS})


def fn_of(matcher):
    A = _A()
    return A.compute_disparity_sgbm if matcher == "sgbm" else A.compute_disparity_bm


def stack_dev(a, pad=0, gap=0):
    """(B, H, W) on the device as a view of a (B, H + gap, W + pad) tensor."""
    import torch
    nb, H, W = a.shape
    wide = torch.full((nb, H + gap, W + pad), 77, dtype=torch.uint8, device="cuda")
    wide[:, :H, :W] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return wide[:, :H, :W]


def run_batch(m, matcher, lefts, rights, p, masks=None, pads=(0, 0, 0), gaps=(0, 0, 0)):
    dm = stack_dev(masks, pads[2], gaps[2]) if masks is not None else None
    f, raw = fn_of(matcher)(m, stack_dev(lefts, pads[0], gaps[0]), stack_dev(rights, pads[1], gaps[1]),
                            gpu_params(matcher, p), mask=dm, raw=True)
    assert tuple(f.shape) == tuple(lefts.shape) == tuple(raw.shape)
    return f.cpu().numpy(), raw.cpu().numpy()


def run_each(m, matcher, lefts, rights, p, masks=None):
    outs = []
    for b in range(lefts.shape[0]):
        dm = TS.to_dev(masks[b], 3) if masks is not None else None
        f, raw = fn_of(matcher)(m, TS.to_dev(lefts[b], 5), TS.to_dev(rights[b], 0), gpu_params(matcher, p),
                                mask=dm, raw=True)
        outs.append((f.cpu().numpy(), raw.cpu().numpy()))
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def same(got, want, what=""):
    for b in range(want[1].shape[0]):
        bad = got[1][b] != want[1][b]
        assert not bad.any(), (what, "pair %d" % b, int(bad.sum()), np.argwhere(bad)[:5])
        assert np.array_equal(got[0][b].view(np.uint32), want[0][b].view(np.uint32)), (what, "pair %d" % b)


def three_pairs(W, H, D):
    disp = (2, 12) if D == 16 else (6, 28)
    ps = [TS.pair(seed, W, H, disp) for seed in (3, 4, 5)]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])


# ---- 1. three different pairs ---------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", SB.SHAPES)
@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_three_different_pairs(gmap, matcher, W, H, D):
    p = SB.params(matcher, D, 100)
    lefts, rights = three_pairs(W, H, D)
    want = SB.restate_each(matcher, lefts, rights, p)
    assert (want[1] != (p.min_disparity - 1) * 16).mean() > 0.05
    assert not np.array_equal(want[1][0], want[1][1]) and not np.array_equal(want[1][1], want[1][2])
    got = run_batch(gmap, matcher, lefts, rights, p)
    same(got, want, "against the restatement")
    same(got, run_each(gmap, matcher, lefts, rights, p), "against three one-pair calls")


# ---- 2. the seam inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", SB.SHAPES)
@pytest.mark.parametrize("win", [0, 100])
@pytest.mark.parametrize("matcher,kind", [("sgbm", "half"), ("sgbm", "noise"), ("sgbm", "speckle"),
                                          ("bm", "half"), ("bm", "noise"), ("bm", "speckle")])
def test_seam_inputs(gmap, matcher, kind, win, W, H, D):
    p = SB.params(matcher, D, win)
    if kind == "speckle":
        p = p.replace(speckle_range=2)
        lefts, rights = SB.speckle_stack(W, H)
    else:
        lefts, rights = SB.noise_stack(W, H, kind)
    want = SB.restate_each(matcher, lefts, rights, p)
    same(run_batch(gmap, matcher, lefts, rights, p), want, "%s %s" % (matcher, kind))


# ---- 3. batch of one; five pairs ------------------------------------------------------------------
@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_batch_of_one_equals_the_one_pair_call(gmap, matcher):
    W, H, D = SB.SHAPES[1]
    p = SB.params(matcher, D, 100)
    lefts, rights = three_pairs(W, H, D)
    got = run_batch(gmap, matcher, lefts[1:2], rights[1:2], p)
    same(got, run_each(gmap, matcher, lefts[1:2], rights[1:2], p))
    same(got, SB.restate_each(matcher, lefts[1:2], rights[1:2], p))


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_five_pairs_default_parameters(gmap, matcher):
    W, H = 333, 211
    p = (R if matcher == "sgbm" else B).Params()
    ps = [TS.pair(seed, W, H) for seed in range(20, 25)]
    lefts, rights = np.stack([q[0] for q in ps]), np.stack([q[1] for q in ps])
    got = run_batch(gmap, matcher, lefts, rights, p)
    same(got, run_each(gmap, matcher, lefts, rights, p), "against five one-pair calls")
    # (one pair of the five against the restatement; the one-pair call's own tests cover the rest)
    want = (R if matcher == "sgbm" else B).restate(lefts[3], rights[3], p)
    assert (want[1] != (p.min_disparity - 1) * 16).mean() > 0.3
    assert np.array_equal(got[1][3], want[1]) and np.array_equal(got[0][3].view(np.uint32), want[0].view(np.uint32))


# ---- 4. padded layouts through the C ABI -----------------------------------------------------------
@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_row_steps_and_batch_strides_beyond_the_dense_layout(gmap, matcher):
    """Inputs: rows wider than W and images further apart than H rows.  Outputs: the float map and
    the CV_16S map go into views of wider, taller tensors through the C ABI, and every canary value
    beside the rows and between the images stays untouched."""
    import torch
    from aerial_mapper_amd import hip_lib as L
    W, H, D = SB.SHAPES[1]
    p = SB.params(matcher, D, 100)
    lefts, rights = SB.noise_stack(W, H, "half")
    masks = np.full(lefts.shape, 255, np.uint8)
    masks[:, ::3, ::5] = 0
    want = SB.restate_each(matcher, lefts, rights, p, masks)
    lt, rt, mt = stack_dev(lefts, 7, 3), stack_dev(rights, 0, 1), stack_dev(masks, 30, 0)
    nb = lefts.shape[0]
    dwide = torch.full((nb, H + 2, W + 9), -7.0, dtype=torch.float32, device="cuda")
    rwide = torch.full((nb, H + 5, W + 34), -77, dtype=torch.int16, device="cuda")
    dv, rv = dwide[:, 1:1 + H, 4:4 + W], rwide[:, 2:2 + H, 21:21 + W]
    if matcher == "sgbm":
        cp = L.SgbmParams(*(int(getattr(p, n)) for n, _ in L.SgbmParams._fields_))
        fn = L.load().amhip_sgbm_disparity_batch_dev
    else:
        cp = L.BmParams(*(int(getattr(p, n)) for n, _ in L.BmParams._fields_))
        fn = L.load().amhip_bm_disparity_batch_dev
    gmap.wait_for_torch(lt)
    L.check(fn(gmap.handle, C.byref(cp), W, H, nb,
               C.c_void_p(lt.data_ptr()), lt.stride(1), lt.stride(0),
               C.c_void_p(rt.data_ptr()), rt.stride(1), rt.stride(0),
               C.c_void_p(mt.data_ptr()), mt.stride(1), mt.stride(0),
               C.c_void_p(dv.data_ptr()), dv.stride(1) * 4, dv.stride(0) * 4,
               C.c_void_p(rv.data_ptr()), rv.stride(1) * 2, rv.stride(0) * 2))
    gmap.synchronize()
    d, r = dwide.cpu().numpy(), rwide.cpu().numpy()
    same((d[:, 1:1 + H, 4:4 + W], r[:, 2:2 + H, 21:21 + W]), want)
    keep_d, keep_r = np.ones(d.shape, bool), np.ones(r.shape, bool)
    keep_d[:, 1:1 + H, 4:4 + W] = False
    keep_r[:, 2:2 + H, 21:21 + W] = False
    assert (d[keep_d] == -7.0).all() and (r[keep_r] == -77).all()
    # the same through the Python wrapper's padded input views
    same(run_batch(gmap, matcher, lefts, rights, p, masks, pads=(1, 63, 7), gaps=(2, 0, 5)), want)


# ---- 5. masks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_masks_that_differ_per_pair_and_no_mask(gmap, matcher):
    W, H, D = SB.SHAPES[0]
    p = SB.params(matcher, D, 100)
    lefts, rights = three_pairs(W, H, D)
    rng = np.random.default_rng(8)
    masks = rng.choice(np.array([0, 1, 128, 255], np.uint8), lefts.shape)
    masks[1] = 0
    masks[2, :, :W // 2] = 255
    want = SB.restate_each(matcher, lefts, rights, p, masks)
    got = run_batch(gmap, matcher, lefts, rights, p, masks)
    same(got, want)
    assert (got[0][1] == 1.0).all() and (got[0][0] != 1.0).any()
    same(run_batch(gmap, matcher, lefts, rights, p, None), SB.restate_each(matcher, lefts, rights, p))


# ---- 6. mixed calls on one context ----------------------------------------------------------------
def test_batched_and_one_pair_calls_share_one_context():
    """The scratch grows to the batch and is shared by both matchers and by the one-pair calls: batched
    SGBM (4 pairs), one BM pair, batched BM (2), one SGBM pair, on a fresh context."""
    A = _A()
    W, H, D = SB.SHAPES[1]
    l4, r4 = SB.noise_stack(W, H, "half", nb=4)
    sp, bp = SB.params("sgbm", D, 100), SB.params("bm", D, 100)
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        same(run_batch(m, "sgbm", l4, r4, sp), SB.restate_each("sgbm", l4, r4, sp), "batched SGBM")
        same(run_each(m, "bm", l4[3:], r4[3:], bp), SB.restate_each("bm", l4[3:], r4[3:], bp), "one BM pair")
        same(run_batch(m, "bm", l4[:2], r4[:2], bp), SB.restate_each("bm", l4[:2], r4[:2], bp), "batched BM")
        same(run_each(m, "sgbm", l4[2:3], r4[2:3], sp), SB.restate_each("sgbm", l4[2:3], r4[2:3], sp),
             "one SGBM pair")


def test_python_wrapper_refuses_a_batch_of_17(gmap):
    import torch
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    z = torch.zeros((17, 48, 80), dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AmhipError) as ei:
        A.compute_disparity_bm(gmap, z, z)
    assert ei.value.status == L.ERR_ARG and "batch" in str(ei.value)


# ---- 7. Stereo with n pairs in flight --------------------------------------------------------------
SEQ = dict(F=7, W=160, H=120)
_seq = []


def the_seq():
    if not _seq:
        _seq.append(SS.Sequence(SEQ["F"], SEQ["W"], SEQ["H"]))
    return _seq[0]


def ncam(seq, distortion=0, dist=(0.0, 0.0, 0.0, 0.0)):
    K = seq.K
    return _A().NCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], seq.W, seq.H, distortion, dist, seq.T_C_B)


def make(gmap, seq, use_bm, nth=1, n=1, undistort=False, distortion=0, dist=(0.0, 0.0, 0.0, 0.0)):
    A = _A()
    return A.Stereo(ncam(seq, distortion, dist),
                    A.StereoSettings(use_every_nth_image=nth, images_need_undistortion=undistort),
                    A.BlockMatchingParameters(use_BM=use_bm), gmap, pairs_in_flight=n)


def snapshot(st, got):
    """(xyz bits, intensities, pairs, payload) as host copies"""
    return (got[0].cpu().numpy().copy().view(np.uint64), got[1].cpu().numpy().copy(), st.pairs,
            st.point_cloud2().cpu().numpy().copy())


def assert_same_run(a, b, what=""):
    assert a[2] == b[2], (what, a[2], b[2])
    assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]), what
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[3], b[3]), what + ": PointCloud2 payload"


def expected(seq, nth, use_bm):
    return SB.cpu_chain(seq, SS.pairs_of(seq.F, nth), use_bm, key=("batch", seq.F, seq.W, seq.H, nth, use_bm))


@pytest.mark.parametrize("nth", [1, 2])
@pytest.mark.parametrize("use_bm", [True, False])
def test_add_frames_with_pairs_in_flight(gmap, use_bm, nth):
    import torch
    seq = the_seq()
    want_xyz, want_i, ns, _ = expected(seq, nth, use_bm)
    assert len(ns) == len(SS.pairs_of(seq.F, nth)) and min(ns) > 0.25 * seq.W * seq.H
    host_frames = [f for f in seq.frames]
    dev_frames = torch.from_numpy(seq.frames).cuda()
    base = None
    for n in (1, 2, 3, 8):
        with make(gmap, seq, use_bm, nth=nth, n=n) as st:
            assert st.pairs_in_flight == n
            for what, frames in (("host", host_frames), ("device", dev_frames)):
                run = snapshot(st, st.add_frames(seq.T_G_B, frames))
                tag = "n = %d, %s frames" % (n, what)
                assert run[2] == len(ns), tag
                assert np.array_equal(run[0], np.ascontiguousarray(want_xyz).view(np.uint64)), tag
                assert np.array_equal(run[1], want_i), tag
                if base is None:
                    base = run
                assert_same_run(run, base, tag)
                st.reset()
            # reset, then a second sequence: the same bits again
            assert_same_run(snapshot(st, st.add_frames(seq.T_G_B, dev_frames)), base, "n = %d after reset" % n)


def test_one_matcher_call_per_group(gmap):
    seq = the_seq()
    # six pairs: six groups of one at n = 1; a group of four and a group of two at n = 4
    for n, calls in ((1, 6), (4, 2)):
        with make(gmap, seq, True, n=n) as st:
            gmap.enable_timing(True)
            gmap.timing_reset()
            st.add_frames(seq.T_G_B, [f for f in seq.frames])
            times = gmap.kernel_times()
            gmap.enable_timing(False)
            assert st.pairs == 6
        assert times["k_stereo"][1] == calls, n


def test_undistortion_with_pairs_in_flight(gmap):
    import oracle_ffi as O
    from test_gpu_stereo_sequence import oracle_undistort
    distortion, dist = O.DIST_RADTAN, (-0.25, 0.06, 3e-4, -2e-4)
    seq = SS.Sequence(5, 160, 120, distortion=(distortion, dist))
    cam = O.Camera()
    cam.fu, cam.fv, cam.cu, cam.cv = seq.K[0, 0], seq.K[1, 1], seq.K[0, 2], seq.K[1, 2]
    cam.width, cam.height, cam.distortion = seq.W, seq.H, distortion
    for k in range(4):
        cam.dist[k] = dist[k]
    und = oracle_undistort(cam, seq.frames)
    want_xyz, want_i, ns, _ = SB.cpu_chain(seq, SS.pairs_of(5, 1), True, frames=und)
    runs = []
    for n in (1, 3):
        with make(gmap, seq, True, n=n, undistort=True, distortion=distortion, dist=dist) as st:
            runs.append(snapshot(st, st.add_frames(seq.T_G_B, [f for f in seq.frames])))
    assert runs[0][2] == 4 and np.array_equal(runs[0][0], np.ascontiguousarray(want_xyz).view(np.uint64))
    assert np.array_equal(runs[0][1], want_i)
    assert_same_run(runs[1], runs[0], "undistorted, n = 3")


def test_add_frame_is_unaffected_and_a_carried_frame_is_kept(gmap):
    import torch
    seq = the_seq()
    dev = torch.from_numpy(seq.frames).cuda()
    with make(gmap, seq, True) as a, make(gmap, seq, True) as b:
        b.set_pairs_in_flight(4)
        for k in range(4):
            ra = snapshot(a, a.add_frame(seq.T_G_B[k], seq.frames[k]))
            rb = snapshot(b, b.add_frame(seq.T_G_B[k], seq.frames[k]))
            assert ra[2] == (1 if k else 0)
            assert_same_run(rb, ra, "add_frame %d" % k)
        # frame 3 is carried over: it pairs with the first frame of the next call, in both objects
        ra = snapshot(a, a.add_frames(seq.T_G_B[4:], dev[4:]))
        rb = snapshot(b, b.add_frames(seq.T_G_B[4:], dev[4:]))
        assert ra[2] == 3
        assert_same_run(rb, ra, "carry-over into a group")
        # growing n while a frame is carried keeps that frame
        b.set_pairs_in_flight(8)
        ra = snapshot(a, a.add_frames(seq.T_G_B[:5], dev[:5]))
        rb = snapshot(b, b.add_frames(seq.T_G_B[:5], dev[:5]))
        assert ra[2] == 5
        assert_same_run(rb, ra, "after growing n")
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    with make(gmap, seq, True) as st:
        for bad in (0, 17):
            with pytest.raises(A.AmhipError) as ei:
                st.set_pairs_in_flight(bad)
            assert ei.value.status == L.ERR_ARG and st.pairs_in_flight == 1


# ---- 8. a failing pair inside a group -------------------------------------------------------------
@pytest.mark.parametrize("use_bm", [True, False])
def test_zero_baseline_pair_cuts_its_group(gmap, use_bm):
    """Frames 2 and 3 at one position: the third pair of the sequence, inside the first group of four.
    The two pairs before it are kept and the call fails as it does pair after pair."""
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    seq = the_seq()
    want_xyz, want_i, ns, _ = expected(seq, 1, use_bm)
    T = seq.T_G_B.copy()
    T[3] = T[2]
    seen = []
    for n in (1, 4):
        with make(gmap, seq, use_bm, n=n) as st:
            with pytest.raises(A.AmhipError) as ei:
                st.add_frames(T, [f for f in seq.frames])
            assert ei.value.status == L.ERR_ARG
            num, pairs = C.c_size_t(), C.c_size_t()
            xyz, inten = C.c_void_p(), C.c_void_p()
            assert L.load().amhip_stereo_cloud(st._h, C.byref(xyz), C.byref(inten), C.byref(num),
                                               C.byref(pairs)) == L.OK
            assert pairs.value == 2 and num.value == ns[0] + ns[1]
            seen.append((str(ei.value), snapshot(st, st._cloud())))
            # the object recovers after a reset
            st.reset()
            run = snapshot(st, st.add_frames(seq.T_G_B, [f for f in seq.frames]))
            assert run[2] == 6 and np.array_equal(run[0], np.ascontiguousarray(want_xyz).view(np.uint64))
    assert seen[0][0] == seen[1][0] and "baseline" in seen[0][0]
    assert np.array_equal(seen[1][1][0], np.ascontiguousarray(want_xyz[:ns[0] + ns[1]]).view(np.uint64))
    assert_same_run(seen[1][1], seen[0][1], "the pairs before the failing one")


# ---- 9. groups at their edges -----------------------------------------------------------------------
def chain_prefix(want, pairs):
    """the first `pairs` pairs of a chain as (xyz bits, intensities)"""
    k = sum(want[2][:pairs])
    return np.ascontiguousarray(want[0][:k]).view(np.uint64), want[1][:k]


def assert_prefix(run, want, pairs, what):
    xyz, inten = chain_prefix(want, pairs)
    assert run[2] == pairs, (what, run[2])
    assert run[0].shape == xyz.shape and np.array_equal(run[0], xyz), what
    assert np.array_equal(run[1], inten), what


def cloud_counts(st):
    from aerial_mapper_amd import hip_lib as L
    num, pairs = C.c_size_t(), C.c_size_t()
    xyz, inten = C.c_void_p(), C.c_void_p()
    assert L.load().amhip_stereo_cloud(st._h, C.byref(xyz), C.byref(inten), C.byref(num), C.byref(pairs)) == L.OK
    return pairs.value, num.value


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("use_bm", [True, False])
def test_one_frame_then_one_more(gmap, use_bm, n):
    """A call with one frame: no pair, an empty cloud.  The next call's single frame pairs with the
    carried one: at n = 4 a carried frame plus a group of one."""
    seq = the_seq()
    want = expected(seq, 1, use_bm)
    with make(gmap, seq, use_bm, n=n) as st:
        run = snapshot(st, st.add_frames(seq.T_G_B[:1], [seq.frames[0]]))
        assert run[2] == 0 and run[0].shape[0] == 0 and run[1].shape[0] == 0
        assert cloud_counts(st) == (0, 0)
        assert_prefix(snapshot(st, st.add_frames(seq.T_G_B[1:2], [seq.frames[1]])), want, 1, "pair (0, 1)")


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("use_bm", [True, False])
def test_a_full_group_and_a_full_group_plus_one(gmap, use_bm, n):
    seq = the_seq()
    want = expected(seq, 1, use_bm)
    with make(gmap, seq, use_bm, n=n) as st:
        for F in (n + 1, n + 2):
            run = snapshot(st, st.add_frames(seq.T_G_B[:F], [f for f in seq.frames[:F]]))
            assert_prefix(run, want, F - 1, "%d frames at n = %d" % (F, n))
            st.reset()


@pytest.mark.parametrize("use_bm", [True, False])
def test_refused_first_pair_of_a_call(gmap, use_bm):
    """Frames 0 and 1 at one position: no pair goes through, the object recovers after a reset."""
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    seq = the_seq()
    want = expected(seq, 1, use_bm)
    T = seq.T_G_B.copy()
    T[1] = T[0]
    texts = []
    for n in (1, 4):
        with make(gmap, seq, use_bm, n=n) as st:
            with pytest.raises(A.AmhipError) as ei:
                st.add_frames(T, [f for f in seq.frames])
            assert ei.value.status == L.ERR_ARG
            texts.append(str(ei.value))
            assert cloud_counts(st) == (0, 0)
            st.reset()
            assert_prefix(snapshot(st, st.add_frames(seq.T_G_B, [f for f in seq.frames])), want, 6,
                          "after the reset, n = %d" % n)
    assert "CHECK_NE(baseline, 0.0) (densifier.cpp:39): both frames have the same position" in texts[0]
    assert texts[0] == texts[1]


@pytest.mark.parametrize("use_bm", [True, False])
def test_baseline_that_underflows_to_zero(gmap, use_bm):
    """Frames 2 and 3 differ by 1e-200 in x: unequal positions whose squared distance underflows, so
    the rectifier's baseline is exactly 0.0 -- the refusal that is not "same position".  The camera
    poses are the sequence's own, moved so that frame 2 sits at x = 0, with an identity T_C_B (the
    composed positions are then the given ones)."""
    import copy
    import oracle_ffi as O
    A = _A()
    from aerial_mapper_amd import hip_lib as L
    seq = copy.copy(the_seq())
    T = O.compose_T_G_C(seq.T_G_B, seq.T_C_B)
    T[:, 0] -= T[2, 0]
    T[3] = T[2]
    T[3, 0] = 1e-200
    seq.T_G_B, seq.T_C_B = T, np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    ts = seq.camera_poses()[1]
    d = ts[3] - ts[2]
    assert not np.array_equal(ts[3], ts[2]) and np.sqrt((d * d).sum()) == 0.0
    want = SB.cpu_chain(seq, [(0, 1), (1, 2)], use_bm, key=("underflow", use_bm))
    seen = []
    for n in (1, 4):
        with make(gmap, seq, use_bm, n=n) as st:
            with pytest.raises(A.AmhipError) as ei:
                st.add_frames(seq.T_G_B, [f for f in seq.frames])
            assert ei.value.status == L.ERR_ARG
            assert cloud_counts(st) == (2, want[2][0] + want[2][1])
            seen.append((str(ei.value), snapshot(st, st._cloud())))
            assert_prefix(seen[-1][1], want, 2, "the pairs before the refused one, n = %d" % n)
    assert "CHECK_NE(baseline, 0.0) (densifier.cpp:39)" in seen[0][0] and "same position" not in seen[0][0]
    assert seen[0][0] == seen[1][0]
    assert_same_run(seen[1][1], seen[0][1], "n = 4 against n = 1")
