"""GPU: the blended backward-grid mosaic (OrthoSettings(blend=True), amhip_*ortho_backward_process_blend*,
k_ortho_blend_backward) against the rule's numpy statement
(tests/ortho_blend_reference.py), all five layers bit for bit unless stated otherwise, on the scenes
of tests/ortho_blend_scenes.py: the 80 x 72-cell map of the occlusion tests -- two tiles each way,
the second ones partial -- under its 96 x 54 camera, five frames of high-frequency noise."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
import ortho_blend_reference as B
import ortho_blend_scenes as BS
import ortho_occlusion_reference as R
import ortho_occlusion_scenes as SC
import scenarios as S
from aerial_mapper_amd import synth

pytestmark = pytest.mark.gpu

LAYERS = B.LAYERS
ALL = tuple(range(BS.F_MAIN))


def _settings(A):
    g = SC.grid()
    return A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)


def _ncam(A, cam):
    return A.NCamera(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height, cam.distortion,
                     tuple(cam.dist))


def _ortho_settings(A, colored, sharpness, occl, blend=True):
    return A.OrthoSettings(colored_ortho=colored, blend=blend, blend_sharpness=sharpness,
                           occlusion_test=occl, occlusion_margin_m=SC.MARGIN if occl else 0.0)


def run_gpu(calls, colored=False, sharpness=2, occl=False, elev="block", kind="none", device=False,
            blend=True, poses=None, frames=None, reset_after=None):
    """calls: tuples of frame indices, folded one after the other into one map; an entry may be
    (indices, colored) to switch between gray and colour.  blend False: the plain or the
    occlusion-tested mosaic.  reset_after: AerialGridMap.reset() after that many calls (the
    elevation is set again).  Returns the layers."""
    import aerial_mapper_amd as A
    poses = BS.main_poses() if poses is None else poses
    z = BS.elevation(elev) if isinstance(elev, str) else elev
    with A.AerialGridMap(_settings(A)) as m:
        m.set("elevation", z)
        for n, call in enumerate(calls):
            idx, col = call if len(call) == 2 and isinstance(call[1], bool) else (call, colored)
            fr = (BS.frames(col) if frames is None else frames)
            mosaic = A.OrthoBackwardGrid(_ncam(A, BS.camera(kind)), _ortho_settings(A, col, sharpness, occl, blend), m)
            images = [fr[f] for f in idx]
            if device:
                import torch
                images = torch.from_numpy(np.stack(images)).cuda()
            mosaic.process(poses[list(idx)], images, m)
            if reset_after is not None and n + 1 == reset_after:
                m.reset()
                m.set("elevation", z)
        return {n: m.get(n) for n in LAYERS}


# ---- 1. the main scene ----------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
@pytest.mark.parametrize("sharpness", [0, 2, 4])
def test_main_scene_matches_the_reference(sharpness, colored, device):
    want, count = BS.expected(colored=colored, sharpness=sharpness)
    assert (count >= 3).mean() >= 0.5   # not a one-view scene
    S.assert_layers_equal(run_gpu([ALL], colored, sharpness, device=device), want, LAYERS)


# ---- 2. the three other layers are the existing modes' ------------------------------------------
@pytest.mark.parametrize("occl", [False, True], ids=["plain", "occlusion"])
def test_the_fold_layers_are_the_unblended_mosaics(occl):
    rest = ["elevation_angle", "observation_index", "num_observations"]
    for calls in ([ALL], [(1, 2), (0, 3, 4)]):   # (the second call is incremental)
        blended = run_gpu(calls, occl=occl)
        unblended = run_gpu(calls, occl=occl, blend=False)
        S.assert_layers_equal(blended, unblended, rest)
        assert not np.array_equal(blended["ortho"], unblended["ortho"], equal_nan=True)


# ---- 3. one frame per call ------------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_one_frame_gives_the_plain_mosaic(colored):
    for f in (0, 1, 4):
        S.assert_layers_equal(run_gpu([(f,)], colored), run_gpu([(f,)], colored, blend=False), LAYERS)


# ---- 4. ties round to even ------------------------------------------------------------------------
@pytest.mark.parametrize("values, want", [((10, 11), 10.0), ((11, 12), 12.0)])
def test_ties_round_to_even(values, want):
    """Two frames share one pose straight above cell (I0, J0): cx = cy = 0 there, so w = 1 exactly
    and the cell is the mean of the two constants, half-way between two integers."""
    x, y = SC.cell_xy(SC.I0, SC.J0)
    pose = np.array([x, y, 8.0, 0.0, 1.0, 0.0, 0.0])   # level, looking straight down
    poses = np.stack([pose, pose])
    z = np.zeros((SC.COLS, SC.ROWS), np.float32)
    fr = [np.full((54, 96), v, np.uint8) for v in values]
    g, cam = SC.grid(), BS.camera()
    pairs = B.probe(g, cam, O.compose_T_G_C(poses, synth.IDENTITY_POSE), z)
    assert np.array_equal(pairs["C"][:, SC.J0, SC.I0], [[0.0, 0.0, 8.0]] * 2)
    lay = SC.fresh_layers(z)
    count = B.process(cam, pairs, fr, lay, B.new_sums(g, False), False, 2)
    assert count[SC.J0, SC.I0] == 2 and lay["ortho"][SC.J0, SC.I0] == want
    got = run_gpu([(0, 1)], elev=z, poses=poses, frames=fr)
    S.assert_layers_equal(got, lay, LAYERS)
    assert got["ortho"][SC.J0, SC.I0] == want


# ---- 5. split equals whole ------------------------------------------------------------------------
def _shift_index(whole, first_frames):
    """observation_index counts within a call: the whole call's layer as the split run leaves it."""
    idx = whole["observation_index"]
    second = idx >= first_frames
    assert second.sum() > 50 and (idx < first_frames).sum() > 50
    out = dict(whole)
    out["observation_index"] = np.where(second, idx - np.float32(first_frames), idx)
    return out


@pytest.mark.parametrize("occl", [False, True], ids=["plain", "occlusion"])
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_split_equals_whole(colored, occl):
    split = run_gpu([(0, 1), (2, 3, 4)], colored, occl=occl)
    want, _ = BS.expected(colored=colored, occl=occl, calls=[(0, 1), (2, 3, 4)])
    S.assert_layers_equal(split, want, LAYERS)
    # and the layers of one call of all five (only observation_index, which counts within a call,
    # names the second call's winners differently)
    whole = run_gpu([ALL], colored, occl=occl)
    S.assert_layers_equal(split, _shift_index(whole, 2), LAYERS)


@pytest.mark.parametrize("order", [(False, True), (True, False)], ids=["gray-colour", "colour-gray"])
def test_gray_and_colour_keep_sums_of_their_own(order):
    """gray 0..1, colour 0..1, gray 2..4, colour 2..4 on one map (and the other order): the
    reference runs the same four calls, and each output layer is that of its own two calls."""
    a, b = order
    calls = [((0, 1), a), ((0, 1), b), ((2, 3, 4), a), ((2, 3, 4), b)]
    got = run_gpu(calls)
    g = SC.grid()
    lay = SC.fresh_layers(BS.elevation("block"))
    sums = {False: B.new_sums(g, False), True: B.new_sums(g, True)}
    for idx, col in calls:
        B.process(BS.camera(), BS.pairs(), BS.frames(col), lay, sums[col], col, 2, None, idx)
    S.assert_layers_equal(got, lay, LAYERS)
    # each kind's second call continued its own sums: both output layers are a split run's
    for col in (False, True):
        n = "colored_ortho" if col else "ortho"
        want, _ = BS.expected(colored=col, calls=[(0, 1), (2, 3, 4)])
        S.assert_layers_equal(got, want, [n])


# ---- 6. restart -----------------------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_a_reset_map_restarts_the_sums(colored):
    want, _ = BS.expected(colored=colored)
    # (another sharpness and other frames first: nothing of those sums may leak)
    got = run_gpu([(1, 2, 3), ALL], colored, reset_after=1)
    S.assert_layers_equal(got, want, LAYERS)


@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_host_session_restarts_on_initial_layers(colored):
    import aerial_mapper_amd as A
    want, _ = BS.expected(colored=colored)
    poses, fr = BS.main_poses(), BS.frames(colored)
    st = _ortho_settings(A, colored, 2, False)
    with A.HostSession(_settings(A)) as hs:
        hs.layers["elevation"][...] = BS.elevation("block")
        hs.ortho_process(_ncam(A, BS.camera()), st, poses[1:4], fr[1:4])
        assert not np.isnan(hs.layers["observation_index"]).all()
        for n, v in O.new_layers(SC.grid()).items():
            if n != "elevation":
                hs.layers[n][...] = v
        hs.ortho_process(_ncam(A, BS.camera()), st, poses, fr)
        S.assert_layers_equal(hs.layers, want, LAYERS)
        # and the next call continues: the same frames again double both sums -- the same means
        hs.ortho_process(_ncam(A, BS.camera()), st, poses, fr)
        again, _ = BS.expected(colored=colored, calls=[ALL, ALL])
        S.assert_layers_equal(hs.layers, again, LAYERS)


# ---- 7. occlusion on ------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_occlusion_on_matches_the_reference(colored, device):
    want, count = BS.expected(colored=colored, occl=True)
    assert (count >= 3).mean() >= 0.5
    # the oblique frame contributes nothing to the ground the block hides from it, whether it
    # loses the fold there or not: the result differs from the blend without the test there
    hidden = BS.pairs()["visible"][0] & BS.occluded()[0]
    free, _ = BS.expected(colored=colored, occl=False)
    n = "colored_ortho" if colored else "ortho"
    assert hidden.sum() >= 50 and (want[n][hidden].view(np.uint32) != free[n][hidden].view(np.uint32)).sum() >= 25
    assert (free["observation_index"][hidden] == 0).all()   # (without the test it wins all of it)
    # ... and the nadir-ish frame is hidden beside the block's walls, where it loses the fold anyway
    loses = BS.pairs()["visible"][1] & BS.occluded()[1] & (free["observation_index"] != 1)
    assert loses.sum() >= 50 and (want[n][loses].view(np.uint32) != free[n][loses].view(np.uint32)).sum() >= 25
    S.assert_layers_equal(run_gpu([ALL], colored, occl=True, device=device), want, LAYERS)


def test_occlusion_on_nan_elevation():
    want, _ = BS.expected(elev="nan", occl=True, nframes=2)
    got = run_gpu([(0, 1)], occl=True, elev="nan")
    S.assert_layers_equal(got, want, LAYERS)
    holes = np.isnan(BS.elevation("nan"))
    init = O.new_layers(SC.grid())
    for n in LAYERS:   # NaN cells stay initial
        assert np.array_equal(got[n][holes], init[n][holes], equal_nan=True), n
    # NaN samples do not occlude: rays cross holes and go on (on the reference)
    why, crossed = [], 0
    for j in range(0, SC.COLS, 3):
        for i in range(0, SC.ROWS, 3):
            R.occluded(BS.elevation("nan"), SC.grid(), i, j, BS.T_G_C()[0, 0:3], SC.MARGIN, why)
            crossed += why[1] >= 8
    assert crossed > 100
    # every elevation NaN: every layer stays initial
    got = run_gpu([(0, 1)], occl=True, elev=np.full((SC.COLS, SC.ROWS), np.nan, np.float32))
    S.assert_layers_equal(got, init, LAYERS)


# ---- 8. distortion models -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["radtan", "equidistant"])
def test_distortion_models(kind):
    want, count = BS.expected(kind=kind)
    assert (count >= 3).mean() >= 0.5
    S.assert_layers_equal(run_gpu([ALL], kind=kind), want, LAYERS)


# ---- 9. more frames than one list holds -----------------------------------------------------------
def test_more_frames_than_one_frame_list_holds():
    """1100 frames -- the five poses repeated with small offsets --: beyond 1024 the kernel culls and
    folds chunk by chunk, per slab, and the sums run on across the chunks.  On the 6 x 6 cells
    around the tile corner the reference decides; the rest of the map is compared between two runs."""
    F = 1100
    rng = np.random.Generator(np.random.PCG64(91))
    poses = BS.main_poses()[np.arange(F) % BS.F_MAIN].copy()
    poses[:, 0:3] += rng.uniform(-1.5, 1.5, size=(F, 3))
    fr = SC.frames(F)
    g, cam, z = SC.grid(), BS.camera(), BS.elevation("block")
    cells = np.zeros((SC.COLS, SC.ROWS), bool)
    cells[61:67, 61:67] = True
    pairs = B.probe(g, cam, O.compose_T_G_C(poses, synth.IDENTITY_POSE), z, cells)
    want = SC.fresh_layers(z)
    count = B.process(cam, pairs, fr, want, B.new_sums(g, False), False, 2)
    assert count[cells].min() > 1024 // 2 and (pairs["visible"][1024:][:, cells].sum(axis=0) > 10).all()
    calls = [tuple(range(F))]
    a = run_gpu(calls, poses=poses, frames=fr)
    for n in LAYERS:
        assert np.array_equal(a[n][cells].view(np.uint32), want[n][cells].view(np.uint32)), n
    b = run_gpu(calls, poses=poses, frames=fr)
    for n in LAYERS:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n
    assert (~np.isnan(a["observation_index"])).mean() > 0.9


# ---- 10. two runs, same bits ----------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    a = run_gpu([(0, 1), (2, 3, 4)], True, 3, occl=True, elev="nan")
    b = run_gpu([(0, 1), (2, 3, 4)], True, 3, occl=True, elev="nan")
    for n in LAYERS:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


# ---- 11. several windows --------------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_a_two_window_session_gives_the_one_window_layers(colored):
    import aerial_mapper_amd as A
    poses, fr = BS.main_poses(), BS.frames(colored)
    st = _ortho_settings(A, colored, 2, False)
    got = {}
    for tiles in ((1, 1), (2, 1)):
        with A.HostSession(_settings(A), tiles=tiles) as hs:
            assert hs.num_windows == tiles[0] * tiles[1]
            hs.layers["elevation"][...] = BS.elevation("block")
            hs.ortho_process(_ncam(A, BS.camera()), st, poses[0:2], fr[0:2])
            hs.ortho_process(_ncam(A, BS.camera()), st, poses[2:5], fr[2:5])
            got[tiles] = {n: hs.layers[n].copy() for n in LAYERS}
    S.assert_layers_equal(got[(2, 1)], got[(1, 1)], LAYERS)
    want, _ = BS.expected(colored=colored, calls=[(0, 1), (2, 3, 4)])
    S.assert_layers_equal(got[(2, 1)], want, LAYERS)


def test_a_window_context_runs_it_without_the_occlusion_test():
    import aerial_mapper_amd as A
    want, _ = BS.expected()
    with A.AerialGridMap(_settings(A), window=(0, 0, 64, SC.COLS)) as m:
        m.set("elevation", BS.elevation("block")[:, 0:64])
        A.OrthoBackwardGrid(_ncam(A, BS.camera()), _ortho_settings(A, False, 2, False), m).process(
            BS.main_poses(), BS.frames(), m)
        S.assert_layers_equal({n: m.get(n) for n in LAYERS}, {n: want[n][:, 0:64] for n in LAYERS}, LAYERS)


# ---- 12. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_layers_untouched():
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    cam, z = BS.camera(), BS.elevation("block")
    poses, fr = BS.main_poses(), BS.frames()
    init = O.new_layers(SC.grid())
    ncam = _ncam(A, cam)

    def refused(call, *words):
        with pytest.raises(L.AmhipError) as e:
            call()
        assert e.value.status == L.ERR_ARG, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    def both(m, st, *words):   # host frames and device frames
        import torch
        refused(lambda: A.OrthoBackwardGrid(ncam, st, m).process(poses, fr, m), *words)
        refused(lambda: A.OrthoBackwardGrid(ncam, st, m).process(poses, torch.from_numpy(np.stack(fr)).cuda(), m),
                *words)

    with A.AerialGridMap(_settings(A)) as m:
        m.set("elevation", z)
        for bad in (-1, 5):
            both(m, A.OrthoSettings(blend=True, blend_sharpness=bad), "sharpness")
        for bad in (-0.5, -float("inf"), float("nan")):
            both(m, A.OrthoSettings(blend=True, occlusion_test=True, occlusion_margin_m=bad), "margin")
        # null options, straight through the C ABI
        T = np.ascontiguousarray(O.compose_T_G_C(poses, synth.IDENTITY_POSE))
        f64p = C.POINTER(C.c_double)
        ptrs = (C.c_void_p * len(fr))(*[im.ctypes.data for im in fr])
        steps = (C.c_size_t * len(fr))(*[im.strides[0] for im in fr])
        assert lib.amhip_ortho_backward_process_blend(m.handle, C.byref(ncam.camera), T.ctypes.data_as(f64p),
                                                      len(fr), ptrs, steps, 1, 0, None, None, None, None, None,
                                                      None, None) == L.ERR_ARG
        assert b"null options" in lib.amhip_last_error()
        assert lib.amhip_ortho_backward_process_blend_dev(m.handle, C.byref(ncam.camera), T.ctypes.data_as(f64p),
                                                          len(fr), C.c_void_p(16), 96 * 54, 96, 1, 0,
                                                          None) == L.ERR_ARG
        for n in LAYERS:   # nothing was written
            assert np.array_equal(m.get(n), init[n], equal_nan=True), n
    # a context that holds a window of the map: refused with the occlusion test only
    on = A.OrthoSettings(blend=True, occlusion_test=True, occlusion_margin_m=SC.MARGIN)
    with A.AerialGridMap(_settings(A), window=(0, 0, 64, SC.COLS)) as m:
        m.set("elevation", z[:, 0:64])
        both(m, on, "window", "halo")
        for n in LAYERS:
            assert np.array_equal(m.get(n), init[n][:, 0:64], equal_nan=True), n
    # a session of two windows: the same; bad options are refused whatever the windows
    with A.HostSession(_settings(A), tiles=(2, 1)) as hs:
        hs.layers["elevation"][...] = z
        refused(lambda: hs.ortho_process(ncam, on, poses, fr), "window", "halo")
        refused(lambda: hs.ortho_process(ncam, A.OrthoSettings(blend=True, blend_sharpness=7), poses, fr), "sharpness")
        refused(lambda: hs.ortho_process(ncam, A.OrthoSettings(blend=True, occlusion_test=True,
                                                               occlusion_margin_m=-1.0), poses, fr), "margin")
        for n in LAYERS:
            assert np.array_equal(hs.layers[n], init[n], equal_nan=True), n
    with A.HostSession(_settings(A)) as hs:   # one window: the occlusion test runs
        hs.layers["elevation"][...] = z
        hs.ortho_process(ncam, on, poses, fr)
        want, _ = BS.expected(occl=True)
        S.assert_layers_equal(hs.layers, want, LAYERS)
