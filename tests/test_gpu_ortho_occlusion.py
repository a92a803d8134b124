"""GPU: the occlusion-tested backward-grid mosaic ("true ortho": OrthoSettings(occlusion_test=True),
amhip_ortho_backward_process_occl*, k_ortho_occl_backward) against the rule's numpy statement
(tests/ortho_occlusion_reference.py), bit for bit, on the scenes of tests/ortho_occlusion_scenes.py:
an 80 x 72-cell map -- two tiles each way, the second ones partial, rays crossing the borders --
under a 96 x 54 camera and frames of high-frequency noise."""
import numpy as np
import pytest

import oracle_ffi as O
import ortho_occlusion_reference as R
import ortho_occlusion_scenes as SC
import scenarios as S
from aerial_mapper_amd import synth

pytestmark = pytest.mark.gpu

LAYERS = R.LAYERS
INF = float("inf")


def _settings(A):
    g = SC.grid()
    return A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)


def _ncam(A, cam):
    return A.NCamera(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height, cam.distortion,
                     tuple(cam.dist))


def run_gpu(cam, elevation, calls, colored=False, margin=SC.MARGIN, device=False, reset_first=False):
    """calls: list of (poses, frames), folded one after the other into one map.
    margin None: the plain mosaic.  device: the frames as one CUDA tensor.  reset_first: a first
    call, then AerialGridMap.reset() -- the layers are lazily initial when the calls begin."""
    import aerial_mapper_amd as A
    with A.AerialGridMap(_settings(A)) as m:
        assert (m.rows, m.cols) == (SC.ROWS, SC.COLS)
        st = A.OrthoSettings(colored_ortho=colored, occlusion_test=margin is not None,
                             occlusion_margin_m=0.0 if margin is None else margin)
        mosaic = A.OrthoBackwardGrid(_ncam(A, cam), st, m)
        if reset_first:
            m.set("elevation", elevation)
            mosaic.process(calls[0][0], calls[0][1], m)
            m.reset()
        m.set("elevation", elevation)
        for poses, frames in calls:
            if device:
                import torch
                frames = torch.from_numpy(np.stack(frames)).cuda()
            mosaic.process(poses, frames, m)
        return {n: m.get(n) for n in LAYERS}


# ---- 1. nothing occludes => the plain mosaic --------------------------------------------------
CAMERAS = {"none": (O.DIST_NONE, (0.0, 0.0, 0.0, 0.0)),
           "radtan": (O.DIST_RADTAN, (-0.25, 0.06, 3e-4, -2e-4)),
           "equidistant": (O.DIST_EQUIDISTANT, (-0.02, 0.004, -0.001, 0.0002))}


def _rough_elevation():
    rng = np.random.Generator(np.random.PCG64(21))
    z = rng.uniform(0.0, 3.0, size=(SC.COLS, SC.ROWS)).astype(np.float32)
    z[SC.BLOCK_J, SC.BLOCK_I] += np.float32(SC.BLOCK_HEIGHT)
    z[10:14, 30:50] += np.float32(7.0)
    z[rng.uniform(size=z.shape) < 0.02] = np.nan
    return z


@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
@pytest.mark.parametrize("kind", sorted(CAMERAS))
def test_infinite_margin_gives_the_plain_mosaic(kind, colored):
    cam = SC.camera(*CAMERAS[kind])
    z = _rough_elevation()
    poses = np.concatenate([SC.block_poses(), synth.make_lawnmower_poses(2, 8.0, 60.0, 5, tilt_deg=4.0)])
    fr = SC.frames(4, colored)
    first, second = (poses[0:3], fr[0:3]), (poses[1:4], fr[1:4])   # the second call is incremental
    for device in (False, True):
        plain = run_gpu(cam, z, [first], colored, None, device)
        assert (~np.isnan(plain["observation_index"])).mean() > 0.5
        S.assert_layers_equal(run_gpu(cam, z, [first], colored, INF, device), plain, LAYERS)
        plain2 = run_gpu(cam, z, [first, second], colored, None, device)
        assert not np.array_equal(plain2["elevation_angle"], plain["elevation_angle"])
        S.assert_layers_equal(run_gpu(cam, z, [first, second], colored, INF, device), plain2, LAYERS)
    # (and with a finite margin this terrain does occlude: the test above is not one of flat ground)
    some = run_gpu(cam, z, [first], colored, 0.0)
    assert (some["elevation_angle"] != plain["elevation_angle"]).sum() > 50


# ---- 2. the block scene against the reference -------------------------------------------------
# (that the reference is not vacuous on this scene -- the occlusion term changes >= 50 cells, leaves
# >= 10 initial with the oblique frame alone, occludes no roof cell -- is checked without a GPU:
# tests/test_ortho_occlusion_host.py)
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_block_scene_matches_the_reference(colored, device):
    cam, z = SC.camera(), SC.block_elevation()
    poses, fr = SC.block_poses(), SC.frames(2, colored)
    got = run_gpu(cam, z, [(poses, fr)], colored, SC.MARGIN, device)
    S.assert_layers_equal(got, SC.expected("block", colored), LAYERS)
    if not colored:
        got = run_gpu(cam, z, [(poses[0:1], fr[0:1])], colored, SC.MARGIN, device)
        S.assert_layers_equal(got, SC.expected("oblique"), LAYERS)
        # lazily initial layers (a reset after an earlier mosaic): cells every view of which is
        # occluded come out in the initial state
        got = run_gpu(cam, z, [(poses[0:1], fr[0:1])], colored, SC.MARGIN, device, reset_first=True)
        S.assert_layers_equal(got, SC.expected("oblique"), LAYERS)


# ---- 3. the strict comparison and the rounding rule -------------------------------------------
def _exact_cell_is_occluded(k, dj_cells, height):
    cam, z = SC.camera(), SC.exact_elevation(k, dj_cells, height)
    pose, fr = SC.exact_pose(), SC.frames(1)
    g = SC.grid()
    assert R.occluded(np.zeros_like(z), g, SC.I0, SC.J0, pose[0, 0:3], SC.EXACT_MARGIN) is False
    want = SC.fresh_layers(z)
    R.process(g, cam, pose, synth.IDENTITY_POSE, fr, want, False, SC.EXACT_MARGIN)
    got = run_gpu(cam, z, [(pose, fr)], False, SC.EXACT_MARGIN)
    S.assert_layers_equal(got, want, LAYERS)
    seen = not np.isnan(got["observation_index"][SC.J0, SC.I0])
    assert seen == (not R.occluded(z, g, SC.I0, SC.J0, pose[0, 0:3], SC.EXACT_MARGIN))
    return not seen


def test_a_sample_on_the_ray_plus_margin_does_not_occlude():
    # step 3: z = 3, margin 0.25; 1.5 rounds to 2
    assert _exact_cell_is_occluded(3, 2, np.float32(3.25)) is False
    assert _exact_cell_is_occluded(3, 2, np.nextafter(np.float32(3.25), np.float32(10.0))) is True


@pytest.mark.parametrize("k, even, other", [(1, 0, 1), (5, 2, 3)])
def test_half_way_steps_round_to_even(k, even, other):
    # s * dj = k / 2 exactly: 0.5 -> 0, 2.5 -> 2 (round half away from zero would take the other)
    assert _exact_cell_is_occluded(k, even, np.float32(k + 1.0)) is True
    assert _exact_cell_is_occluded(k, other, np.float32(k + 1.0)) is False


# ---- 4. NaN -----------------------------------------------------------------------------------
def test_nan_samples_do_not_occlude_and_nan_cells_stay_untouched():
    cam, z = SC.camera(), SC.nan_elevation()
    poses, fr = SC.block_poses(), SC.frames(2)
    want = SC.expected("nan")
    holes = np.isnan(z)
    assert holes.sum() > 500
    # (on the reference: holes lie on rays that go on, and the block still casts its shadow)
    T = O.compose_T_G_C(poses, synth.IDENTITY_POSE)
    why, crossed = [], 0
    for j in range(0, SC.COLS, 3):
        for i in range(0, SC.ROWS, 3):
            R.occluded(z, SC.grid(), i, j, T[0, 0:3], SC.MARGIN, why)
            crossed += why[1] >= 8
    assert crossed > 100
    plain = SC.fresh_layers(z)
    R.process(SC.grid(), cam, poses, synth.IDENTITY_POSE, fr, plain, False, None)
    assert (want["observation_index"] != plain["observation_index"])[~holes].sum() >= 50
    got = run_gpu(cam, z, [(poses, fr)])
    S.assert_layers_equal(got, want, LAYERS)
    init = O.new_layers(SC.grid())
    for n in LAYERS:
        assert np.array_equal(got[n][holes], init[n][holes], equal_nan=True), n
    # every elevation NaN: every layer stays initial
    got = run_gpu(cam, np.full_like(z, np.nan), [(poses, fr)])
    S.assert_layers_equal(got, init, LAYERS)


# ---- 5. incremental ---------------------------------------------------------------------------
def test_an_occluded_later_frame_does_not_displace_the_earlier_winner():
    cam, z = SC.camera(), SC.block_elevation()
    poses, fr = SC.block_poses(), SC.frames(2)
    want, plain = SC.expected("incremental"), SC.expected("incremental", margin=None)
    first = SC.fresh_layers(z)
    R.process(SC.grid(), cam, poses[1:2], synth.IDENTITY_POSE, fr[1:2], first, False, SC.MARGIN)
    # (on the reference) the oblique frame, folded second, has the larger angle behind the block --
    # the plain mosaic takes it -- and is occluded there: the first call's values stay
    kept = (plain["elevation_angle"] > first["elevation_angle"]) & \
        (want["elevation_angle"] == first["elevation_angle"])
    assert kept.sum() >= 50
    assert np.array_equal(want["ortho"][kept], first["ortho"][kept])
    got = run_gpu(cam, z, [(poses[1:2], fr[1:2]), (poses[0:1], fr[0:1])])
    S.assert_layers_equal(got, want, LAYERS)


# ---- 6. determinism ---------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    cam, z = SC.camera(), SC.nan_elevation()
    poses, fr = SC.block_poses(), SC.frames(2, True)
    a = run_gpu(cam, z, [(poses, fr)], True)
    b = run_gpu(cam, z, [(poses, fr)], True)
    for n in LAYERS:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


# ---- 7. refusals ------------------------------------------------------------------------------
def test_windows_and_bad_margins_are_refused():
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib as L
    cam, z = SC.camera(), SC.block_elevation()
    poses, fr = SC.block_poses(), SC.frames(2)
    on = A.OrthoSettings(occlusion_test=True, occlusion_margin_m=SC.MARGIN)
    # a context that holds a window of the map
    with A.AerialGridMap(_settings(A), window=(0, 0, 64, SC.COLS)) as m:
        m.set("elevation", z[:, 0:64])
        for images in (fr, None):
            with pytest.raises(L.AmhipError) as e:
                if images is None:
                    import torch
                    images = torch.from_numpy(np.stack(fr)).cuda()
                A.OrthoBackwardGrid(_ncam(A, cam), on, m).process(poses, images, m)
            assert e.value.status == L.ERR_ARG and "window" in str(e.value) and "halo" in str(e.value)
        # (the plain mosaic runs on it)
        A.OrthoBackwardGrid(_ncam(A, cam), A.OrthoSettings(), m).process(poses, fr, m)
    # a session of two windows
    with A.HostSession(_settings(A), tiles=(2, 1)) as hs:
        hs.layers["elevation"][...] = z
        with pytest.raises(L.AmhipError) as e:
            hs.ortho_process(_ncam(A, cam), on, poses, fr)
        assert e.value.status == L.ERR_ARG and "window" in str(e.value) and "halo" in str(e.value)
        for n in LAYERS:
            assert np.array_equal(hs.layers[n], O.new_layers(SC.grid())[n], equal_nan=True)
    # margins
    with A.AerialGridMap(_settings(A)) as m:
        m.set("elevation", z)
        for bad in (-0.5, -INF, float("nan")):
            st = A.OrthoSettings(occlusion_test=True, occlusion_margin_m=bad)
            with pytest.raises(L.AmhipError) as e:
                A.OrthoBackwardGrid(_ncam(A, cam), st, m).process(poses, fr, m)
            assert e.value.status == L.ERR_ARG and "margin" in str(e.value)
        for n in LAYERS:   # nothing was written
            assert np.array_equal(m.get(n), O.new_layers(SC.grid())[n], equal_nan=True)


# ---- 8. HostSession ---------------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_host_session_with_the_switch(colored):
    import aerial_mapper_amd as A
    cam, z = SC.camera(), SC.block_elevation()
    poses, fr = SC.block_poses(), SC.frames(2, colored)
    with A.HostSession(_settings(A)) as hs:
        hs.layers["elevation"][...] = z
        st = A.OrthoSettings(colored_ortho=colored, occlusion_test=True, occlusion_margin_m=SC.MARGIN)
        hs.ortho_process(_ncam(A, cam), st, poses, fr)
        S.assert_layers_equal(hs.layers, SC.expected("block", colored), LAYERS)
        # without the switch, onto fresh layers: the plain mosaic
        for n, v in O.new_layers(SC.grid()).items():
            if n != "elevation":
                hs.layers[n][...] = v
        hs.ortho_process(_ncam(A, cam), A.OrthoSettings(colored_ortho=colored), poses, fr)
        S.assert_layers_equal(hs.layers, SC.expected("block", colored, margin=None), LAYERS)


# ---- 9. more frames than one cull pass lists --------------------------------------------------
def test_more_frames_than_one_frame_list_holds():
    """Beyond 1024 frames the kernel culls and folds chunk by chunk, per slab.  1030 frames that all
    see the map: with margin +inf the plain mosaic, bit for bit; with the scene's margin the same
    angles, pixels and counts as the same frames folded in two calls of fewer than 1024 (only
    observation_index, which counts within a call, differs for the second call's winners)."""
    cam, z = SC.camera(), SC.block_elevation()
    rng = np.random.Generator(np.random.PCG64(77))
    F = 1030
    poses = SC.block_poses()[np.arange(F) % 2].copy()
    poses[:, 0:3] += rng.uniform(-2.0, 2.0, size=(F, 3))
    # (the last frame, in the second chunk, looks straight at ground no other frame's axis is near:
    # it wins there)
    poses[F - 1] = R.look_at_pose((10.0, 8.0, 60.0), (12.0, 10.0, 0.0), yaw=0.9)
    fr = SC.frames(F)
    plain = run_gpu(cam, z, [(poses, fr)], False, None)
    assert (plain["observation_index"] == F - 1).sum() > 50
    S.assert_layers_equal(run_gpu(cam, z, [(poses, fr)], False, INF), plain, LAYERS)
    one = run_gpu(cam, z, [(poses, fr)])
    two = run_gpu(cam, z, [(poses[:600], fr[:600]), (poses[600:], fr[600:])])
    assert (one["elevation_angle"] != plain["elevation_angle"]).sum() >= 50
    assert (one["observation_index"] == F - 1).sum() > 50
    rest = [n for n in LAYERS if n != "observation_index"]
    S.assert_layers_equal(one, two, rest)
    second = one["observation_index"] >= 600
    assert second.sum() > 50
    want_index = np.where(second, one["observation_index"] - np.float32(600.0), one["observation_index"])
    later = ~np.isnan(two["observation_index"]) & second
    assert np.array_equal(two["observation_index"][later], want_index[later])
