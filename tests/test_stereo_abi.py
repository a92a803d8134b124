"""CPU: the C ABI of the stereo::Stereo sequence object (amhip_stereo_*): exports, the reference's
defaults, the struct layout, the argument errors that are reported before a device is looked at, the
Python mirror of stereo::Settings, and the sequence generator's own conditions."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("amhip_stereo_default_settings", "amhip_stereo_create", "amhip_stereo_destroy",
         "amhip_stereo_reset", "amhip_stereo_add_frame", "amhip_stereo_add_frame_dev",
         "amhip_stereo_add_frames", "amhip_stereo_add_frames_dev", "amhip_stereo_cloud",
         "amhip_stereo_point_cloud2_dev")


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports(L):
    lib = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in L.EXPORTS
    assert L.NUM_KERNELS == 8   # (the sequence times into k_stereo and the misc slot)


def test_struct_size_and_offsets(L):
    S = L.StereoSettings
    assert C.sizeof(S) == 104
    assert (S.use_every_nth_image.offset, S.images_need_undistortion.offset, S.use_bm.offset,
            S.sgbm.offset, S.bm.offset) == (0, 8, 12, 24, 64)


def test_defaults_are_the_references(L):
    s = L.StereoSettings()
    s.use_every_nth_image, s.use_bm, s.images_need_undistortion = 99, 7, 7
    L.load().amhip_stereo_default_settings(C.byref(s))
    # stereo::Settings (common.h:31-35), BlockMatchingParameters (common.h:81-110)
    assert (s.use_every_nth_image, s.images_need_undistortion, s.use_bm) == (1, 0, 0)
    assert [getattr(s.sgbm, n) for n, _ in L.SgbmParams._fields_] == [1, 80, 35, 10, 100, 20, 0, 120, 250, 9]
    assert [getattr(s.bm, n) for n, _ in L.BmParams._fields_] == [1, 80, 31, 9, 80, 20, 100, 5, 0, 15]
    import aerial_mapper_amd as A
    mine = A.StereoSettings()
    assert (mine.use_every_nth_image, mine.images_need_undistortion, mine.show_rectification) == (1, False, True)
    for name in ("Stereo", "StereoSettings"):
        assert name in A.__all__


def _camera(L, W=64, H=48):
    cam = L.Camera()
    cam.fu = cam.fv = 50.0
    cam.cu, cam.cv, cam.width, cam.height = (W - 1) / 2.0, (H - 1) / 2.0, W, H
    return cam


def test_create_refuses_bad_arguments_without_a_gpu(L):
    lib = L.load()
    f64p = C.POINTER(C.c_double)
    tcb = np.array([0.0, 0, 0, 1, 0, 0, 0])
    T = tcb.ctypes.data_as(f64p)
    base = L.StereoSettings()
    lib.amhip_stereo_default_settings(C.byref(base))
    out = C.c_void_p()

    def err(ctx=None, cam=_camera(L), t=T, s=base, o=out):
        rc = lib.amhip_stereo_create(ctx, C.byref(cam) if cam is not None else None, t,
                                     C.byref(s) if s is not None else None,
                                     C.byref(o) if o is not None else None)
        assert rc == L.ERR_ARG and not out.value
        return lib.amhip_last_error().decode()

    def with_(**kw):
        s = L.StereoSettings.from_buffer_copy(bytes(base))
        for k, v in kw.items():
            obj, name = (s, k) if "." not in k else (getattr(s, k.split(".")[0]), k.split(".")[1])
            setattr(obj, name, v)
        return s

    assert "null context" in err()                       # everything else is in order
    assert "null argument" in err(cam=None)
    assert "null argument" in err(t=None)
    assert "null argument" in err(s=None)
    assert "null argument" in err(o=None)
    assert "use_every_nth_image" in err(s=with_(use_every_nth_image=0))
    assert "width and height" in err(cam=_camera(L, 0, 48))
    assert "width and height" in err(cam=_camera(L, 64, 40000))
    bad = _camera(L)
    bad.distortion = 9
    assert "distortion" in err(cam=bad)
    # the parameters of the SELECTED matcher, by the matcher's own rules
    assert "multiple of 16" in err(s=with_(**{"sgbm.num_disparities": 72}))
    assert "block_size" in err(s=with_(**{"sgbm.block_size": 13}))
    assert "CV_16S" in err(s=with_(**{"sgbm.min_disparity": 2040}))
    assert "null context" in err(s=with_(**{"bm.num_disparities": 72}))          # (BM is not selected)
    assert "multiple of 16" in err(s=with_(use_bm=1, **{"bm.num_disparities": 72}))
    assert "block_size" in err(s=with_(use_bm=1, **{"bm.block_size": 4}))
    assert "block_size" in err(s=with_(use_bm=1), cam=_camera(L, 64, 13))         # above min(W, H)
    assert "pre_filter_size" in err(s=with_(use_bm=1, **{"bm.pre_filter_size": 0}))
    assert "null context" in err(s=with_(use_bm=1, **{"sgbm.num_disparities": 72}))


def test_frame_calls_refuse_bad_arguments_without_a_gpu(L):
    lib = L.load()
    T = np.zeros(14)
    T[3] = T[10] = 1.0
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    img = C.c_void_p(0x1000)   # (never dereferenced: refused first)

    def msg(rc):
        assert rc == L.ERR_ARG
        return lib.amhip_last_error().decode()

    for fn in (lib.amhip_stereo_add_frame, lib.amhip_stereo_add_frame_dev):
        assert "8UC3" in msg(fn(None, Tp, img, 64, 3))
        assert "8UC1 only" in msg(fn(None, Tp, img, 64, 4))
        assert "8UC1 only" in msg(fn(None, Tp, img, 64, 0))
        assert "null argument" in msg(fn(None, None, img, 64, 1))
        assert "null argument" in msg(fn(None, Tp, None, 64, 1))
        assert "null stereo object" in msg(fn(None, Tp, img, 64, 1))
    ptrs = (C.c_void_p * 2)(0x1000, 0x2000)
    steps = (C.c_size_t * 2)(64, 64)
    assert "8UC3" in msg(lib.amhip_stereo_add_frames(None, Tp, ptrs, steps, 3, 2))
    assert "null argument" in msg(lib.amhip_stereo_add_frames(None, None, ptrs, steps, 1, 2))
    assert "null argument" in msg(lib.amhip_stereo_add_frames(None, Tp, None, steps, 1, 2))
    assert "null argument" in msg(lib.amhip_stereo_add_frames(None, Tp, ptrs, None, 1, 2))
    assert "null stereo object" in msg(lib.amhip_stereo_add_frames(None, Tp, ptrs, steps, 1, 2))
    assert "8UC3" in msg(lib.amhip_stereo_add_frames_dev(None, Tp, img, 4096, 64, 3, 2))
    assert "null argument" in msg(lib.amhip_stereo_add_frames_dev(None, Tp, None, 4096, 64, 1, 2))
    assert "null stereo object" in msg(lib.amhip_stereo_add_frames_dev(None, Tp, img, 4096, 64, 1, 2))
    for fn in (lib.amhip_stereo_destroy, lib.amhip_stereo_reset):
        assert "null stereo object" in msg(fn(None))
    assert "null stereo object" in msg(lib.amhip_stereo_cloud(None, None, None, None, None))
    assert "null stereo object" in msg(lib.amhip_stereo_point_cloud2_dev(None, None, None))


def test_python_class_refuses_before_any_device_work():
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib
    with pytest.raises(A.AmhipError) as ei:
        A.Stereo(None, A.StereoSettings(), A.BlockMatchingParameters(), None)
    assert ei.value.status == hip_lib.ERR_ARG
    with pytest.raises(A.AmhipError) as ei:
        A.Stereo(A.NCamera(50.0, 50.0, 31.5, 23.5, 64, 48), A.StereoSettings(), None, None)
    assert ei.value.status == hip_lib.ERR_ARG


def test_frame_selection_rule():
    import stereo_sequence as SS
    # stereo.cpp:91-93: ++skip % n == 0
    assert SS.selected(5, 1) == [0, 1, 2, 3, 4]
    assert SS.pairs_of(7, 2) == [(1, 3), (3, 5)]
    assert SS.pairs_of(7, 3) == [(2, 5)]
    assert SS.pairs_of(3, 2) == [] and SS.pairs_of(5, 3) == []


def test_generated_sequence_composes_to_the_intended_camera_poses():
    import stereo_sequence as SS
    seq = SS.Sequence(3, 96, 64)
    assert np.abs(seq.T_C_B[:3]).min() > 0.01 and abs(seq.T_C_B[3]) < 0.9999     # not the identity
    Rs, ts = seq.camera_poses()
    for i in range(3):
        assert abs(ts[i][0] - (10.0 + 6.0 * i)) < 1e-9 and abs(ts[i][2] - 80.0) < 2.0
        assert np.allclose(Rs[i] @ Rs[i].T, np.eye(3), atol=1e-12)
        assert Rs[i][2, 2] < -0.99                                               # looking down
    assert seq.frames.shape == (3, 64, 96) and seq.frames.std() > 20.0
