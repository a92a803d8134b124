"""GPU: the PNG encoder behind the layer, session and mosaic calls: each file equals
tests/png_encode_reference.py applied to the raster the call encodes."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
import png_encode_reference as R
import scenarios as S
from aerial_mapper_amd import synth

pytestmark = pytest.mark.gpu


def _where(got, ref):
    at = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    return "sizes %d / %d, first differing byte %d" % (len(got), len(ref), at)


@pytest.mark.parametrize("rows,cols", [(24, 40), (300, 200)])
def test_layer_to_png_equals_the_restatement_of_the_layer_image(rows, cols, tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    res = 0.5
    rng = np.random.default_rng(rows + cols)
    layer = (rng.random((cols, rows)) * 300.0 - 20.0).astype(np.float32)
    layer[rng.random((cols, rows)) < 0.1] = np.nan
    layer[: cols // 3] = 17.0                      # a flat area: runs
    packed = np.full((cols, rows), np.nan, np.float32)
    bits = rng.integers(0, 1 << 24, (cols, rows), dtype=np.uint32)
    keep = rng.random((cols, rows)) < 0.8
    packed.view(np.uint32)[keep] = bits[keep]
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, rows * res, cols * res, res), device=0) as m:
        assert (m.rows, m.cols) == (rows, cols)
        m.set("ortho", layer)
        m.set("colored_ortho", packed)
        for name, bgr in (("ortho", False), ("colored_ortho", True)):
            f = str(tmp_path / (name + ".png"))
            E.layer_to_png(m, name, f, 0.0, 255.0, bgr=bgr)
            img = E.layer_to_image(m, name, 0.0, 255.0, bgr=bgr)
            assert (img == 0).any() and img.shape[:2] == (rows, cols)     # (the NaN cells)
            got = open(f, "rb").read()
            ref = R.encode(img)
            assert got == ref, (name, _where(got, ref))
            assert E.encode_png(m, img) == ref


def test_session_layer_to_png_works_from_the_assembled_image(tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    sc = S.Scene(48.0, 32.0, 0.5, 8000, seed=5, num_frames=3)
    g = sc.grid
    with A.HostSession(A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution),
                       tiles=(2, 2)) as hs:
        hs.dsm_process(A.DsmSettings(1), sc.points)
        for layer, lo, hi, bgr in (("elevation", 380.0, 420.0, False), ("colored_ortho", 0.0, 255.0, True)):
            f = str(tmp_path / (layer + ".png"))
            E.session_layer_to_png(hs, layer, f, lo, hi, bgr=bgr)
            img = E.session_layer_to_image(hs, layer, lo, hi, bgr=bgr)
            got = open(f, "rb").read()
            assert got == R.encode(img), (layer, _where(got, R.encode(img)))


def _mosaic(channels):
    import aerial_mapper_amd as A
    cam = S.camera(128, 96, 100.0)
    desc = O.mosaic_desc(240, 200, 400.0)
    ncam = A.NCamera(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height, cam.distortion, tuple(cam.dist))
    st = A.OrthoForwardHomographySettings(ground_plane_elevation_m=400.0, width_mosaic_pixels=240,
                                          height_mosaic_pixels=200, origin=tuple(desc.origin))
    return A.OrthoForwardHomography(ncam, st)


@pytest.mark.parametrize("channels", [1, 3], ids=["gray", "coloured"])
def test_mosaic_png_equals_the_restatement_of_its_clamped_result(channels, tmp_path):
    import torch
    from aerial_mapper_amd import hip_lib as L
    poses = synth.make_lawnmower_poses(6, 50.0, 500.0, 23, tilt_deg=4.0)
    frames = synth.make_frames(6, 96, 128, channels, salt=9)
    with _mosaic(channels) as mosaic:
        mosaic.batch(poses, [f for f in frames])
        # values outside 0..255 into the device-resident result_ itself, as a later blend could leave them
        ptr = C.c_void_p()
        L.check(L.load().amhip_mosaic_device_ptr(mosaic.handle, C.byref(ptr), None))

        class _Holder(object):
            pass
        holder = _Holder()
        holder.__cuda_array_interface__ = {"shape": (200, 240, 3), "typestr": "<i2",
                                           "data": (int(ptr.value), False), "version": 2}
        view = torch.as_tensor(holder, device="cuda:0")
        view[10:30, 20:60, :] = -300
        view[50:70, 100:150, 1] = 700
        view[199, 239, :] = torch.tensor([-1, 256, 32767], dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        res, _ = mosaic.result()
        assert (res < 0).any() and (res > 255).any() and (res != 0).mean() > 0.2 and (res == 0).mean() > 0.05
        ref = R.encode(R.clamp16(res))
        f = str(tmp_path / "mosaic.png")
        mosaic.write_png(f)
        got = open(f, "rb").read()
        assert got == ref, _where(got, ref)
        assert mosaic.encode_png() == ref


def test_an_uncovered_mosaic_is_one_run_per_row_end_to_end(tmp_path):
    """nothing blended: result_ is zero, every row one run behind its filter byte"""
    with _mosaic(3) as mosaic:
        res, _ = mosaic.result()
        assert not res.any()
        ref = R.encode(R.clamp16(res))
        assert len(ref) < 1000          # (144 000 bytes of pixels)
        assert mosaic.encode_png() == ref
        f = str(tmp_path / "blank.png")
        mosaic.write_png(f)
        assert open(f, "rb").read() == ref
