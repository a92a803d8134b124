"""GPU: the JPEG encoder (aerial_mapper_amd/csrc/amhip_jpeg.hip) against tests/jpeg_reference.py,
byte for byte: the whole input list from host arrays and from device tensors with padded rows, the
buffer-capacity rule, scratch reuse, the layer path and the mosaic path.  No Pillow, nothing of the
reference tree."""
import ctypes as C

import numpy as np
import pytest

import jpeg_inputs as I
import jpeg_reference as J
import oracle_ffi as O
import scenarios as S
from aerial_mapper_amd import synth

pytestmark = pytest.mark.gpu

CASES = I.cases()
IDS = [c.name for c in CASES]


def _first_difference(got, want, image, quality):
    """where two files part: byte offset, and block / coefficient when `got` still decodes"""
    at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    where = "sizes %d / %d, first differing byte %d" % (len(got), len(want), at)
    try:
        bad = np.argwhere(J.decode(got).coef != J.blocks_of(image, quality).coef)
        where += ", first (block, coefficient) %s of %d" % (bad[0].tolist() if len(bad) else None, len(bad))
    except Exception as e:   # noqa: BLE001 (the decoder's own assertion is the information)
        where += ", does not decode: %s" % e
    return where


def _assert_file(got, image, quality, what):
    want = J.encode(image, quality)
    assert got == want, "%s q%d: %s" % (what, quality, _first_difference(got, want, image, quality))


@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 8.0, 8.0, 1.0), device=0) as m:
        yield m


def _padded_device(image, pad):
    """a device tensor whose rows are `pad` bytes further apart than they are long"""
    import torch
    h, w = image.shape[:2]
    row = w * (1 if image.ndim == 2 else 3)
    buf = torch.full((h, row + pad), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:, :row] = torch.from_numpy(image.reshape(h, row)).cuda()
    view = buf[:, :row] if image.ndim == 2 else buf[:, :row].unflatten(1, (w, 3))
    assert h == 1 or view.stride(0) == row + pad     # (a single row has no step to speak of)
    return view


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encode_equals_the_restatement(case, gmap):
    from aerial_mapper_amd import export as E
    img = case.image()
    dev = _padded_device(img, 13)
    for q in I.QUALITIES:
        _assert_file(E.encode_jpeg(gmap, img, q), img, q, "%s from the host" % case)
        _assert_file(E.encode_jpeg(gmap, dev, q), img, q, "%s from a padded device tensor" % case)


def test_large_scan_crosses_the_top_level_of_the_bit_count_scan(gmap):
    """1032 x 1024 gray = 16 512 blocks: 65 workgroup sums, one more than the single wave of
    k_jpeg_scan_top takes per step"""
    from aerial_mapper_amd import export as E
    img = I.large_case().image()
    assert ((img.shape[0] + 7) // 8) * ((img.shape[1] + 7) // 8) > 64 * 256
    _assert_file(E.encode_jpeg(gmap, img, 95), img, 95, "large")


def test_default_quality_is_95(gmap):
    from aerial_mapper_amd import export as E
    img = I.Case("noise", 33, 15, 3).image()
    assert E.encode_jpeg(gmap, img, 0) == J.encode(img, 95) == E.encode_jpeg(gmap, img)


def test_capacity_one_short_is_an_argument_error_and_writes_nothing(gmap):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    for case in (I.Case("stuffed", 129, 47, 3), I.Case("noise", 17, 17, 1)):
        img = case.image()
        want = J.encode(img, 100)
        size = len(want)
        dev = torch.from_numpy(img).cuda()
        ch = 1 if img.ndim == 2 else 3
        guard = 64
        n = C.c_size_t()
        out = torch.full((size + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.amhip_jpeg_encode_dev(gmap._h, C.c_void_p(dev.data_ptr()), dev.stride(0), case.width,
                                       case.height, ch, 100, C.c_void_p(out.data_ptr()), size - 1, C.byref(n))
        assert rc == L.ERR_ARG and lib.amhip_last_error()
        assert n.value == size            # (the size it would have taken)
        assert bool((out[size - 1:] == 0x5A).all()), "bytes behind cap were written"
        rc = lib.amhip_jpeg_encode_dev(gmap._h, C.c_void_p(dev.data_ptr()), dev.stride(0), case.width,
                                       case.height, ch, 100, C.c_void_p(out.data_ptr()), size, C.byref(n))
        assert rc == L.OK and n.value == size
        got = out.cpu().numpy()
        assert got[:size].tobytes() == want and (got[size:] == 0x5A).all()


def test_back_to_back_images_on_one_context_keep_their_own_bytes(gmap):
    """scratch is reused, the packed words are zeroed in between: a long file, a short one of a
    smaller image, the long one again"""
    from aerial_mapper_amd import export as E
    a, b = I.Case("stuffed", 129, 47, 1).image(), I.Case("checker", 17, 17, 3).image()
    for img, q in ((a, 100), (b, 1), (a, 100), (b, 100), (a, 50)):
        _assert_file(E.encode_jpeg(gmap, img, q), img, q, "back to back")


@pytest.mark.parametrize("rows,cols", [(24, 40), (1000, 1000)])
def test_layer_to_jpeg_equals_encoding_the_layer_image(rows, cols, tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    res = 0.5
    rng = np.random.default_rng(rows + cols)
    layer = (rng.random((cols, rows)) * 300.0 - 20.0).astype(np.float32)
    layer[rng.random((cols, rows)) < 0.1] = np.nan
    packed = np.full((cols, rows), np.nan, np.float32)
    bits = rng.integers(0, 1 << 24, (cols, rows), dtype=np.uint32)
    keep = rng.random((cols, rows)) < 0.8
    packed.view(np.uint32)[keep] = bits[keep]
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, rows * res, cols * res, res), device=0) as m:
        assert (m.rows, m.cols) == (rows, cols)
        m.set("ortho", layer)
        m.set("colored_ortho", packed)
        for name, bgr, q in (("ortho", False, 95), ("colored_ortho", True, 50)):
            f = str(tmp_path / (name + ".jpg"))
            E.layer_to_jpeg(m, name, f, 0.0, 255.0, bgr=bgr, quality=q)
            img = E.layer_to_image(m, name, 0.0, 255.0, bgr=bgr)
            assert (img == 0).any() and img.shape[:2] == (rows, cols)     # (the NaN cells)
            got = open(f, "rb").read()
            assert got == E.encode_jpeg(m, img, q)
            if rows < 100:
                _assert_file(got, img, q, name)
            f2 = str(tmp_path / (name + "_2.jpg"))
            E.write_jpeg(m, f2, img, q)
            assert open(f2, "rb").read() == got


def test_session_layer_to_jpeg_works_from_the_assembled_image(tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    sc = S.Scene(48.0, 32.0, 0.5, 8000, seed=5, num_frames=3)
    g = sc.grid
    with A.HostSession(A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution),
                       tiles=(2, 2)) as hs:
        hs.dsm_process(A.DsmSettings(1), sc.points)
        f = str(tmp_path / "elevation.jpg")
        E.session_layer_to_jpeg(hs, "elevation", f, 380.0, 420.0, quality=95)
        img = E.session_layer_to_image(hs, "elevation", 380.0, 420.0)
        _assert_file(open(f, "rb").read(), img, 95, "session")


def test_mosaic_write_jpeg_clamps_result_in_the_kernel(tmp_path):
    import torch
    import aerial_mapper_amd as A
    cam = S.camera(128, 96, 100.0)
    desc = O.mosaic_desc(240, 200, 400.0)
    poses = synth.make_lawnmower_poses(6, 50.0, 500.0, 23, tilt_deg=4.0)
    frames = synth.make_frames(6, 96, 128, 3, salt=9)
    ncam = A.NCamera(cam.fu, cam.fv, cam.cu, cam.cv, cam.width, cam.height, cam.distortion, tuple(cam.dist))
    st = A.OrthoForwardHomographySettings(ground_plane_elevation_m=400.0, width_mosaic_pixels=240,
                                          height_mosaic_pixels=200, origin=tuple(desc.origin))
    with A.OrthoForwardHomography(ncam, st) as mosaic:
        mosaic.batch(poses, [f for f in frames])
        res, _ = mosaic.result()
        if not ((res < 0).any() and (res > 255).any()):
            # the blender keeps this scene inside 0..255: put out-of-range values into the
            # device-resident result_ itself (amhip_mosaic_device_ptr), as a later blend could
            ptr = C.c_void_p()
            from aerial_mapper_amd import hip_lib as L
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
            view[0, 0, :] = torch.tensor([-32768, 255, 0], dtype=torch.int16, device="cuda:0")
            torch.cuda.synchronize()
            res, _ = mosaic.result()
        assert (res < 0).any() and (res > 255).any() and (res != 0).mean() > 0.2
        img = np.clip(res, 0, 255).astype(np.uint8)
        for q in (95, 1):
            f = str(tmp_path / ("mosaic_q%d.jpg" % q))
            mosaic.write_jpeg(f, q)
            got = open(f, "rb").read()
            _assert_file(got, img, q, "mosaic")
            assert mosaic.encode_jpeg(q) == got
