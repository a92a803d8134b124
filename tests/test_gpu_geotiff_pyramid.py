"""GPU: GeoTIFF overviews (amhip_tiff_overview.hip) -- the pyramid the writer produces against
tests/geotiff_pyramid_reference.py, bit for bit, and the reader by level."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import geotiff_pyramid_inputs as PI
import geotiff_pyramid_reference as P
import geotiff_read_reference as R
import geotiff_reference as GR
import scenarios as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.5
CENTER = (464980.0, 5272690.0)


def _where(got, ref):
    at = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    return "sizes %d / %d, first differing byte %d" % (len(got), len(ref), at)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _host(t):
    return t.cpu().numpy()


def _map(rows=8, cols=8, window=None, center=CENTER, res=RES):
    import aerial_mapper_amd as A
    return A.AerialGridMap(A.GridMapSettings(center[0], center[1], rows * res, cols * res, res), device=0, window=window)


@pytest.fixture(scope="module")
def m8():
    with _map() as m:
        yield m


# ---- the writer: rasters ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PI.KINDS)
@pytest.mark.parametrize("w,h,tile", PI.SIZES)
def test_the_pyramid_is_the_references_byte_for_byte(m8, kind, w, h, tile):
    from aerial_mapper_amd import export as E
    raster = PI.raster(kind, w, h)
    seen = set()
    for n in (1, 2, -1):
        try:
            count = P.level_count(w, h, tile, n)
        except ValueError:       # (2 x 2 has one overview)
            with pytest.raises(Exception) as ei:
                E.encode_geotiff(m8, raster, PI.GT, 32, True, tile, overviews=n)
            assert "amhip_geotiff_encode_ovr_dev" in str(ei.value) and "overviews" in str(ei.value)
            continue
        want = P.encode(raster, PI.GT, 32, True, tile, n)
        got = E.encode_geotiff(m8, raster, PI.GT, 32, True, tile, overviews=n)
        assert got == want, (n, _where(got, want))
        seen.add(count)
        levels = P.pyramid(raster, tile, n)
        for k, lvl in enumerate(levels):
            assert same(P.decode(got, k)[0], lvl), (n, k)
    assert seen - {0}


@pytest.mark.parametrize("name", sorted(PI.fixtures()))
def test_the_committed_pyramids_are_matched_byte_for_byte(m8, name):
    from aerial_mapper_amd import export as E
    raster, tile, n = PI.fixtures()[name]
    want = open(os.path.join(PI.GOLDEN, name + ".tif"), "rb").read()
    got = E.encode_geotiff(m8, raster, PI.GT, 32, True, tile, overviews=n)
    assert got == want, _where(got, want)


def test_contents_that_separate_right_from_nearly_right(m8):
    """level 1 and 2 of the hard rasters, decoded from the GPU's file, against numpy's float64 / integers"""
    from aerial_mapper_amd import export as E
    for raster in (PI.f32_hard(), PI.u8_hard(), PI.rgb8_hard()):
        got = E.encode_geotiff(m8, raster, PI.GT, 32, True, 16, overviews=2)
        l1 = P.reduce(raster)
        assert same(P.decode(got, 1)[0], l1) and same(P.decode(got, 2)[0], P.reduce(l1))
    hard = P.decode(E.encode_geotiff(m8, PI.f32_hard(), PI.GT, 32, True, 16, overviews=1), 1)[0]
    bits = hard.view(np.uint32)
    assert bits[0, 4] == 0x7FC00000 and bits[1, 5] == 0x7FC00000 and (bits[:, 6] == 0x7FC00000).all()
    assert hard[3, 4] == 0.25 and hard[3, 5] == 0.0 and hard[4, 0] == np.float32(16777219.0 / 4.0)
    assert hard[4, 1] == np.float32((np.float64(np.float32(1.0000001)) + np.float64(np.float32(1.0000002)) +
                                     np.float64(np.float32(1.0000004)) + np.float64(np.float32(3.4e38))) / 4.0)
    assert hard[4, 2] == np.float32(3.4e38) and hard[1, 4] == np.inf      # (four of them: a float sum overflows)
    assert hard[5, 0] == -np.inf


def test_a_device_raster_with_padded_rows_and_written_files(m8, tmp_path):
    import torch
    from aerial_mapper_amd import export as E
    for kind in PI.KINDS:
        raster = PI.raster(kind, 33, 21)
        want = P.encode(raster, PI.GT, 33, False, 16, -1)
        t = torch.from_numpy(np.ascontiguousarray(raster)).to("cuda:0")
        pad = torch.zeros((21, 38) + raster.shape[2:], dtype=t.dtype, device="cuda:0")
        pad[:, :33] = t
        assert E.encode_geotiff(m8, pad[:, :33], PI.GT, 33, False, 16, overviews=-1) == want
        f = str(tmp_path / (kind + ".tif"))
        E.write_geotiff_deflate(m8, f, raster, PI.GT, 33, False, 16, overviews=-1)
        assert open(f, "rb").read() == want
        E.write_geotiff_deflate(m8, f, t, PI.GT, 33, False, 16, overviews=-1)
        assert open(f, "rb").read() == want


# ---- the writer: layers ----------------------------------------------------------------------------------
def _layers(rows, cols, seed=3):
    rng = np.random.default_rng(seed)
    elev = (400.0 + 10.0 * rng.random((cols, rows))).astype(np.float32)
    elev[rng.random((cols, rows)) < 0.3] = np.nan
    packed = np.full((cols, rows), np.nan, np.float32)
    keep = rng.random((cols, rows)) < 0.8
    packed.view(np.uint32)[keep] = rng.integers(0, 1 << 24, (cols, rows), dtype=np.uint32)[keep]
    return {"elevation": elev, "colored_ortho": packed}


def test_layer_forms_on_a_windowed_map(tmp_path):
    from aerial_mapper_amd import export as E
    rows, cols, window = 60, 50, (8, 5, 37, 35)
    with _map(rows, cols, window=window) as m:
        for name, a in _layers(37, 35).items():
            m.set(name, a)
        for name, kind, lo, hi in (("elevation", "f32", 0.0, 255.0), ("elevation", "u8", 398.0, 409.0),
                                   ("colored_ortho", "rgb8", 0.0, 255.0)):
            old = E.encode_layer_geotiff(m, name, kind, lo, hi, 32, True, 16)
            base = GR.decode(old)
            got = E.encode_layer_geotiff(m, name, kind, lo, hi, 32, True, 16, overviews=-1)
            assert len(P.levels(got)) == 3                         # 37 x 35 -> 19 x 18 -> 10 x 9
            # level 0 is today's raster; level k the reduction of level k - 1 as it lies in the file
            level = P.decode(got, 0)[0]
            assert same(level, base["raster"]) and same(level, GR.layer_raster(m.get(name), kind, lo, hi))
            for k in (1, 2):
                nxt = P.decode(got, k)[0]
                assert same(nxt, P.reduce(level)), (kind, k)
                level = nxt
            want = P.encode(base["raster"], base["geotransform"], 32, True, 16, -1)
            assert got == want, (kind, _where(got, want))
            f = str(tmp_path / (kind + ".tif"))
            E.layer_to_geotiff(m, name, f, kind, lo, hi, 32, True, 16, overviews=-1)
            assert open(f, "rb").read() == want


# ---- grouping, zero, caps, arguments --------------------------------------------------------------------------
def test_the_bytes_do_not_depend_on_the_grouping(m8):
    from aerial_mapper_amd import export as E
    from aerial_mapper_amd import hip_lib as L
    raster = PI.raster("f32", 48, 16)          # three tiles, then two (24 x 8), then one (12 x 4)
    one = E.encode_geotiff(m8, raster, PI.GT, 32, True, 16, overviews=2)
    assert one == P.encode(raster, PI.GT, 32, True, 16, 2)
    # a tile of 1024 predictor bytes costs 17 920 bytes of scratch (tests/test_gpu_geotiff.py): two fit 0.04 MB,
    # so the groups are (0, 1), (2 | level 1's first), (level 1's second | level 2's): two of them span a level
    # boundary; 0.02 MB holds one tile
    try:
        for mb, groups in ((0.04, "pairs across the level boundaries"), (0.02, "one each")):
            L.set_tuning("tiffe_scratch_budget_mb", mb)
            assert E.encode_geotiff(m8, raster, PI.GT, 32, True, 16, overviews=2) == one, groups
    finally:
        L.set_tuning("tiffe_scratch_budget_mb", None)


def test_zero_overviews_through_the_new_exports_are_the_old_files(m8, tmp_path):
    import torch
    from aerial_mapper_amd import export as E
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    gt = (C.c_double * 6)(*PI.GT)
    n = C.c_size_t()
    for kind in PI.KINDS:
        raster = PI.raster(kind, 33, 21)
        want = E.encode_geotiff(m8, raster, PI.GT, 32, True, 16)
        assert want == GR.encode(raster, PI.GT, 32, True, 16)
        dev = torch.from_numpy(raster).to("cuda:0")
        out = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        k, px = GR.KINDS[kind], raster.strides[0]
        assert lib.amhip_geotiff_encode_ovr_dev(m8._h, C.c_void_p(dev.data_ptr()), px, 33, 21, k, 16, 0, gt, 32, 1,
                                                C.c_void_p(out.data_ptr()), out.numel(), C.byref(n)) == L.OK
        assert out[:n.value].cpu().numpy().tobytes() == want
        f = str(tmp_path / (kind + ".tif")).encode()
        assert lib.amhip_geotiff_write_ovr(m8._h, f, C.c_void_p(raster.ctypes.data), 0, px, 33, 21, k, 16, 0, gt, 32,
                                           1) == L.OK
        assert open(f, "rb").read() == want
        assert lib.amhip_geotiff_bound_ovr(33, 21, k, 16, 0) == lib.amhip_geotiff_bound(33, 21, k, 16)
    with _map(21, 19) as m:
        m.set("elevation", _layers(21, 19)["elevation"])
        want = E.encode_layer_geotiff(m, "elevation", "f32", tile=16)
        out = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        lid = L.LAYER_NAMES.index("elevation")
        assert lib.amhip_layer_encode_geotiff_ovr_dev(m._h, lid, 0, 0.0, 255.0, 16, 0, 32, 1, C.c_void_p(out.data_ptr()),
                                                      out.numel(), C.byref(n)) == L.OK
        assert out[:n.value].cpu().numpy().tobytes() == want
        f = str(tmp_path / "layer.tif").encode()
        assert lib.amhip_layer_write_geotiff_ovr(m._h, lid, 0, 0.0, 255.0, 16, 0, 32, 1, f) == L.OK
        assert open(f, "rb").read() == want


def test_a_buffer_one_byte_too_small_is_refused_and_left_untouched(m8):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    raster = PI.raster("u8", 47, 33)
    want = P.encode(raster, PI.GT, 32, True, 16, -1)
    dev = torch.from_numpy(raster).to("cuda:0")
    gt = (C.c_double * 6)(*PI.GT)
    n = C.c_size_t()
    for cap, ok in ((len(want) - 1, False), (len(want), True)):
        out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rc = lib.amhip_geotiff_encode_ovr_dev(m8._h, C.c_void_p(dev.data_ptr()), 47, 47, 33, 1, 16, -1, gt, 32, 1,
                                              C.c_void_p(out.data_ptr()), cap, C.byref(n))
        host = out.cpu().numpy()
        assert n.value == len(want)
        if ok:
            assert rc == L.OK and host[:len(want)].tobytes() == want and (host[len(want):] == 0xA5).all()
        else:
            assert rc == L.ERR_ARG and "nothing written" in L.last_error() and (host == 0xA5).all()
    for kind in PI.KINDS:
        for (w, h, tile) in PI.SIZES:
            for nn in (-1, 1):
                size = len(P.encode(PI.raster(kind, w, h), PI.GT, 32, True, tile, nn, stream=P.PR.zlib_rle_stream))
                assert lib.amhip_geotiff_bound_ovr(w, h, GR.KINDS[kind], tile, nn) >= size


def test_every_argument_error_names_the_export_and_the_field(m8):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    dev = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p, o = C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr())
    up = (C.c_double * 6)(*PI.GT)
    n = C.c_size_t()
    h = m8._h

    def enc(raster=p, step=64, w=16, hh=16, kind=1, tile=16, ovr=1, gt=up, zone=32, dst=o, nb=C.byref(n), ctx=h):
        return lib.amhip_geotiff_encode_ovr_dev(ctx, raster, step, w, hh, kind, tile, ovr, gt, zone, 1, dst, 1 << 16, nb)

    def wr(name=b"unused.tif", raster=p, step=64, w=16, hh=16, kind=1, tile=16, ovr=1, gt=up, zone=32, ctx=h):
        return lib.amhip_geotiff_write_ovr(ctx, name, raster, 1, step, w, hh, kind, tile, ovr, gt, zone, 1)

    rot = (C.c_double * 6)(1.0, 0.5, 0.25, 2.0, 0.0, -0.5)
    for fn, call in (("amhip_geotiff_encode_ovr_dev", enc), ("amhip_geotiff_write_ovr", wr)):
        for kw, word in [(dict(ctx=None), "null"), (dict(raster=None), "null"), (dict(gt=None), "null"),
                         (dict(w=0), "width"), (dict(hh=65536), "height"), (dict(kind=3), "kind"), (dict(tile=24), "tile"),
                         (dict(step=15), "step"), (dict(gt=rot), "geotransform"), (dict(zone=61), "utm_zone"),
                         (dict(ovr=17), "overviews"), (dict(ovr=-2), "overviews"), (dict(ovr=5), "overviews"),
                         (dict(w=1, hh=1, ovr=1), "overviews")]:
            assert call(**kw) == L.ERR_ARG, (fn, kw)
            assert fn in L.last_error() and word in L.last_error(), (fn, word, L.last_error())
    assert enc(ovr=4) == L.OK             # 16 -> 8 -> 4 -> 2 -> 1: four overviews is the most

    def lay(fn, layer=1, kind=0, lo=0.0, hi=255.0, tile=16, ovr=1, zone=32, ctx=h, name=b"unused.tif", dst=o,
            nb=C.byref(n)):
        if fn == "amhip_layer_encode_geotiff_ovr_dev":
            return lib.amhip_layer_encode_geotiff_ovr_dev(ctx, layer, kind, lo, hi, tile, ovr, zone, 1, dst, 1 << 16, nb)
        return lib.amhip_layer_write_geotiff_ovr(ctx, layer, kind, lo, hi, tile, ovr, zone, 1, name)

    for fn in ("amhip_layer_encode_geotiff_ovr_dev", "amhip_layer_write_geotiff_ovr"):
        cases = [(dict(ctx=None), "null"), (dict(layer=6), "layer"), (dict(kind=3), "kind"), (dict(tile=100), "tile"),
                 (dict(zone=0), "utm_zone"), (dict(kind=1, lo=5.0, hi=5.0), "upper <= lower"),
                 (dict(ovr=17), "overviews"), (dict(ovr=-2), "overviews"), (dict(ovr=5), "overviews")]   # (the map is 8 x 8)
        cases += [(dict(dst=None), "null"), (dict(nb=None), "null")] if fn.endswith("_dev") else [(dict(name=None), "null")]
        for kw, word in cases:
            assert lay(fn, **kw) == L.ERR_ARG
            assert fn in L.last_error() and word in L.last_error(), (fn, word, L.last_error())
    assert lib.amhip_geotiff_bound_ovr(16, 16, 0, 16, 17) == 0 and lib.amhip_geotiff_bound_ovr(16, 16, 0, 16, 6) == 0
    assert lib.amhip_session_layer_write_geotiff_ovr(None, 1, 0, 0.0, 255.0, 16, 1, 32, 1, b"unused.tif") == L.ERR_ARG
    assert "amhip_session_layer_write_geotiff_ovr" in L.last_error() and "null" in L.last_error()
    blob = open(os.path.join(PI.GOLDEN, "u8_31x16_t16_o1.tif"), "rb").read()
    d = L.GeotiffDesc()
    k = C.c_int()
    for call, fn, word in [
            (lambda: lib.amhip_geotiff_levels(None, 8, C.byref(k)), "amhip_geotiff_levels", "null"),
            (lambda: lib.amhip_geotiff_levels(blob, len(blob), None), "amhip_geotiff_levels", "null"),
            (lambda: lib.amhip_geotiff_level_info(blob, len(blob), 2, C.byref(d)), "amhip_geotiff_level_info", "level 2"),
            (lambda: lib.amhip_geotiff_level_info(blob, len(blob), -1, C.byref(d)), "amhip_geotiff_level_info", "level -1"),
            (lambda: lib.amhip_geotiff_decode_level_dev(h, blob, len(blob), 1, 0, 0, 17, 8, o, 17),
             "amhip_geotiff_decode_level_dev", "window"),
            (lambda: lib.amhip_geotiff_decode_level_dev(h, blob, len(blob), 3, 0, 0, 1, 1, o, 16),
             "amhip_geotiff_decode_level_dev", "level 3"),
            (lambda: lib.amhip_layer_decode_geotiff_level(h, 0, blob, len(blob), -2), "amhip_layer_decode_geotiff_level", "level"),
            (lambda: lib.amhip_layer_decode_geotiff_level(h, 9, blob, len(blob), 1), "amhip_layer_decode_geotiff_level", "layer"),
            (lambda: lib.amhip_layer_read_geotiff_level(h, 0, None, 1), "amhip_layer_read_geotiff_level", "null"),
            (lambda: lib.amhip_session_layer_read_geotiff_level(None, 0, b"x.tif", 1, o),
             "amhip_session_layer_read_geotiff_level", "null")]:
        assert call() == L.ERR_ARG
        assert fn in L.last_error() and word in L.last_error(), (fn, word, L.last_error())


# ---- the reader ------------------------------------------------------------------------------------------
def _files():
    out = {n: (open(os.path.join(PI.GOLDEN, n + ".tif"), "rb").read(), P.pyramid(r, t, o))
           for n, (r, t, o) in PI.fixtures().items()}
    out.update(PI.foreign())
    return out


@pytest.mark.parametrize("name", sorted(_files()))
def test_every_level_decodes_to_its_raster(m8, name):
    import aerial_mapper_amd as A
    data, levels = _files()[name]
    infos = A.geotiff_levels(data)
    assert len(infos) == len(levels)                     # (masks and pages are passed over)
    for k, lvl in enumerate(levels):
        got, info = A.decode_geotiff(m8, data, level=k)
        assert same(_host(got), lvl), (name, k)
        assert (info["width"], info["height"]) == (lvl.shape[1], lvl.shape[0]) and repr(info) == repr(infos[k])
        want = P.level_info(data, k)
        assert np.array(info["geotransform"]).tobytes() == np.array(want["geotransform"]).tobytes()


def test_a_window_that_crosses_tiles_of_a_level(m8):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    raster = PI.raster("f32", 100, 70)
    data = E.encode_geotiff(m8, raster, PI.GT, 32, True, 16, overviews=2)
    l1 = P.reduce(raster)                                # 50 x 35: 4 x 3 tiles
    got, _ = A.decode_geotiff(m8, data, window=(9, 11, 30, 20), level=1)
    assert same(_host(got), l1[11:31, 9:39])
    got, _ = A.decode_geotiff(m8, data, window=(3, 2, 20, 15), level=2)
    assert same(_host(got), P.reduce(l1)[2:17, 3:23])


def _dem(w=128, h=96, res=0.25):
    """a file at `res` with three levels (tile 16: 128 x 96 -> 64 x 48 -> 32 x 24), its map's centre"""
    rng = np.random.default_rng(21)
    raster = (rng.random((h, w)) * 50.0 + 300.0).astype(np.float32)
    raster[rng.random((h, w)) < 0.1] = np.nan
    gt = (CENTER[0] - w * res / 2, res, 0.0, CENTER[1] + h * res / 2, 0.0, -res)
    return P.encode(raster, gt, 32, True, 16, 2, stream=P.PR.zlib_rle_stream), raster


def _placed(m, data, level):
    import aerial_mapper_amd as A
    m.reset()
    A.layer_from_geotiff(m, "elevation", data, level=level)
    return m.get("elevation")


def test_layers_take_a_level_and_the_automatic_choice(tmp_path):
    import aerial_mapper_amd as A
    data, raster = _dem()
    assert [d["geotransform"][1] for d in A.geotiff_levels(data)] == [0.25, 0.5, 1.0]
    path = str(tmp_path / "dem.tif")
    open(path, "wb").write(data)
    for window in (None, (3, 2, 20, 15)):
        with _map(32, 24, window=window, res=1.0) as m:           # a 1 m map over the 0.25 m file
            nan = np.full((m.cols, m.rows), np.nan, np.float32)
            by_level = []
            for k in range(3):
                lvl, info = P.decode(data, k)
                want = R.place(nan, m.grid, m.window, info, lvl)
                got = _placed(m, data, k)
                assert same(got, want), (window, k)
                assert same(_placed(m, path, k), want)
                by_level.append(got)
            auto = _placed(m, data, -1)
            assert P.auto_level(data, 1.0) == 2
            assert same(auto, by_level[2]) and not same(auto, by_level[0])
            assert same(_placed(m, path, -1), by_level[2])
    with _map(64, 48, res=0.5) as m:                               # between two levels: the finer one that fits
        assert P.auto_level(data, 0.5) == 1
        assert same(_placed(m, data, -1), _placed(m, data, 1))
    with _map(64, 48, res=0.125) as m:                             # a map finer than the base
        assert P.auto_level(data, 0.125) == 0
        assert same(_placed(m, data, -1), _placed(m, data, 0))
        lvl, info = P.decode(data, 0)
        assert same(_placed(m, data, -1), R.place(np.full((m.cols, m.rows), np.nan, np.float32), m.grid, m.window,
                                                  info, lvl))


def _broken_level(data, level, t):
    """the file with the last byte (the Adler sum) of chunk t of `level` damaged"""
    off, cnt, _ = P.level_info(data, level)["chunks"][t]
    q = bytearray(data)
    q[off + cnt - 1] ^= 0x01
    return bytes(q)


def test_a_corrupt_chunk_matters_in_the_chosen_level_only():
    import aerial_mapper_amd as A
    data, raster = _dem()
    with _map(32, 24, res=1.0) as m:
        rng = np.random.default_rng(5)
        before = rng.random((m.cols, m.rows)).astype(np.float32)
        m.set("elevation", before)
        for level in (2, -1):
            with pytest.raises(A.AmhipError) as ei:
                A.layer_from_geotiff(m, "elevation", _broken_level(data, 2, 1), level=level)
            text = str(ei.value)
            assert "amhip_layer_decode_geotiff_level" in text and "level 2: chunk 1 (tile row 0, column 1)" in text, text
            assert "Adler-32" in text
            assert same(m.get("elevation"), before)
        want = _placed(m, data, 2)
        for other in (0, 1):
            assert same(_placed(m, _broken_level(data, other, 3), 2), want)
            assert same(_placed(m, _broken_level(data, other, 3), -1), want)
    with pytest.raises(A.AmhipError) as ei, _map() as m:
        A.decode_geotiff(m, _broken_level(data, 1, 5), level=1)
    assert "amhip_geotiff_decode_level_dev" in str(ei.value) and "level 1: chunk 5 (tile row 1, column 1)" in str(ei.value)


def test_levels_the_rules_refuse_are_named(m8):
    import aerial_mapper_amd as A
    for name, (data, level, word) in PI.refused_chains().items():
        with pytest.raises(A.AmhipError) as ei:
            A.decode_geotiff(m8, data, level=level) if level else A.layer_from_geotiff(m8, "elevation", data, level=-1)
        assert word in str(ei.value), (name, str(ei.value))


# ---- the session and the C++ members ------------------------------------------------------------------------
def _ncam(A, sc):
    c = sc.cam
    return A.NCamera(c.fu, c.fv, c.cu, c.cv, c.width, c.height)


def test_a_session_writes_the_single_contexts_pyramid_and_reads_a_level(tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    sc = S.Scene(24.0, 16.0, 0.5, 3000, seed=11, num_frames=3, point_extent=6.0)
    g = sc.grid
    st = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)
    f = str(tmp_path / "dsm.tif")
    with A.HostSession(st, tiles=(2, 1)) as hs, A.AerialGridMap(st, device=0) as m:
        assert hs.num_windows == 2
        hs.dsm_process(A.DsmSettings(1), sc.points)
        elev = hs.layers["elevation"].copy()
        m.set("elevation", elev)
        for kind, lo, hi in (("f32", 0.0, 255.0), ("u8", 380.0, 420.0)):
            E.session_layer_to_geotiff(hs, "elevation", f, kind, lo, hi, 32, True, 16, overviews=-1)
            got = open(f, "rb").read()
            want = E.encode_layer_geotiff(m, "elevation", kind, lo, hi, 32, True, 16, overviews=-1)
            assert got == want and len(P.levels(got)) >= 2, (kind, _where(got, want))
        E.session_layer_to_geotiff(hs, "elevation", f, "f32", tile=16, overviews=1)
    data = open(f, "rb").read()
    lvl, info = P.decode(data, 1)
    # a map of twice the cell size over the same ground takes level 1, by number and by choice
    st2 = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, 2 * g.resolution)
    for level in (1, -1):
        with A.HostSession(st2, tiles=(2, 2)) as hs:
            before = hs.layers["elevation"].copy()
            A.session_layer_from_geotiff(hs, "elevation", f, hs.layers["elevation"], level=level)
            want = R.place(before, hs.grid, (0, 0, hs.grid.rows, hs.grid.cols), info, lvl)
            assert same(hs.layers["elevation"], want) and np.isfinite(want).any()
    with A.HostSession(st, tiles=(2, 2)) as hs:
        A.session_layer_from_geotiff(hs, "elevation", f, hs.layers["elevation"], level=-1)     # the base fits
        assert same(hs.layers["elevation"], elev)
        up0 = hs.transfer_stats()[0]
        hs.ortho_process(_ncam(A, sc), A.OrthoSettings(), sc.poses, sc.frames)
        assert hs.transfer_stats()[0] == up0           # the content sums agree: no layer byte went up
        bad = str(tmp_path / "bad.tif")
        open(bad, "wb").write(_broken_level(data, 1, 0))
        with pytest.raises(A.AmhipError) as ei:
            A.session_layer_from_geotiff(hs, "elevation", bad, hs.layers["elevation"], level=1)
        assert "amhip_session_layer_read_geotiff_level" in str(ei.value) and "level 1: chunk 0" in str(ei.value)
        assert same(hs.layers["elevation"], elev)


def test_the_cpp_members_write_and_read_what_the_python_calls_do(tmp_path):
    """tests/cpp/shim_geotiff_pyramid.cc: writeLayerToGeoTiff with overviews, loadLayerFromGeoTiff with a level"""
    from aerial_mapper_amd import build
    from aerial_mapper_amd import export as E
    import aerial_mapper_amd as A
    build.build_all()
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    exe = str(tmp_path / "shim_geotiff_pyramid")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_geotiff_pyramid.cc"), "-o", exe,
                           "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["ok", "66", "94"], (out.stdout, out.stderr[-2000:])
    blob = open(str(tmp_path / "layers.bin"), "rb").read()
    rows, cols = struct.unpack_from("<ii", blob, 0)
    layers = np.frombuffer(blob[8:], np.float32).reshape(3, cols, rows)     # written, read at level 1, read by choice
    with A.AerialGridMap(A.GridMapSettings(464980.0, 5272690.0, 16.5, 23.5, 0.25), device=0) as m:
        assert (m.rows, m.cols) == (rows, cols)
        m.set("elevation", layers[0])
        got = open(str(tmp_path / "elevation.tif"), "rb").read()
        want = E.encode_layer_geotiff(m, "elevation", "f32", 0.0, 255.0, 32, True, 256, overviews=2)
        assert got == want and len(P.levels(got)) == 3, _where(got, want)
        assert same(layers[1], _placed(m, got, 1)) and not same(layers[1], layers[0])
        assert same(layers[2], _placed(m, got, -1)) and same(layers[2], layers[0])
