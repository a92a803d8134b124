"""GPU: the tiled Deflate GeoTIFF encoder (amhip_tiff_encode.hip).  Byte identity with
tests/golden/geotiff/ (zlib 1.2.11's own streams) and with tests/geotiff_reference.py; round trips
through its inverse; Pillow only where it imports."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import geotiff_inputs as GI
import geotiff_reference as GR
import scenarios as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "geotiff")
RES = 0.5


def _where(got, ref):
    at = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    return "sizes %d / %d, first differing byte %d" % (len(got), len(ref), at)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _map(rows=8, cols=8, window=None, center=(464980.0, 5272690.0)):
    import aerial_mapper_amd as A
    m = A.AerialGridMap(A.GridMapSettings(center[0], center[1], rows * RES, cols * RES, RES), device=0, window=window)
    if window is None:
        assert (m.rows, m.cols) == (rows, cols)
    return m


@pytest.fixture(scope="module")
def m8():
    with _map() as m:
        yield m


def _check_pillow(data, raster):
    try:
        from PIL import Image
    except ImportError:
        return
    assert same(np.array(Image.open(io.BytesIO(data))), raster)


# ---- rasters ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GI.golden_cases()))
def test_the_committed_files_are_matched_byte_for_byte(m8, name):
    from aerial_mapper_amd import export as E
    raster, tile = GI.golden_cases()[name]
    assert same(np.load(os.path.join(GOLDEN, name + ".npy")), raster)
    want = open(os.path.join(GOLDEN, name + ".tif"), "rb").read()
    got = E.encode_geotiff(m8, raster, GI.GT, 32, True, tile)
    assert got == want, _where(got, want)
    assert same(GR.decode(got)["raster"], raster)


@pytest.mark.parametrize("kind", ["f32", "u8", "rgb8"])
@pytest.mark.parametrize("h,w", GI.EDGE_SIZES)
def test_the_smallest_rasters_that_reach_each_edge(m8, kind, h, w):
    from aerial_mapper_amd import export as E
    raster = GI.edge_raster(kind, h, w)
    got = E.encode_geotiff(m8, raster, GI.GT, 33, False, 16)
    want = GR.encode(raster, GI.GT, 33, False, 16)
    assert got == want, _where(got, want)
    back = GR.decode(got)
    assert back["kind"] == kind and same(back["raster"], raster) and back["geotransform"] == GI.GT
    assert back["epsg"] == 32733
    _check_pillow(got, raster)


def _big_cases():
    one = np.full((200, 150), np.float32(7.0))
    one[131, 77] = np.float32(7.5)
    return {
        "f32_noise_t128": (GI.noise("f32", 128), 128),                 # 64 KB a tile: several stored blocks
        "rgb8_noise_t128": (GI.noise("rgb8", 128), 128),               # 48 KB a tile
        "f32_noise_200x300_t128": (GI.noise("f32", 300, seed=2)[:200], 128),   # six tiles, partial edges
        "terrain_t64": (GI.terrain(150, 170), 64),
        "terrain_t48": (GI.terrain(100, 100), 48),                     # a row of 192 bytes: pieces start mid-row
        "rgb8_t1024": (GI.edge_raster("rgb8", 40, 1100), 1024),        # a row of 3072 bytes
        "f32_t1024": (GI.terrain(30, 1030), 1024),                     # a row of 4096 bytes
        "u8_default_tile": (GI.edge_raster("u8", 300, 260), 0),        # 0 means 256
        "constant_but_one": (one, 64),
        "u8_all255": (np.full((70, 90), 255, np.uint8), 32),
    }


@pytest.mark.parametrize("name", sorted(_big_cases()))
def test_more_pieces_blocks_and_runs_per_tile(m8, name):
    import torch
    from aerial_mapper_amd import export as E
    raster, tile = _big_cases()[name]
    want = GR.encode(raster, GI.GT, 32, True, tile)
    got = E.encode_geotiff(m8, raster, GI.GT, 32, True, tile)
    assert got == want, _where(got, want)
    # a device raster with padded rows
    t = torch.from_numpy(np.ascontiguousarray(raster)).to("cuda:0")
    pad = torch.zeros((raster.shape[0], raster.shape[1] + 5) + raster.shape[2:], dtype=t.dtype, device="cuda:0")
    pad[:, :raster.shape[1]] = t
    view = pad[:, :raster.shape[1]]
    assert view.stride(0) != t.stride(0)
    assert E.encode_geotiff(m8, view, GI.GT, 32, True, tile) == want
    assert same(GR.decode(got)["raster"], raster)


# ---- layers ----------------------------------------------------------------------------------------
def _layers(rows, cols, seed=3):
    rng = np.random.default_rng(seed)
    elev = (400.0 + 10.0 * rng.random((cols, rows))).astype(np.float32)
    elev[rng.random((cols, rows)) < 0.15] = np.nan
    elev[: cols // 4] = 401.25                      # a flat area: runs
    ortho = (rng.random((cols, rows)) * 300.0 - 20.0).astype(np.float32)
    ortho[rng.random((cols, rows)) < 0.1] = np.nan
    packed = np.full((cols, rows), np.nan, np.float32)
    keep = rng.random((cols, rows)) < 0.8
    packed.view(np.uint32)[keep] = rng.integers(0, 1 << 24, (cols, rows), dtype=np.uint32)[keep]
    return {"elevation": elev, "ortho": ortho, "colored_ortho": packed}


LAYER_KINDS = [("elevation", "f32", 0.0, 255.0), ("ortho", "u8", 0.0, 255.0), ("elevation", "u8", 395.0, 412.0),
               ("colored_ortho", "rgb8", 0.0, 255.0)]


@pytest.mark.parametrize("tile", [16, 256])
def test_layers_leave_as_the_north_up_raster_of_their_definition(tile, tmp_path):
    from aerial_mapper_amd import export as E
    rows, cols = 33, 47
    with _map(rows, cols) as m:
        for name, a in _layers(rows, cols).items():
            m.set(name, a)
        gt = GR.layer_geotransform(m.grid, m.window)
        assert gt == (464980.0 - rows * RES / 2, RES, 0.0, 5272690.0 + cols * RES / 2, 0.0, -RES)
        for name, kind, lo, hi in LAYER_KINDS:
            raster = GR.layer_raster(m.get(name), kind, lo, hi)
            assert raster.shape[:2] == (cols, rows)          # width = rows: a transposition shows
            want = GR.encode(raster, gt, 32, True, tile)
            got = E.encode_layer_geotiff(m, name, kind, lo, hi, 32, True, tile)
            assert got == want, (name, kind, _where(got, want))
            f = str(tmp_path / ("%s_%s.tif" % (name, kind)))
            E.layer_to_geotiff(m, name, f, kind, lo, hi, 32, True, tile)
            assert open(f, "rb").read() == want
            back = GR.decode(got)
            assert same(back["raster"], raster) and back["geotransform"] == gt
            if kind == "u8":
                # the pixels of layer_to_image, reoriented
                img = E.layer_to_image(m, name, lo, hi)
                assert np.array_equal(raster, img[::-1, :].T)
            _check_pillow(got, raster)


def test_a_windowed_map_carries_its_own_geotransform():
    from aerial_mapper_amd import export as E
    rows, cols = 40, 30
    window = (8, 5, 17, 21)
    with _map(rows, cols, window=window) as m:
        a = _layers(17, 21, seed=9)["elevation"]
        m.set("elevation", a)
        got = E.encode_layer_geotiff(m, "elevation", "f32", tile=16)
        back = GR.decode(got)
        x0 = 464980.0 - rows * RES / 2 + RES * float(rows - 8 - 17)
        y0 = 5272690.0 + cols * RES / 2 - RES * 5.0
        assert back["geotransform"] == (x0, RES, 0.0, y0, 0.0, -RES)
        assert back["raster"].shape == (21, 17) and same(back["raster"], GR.layer_raster(a, "f32"))
        assert got == GR.encode(GR.layer_raster(a, "f32"), back["geotransform"], 32, True, 16)
        # the cell behind raster pixel (r, c): its centre lies half a pixel inside the pixel's corner
        from aerial_mapper_amd import hip_lib as L
        r, c = 3, 4
        x, y = L.cell_position(m.grid, 8 + (17 - 1 - c), 5 + r)
        assert abs(x - (x0 + (c + 0.5) * RES)) < 1e-9 and abs(y - (y0 - (r + 0.5) * RES)) < 1e-9


def test_the_map_as_initialised_and_an_all_255_ortho_are_runs_across_pieces_planes_and_rows():
    from aerial_mapper_amd import export as E
    rows, cols = 70, 50
    with _map(rows, cols) as m:
        gt = GR.layer_geotransform(m.grid, m.window)
        nan = m.get("elevation")
        assert np.isnan(nan).all()
        got = E.encode_layer_geotiff(m, "elevation", "f32", tile=64)
        want = GR.encode(GR.layer_raster(nan, "f32"), gt, 32, True, 64)
        assert got == want, _where(got, want)
        assert len(got) < 2000                       # (14 000 bytes of samples, 65 536 of tiles)
        m.set("ortho", np.full((cols, rows), 255.0, np.float32))
        got = E.encode_layer_geotiff(m, "ortho", "u8", tile=64)
        raster = GR.layer_raster(m.get("ortho"), "u8")
        assert (raster == 255).all()
        want = GR.encode(raster, gt, 32, True, 64)
        assert got == want, _where(got, want)


def test_heights_of_a_real_dsm_come_back_bit_for_bit():
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    sc = S.Scene(24.0, 16.0, 0.5, 3000, seed=11, num_frames=1, point_extent=6.0)   # (the map's rim stays NaN)
    g = sc.grid
    with A.AerialGridMap(A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution), device=0) as m:
        A.Dsm(A.DsmSettings(1), m).process(sc.points, m)
        elev = m.get("elevation")
        assert np.isnan(elev).any() and np.isfinite(elev).any()
        back = GR.decode(E.encode_layer_geotiff(m, "elevation", "f32", tile=32))
        north = back["raster"]
        assert north.shape == (m.cols, m.rows)
        assert same(north, np.ascontiguousarray(elev[:, ::-1]))
        assert np.array_equal(np.isnan(north), np.isnan(elev[:, ::-1]))


# ---- grouping, caps, files ---------------------------------------------------------------------------
def test_the_bytes_do_not_depend_on_the_grouping(m8):
    from aerial_mapper_amd import export as E
    from aerial_mapper_amd import hip_lib as L
    raster = GI.edge_raster("f32", 16, 80)          # five tiles of 1024 predictor bytes
    one = E.encode_geotiff(m8, raster, GI.GT, 32, True, 16)
    assert one == GR.encode(raster, GI.GT, 32, True, 16) and len(GR.decode(one)["streams"]) == 5
    # What a tile of 1024 bytes costs (amhip_deflate_rle.h: make_layout, every buffer rounded up to 256
    # bytes): 4096 of pieces + 8192 of symbols + 6 tables of 256 + 256 + 256 of block places + 1536 of
    # block codes + 1280 of stream + 3 * 256 = 17 920 bytes.  Two fit 0.04 MB (41 943 bytes), three do not;
    # 0.02 MB holds one.
    try:
        for mb, groups in ((0.04, "2 + 2 + 1"), (0.02, "one each")):
            L.set_tuning("tiffe_scratch_budget_mb", mb)
            assert E.encode_geotiff(m8, raster, GI.GT, 32, True, 16) == one, groups
    finally:
        L.set_tuning("tiffe_scratch_budget_mb", None)


def test_a_buffer_one_byte_too_small_is_refused_and_left_untouched(m8):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    raster = GI.edge_raster("u8", 33, 47)
    want = GR.encode(raster, GI.GT, 32, True, 16)
    dev = torch.from_numpy(raster).to("cuda:0")
    gt = (C.c_double * 6)(*GI.GT)
    n = C.c_size_t()
    for cap, ok in ((len(want) - 1, False), (len(want), True)):
        out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rc = lib.amhip_geotiff_encode_dev(m8._h, C.c_void_p(dev.data_ptr()), 47, 47, 33, 1, 16, gt, 32, 1,
                                          C.c_void_p(out.data_ptr()), cap, C.byref(n))
        host = out.cpu().numpy()
        assert n.value == len(want)
        if ok:
            assert rc == L.OK and host[:len(want)].tobytes() == want and (host[len(want):] == 0xA5).all()
        else:
            assert rc == L.ERR_ARG and "nothing written" in L.last_error() and (host == 0xA5).all()
    assert lib.amhip_geotiff_bound(47, 33, 1, 16) >= len(want)


def test_written_files_equal_encoded_ones_and_a_bad_path_names_the_file(m8, tmp_path):
    from aerial_mapper_amd import export as E
    from aerial_mapper_amd import hip_lib as L
    import torch
    for kind in ("f32", "u8", "rgb8"):
        raster = GI.edge_raster(kind, 33, 47)
        want = GR.encode(raster, GI.GT, 32, True, 16)
        f = str(tmp_path / (kind + ".tif"))
        E.write_geotiff_deflate(m8, f, raster, GI.GT, 32, True, 16)
        assert open(f, "rb").read() == want
        E.write_geotiff_deflate(m8, f + ".dev", torch.from_numpy(raster).to("cuda:0"), GI.GT, 32, True, 16)
        assert open(f + ".dev", "rb").read() == want
    bad = str(tmp_path / "no_such_dir" / "x.tif")
    with pytest.raises(L.AmhipError) as ei:
        E.write_geotiff_deflate(m8, bad, GI.edge_raster("u8", 16, 16), GI.GT, 32, True, 16)
    assert ei.value.status == L.ERR_ARG and bad in str(ei.value) and "No such file" in str(ei.value)
    with pytest.raises(L.AmhipError) as ei:
        E.layer_to_geotiff(m8, "elevation", bad)
    assert ei.value.status == L.ERR_ARG and bad in str(ei.value)


def test_every_argument_error_names_the_export_and_the_field(m8):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    dev = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p, o = C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr())
    up = (C.c_double * 6)(*GI.GT)
    n = C.c_size_t()
    h = m8._h

    def enc(raster=p, step=64, w=16, hh=16, kind=1, tile=16, gt=up, zone=32, dst=o, nb=C.byref(n), ctx=h):
        return lib.amhip_geotiff_encode_dev(ctx, raster, step, w, hh, kind, tile, gt, zone, 1, dst, 1 << 16, nb)

    def wr(name=b"unused.tif", raster=p, step=64, w=16, hh=16, kind=1, tile=16, gt=up, zone=32, ctx=h):
        return lib.amhip_geotiff_write(ctx, name, raster, 1, step, w, hh, kind, tile, gt, zone, 1)

    rot = (C.c_double * 6)(1.0, 0.5, 0.25, 2.0, 0.0, -0.5)
    flip = (C.c_double * 6)(1.0, 0.5, 0.0, 2.0, 0.0, 0.5)
    cases = [
        (lambda: enc(ctx=None), "null"), (lambda: enc(raster=None), "null"), (lambda: enc(gt=None), "null"),
        (lambda: enc(dst=None), "null"), (lambda: enc(nb=None), "null"),
        (lambda: enc(w=0), "width"), (lambda: enc(w=65536), "width"), (lambda: enc(hh=0), "height"),
        (lambda: enc(hh=65536), "height"), (lambda: enc(kind=3), "kind"), (lambda: enc(kind=-1), "kind"),
        (lambda: enc(tile=8), "tile"), (lambda: enc(tile=24), "tile"), (lambda: enc(tile=1040), "tile"),
        (lambda: enc(step=15), "step"), (lambda: enc(kind=0, step=63), "step"), (lambda: enc(kind=2, step=47), "step"),
        (lambda: enc(gt=rot), "geotransform"), (lambda: enc(gt=flip), "geotransform"),
        (lambda: enc(zone=0), "utm_zone"), (lambda: enc(zone=61), "utm_zone"),
    ]
    for call, word in cases:
        assert call() == L.ERR_ARG
        assert "amhip_geotiff_encode_dev" in L.last_error() and word in L.last_error(), (word, L.last_error())
    for call, word in [(lambda: wr(ctx=None), "null"), (lambda: wr(name=None), "null"), (lambda: wr(raster=None), "null"),
                       (lambda: wr(gt=None), "null"), (lambda: wr(w=0), "width"), (lambda: wr(kind=5), "kind"),
                       (lambda: wr(tile=17), "tile"), (lambda: wr(step=3), "step"), (lambda: wr(gt=rot), "geotransform"),
                       (lambda: wr(zone=99), "utm_zone")]:
        assert call() == L.ERR_ARG
        assert "amhip_geotiff_write" in L.last_error() and word in L.last_error(), (word, L.last_error())

    def lay(fn, layer=1, kind=0, lo=0.0, hi=255.0, tile=16, zone=32, ctx=h, name=b"unused.tif", dst=o, nb=C.byref(n)):
        if fn == "amhip_layer_encode_geotiff_dev":
            return lib.amhip_layer_encode_geotiff_dev(ctx, layer, kind, lo, hi, tile, zone, 1, dst, 1 << 16, nb)
        return lib.amhip_layer_write_geotiff(ctx, layer, kind, lo, hi, tile, zone, 1, name)

    for fn in ("amhip_layer_encode_geotiff_dev", "amhip_layer_write_geotiff"):
        cases = [(dict(ctx=None), "null"), (dict(layer=6), "layer"), (dict(layer=-1), "layer"), (dict(kind=3), "kind"),
                 (dict(tile=100), "tile"), (dict(zone=0), "utm_zone"), (dict(kind=1, lo=5.0, hi=5.0), "upper <= lower"),
                 (dict(kind=1, lo=5.0, hi=float("nan")), "upper <= lower")]
        cases += [(dict(dst=None), "null"), (dict(nb=None), "null")] if fn.endswith("_dev") else [(dict(name=None), "null")]
        for kw, word in cases:
            assert lay(fn, **kw) == L.ERR_ARG
            assert fn in L.last_error() and word in L.last_error(), (fn, word, L.last_error())
    assert lib.amhip_geotiff_bound(0, 5, 0, 16) == 0 and lib.amhip_geotiff_bound(5, 5, 0, 20) == 0
    assert lib.amhip_session_layer_write_geotiff(None, 1, 0, 0.0, 255.0, 16, 32, 1, b"unused.tif") == L.ERR_ARG
    assert "amhip_session_layer_write_geotiff" in L.last_error() and "null" in L.last_error()


# ---- session and the C++ member ------------------------------------------------------------------------
def test_a_session_of_two_windows_writes_the_single_contexts_file(tmp_path):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    from aerial_mapper_amd import hip_lib as L
    sc = S.Scene(24.0, 16.0, 0.5, 3000, seed=5, num_frames=1, point_extent=6.0)
    g = sc.grid
    st = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)
    with A.HostSession(st, tiles=(2, 1)) as hs, A.AerialGridMap(st, device=0) as m:
        assert hs.num_windows == 2
        hs.dsm_process(A.DsmSettings(1), sc.points)
        elev = hs.layers["elevation"]
        assert np.isnan(elev).any() and np.isfinite(elev).any()
        m.set("elevation", elev)
        for kind, lo, hi in (("f32", 0.0, 255.0), ("u8", 380.0, 420.0)):
            f = str(tmp_path / (kind + ".tif"))
            E.session_layer_to_geotiff(hs, "elevation", f, kind, lo, hi, 32, True, 16)
            got = open(f, "rb").read()
            want = E.encode_layer_geotiff(m, "elevation", kind, lo, hi, 32, True, 16)
            assert got == want, (kind, _where(got, want))
            assert same(GR.decode(got)["raster"], GR.layer_raster(elev, kind, lo, hi))
        f = str(tmp_path / "colour.tif")
        E.session_layer_to_geotiff(hs, "colored_ortho", f, "rgb8", tile=16)
        assert open(f, "rb").read() == E.encode_layer_geotiff(m, "colored_ortho", "rgb8", tile=16)
        with pytest.raises(L.AmhipError) as ei:
            E.session_layer_to_geotiff(hs, "elevation", f, "u8", 1.0, 1.0)
        assert "amhip_session_layer_write_geotiff" in str(ei.value) and "upper <= lower" in str(ei.value)


def test_the_cpp_member_writes_the_python_calls_bytes(tmp_path):
    """tests/cpp/shim_geotiff.cc: io::AerialMapperIO::writeLayerToGeoTiff"""
    from aerial_mapper_amd import build
    from aerial_mapper_amd import export as E
    import aerial_mapper_amd as A
    build.build_all()
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    exe = str(tmp_path / "shim_geotiff")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_geotiff.cc"), "-o", exe,
                           "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["ok", "33", "47"], (out.stdout, out.stderr[-2000:])
    blob = open(str(tmp_path / "layers.bin"), "rb").read()
    rows, cols = np.frombuffer(blob[:8], np.int32)
    layers = np.frombuffer(blob[8:], np.float32).reshape(2, cols, rows)
    with A.AerialGridMap(A.GridMapSettings(464980.0, 5272690.0, 16.5, 23.5, 0.5), device=0) as m:
        assert (m.rows, m.cols) == (rows, cols)
        m.set("elevation", layers[0])
        m.set("colored_ortho", layers[1])
        for name, kind, zone, north in (("elevation", "f32", 32, True), ("colored_ortho", "rgb8", 19, False)):
            got = open(str(tmp_path / (name + ".tif")), "rb").read()
            want = E.encode_layer_geotiff(m, name, kind, 0.0, 255.0, zone, north, 256)
            assert got == want, (name, _where(got, want))
            back = GR.decode(got)
            assert back["epsg"] == (32600 if north else 32700) + zone
            assert same(back["raster"], GR.layer_raster(layers[0 if kind == "f32" else 1], kind))
