"""GPU: the GeoTIFF reader (amhip_tiff_decode.hip) against tests/geotiff_read_reference.py:
decode and placement bit for bit, round trips with the writer, only the needed chunks decoded, errors
that leave the layer as it was, the session and the tuning key.  Committed files and the test writer
only: nothing here needs Pillow."""
import os
import struct

import numpy as np
import pytest

import geotiff_inputs as GI
import geotiff_read_inputs as RI
import geotiff_read_reference as R
import scenarios as S

pytestmark = pytest.mark.gpu

RES = 0.5
CENTER = (464980.0, 5272690.0)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _host(t):
    """a device tensor of any of the reader's dtypes -> numpy (bytes first: not every torch has a uint16 numpy bridge)"""
    import torch
    np_dtype = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int16: np.int16,
                getattr(torch, "uint16", None): np.uint16}[t.dtype]
    c = t.contiguous()
    raw = c.view(torch.uint8).cpu().numpy() if c.numel() else np.zeros(0, np.uint8)
    return np.ascontiguousarray(raw).view(np_dtype).reshape(tuple(t.shape))


def _map(rows=8, cols=8, window=None, center=CENTER, res=RES):
    import aerial_mapper_amd as A
    return A.AerialGridMap(A.GridMapSettings(center[0], center[1], rows * res, cols * res, res), device=0, window=window)


@pytest.fixture(scope="module")
def m8():
    with _map() as m:
        yield m


@pytest.fixture(scope="module")
def variants():
    return RI.variants()


# ---- decode equals the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RI.variants()))
def test_every_variant_decodes_to_its_raster_bit_for_bit(m8, variants, name):
    import aerial_mapper_amd as A
    data, raster = variants[name]
    got, info = A.decode_geotiff(m8, data)
    assert same(_host(got), raster), name
    want = R.parse(data)
    assert info["kind"] == want["kind"] and info["geotransform"] == want["geotransform"]
    assert info["has_geo"] == want["has_geo"] and info["predictor"] == want["predictor"]


@pytest.mark.parametrize("path", RI.fixture_paths(), ids=os.path.basename)
def test_the_committed_files_decode_to_their_rasters(m8, path):
    """libtiff's files (dynamic blocks at its default level, strips of about 64 KB or of a chosen
    RowsPerStrip) and the GPU writer's own"""
    import aerial_mapper_amd as A
    got, info = A.decode_geotiff(m8, path)
    assert same(_host(got), np.load(path[:-4] + ".npy")), path


WINDOW_FILES = ["f32_p3_33x47_t16", "f32_p3_33x47_t32x16", "f32_p3_17x16_rps_3", "rgb8_p2_33x47_t16",
                "i16_p2_33x47_t16", "f32_p2_3x300_strip", "u8_p2_33x47_strip_none", "f32_p3_33x47_t16_none"]


@pytest.mark.parametrize("name", WINDOW_FILES)
def test_pixel_windows_that_cut_tiles_and_strips(m8, variants, name):
    import aerial_mapper_amd as A
    data, raster = variants[name]
    h, w = raster.shape[:2]
    px = R.pixel_bytes(R.kind_of(raster))
    windows = [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 3, h // 3, w - w // 3, h - h // 3),
               (0, h // 2, w, 1), (w // 2, 0, 1, h), (min(15, w - 1), min(15, h - 1), min(3, w - min(15, w - 1)),
                                                      min(3, h - min(15, h - 1)))]
    for x0, y0, ww, hh in windows:
        got, _ = A.decode_geotiff(m8, data, (x0, y0, ww, hh))
        assert same(_host(got), raster[y0:y0 + hh, x0:x0 + ww]), (name, x0, y0, ww, hh)
        # rows further apart than they are long: the padding stays as it was (zero)
        step = ww * px + 8
        padded, _ = A.decode_geotiff(m8, data, (x0, y0, ww, hh), step=step)
        assert same(_host(padded), raster[y0:y0 + hh, x0:x0 + ww]), (name, x0, y0, ww, hh, "step")


def test_a_window_outside_the_raster_and_a_short_step_are_refused(m8, variants):
    import aerial_mapper_amd as A
    data, raster = variants["f32_p3_33x47_t16"]
    for window, word in (((40, 0, 8, 8), "window"), ((0, 0, 0, 4), "window"), ((-1, 0, 4, 4), "window"),
                         ((0, 30, 4, 4), "window")):
        with pytest.raises(A.AmhipError) as ei:
            A.decode_geotiff(m8, data, window)
        assert "amhip_geotiff_decode_dev" in str(ei.value) and word in str(ei.value)
    with pytest.raises(A.AmhipError) as ei:
        A.decode_geotiff(m8, data, (0, 0, 8, 8), step=28)
    assert "step" in str(ei.value)
    with pytest.raises(A.AmhipError) as ei:
        A.decode_geotiff(m8, data, (0, 0, 8, 8), step=34)
    assert "multiples of the sample's size" in str(ei.value)


# ---- only what is needed is decoded; errors ----------------------------------------------------------------
def _tag_values_at(data, tag):
    """file offset of the values of `tag` in the first IFD (LONGs)"""
    ifd, = struct.unpack_from("<I", data, 4)
    n, = struct.unpack_from("<H", data, ifd)
    for k in range(n):
        t, typ, count, value = struct.unpack_from("<HHII", data, ifd + 2 + 12 * k)
        if t == tag:
            return value if count * 4 > 4 else ifd + 2 + 12 * k + 8
    raise KeyError(tag)


def _broken(data, t, how):
    """the file with chunk t damaged"""
    p = R.parse(data)
    off, cnt, _ = p["chunks"][t]
    q = bytearray(data)
    if how == "flip":
        q[off + cnt // 2] ^= 0x55
    elif how == "adler":
        q[off + cnt - 1] ^= 0x01
    else:   # the stream ends early: the chunk's byte count says so
        struct.pack_into("<I", q, _tag_values_at(data, 325) + 4 * t, cnt - 8)
    return bytes(q)


@pytest.fixture(scope="module")
def nine():
    raster = RI.nine_tiles()
    return R.write(raster, tile=(16, 16), predictor=3, gt=GI.GT, level=6), raster


def test_a_damaged_tile_outside_the_window_does_not_matter_and_one_inside_is_named(m8, nine):
    import aerial_mapper_amd as A
    data, raster = nine
    assert len(R.parse(data)["chunks"]) == 9
    window = (0, 0, 32, 32)                       # tiles (0..1, 0..1)
    for how in ("flip", "adler", "short"):
        outside = _broken(data, 8, how)           # tile row 2, column 2
        got, _ = A.decode_geotiff(m8, outside, window)
        assert same(_host(got), raster[:32, :32]), how
        inside = _broken(data, 4, how)            # tile row 1, column 1
        with pytest.raises(A.AmhipError) as ei:
            A.decode_geotiff(m8, inside, window)
        text = str(ei.value)
        assert "chunk 4 (tile row 1, column 1)" in text and "inflate status" in text, (how, text)
        if how == "adler":
            assert "Adler-32 mismatch" in text
        if how == "short":
            assert "ends before" in text or "undefined" in text or "fewer" in text, text
        # a window that leaves the damaged tile out still decodes
        got, _ = A.decode_geotiff(m8, inside, (0, 0, 16, 48))
        assert same(_host(got), raster[:48, :16]), how


def test_strips_are_named_by_their_number(m8, variants):
    import aerial_mapper_amd as A
    data, _ = variants["f32_p3_17x16_rps_3"]
    with pytest.raises(A.AmhipError) as ei:
        A.decode_geotiff(m8, _broken(data, 2, "adler"))
    assert "chunk 2 (strip 2)" in str(ei.value)


def test_after_an_error_the_layer_is_bit_for_bit_what_it_was(nine):
    import aerial_mapper_amd as A
    data, raster = nine
    rows, cols = 48, 48
    # a map that lies exactly on the file
    center = (GI.GT[0] + rows * RES / 2, GI.GT[3] - cols * RES / 2)
    with _map(rows, cols, center=center) as m:
        rng = np.random.default_rng(5)
        before = rng.random((cols, rows)).astype(np.float32)
        before[3, 4] = np.nan
        m.set("elevation", before)
        for how in ("flip", "adler", "short"):
            with pytest.raises(A.AmhipError) as ei:
                A.layer_from_geotiff(m, "elevation", _broken(data, 4, how))
            assert "amhip_layer_decode_geotiff" in str(ei.value) and "chunk 4 (tile row 1, column 1)" in str(ei.value)
            assert same(m.get("elevation"), before), how
        # ... and on a freshly reset map the pending reset is still pending: every cell NaN
        m.reset()
        with pytest.raises(A.AmhipError):
            A.layer_from_geotiff(m, "elevation", _broken(data, 4, "adler"))
        assert np.isnan(m.get("elevation")).all()
        A.layer_from_geotiff(m, "elevation", data)
        assert same(m.get("elevation"), np.ascontiguousarray(raster[:, ::-1]))


def test_layer_calls_refuse_what_they_cannot_place(m8, variants, tmp_path):
    import aerial_mapper_amd as A
    with pytest.raises(A.AmhipError) as ei:
        A.layer_from_geotiff(m8, "elevation", variants["f32_p3_33x47_t16_nogeo"][0])
    assert "no geo tags" in str(ei.value)
    with pytest.raises(A.AmhipError) as ei:
        A.layer_from_geotiff(m8, "elevation", variants["rgb8_p2_33x47_t16"][0])
    assert "colored_ortho" in str(ei.value)
    with pytest.raises(A.AmhipError) as ei:
        A.layer_from_geotiff(m8, 6, variants["f32_p3_33x47_t16"][0])
    assert "layer" in str(ei.value)
    missing = str(tmp_path / "no_such.tif")
    with pytest.raises(A.AmhipError) as ei:
        A.layer_from_geotiff(m8, "elevation", missing)
    assert missing in str(ei.value) and "amhip_layer_read_geotiff" in str(ei.value)
    for what, (data, word) in list(RI.refusals().items())[:6]:
        with pytest.raises(A.AmhipError) as ei:
            A.decode_geotiff(m8, data)
        assert word in str(ei.value), what


# ---- round trips with the writer ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GI.golden_cases()))
def test_what_the_gpu_writer_encodes_the_gpu_reader_decodes(m8, name):
    import aerial_mapper_amd as A
    raster, tile = GI.golden_cases()[name]
    data = A.encode_geotiff(m8, raster, GI.GT, 32, True, tile)
    got, info = A.decode_geotiff(m8, data)
    assert same(_host(got), raster)
    assert info["geotransform"] == GI.GT and info["epsg"] == 32632 and info["tile_width"] == tile


@pytest.mark.parametrize("kind", ["f32", "u8", "rgb8"])
def test_edge_rasters_round_trip_through_both_hemispheres(m8, kind):
    import aerial_mapper_amd as A
    for h, w in GI.EDGE_SIZES:
        raster = GI.edge_raster(kind, h, w)
        got, info = A.decode_geotiff(m8, A.encode_geotiff(m8, raster, GI.GT, 33, False, 16))
        assert same(_host(got), raster), (kind, h, w)
        assert info["geotransform"] == GI.GT and info["epsg"] == 32733 and info["kind"] == kind


def _elevation(rows, cols, seed=3):
    rng = np.random.default_rng(seed)
    elev = (400.0 + 10.0 * rng.random((cols, rows))).astype(np.float32)
    elev[rng.random((cols, rows)) < 0.15] = np.nan
    return elev


def test_a_layer_round_trips_onto_a_fresh_map_and_through_a_window(tmp_path):
    import aerial_mapper_amd as A
    rows, cols = 33, 47
    elev = _elevation(rows, cols)
    packed = np.random.default_rng(4).integers(0, 1 << 24, (cols, rows), dtype=np.uint32).view(np.float32)
    with _map(rows, cols) as src:
        src.set("elevation", elev)
        src.set("colored_ortho", packed)
        data = A.encode_layer_geotiff(src, "elevation", "f32", tile=16)
        colour = A.encode_layer_geotiff(src, "colored_ortho", "rgb8", tile=16)
        path = str(tmp_path / "elevation.tif")
        A.layer_to_geotiff(src, "elevation", path, "f32", tile=16)
    with _map(rows, cols) as m:
        A.layer_from_geotiff(m, "elevation", data)
        assert same(m.get("elevation"), elev) and np.isnan(elev).any()      # the NaN cells: the fresh map's own
        m.reset()
        A.layer_from_geotiff(m, "elevation", path)
        assert same(m.get("elevation"), elev)
        # the file's NaN pixels leave a sentinel alone
        m.set("ortho", np.full((cols, rows), -7.0, np.float32))
        A.layer_from_geotiff(m, "ortho", data)
        want = np.where(np.isnan(elev), np.float32(-7.0), elev)
        assert same(m.get("ortho"), want)
        A.layer_from_geotiff(m, "colored_ortho", colour)
        assert same(m.get("colored_ortho"), packed)
    window = (8, 5, 17, 21)
    with _map(rows, cols, window=window) as m:
        A.layer_from_geotiff(m, "elevation", data)
        assert same(m.get("elevation"), elev[5:26, 8:25])


# ---- placement on a foreign grid ------------------------------------------------------------------------
def _file_for_placement(kind, h, w, gt, **kw):
    if kind == "f32":
        raster = GI.terrain(h, w) + np.arange(w, dtype=np.float32)[None, :] * np.float32(0.01)
        raster[2, 3] = np.nan
    else:
        raster = RI.words16(h, w, True)
    if "nodata" in kw:
        raster = raster.copy()
        raster[::3, ::4] = -9999
    return R.write(raster, tile=(16, 16), predictor=3 if kind == "f32" else 2, gt=gt, **kw), raster


PLACEMENTS = {
    # name: (kind, file height, width, geotransform, writer options)
    "coarser file under a finer map": ("f32", 20, 22, (CENTER[0] - 10.0, 1.0, 0.0, CENTER[1] + 9.0, 0.0, -1.0), {}),
    "finer file with an offset origin": ("f32", 70, 60, (CENTER[0] - 7.13, 0.3, 0.0, CENTER[1] + 9.41, 0.0, -0.3), {}),
    "a file over a part of the map": ("f32", 20, 18, (CENTER[0] - 2.2, 0.5, 0.0, CENTER[1] + 3.1, 0.0, -0.5), {}),
    "a file that reaches past the map": ("f32", 90, 80, (CENTER[0] - 20.0, 0.5, 0.0, CENTER[1] + 20.0, 0.0, -0.5), {}),
    "nodata in floats": ("f32", 40, 40, (CENTER[0] - 10.0, 0.5, 0.0, CENTER[1] + 10.0, 0.0, -0.5), {"nodata": "-9999"}),
    "nodata in 16-bit integers": ("i16", 40, 40, (CENTER[0] - 10.0, 0.5, 0.0, CENTER[1] + 10.0, 0.0, -0.5),
                                  {"nodata": "-9999"}),
    "pixel is point": ("f32", 40, 40, (CENTER[0] - 10.0, 0.5, 0.0, CENTER[1] + 10.0, 0.0, -0.5),
                       {"pixel_is_point": True}),
    "a transformation matrix": ("f32", 40, 40, (CENTER[0] - 10.1, 0.7, 0.0, CENTER[1] + 10.3, 0.0, -0.6),
                                {"geo_form": "matrix"}),
    "a file beside the map": ("f32", 16, 16, (CENTER[0] + 100.0, 0.5, 0.0, CENTER[1], 0.0, -0.5), {}),
}


@pytest.mark.parametrize("name", sorted(PLACEMENTS))
def test_placement_equals_the_reference_bit_for_bit(name):
    import aerial_mapper_amd as A
    kind, h, w, gt, kw = PLACEMENTS[name]
    data, raster = _file_for_placement(kind, h, w, gt, **kw)
    info = R.parse(data)
    rows, cols = 33, 29
    sentinel = np.full((cols, rows), -123.5, np.float32)
    for window in (None, (4, 3, 20, 19)):
        with _map(rows, cols, window=window) as m:
            before = sentinel[:m.cols, :m.rows]
            m.set("elevation", before)
            A.layer_from_geotiff(m, "elevation", data)
            want = R.place(before, m.grid, m.window, info, raster)
            got = m.get("elevation")
            assert same(got, want), (name, window, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            changed = int((want != before).sum())
            if name == "a file beside the map":
                assert changed == 0
            else:
                assert 0 < changed
            if name in ("a file over a part of the map", "nodata in floats", "nodata in 16-bit integers") and window is None:
                assert changed < rows * cols          # cells that kept the sentinel
            # a fresh map: what the file does not give stays NaN
            m.reset()
            A.layer_from_geotiff(m, "elevation", data)
            want = R.place(np.full((m.cols, m.rows), np.nan, np.float32), m.grid, m.window, info, raster)
            assert same(m.get("elevation"), want), (name, window, "fresh")


# ---- the tuning key --------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_grouping(m8, nine):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib as L
    data, raster = nine
    one, _ = A.decode_geotiff(m8, data)
    assert same(_host(one), raster)
    # an inflated tile of 16 x 16 floats costs 1024 bytes of the budget: four tiles fit 0.004 MB (4194 bytes),
    # five do not; 0.0005 MB holds none, so every tile runs alone
    try:
        for mb, groups in ((0.004, "4 + 4 + 1"), (0.0005, "one each")):
            L.set_tuning("tiffd_scratch_budget_mb", mb)
            got, _ = A.decode_geotiff(m8, data)
            assert same(_host(got), raster), groups
            got, _ = A.decode_geotiff(m8, _broken(data, 8, "adler"), (0, 0, 32, 48))     # (all but tile column 2)
            assert same(_host(got), raster[:48, :32]), groups
            with pytest.raises(A.AmhipError) as ei:
                A.decode_geotiff(m8, _broken(data, 7, "adler"))
            assert "chunk 7 (tile row 2, column 1)" in str(ei.value), groups
    finally:
        L.set_tuning("tiffd_scratch_budget_mb", None)


# ---- the session -----------------------------------------------------------------------------------------
def _ncam(A, sc):
    c = sc.cam
    return A.NCamera(c.fu, c.fv, c.cu, c.cv, c.width, c.height)


@pytest.mark.parametrize("tiles", [(1, 1), (2, 2)])
def test_a_session_takes_its_heights_from_a_file_and_the_mosaic_uploads_none_of_them(tiles, tmp_path):
    import aerial_mapper_amd as A
    sc = S.Scene(24.0, 16.0, 0.5, 3000, seed=11, num_frames=3, point_extent=6.0)   # (the map's rim stays NaN)
    g = sc.grid
    st = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)
    path = str(tmp_path / "dsm.tif")
    with A.AerialGridMap(st, device=0) as m:
        A.Dsm(A.DsmSettings(1), m).process(sc.points, m)
        elev = m.get("elevation")
        assert np.isnan(elev).any() and np.isfinite(elev).any()
        A.layer_to_geotiff(m, "elevation", path, "f32", tile=16)
    with A.HostSession(st, tiles=tiles) as hs:
        assert hs.num_windows == tiles[0] * tiles[1]
        A.session_layer_from_geotiff(hs, "elevation", path, hs.layers["elevation"])
        assert same(hs.layers["elevation"], elev)
        up0 = hs.transfer_stats()[0]
        hs.ortho_process(_ncam(A, sc), A.OrthoSettings(), sc.poses, sc.frames)
        assert hs.transfer_stats()[0] == up0           # resident and known: no layer byte went up
        from_file = {k: v.copy() for k, v in hs.layers.items()}
        assert np.isfinite(from_file["ortho"]).any()
        # a damaged file changes neither the matrix nor a window
        bad = str(tmp_path / "bad.tif")
        data = open(path, "rb").read()
        open(bad, "wb").write(_broken(data, len(R.parse(data)["chunks"]) // 2, "adler"))
        with pytest.raises(A.AmhipError) as ei:
            A.session_layer_from_geotiff(hs, "elevation", bad, hs.layers["elevation"])
        assert "amhip_session_layer_read_geotiff" in str(ei.value) and "Adler-32" in str(ei.value)
        assert same(hs.layers["elevation"], elev)
    with A.HostSession(st, tiles=tiles) as hs:
        hs.layers["elevation"][:] = elev
        up0 = hs.transfer_stats()[0]
        hs.ortho_process(_ncam(A, sc), A.OrthoSettings(), sc.poses, sc.frames)
        # the plain matrix has to travel: every window's part of it that is not the initial NaN throughout
        travels = 0
        for k in range(hs.num_windows):
            i0, j0, r, c = hs.window(k)
            if not np.isnan(elev[j0:j0 + c, i0:i0 + r]).all():
                travels += 4 * r * c
        assert hs.transfer_stats()[0] - up0 == travels > elev.nbytes // 2
        S.assert_layers_equal(hs.layers, from_file, sorted(from_file))


def test_a_session_keeps_what_the_file_does_not_reach(tmp_path):
    import aerial_mapper_amd as A
    kind, h, w, gt, kw = PLACEMENTS["a file over a part of the map"]
    data, raster = _file_for_placement(kind, h, w, gt, **kw)
    path = str(tmp_path / "part.tif")
    open(path, "wb").write(data)
    rows, cols = 33, 29
    st = A.GridMapSettings(CENTER[0], CENTER[1], rows * RES, cols * RES, RES)
    with A.HostSession(st, tiles=(2, 2)) as hs:
        rng = np.random.default_rng(8)
        hs.layers["elevation"][:] = rng.random((cols, rows)).astype(np.float32)
        before = hs.layers["elevation"].copy()
        A.session_layer_from_geotiff(hs, "elevation", path, hs.layers["elevation"])
        want = R.place(before, hs.grid, (0, 0, rows, cols), R.parse(data), raster)
        assert same(hs.layers["elevation"], want) and not same(want, before)
