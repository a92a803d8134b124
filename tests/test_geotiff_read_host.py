"""The GeoTIFF reader without a GPU: the numpy restatement (tests/geotiff_read_reference.py) against
the committed files and against Pillow, amhip_geotiff_info against the restatement, and the host parser
(amhip_tiff_decode_host.h) as a stand-alone program (tests/cpp/tiff_decode_host_main.cc) under the
address and undefined-behaviour sanitizers.  Nothing loaded into python runs under a sanitizer."""
import io
import os
import subprocess

import numpy as np
import pytest

import geotiff_read_inputs as RI
import geotiff_read_reference as R
import geotiff_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_reference_decodes_every_committed_file():
    paths = RI.fixture_paths()
    assert len(paths) >= 20
    for path in paths:
        data = open(path, "rb").read()
        raster, info = R.decode(data)
        want = np.load(path[:-4] + ".npy")
        assert raster.dtype == want.dtype and raster.shape == want.shape, path
        assert _bits(raster) == _bits(want), path
    # the writer's own files: its inverse agrees on everything it reports
    for path in paths:
        if os.sep + "geotiff" + os.sep not in path:
            continue
        data = open(path, "rb").read()
        old = W.decode(data)
        _, info = R.decode(data)
        assert info["geotransform"] == tuple(old["geotransform"]) and info["epsg"] == old["epsg"]
        assert info["kind"] == old["kind"] and info["tile_width"] == info["tile_height"] == old["tile"]


def test_reference_inverts_its_own_writer():
    cases = RI.variants()
    assert len(cases) >= 40
    for name, (data, raster) in cases.items():
        got, info = R.decode(data)
        assert got.dtype == raster.dtype and _bits(got) == _bits(raster), name
        if "nogeo" in name:
            assert not info["has_geo"]
        else:
            assert info["has_geo"] and info["geotransform"] == tuple(RI.GT) and info["epsg"] == 32632, name
    assert cases["f32_p3_33x47_t16_point"][0] != cases["f32_p3_33x47_t16"][0]
    assert R.parse(cases["f32_p3_33x47_t16_point"][0])["raster_type"] == 2
    assert R.parse(cases["f32_p3_33x47_t16_nodata"][0])["nodata"] == -9999.0
    assert np.isnan(R.parse(cases["f32_p3_33x47_t16_nodata_nan"][0])["nodata"])
    # every block type is in there: a stored block, a fixed one, dynamic ones
    first = lambda n: cases[n][0][R.parse(cases[n][0])["chunks"][0][0] + 2] & 7
    assert first("f32_p3_noise_128_t128_level0") >> 1 == 0
    assert first("f32_p3_33x47_t16_fixed") >> 1 == 1
    assert first("f32_p3_terrain_128_t128_level9") >> 1 == 2


def test_pillow_reads_what_the_test_writer_writes():
    """tiled and 16-bit signed files come from the test writer only: libtiff has to agree with it"""
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for name, (data, raster) in RI.variants().items():
        try:
            im = Image.open(io.BytesIO(data))
            got = np.asarray(im)
        except Exception as e:   # (a type this Pillow does not take: not a statement about the file)
            if raster.dtype in (np.int16, np.uint16) or "32946" in name:
                continue
            raise AssertionError((name, e))
        assert got.shape == raster.shape, name
        assert _bits(got.astype(raster.dtype)) == _bits(raster), name
        seen += 1
    assert seen >= 30


def _desc_of(info):
    return {k: info[k] for k in ("width", "height", "bands", "kind", "tiled", "tile_width", "tile_height",
                                 "rows_per_strip", "compression", "predictor", "has_geo", "geotransform", "epsg",
                                 "raster_type", "nodata")}


def _same(a, b):
    for k in a:
        x, y = a[k], b[k]
        if k == "nodata" and x is not None and y is not None:
            assert np.float64(x).tobytes() == np.float64(y).tobytes() or (np.isnan(x) and np.isnan(y)), k
        elif k == "geotransform":
            assert np.array(x, np.float64).tobytes() == np.array(y, np.float64).tobytes(), (k, x, y)
        else:
            assert x == y, (k, x, y)


def test_info_equals_the_restatement(hip_built):
    import aerial_mapper_amd as A
    for path in RI.fixture_paths():
        data = open(path, "rb").read()
        _same(A.geotiff_info(data), _desc_of(R.parse(data)))
        _same(A.geotiff_info(path), _desc_of(R.parse(data)))
    for name, (data, _) in RI.variants().items():
        _same(A.geotiff_info(data), _desc_of(R.parse(data)))
    for what, (data, word) in RI.refusals().items():
        with pytest.raises(A.AmhipError) as ei:
            A.geotiff_info(data)
        assert "amhip_geotiff_info: " in str(ei.value) and word in str(ei.value), (what, str(ei.value))


# ---- the stand-alone program -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiff_decode_host") / "tiff_decode_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tiff_decode_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as
    # it is, whatever that preloads)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args[:3], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def _records(text):
    out = []
    for line in text.strip().split("\n"):
        k, _, rest = line.partition(" ")
        if k == "file":
            out.append({})
        elif k == "refused":
            out[-1][k] = rest
        else:
            out[-1][k] = [int(x) for x in rest.split()]
    return out


def _check(name, r, data):
    assert "refused" not in r, (name, r)
    p = R.parse(data)
    assert r["size"] == [p["width"], p["height"], p["bands"], R.KINDS[p["kind"]]], name
    assert r["layout"] == [p["tiled"], p["chunk_w"], p["chunk_h"], p["across"], p["down"]], name
    assert r["coding"] == [p["compression"], p["predictor"]], name
    assert r["geo"] == [int(p["has_geo"]), p["epsg"], p["raster_type"]], name
    assert r["gt"] == [int(np.float64(v).view(np.uint64)) for v in p["geotransform"]], name
    if p["nodata"] is None:
        assert r["nodata"][0] == 0, name
    else:
        got = np.uint64(r["nodata"][1]).view(np.float64)
        assert r["nodata"][0] == 1 and (got == p["nodata"] or (np.isnan(got) and np.isnan(p["nodata"]))), name
    assert r["chunks"] == [len(p["chunks"])] + [v for c in p["chunks"] for v in c], name


def test_descriptors_equal_the_restatement(exe, tmp_path):
    paths, datas = [], []
    for path in RI.fixture_paths():
        paths.append(path)
        datas.append(open(path, "rb").read())
    for k, (name, (data, _)) in enumerate(RI.variants().items()):
        p = tmp_path / ("variant_%d.tif" % k)
        p.write_bytes(data)
        paths.append(str(p))
        datas.append(data)
    recs = _records(_run(exe, "desc", *paths))
    assert len(recs) == len(paths)
    for path, data, r in zip(paths, datas, recs):
        _check(path, r, data)


def test_every_refusal_is_refused_with_a_text_that_names_the_tag(exe, tmp_path):
    cases = RI.refusals()
    assert len(cases) >= 40
    paths = []
    for k, (what, (data, _)) in enumerate(cases.items()):
        p = tmp_path / ("refused_%d.tif" % k)
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    assert len(recs) == len(cases)
    for (what, (data, word)), r in zip(cases.items(), recs):
        assert "refused" in r, what
        assert word in r["refused"], (what, r["refused"])
        with pytest.raises(R.Refused):   # ... and the restatement refuses it too
            R.parse(data)


def test_mutated_and_truncated_files_end_in_ok_or_a_refusal(exe, tmp_path):
    """every committed file and every variant x 40 seeded mutations (a byte of the header, the IFD, an
    out-of-line value or a chunk's zlib header changed, or the file cut short), each parsed from a heap
    buffer of exactly its size and every accepted chunk read through: any read outside it, any overflow
    is a sanitizer report and a non-zero exit"""
    paths = list(RI.fixture_paths())
    for k, (name, (data, _)) in enumerate(RI.variants().items()):
        p = tmp_path / ("variant_%d.tif" % k)
        p.write_bytes(data)
        paths.append(str(p))
    ok, refused, _ = (int(x) for x in _run(exe, "fuzz", 20261020, 40, *paths).split())
    assert ok + refused == len(paths) * 40
    # (accepted: a mutation in a tag the reader does not look at, in padding, or one that left the byte as
    # it was; a cut always loses a chunk or the IFD)
    assert ok >= 10 and refused >= len(paths) * 15
