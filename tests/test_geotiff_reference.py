"""The tiled Deflate GeoTIFF of DESIGN 4.16 without a GPU: tests/geotiff_reference.py against zlib
itself, against Pillow (libtiff) and against amhip_geotiff_write_u8's geo tags; the committed files of
tests/golden/geotiff/; and the host-only container code (amhip_tiff_host.h) as a stand-alone program
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

import geotiff_inputs as GI
import geotiff_reference as GR
import png_encode_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "geotiff")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


CASES = sorted(GI.golden_cases())


def test_the_golden_directory_holds_every_case_and_nothing_else():
    names = sorted(os.listdir(GOLDEN))
    assert names == sorted([n + ".npy" for n in CASES] + [n + ".tif" for n in CASES])
    assert sum(os.path.getsize(os.path.join(GOLDEN, n)) for n in names) < 512 * 1024
    for n in CASES:
        assert same(np.load(os.path.join(GOLDEN, n + ".npy")), GI.golden_cases()[n][0]), n


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_writes_the_committed_file(name):
    raster, tile = GI.golden_cases()[name]
    want = open(os.path.join(GOLDEN, name + ".tif"), "rb").read()
    assert GR.encode(raster, GI.GT, 32, True, tile) == want


@pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the bytes are pinned to zlib 1.2.11")
@pytest.mark.parametrize("name", CASES)
def test_the_tile_streams_are_zlib_1_2_11s(name):
    raster, tile = GI.golden_cases()[name]
    for payload in GR.tile_payloads(raster, tile):
        c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        assert PR.zlib_stream(payload) == c.compress(payload) + c.flush()
    want = open(os.path.join(GOLDEN, name + ".tif"), "rb").read()
    assert GR.encode(raster, GI.GT, 32, True, tile, stream=PR.zlib_rle_stream) == want


def _pillow_cases():
    cases = {n: GI.golden_cases()[n] for n in CASES}
    neg = -np.abs(GI.terrain(40, 23)) - np.float32(0.5)
    cases["f32_negative_40x23_t16"] = (neg, 16)
    for kind in ("f32", "u8", "rgb8"):
        for h, w in GI.EDGE_SIZES:
            cases["%s_%dx%d_t16" % (kind, h, w)] = (GI.edge_raster(kind, h, w), 16)
    return cases


@pytest.mark.parametrize("name", sorted(_pillow_cases()))
def test_pillow_and_the_inverse_read_every_reference_file_back_bit_for_bit(name):
    Image = pytest.importorskip("PIL.Image")
    raster, tile = _pillow_cases()[name]
    data = GR.encode(raster, GI.GT, 33, False, tile)
    back = GR.decode(data)
    assert back["kind"] == GR.kind_of(raster) and back["tile"] == tile and same(back["raster"], raster)
    assert back["geotransform"] == GI.GT and back["epsg"] == 32733
    im = Image.open(io.BytesIO(data))
    assert same(np.array(im), raster)
    if raster.dtype == np.float32:
        assert im.tag_v2[42113] == "nan"


@pytest.mark.parametrize("northern", [True, False])
@pytest.mark.parametrize("kind", ["f32", "u8", "rgb8"])
def test_the_geo_tags_are_those_of_the_uncompressed_writer(hip_built, tmp_path, kind, northern):
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    gt = (-1234.5, 0.25, 0.0, 98765.125, 0.0, -0.25)
    zone = 17 if northern else 60
    img = np.zeros((5, 7, 3) if kind == "rgb8" else (5, 7), np.uint8)
    path = str(tmp_path / "u8.tif")
    L.check(lib.amhip_geotiff_write_u8(path.encode(), C.c_void_p(img.ctypes.data), 7, 5, img.strides[0],
                                       3 if kind == "rgb8" else 1, (C.c_double * 6)(*gt), zone, int(northern)))
    theirs = GR.parse_ifd(open(path, "rb").read())
    raster = GI.edge_raster(kind, 5, 7)
    ours = GR.parse_ifd(GR.encode(raster, gt, zone, northern, 16))
    for tag in (33550, 33922, 34735, 34737):
        assert ours[tag] == theirs[tag], tag
    assert GR.geo_tags(gt, zone, northern)[34737][2] == theirs[34737][2]


# ---- amhip_tiff_host.h under the sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiff_host") / "tiff_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tiff_host_check.cc"), "-o", out])
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args[:8], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize("kind", ["f32", "u8", "rgb8"])
@pytest.mark.parametrize("w,h,tile", [(1, 1, 16), (16, 16, 0), (70, 50, 16), (300, 200, 64), (1025, 3, 1024)])
def test_the_container_code_writes_the_references_header(exe, kind, w, h, tile):
    side = tile or 256
    n = -(-w // side) * -(-h // side)
    rng = np.random.default_rng(w * h + side)
    counts = [int(c) for c in rng.integers(11, 70000, n)]
    gt = (464499.25, 0.1, 0.0, 5272700.75, 0.0, -0.1)
    for zone, northern in ((32, 1), (7, 0)):
        head, size = _run(exe, "head", w, h, GR.KINDS[kind], tile, zone, northern, *gt, *counts).split()
        want_head, want_size = GR.container(w, h, kind, side, gt, zone, bool(northern), counts)
        assert bytes.fromhex(head) == want_head and int(size) == want_size
    tiles, head_bound, bound = (int(x) for x in _run(exe, "bound", w, h, GR.KINDS[kind], tile).split())
    px = {"f32": 4, "u8": 1, "rgb8": 3}[kind]
    raw = side * side * px
    assert tiles == n and head_bound >= len(want_head)
    assert bound == head_bound + n * (raw + 5 * (raw // 16383 + 1) + 7)


def test_the_container_code_refuses_a_file_beyond_4_gb(exe):
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    front = len(GR.container(32, 32, "u8", 16, gt, 32, True, [1, 1, 1, 1])[0])
    fits = [0xFFFFFFFF - 1024, 1024 - front, 0, 0]   # the largest file there is
    head, size = _run(exe, "head", 32, 32, 1, 16, 32, 1, *gt, *fits).split()
    assert int(size) == 0xFFFFFFFF and len(bytes.fromhex(head)) == front
    assert _run(exe, "head", 32, 32, 1, 16, 32, 1, *gt, fits[0], fits[1] + 1, 0, 0).strip() == "refused"
    assert _run(exe, "head", 32, 32, 1, 16, 32, 1, *gt, 3000000000, 3000000000, 5, 5).strip() == "refused"
    assert _run(exe, "head", 32, 32, 1, 16, 32, 1, *gt, 1 << 40, 1, 1, 1).strip() == "refused"
    with pytest.raises(ValueError):
        GR.container(32, 32, "u8", 16, gt, 32, True, [3000000000, 3000000000, 5, 5])


def test_the_argument_checks_name_the_field(exe):
    lines = _run(exe, "args").strip().split("\n")
    words = ["ok", "ok", "width", "height", "kind", "kind", "tile", "tile", "tile", "ok", "geotransform",
             "geotransform", "utm_zone", "utm_zone"]
    assert len(lines) == len(words)
    for line, word in zip(lines, words):
        assert word in line, (line, word)
