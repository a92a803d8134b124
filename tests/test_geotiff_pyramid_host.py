"""The GeoTIFF pyramid without a GPU: the numpy restatement (tests/geotiff_pyramid_reference.py)
against Pillow, against the one-IFD reference at zero overviews and against the committed files; the host
exports amhip_geotiff_levels / amhip_geotiff_level_info against the restatement; and the container and the
chain walk (amhip_tiff_host.h, amhip_tiff_decode_host.h) as a stand-alone program
(tests/cpp/tiff_pyramid_host_main.cc) under the address and undefined-behaviour sanitizers.  Nothing loaded
into python runs under a sanitizer."""
import io
import os
import subprocess

import numpy as np
import pytest

import geotiff_pyramid_inputs as PI
import geotiff_pyramid_reference as P
import geotiff_reference as W
import png_encode_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _cases():
    out = {n: (r, t, o) for n, (r, t, o) in PI.fixtures().items()}
    for kind in PI.KINDS:
        for (w, h, t) in PI.SIZES:
            out["%s_%dx%d_t%d" % (kind, w, h, t)] = (PI.raster(kind, w, h), t, -1 if w > 2 else 1)
    return out


def test_reduce_by_hand():
    f = np.float32
    a = np.array([[1.0, np.nan, 1e30], [2.0, 4.0, 1.0], [np.nan, np.nan, np.nan]], np.float32)
    got = P.reduce(a)
    assert got.shape == (2, 2)
    assert got[0, 0] == f((1.0 + 2.0 + 4.0) / 3.0) and got[0, 1] == f((np.float64(f(1e30)) + 1.0) / 2.0)
    assert got.view(np.uint32)[1, 0] == 0x7FC00000 and got.view(np.uint32)[1, 1] == 0x7FC00000
    u = P.reduce(PI.u8_hard())
    assert u.shape == (3, 4)
    assert u[0].tolist() == [1, 0, 255, 4]          # 2 of 4 rounds up; 1 of 4 down; 1019 / 4 = 254.75; (3 + 4 + 1) / 2
    assert u[2].tolist() == [8, 255, 1, 9]          # clipped blocks of 2 with an odd sum round up; of 1
    c = P.reduce(PI.rgb8_hard())
    for b in range(3):
        assert _bits(c[..., b]) == _bits(P.reduce(np.ascontiguousarray(PI.rgb8_hard()[..., b])))
    hard = P.reduce(PI.f32_hard())
    assert hard.view(np.uint32)[0, 4] == 0x7FC00000          # payloads in, the canonical NaN out
    assert hard[1, 4] == np.inf and hard.view(np.uint32)[1, 5] == 0x7FC00000   # +inf with -inf
    assert hard.view(np.uint32)[2, 4] == 0                   # four times -0.0: the sum starts at +0.0 and stays there
    # 1e30 beside 1: the fixed order decides which ones survive (1e30 + 1 - 1e30 + 1 = 1; 1 + 1e30 + 1 - 1e30 = 0)
    assert hard[3, 4] == 0.25 and hard[3, 5] == 0.0
    assert hard[4, 0] == f(16777219.0 / 4.0) and np.isfinite(hard[4, 2])
    assert np.all(np.isnan(hard[:, 6])) and hard[5, 0] == -np.inf


def test_level_count():
    assert P.level_count(17, 33, 16, -1) == 2 and P.level_count(16, 16, 16, -1) == 0
    assert P.level_count(1, 9, 16, 4) == 4 and P.level_count(40000, 40000, 256, -1) == 8
    for bad in ((1, 9, 16, 5), (2, 2, 16, 2), (8, 8, 16, 17), (8, 8, 16, -2)):
        with pytest.raises(ValueError):
            P.level_count(*bad)


def test_same_bytes_at_zero():
    for name, (raster, tile, _) in _cases().items():
        lib = PR.zlib_rle_stream      # (the library's stream: the restatement is held to it elsewhere)
        assert P.encode(raster, PI.GT, tile=tile, overviews=0, stream=lib) == \
            W.encode(raster, PI.GT, tile=tile, stream=lib), name


def test_restatement_and_library_stream_agree_on_a_pyramid():
    raster, tile, n = PI.fixtures()["f32_17x33_t16_auto"]
    assert P.encode(raster, PI.GT, tile=tile, overviews=n) == \
        P.encode(raster, PI.GT, tile=tile, overviews=n, stream=PR.zlib_rle_stream)


def test_reference_inverts_itself_and_lays_the_file_out_as_stated():
    for name, (raster, tile, n) in _cases().items():
        data = P.encode(raster, PI.GT, tile=tile, overviews=n, stream=PR.zlib_rle_stream)
        want = P.pyramid(raster, tile, n)
        infos = P.levels(data)
        assert len(infos) == len(want), name
        chain = P.ifd_chain(data)
        assert chain[0] == (8, None) and all(sub == 1 for _, sub in chain[1:]), name
        assert all(o % 2 == 0 for o, _ in chain) and [o for o, _ in chain] == sorted(o for o, _ in chain), name
        first = []
        for k, lvl in enumerate(want):
            got, info = P.decode(data, k)
            assert got.dtype == lvl.dtype and _bits(got) == _bits(lvl), (name, k)
            assert (info["width"], info["height"]) == (lvl.shape[1], lvl.shape[0])
            assert info["geotransform"][1] == PI.GT[1] * raster.shape[1] / lvl.shape[1]
            assert info["geotransform"][5] == PI.GT[5] * raster.shape[0] / lvl.shape[0]
            assert info["tile_width"] == info["tile_height"] == tile and info["epsg"] == 32632
            offs = [c[0] for c in info["chunks"]]
            assert offs == sorted(offs)
            first.append(offs[0])
        # the coarsest level first, level 0 last, from a multiple of 16, to the end of the file
        assert first == sorted(first, reverse=True) and first[-1] % 16 == 0, name
        last = P.level_info(data, 0)["chunks"][-1]
        assert last[0] + last[1] == len(data), name


def test_pillow_reads_the_reference_pyramid():
    Image = pytest.importorskip("PIL.Image")
    seen = 0
    for name, (raster, tile, n) in _cases().items():
        data = P.encode(raster, PI.GT, tile=tile, overviews=n, stream=PR.zlib_rle_stream)
        want = P.pyramid(raster, tile, n)
        im = Image.open(io.BytesIO(data))
        assert getattr(im, "n_frames", 1) == len(want), name
        for k, lvl in enumerate(want):
            im.seek(k)
            got = np.asarray(im)
            assert got.shape == lvl.shape, (name, k)
            assert _bits(got.astype(lvl.dtype)) == _bits(lvl), (name, k)     # (NaN positions and bits included)
            seen += 1
    assert seen >= 40


def test_committed_files_are_what_the_reference_writes():
    paths = PI.fixture_paths()
    assert len(paths) == len(PI.fixtures())
    for name, (raster, tile, n) in PI.fixtures().items():
        path = os.path.join(PI.GOLDEN, name + ".tif")
        assert open(path, "rb").read() == P.encode(raster, PI.GT, tile=tile, overviews=n), name
        assert os.path.getsize(path) < 16384


def test_foreign_chains_in_the_reference():
    for name, (data, want) in PI.foreign().items():
        assert len(P.levels(data)) == len(want), name
        for k, lvl in enumerate(want):
            got, _ = P.decode(data, k)
            assert _bits(got) == _bits(lvl), (name, k)
    assert len(P.ifd_chain(PI.foreign()["mask_page"][0])) == 7


def _same(a, b):
    for k in ("width", "height", "bands", "kind", "tiled", "tile_width", "tile_height", "rows_per_strip", "compression",
              "predictor", "has_geo", "epsg", "raster_type"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert np.array(a["geotransform"], np.float64).tobytes() == np.array(b["geotransform"], np.float64).tobytes()
    x, y = a["nodata"], b["nodata"]
    assert (x is None and y is None) or x == y or (np.isnan(x) and np.isnan(y))


def test_levels_equal_the_restatement(hip_built, tmp_path):
    import aerial_mapper_amd as A
    files = {n: open(p, "rb").read() for n, p in zip(sorted(PI.fixtures()), PI.fixture_paths())}
    files.update({n: d for n, (d, _) in PI.foreign().items()})
    for name, data in files.items():
        got, want = A.geotiff_levels(data), P.levels(data)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            _same(g, w)
        _same(got[0], A.geotiff_info(data))
    path = tmp_path / "a.tif"
    path.write_bytes(files["strips"])
    assert len(A.geotiff_levels(str(path))) == 3
    assert [(d["tiled"], d["rows_per_strip"]) for d in A.geotiff_levels(files["strips"])] == [(1, 0), (0, 7), (0, 9)]
    # a file without overviews has one level
    one = open(os.path.join(ROOT, "tests", "golden", "geotiff", "f32_33x47_t16.tif"), "rb").read()
    assert len(A.geotiff_levels(one)) == 1
    for name, (data, level, word) in PI.refused_chains().items():
        with pytest.raises(A.AmhipError) as ei:
            lib_levels = A.geotiff_levels(data)
            assert len(lib_levels) <= level     # (the chain is fine: the level asked for is not there)
            A.io._level_info(data, level)
        assert word in str(ei.value) and "amhip_geotiff_level" in str(ei.value), (name, str(ei.value))
    # another level of a file with one bad level still reads
    lzw = PI.refused_chains()["level_lzw"][0]
    _same(A.io._level_info(lzw, 0), P.level_info(lzw, 0))


def test_bound_and_argument_rules_without_a_device(hip_built):
    import aerial_mapper_amd.hip_lib as L
    lib = L.load()
    for kind in range(3):
        assert lib.amhip_geotiff_bound_ovr(100, 70, kind, 32, 0) == lib.amhip_geotiff_bound(100, 70, kind, 32)
        assert lib.amhip_geotiff_bound_ovr(100, 70, kind, 32, -1) > lib.amhip_geotiff_bound(100, 70, kind, 32)
    for bad in (17, -2, 8):
        assert lib.amhip_geotiff_bound_ovr(100, 70, 0, 32, bad) == 0


# ---- the stand-alone program -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiff_pyramid_host") / "tiff_pyramid_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tiff_pyramid_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as it is)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300)
    assert r.returncode == 0, (args[:3], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def _level_line(info):
    gt = [int(np.float64(v).view(np.uint64)) for v in info["geotransform"]]
    return [info["width"], info["height"], W.KINDS[info["kind"]], info["tiled"], info["chunk_w"], info["chunk_h"],
            gt[0], gt[1], gt[3], gt[5], int(info["nodata"] is not None), len(info["chunks"])]


@pytest.fixture(scope="module")
def foreign_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pyramid_files")
    out = {}
    for name, (data, _) in PI.foreign().items():
        (d / (name + ".tif")).write_bytes(data)
        out[name] = (str(d / (name + ".tif")), data)
    for name, (data, level, word) in PI.refused_chains().items():
        (d / ("refused_" + name + ".tif")).write_bytes(data)
        out["refused_" + name] = (str(d / ("refused_" + name + ".tif")), data)
    return out


def test_program_reads_every_level_of_every_file(exe, foreign_files):
    files = {os.path.basename(p)[:-4]: (p, open(p, "rb").read()) for p in PI.fixture_paths()}
    files.update({n: v for n, v in foreign_files.items() if not n.startswith("refused_")})
    text = _run(exe, "levels", *[p for p, _ in files.values()])
    blocks = text.strip().split("file ")[1:]
    assert len(blocks) == len(files)
    for (name, (path, data)), block in zip(files.items(), blocks):
        lines = block.strip().split("\n")
        want = P.levels(data)
        assert lines[1] == "levels %d" % len(want), (name, lines[:2])
        for k, info in enumerate(want):
            head, _, rest = lines[2 + k].partition(": ")
            assert head == "level %d" % k and [int(v) for v in rest.split()][:-1] == _level_line(info), (name, k)


def test_program_refuses_what_the_rules_refuse(exe, foreign_files):
    for name, (data, level, word) in PI.refused_chains().items():
        text = _run(exe, "levels", foreign_files["refused_" + name][0])
        if name in ("loop", "65_ifds"):
            assert "refused" in text and word in text and "levels" not in text.split("\n", 1)[1], (name, text)
        elif name == "no_such_level":
            assert "levels 2" in text and " refused " not in text and "\nrefused " not in text
        else:
            assert ("level %d refused" % level) in text and word in text, (name, text)
            assert "level 0: " in text, (name, text)


def test_program_survives_mutations_and_truncations(exe, foreign_files):
    paths = PI.fixture_paths() + [p for n, (p, _) in foreign_files.items()]
    out = _run(exe, "mutate", 20251, 300, *paths)
    parses, refusals = int(out.split()[1]), int(out.split()[3])
    assert parses == 300 * len(paths) and 0 < refusals < parses


def test_program_builds_the_reference_container(exe):
    cases = [(w, h, k, t, o) for (w, h, t) in PI.SIZES for k in range(3) for o in (0, 1, -1)] + \
        [(1000, 700, 0, 64, -1), (300, 20, 2, 16, 3)]
    for (w, h, k, t, o) in cases:
        text = _run(exe, "build", w, h, k, t, o)
        try:
            n = P.level_count(w, h, t, o)
        except ValueError:
            assert text.startswith("refused overviews"), (w, h, o, text)
            continue
        sizes = [(w, h)]
        for _ in range(n):
            sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
        counts = [[7 + q % 5 + 3 * lvl for q in range(-(-sw // t) * -(-sh // t))] for lvl, (sw, sh) in enumerate(sizes)]
        head, level_at, total = P.container(sizes, ["f32", "u8", "rgb8"][k], t, PI.GT, 32, True, counts)
        rec = dict(line.split(" ", 1) for line in text.strip().split("\n"))
        assert bytes.fromhex(rec["head"]) == head, (w, h, k, t, o)
        assert [int(v) for v in rec["level_at"].split()] == level_at and int(rec["bytes"]) == total
        assert int(rec["bound"]) >= total
    assert _run(exe, "build", 2, 2, 0, 16, 2).startswith("refused overviews")
    assert _run(exe, "build", 64, 64, 0, 16, 17).startswith("refused overviews")
