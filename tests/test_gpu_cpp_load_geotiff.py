"""GPU: the drop-in io::AerialMapperIO::loadLayerFromGeoTiff (tests/cpp/shim_geotiff_load.cc):
writeLayerToGeoTiff, then loadLayerFromGeoTiff into a second map, the matrices compared in C++."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cpp_member_loads_what_its_sibling_wrote(tmp_path):
    from aerial_mapper_amd import build
    build.build_all()
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    exe = str(tmp_path / "shim_geotiff_load")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_geotiff_load.cc"), "-o", exe,
                           "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    word, rows, cols, took = out.stdout.split()
    assert (word, int(rows), int(cols)) == ("ok", 33, 47)
    assert 0 < int(took) < 30 * 47           # the shifted map took pixels, not on its first three rows, not on holes
