"""stereo::Stereo's public C++ surface is the reference's: tests/cpp/api_conformance_stereo.cc (static
asserts on the constructor, addFrames, addFrame, Settings, BlockMatchingParameters, the typedefs, and
the calls the demo mains make) compiles against include/ of this repository and against the
reference's own headers; the defaults are compared at run time.  CPU only."""
import os
import subprocess

import pytest

from test_api_conformance import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "api_conformance_stereo.cc")


def _syntax(includes, src=SRC):
    cmd = ["g++", "-std=c++11", "-fsyntax-only"] + ["-I" + i for i in includes] + [src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_drop_in_headers_satisfy_the_statements():
    _syntax([os.path.join(ROOT, "include")])


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers")
def test_reference_headers_satisfy_the_same_statements():
    inc = [os.path.join(ROOT, "oracle", "refkit"), os.path.join(ROOT, "oracle")]
    inc += [os.path.join(REF, d, "include") for d in
            ("aerial_mapper_utils", "aerial_mapper_thirdparty", "aerial_mapper_dense_pcl",
             "aerial_mapper_io", "aerial_mapper_grid_map")]
    _syntax(inc)


def test_defaults_are_the_references(tmp_path):
    from aerial_mapper_amd import build
    build.build_all()
    exe = str(tmp_path / "conformance_stereo")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-DAPI_STEREO_MAIN", "-I" + os.path.join(ROOT, "include"),
                           SRC, "-o", exe, "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip",
                           "-Wl,-rpath," + lib])
    assert subprocess.run([exe], timeout=60).returncode == 0


def test_shim_source_compiles_in_its_real_dependencies_branch():
    """As tests/test_api_conformance.py does for the other shim sources: stand-ins under the
    externals' own include paths switch include/aerial-mapper-deps.h to AERIAL_MAPPER_REAL_DEPS."""
    inc = [os.path.join(ROOT, "oracle", "refkit"), os.path.join(ROOT, "oracle"),
           os.path.join(ROOT, "include")]
    _syntax(inc, os.path.join(ROOT, "aerial_mapper_amd", "cpp", "stereo.cc"))


def test_the_demo_build_still_finds_its_own_stereo_header_first():
    """oracle/Makefile compiles the demo mains with -Idemokit before -I../include: the stub there
    must keep winning (the drop-in header is reached only by hosts that do not have one)."""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    assert mk.index("-Idemokit") < mk.index("-I../include")
    assert os.path.exists(os.path.join(ROOT, "oracle", "demokit", "aerial-mapper-dense-pcl", "stereo.h"))
    assert os.path.exists(os.path.join(ROOT, "include", "aerial-mapper-dense-pcl", "stereo.h"))
