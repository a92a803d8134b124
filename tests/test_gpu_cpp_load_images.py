"""GPU: the drop-in C++ io::AerialMapperIO::loadImagesFromFile (tests/cpp/shim_load_images.cc) on
fixtures copied to <tmp>/img_<i>.jpg, gray and coloured: the cv::Mats it appends hold the bytes of
tests/jpeg_decode_reference.py, and so does the stack loadImagesFromFileToDevice leaves in HBM."""
import os
import subprocess

import numpy as np
import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from aerial_mapper_amd import build
    build.build_all()
    out = str(tmp_path_factory.mktemp("shim_load_images") / "shim_load_images")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_load_images.cc"),
                           "-o", out, "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip",
                           "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("mode", ["gray", "colored"])
def test_load_images_from_file_equals_the_restatement(exe, mode, tmp_path):
    names = DI.fixtures_by_size()[(129, 47)]
    for i, n in enumerate(names):
        (tmp_path / ("img_%d.jpg" % i)).write_bytes(DI.fixture_bytes(n))
    out = str(tmp_path / "images.bin")
    r = subprocess.run([exe, str(tmp_path / "img_"), str(len(names)), mode, out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    raw = open(out, "rb").read()
    head, _, body = raw.partition(b"\n")
    ch = 3 if mode == "colored" else 1
    assert head == b"129 47 %d %d" % (ch, len(names))
    got = np.frombuffer(body, np.uint8).reshape((len(names), 47, 129) + ((3,) if ch == 3 else ()))
    for i, n in enumerate(names):
        assert np.array_equal(got[i], D.decode_pixels(DI.fixture_bytes(n), ch == 3)), n


def test_a_missing_or_undecodable_file_is_fatal(exe, tmp_path):
    (tmp_path / "img_0.jpg").write_bytes(DI.fixture_bytes("noise_17x17_444_q95"))
    out = str(tmp_path / "images.bin")
    r = subprocess.run([exe, str(tmp_path / "img_"), "2", "gray", out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"img_1.jpg" in r.stdout, r.stdout.decode()[-2000:]
    (tmp_path / "img_1.jpg").write_bytes(DI.refusals()["progressive"][0])
    r = subprocess.run([exe, str(tmp_path / "img_"), "2", "gray", out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"frame 1" in r.stdout and b"SOF2" in r.stdout, r.stdout.decode()[-2000:]
