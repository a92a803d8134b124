"""GPU: the drop-in C++ io::AerialMapperIO::loadImagesFromFile(directory, image_names, ..)
(tests/cpp/shim_load_images_png.cc) on fixtures copied to <tmp>/<name>.png, gray and coloured: the
cv::Mats it appends hold the committed pixels of tests/golden/png_decode/, and so does the stack
loadImagesFromFileToDevice leaves in HBM.  A missing file and a refused one are fatal and named."""
import os
import subprocess

import numpy as np
import pytest

import png_decode_inputs as PI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from aerial_mapper_amd import build
    build.build_all()
    out = str(tmp_path_factory.mktemp("shim_load_images_png") / "shim_load_images_png")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_load_images_png.cc"),
                           "-o", out, "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip",
                           "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("mode", ["gray", "colored"])
def test_load_images_from_file_equals_the_committed_pixels(exe, mode, tmp_path):
    names = PI.fixtures_by_size()[(129, 47)]
    assert len(names) >= 15
    for n in names:
        (tmp_path / (n + ".png")).write_bytes(PI.fixture_bytes(n))
    out = str(tmp_path / "images.bin")
    r = subprocess.run([exe, str(tmp_path) + os.sep, mode, out] + names, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    raw = open(out, "rb").read()
    head, _, body = raw.partition(b"\n")
    ch = 3 if mode == "colored" else 1
    assert head == b"129 47 %d %d" % (ch, len(names))
    got = np.frombuffer(body, np.uint8).reshape((len(names), 47, 129) + ((3,) if ch == 3 else ()))
    for i, n in enumerate(names):
        assert np.array_equal(got[i], PI.fixture_pixels(n)[1 if ch == 3 else 0]), n


def test_a_missing_or_refused_file_is_fatal_and_named(exe, tmp_path):
    (tmp_path / "a.png").write_bytes(PI.good_17x17())
    out = str(tmp_path / "images.bin")
    r = subprocess.run([exe, str(tmp_path) + os.sep, "gray", out, "a", "b"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"b.png" in r.stdout, r.stdout.decode()[-2000:]
    (tmp_path / "b.png").write_bytes(PI.refusals()["Adam7"][0])
    r = subprocess.run([exe, str(tmp_path) + os.sep, "gray", out, "a", "b"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode != 0 and b"frame 1" in r.stdout and b"Adam7" in r.stdout and b"b.png" in r.stdout, \
        r.stdout.decode()[-2000:]
