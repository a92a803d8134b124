"""GPU: the drop-in C++ ortho::OrthoForwardHomography leaves the file its settings name
(tests/cpp/shim_jpeg.cc): a JPEG file, byte-equal to tests/jpeg_reference.py applied to the pixels
of the <name>.ppm it keeps writing beside it."""
import os
import subprocess

import numpy as np
import pytest

import jpeg_reference as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from aerial_mapper_amd import build
    build.build_all()
    out = str(tmp_path_factory.mktemp("shim_jpeg") / "shim_jpeg")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_jpeg.cc"),
                           "-o", out, "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip",
                           "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("mode", ["gray", "colored"])
def test_batch_leaves_the_jpeg_file_the_settings_name(exe, mode, tmp_path):
    name = str(tmp_path / "result.jpg")
    r = subprocess.run([exe, name, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    # <name>.ppm as before: P6, the 8-bit mosaic's bytes (B, G, R as result8() leaves them)
    ppm = open(name + ".ppm", "rb").read()
    head = b"P6\n250 203\n255\n"
    assert ppm.startswith(head) and len(ppm) == len(head) + 250 * 203 * 3
    img = np.frombuffer(ppm[len(head):], np.uint8).reshape(203, 250, 3)
    assert (img != 0).mean() > 0.2
    got = open(name, "rb").read()
    assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9"
    assert got == J.encode(img, 95)
