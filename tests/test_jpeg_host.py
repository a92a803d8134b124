"""The host-only code of the JPEG encoder (amhip_jpeg_host.h) as a stand-alone program
(tests/cpp/jpeg_host_main.cc) under the address and undefined-behaviour sanitizers, compared with
tests/jpeg_reference.py.  No GPU, nothing loaded into python."""
import os
import subprocess

import pytest

import jpeg_reference as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "jpeg_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as
    # it is, whatever that preloads)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=60)
    assert r.returncode == 0, (args, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize("quality", [95, 100, 50, 1])
@pytest.mark.parametrize("channels", [1, 3])
def test_header_equals_the_restatement(exe, channels, quality):
    for (w, h) in ((1, 1), (17, 17), (513, 24), (65535, 65535), (256, 257)):
        got = bytes.fromhex(_run(exe, "header", w, h, channels, quality).strip())
        assert got == J.header(w, h, channels, quality), (w, h)


def test_huffman_codes_equal_the_restatement(exe):
    lines = _run(exe, "huff").strip().split("\n")
    assert len(lines) == 2
    for t, line in enumerate(lines):
        v = [int(x) for x in line.split()]
        assert len(v) == 12 + 256
        for cat in range(12):
            assert v[cat] == int(J.DC_CODE[t][0][cat]) | (int(J.DC_CODE[t][1][cat]) << 16)
        for sym in range(256):
            assert v[12 + sym] == int(J.AC_CODE[t][0][sym]) | (int(J.AC_CODE[t][1][sym]) << 16)


def test_bound_and_argument_rules(exe):
    assert int(_run(exe, "bound", 65535, 65535, 3)) > 65535 * 65535 * 3
    assert int(_run(exe, "bound", 1, 1, 1)) >= len(J.encode(__import__("numpy").zeros((1, 1), "uint8"), 100))
    assert _run(exe, "check", 24, 8, 8, 3, 95).strip() == "ok"
    for args in ((23, 8, 8, 3, 95), (8, 8, 8, 2, 95), (8, 8, 8, 1, 101), (8, 8, 8, 1, -1), (8, 0, 8, 1, 95),
                 (65536, 65536, 8, 1, 95), (8, 8, 0, 1, 95), (8, 8, 65536, 1, 95)):
        assert _run(exe, "check", *args).strip() != "ok", args
