"""The host-only code of the PNG encoder (amhip_png_encode_host.h) as a stand-alone program
(tests/cpp/png_encode_host_main.cc) under the address and undefined-behaviour sanitizers, compared
with tests/png_encode_reference.py, zlib.crc32 and the committed streams.  No GPU, nothing loaded
into python."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import png_encode_inputs as I
import png_encode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("png_encode_host") / "png_encode_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "png_encode_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as it is)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args[:3], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def test_the_static_tables_equal_the_restatements(exe):
    t = {}
    for line in _run(exe, "tables").strip().split("\n"):
        k, _, rest = line.partition(" ")
        t[k] = [int(x) for x in rest.split()]
    assert t["length_code"] == R.LENGTH_CODE and t["base_length"] == R.BASE_LENGTH
    assert t["extra_lbits"] == R.EXTRA_LBITS and t["extra_dbits"] == R.EXTRA_DBITS
    assert t["extra_blbits"] == R.EXTRA_BLBITS and t["bl_order"] == R.BL_ORDER
    assert t["fixed_llen"] == R.STATIC_LTREE_LEN and t["fixed_lcode"] == R.STATIC_LTREE_CODE
    assert t["fixed_dlen"] == R.STATIC_DTREE_LEN and t["fixed_dcode"] == R.STATIC_DTREE_CODE
    # the register one byte leaves from zero, inversions undone: crc32(b) = ~T[b ^ 0xFF] ^ 0x00FFFFFF
    assert t["crc"] == [zlib.crc32(bytes([i ^ 0xFF])) ^ 0xFF000000 for i in range(256)]
    # x^(2^k) mod P: zlib's x2n_table begins 0x40000000, 0x20000000, 0x08000000, 0x00800000, 0x00008000
    assert t["x2n"][:5] == [0x40000000, 0x20000000, 0x08000000, 0x00800000, 0x00008000]
    assert len(t["x2n"]) == 32


@pytest.mark.parametrize("w,h,c", [(1, 1, 1), (5, 7, 3), (65535, 65535, 3), (126, 129, 1)])
def test_the_header_writer_and_the_bounds(exe, w, h, c):
    head, tail, sizes = _run(exe, "head", w, h, c).strip().split("\n")
    ref = R.frame_file(w, h, c, b"x")
    assert bytes.fromhex(head) == ref[:33] and bytes.fromhex(tail) == ref[-12:]
    raw, zbound, fbound = (int(x) for x in sizes.split())
    assert raw == h * (1 + w * c)
    assert zbound == raw + 5 * (raw // 16383 + 1) + 7
    assert fbound == 33 + zbound + 12 * -(-zbound // 8192) + 12


def test_the_crc_combine_equals_zlib_on_split_buffers(exe, tmp_path):
    rng = np.random.default_rng(3)
    for n in (1, 4, 131, 8196, 70001):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        p = tmp_path / ("crc_%d.bin" % n)
        p.write_bytes(data)
        splits = sorted(k for k in {0, 1, 4, n // 2, max(n - 128, 0), n - 1, n} if k <= n)
        lines = _run(exe, "crc", p, *splits).strip().split("\n")
        assert len(lines) == len(splits)
        for line in lines:
            joined, straight = (int(x) for x in line.split())
            assert joined == straight == zlib.crc32(data)


def test_the_planner_reproduces_every_committed_stream(exe, tmp_path):
    """tokens by rule 4 in the program, every block through plan_block(): block type, code tables, header
    bits and the bit count the offsets pass relies on (the program exits non-zero when the count and the
    packed bits differ)"""
    args, want = [], []
    for k, n in enumerate(I.fixture_names()):
        raw = R.scanlines(I.fixture_pixels(n))
        (tmp_path / ("%d.raw" % k)).write_bytes(raw)
        args += [tmp_path / ("%d.raw" % k), tmp_path / ("%d.z" % k)]
        want.append(I.zlib_stream_of(I.fixture_bytes(n)))
    lines = _run(exe, "deflate", *args).strip().split("\n")
    kinds = np.zeros(3, np.int64)
    for k, w in enumerate(want):
        assert (tmp_path / ("%d.z" % k)).read_bytes() == w, I.fixture_names()[k]
        kinds += np.array([int(x) for x in lines[k].split()][1:])
    assert (kinds > 0).all()         # stored, fixed and dynamic blocks


def test_the_planner_on_inputs_generated_here(exe, tmp_path):
    rng = np.random.default_rng(12)
    raws = [b"", bytes(700000), rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
            (rng.integers(0, 256, 400000, dtype=np.uint8) * (rng.random(400000) < 0.02)).astype(np.uint8).tobytes(),
            np.repeat(rng.integers(0, 9, 9000, dtype=np.uint8), rng.integers(1, 700, 9000)).tobytes()]
    args = []
    for k, raw in enumerate(raws):
        (tmp_path / ("%d.raw" % k)).write_bytes(raw)
        args += [tmp_path / ("%d.raw" % k), tmp_path / ("%d.z" % k)]
    _run(exe, "deflate", *args)
    for k, raw in enumerate(raws):
        assert (tmp_path / ("%d.z" % k)).read_bytes() == R.zlib_stream(raw), k


def test_the_extension_rule_and_the_argument_checks(exe):
    names = ["a.png", "a.PNG", "a.PnG", "/tmp/x/result.png", ".png", "png", "a.png ", "a.jpg", "a.pngx", "a_png", ""]
    assert _run(exe, "ext", *names).split() == ["1", "1", "1", "1", "1", "0", "0", "0", "0", "0", "0"]
    lines = _run(exe, "args").strip().split("\n")
    assert lines[0] == "ok" and lines[5] == "ok" and lines[12] == "ok"
    for line, word in zip(lines[1:5] + lines[6:12], ["channels", "width and height", "width and height", "step",
                                                      "F = 0", "width", "height", "channels", "row_step",
                                                      "frame_stride"]):
        assert word in line, (line, word)
