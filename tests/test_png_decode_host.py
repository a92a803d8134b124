"""The host-only code of the PNG decoder (amhip_png_decode_host.h) as a stand-alone program
(tests/cpp/png_decode_host_main.cc) under the address and undefined-behaviour sanitizers, compared
with tests/png_decode_reference.py.  No GPU, nothing loaded into python."""
import os
import subprocess
import zlib

import pytest

import png_decode_inputs as PI
import png_decode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("png_decode_host") / "png_decode_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "png_decode_host_main.cc"), "-o", out])
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
    h = R.parse(data)
    assert r["size"] == [h.width, h.height, h.colour_type, h.bpp], name
    assert r["raw"] == [h.raw_len], name
    assert r["zlib"] == [h.zlen, 2, h.zlen - 4, h.adler], name
    assert r["plte"] == [h.plte_entries] + list(h.plte), name
    assert r["idat"] == [len(h.idat)] + [v for span in h.idat for v in span], name
    # the joined payloads are the zlib stream, byte for byte
    assert r["stream_crc"] == [zlib.crc32(h.stream)], name


def test_descriptors_equal_the_restatement(exe):
    names = PI.fixture_names()
    recs = _records(_run(exe, "desc", *[PI.fixture_path(n) for n in names]))
    assert len(recs) == len(names) == 56
    for n, r in zip(names, recs):
        _check(n, r, PI.fixture_bytes(n))
    # 1-byte IDAT chunks: as many spans as the stream has bytes
    r = recs[names.index("idat_bytes_64x3_rgb")]
    assert r["idat"][0] == r["zlib"][0] > 100 and set(r["idat"][2::2]) == {1}
    # an empty IDAT in the middle is a span of its own
    assert 0 in recs[names.index("idat_empty_piece_64x3_rgb")]["idat"][2::2]


def test_the_device_error_streams_pass_the_host(exe, tmp_path):
    """their headers, chunks and zlib headers are fine: what is wrong with them only inflate can see"""
    cases = PI.device_errors()
    paths = []
    for k, (what, (data, _)) in enumerate(sorted(cases.items())):
        p = tmp_path / ("device_%d.png" % k)
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    for (what, (data, _)), r in zip(sorted(cases.items()), recs):
        _check(what, r, data)


def test_every_refusal_is_refused_with_a_text(exe, tmp_path):
    cases = PI.refusals()
    assert len(cases) >= 30
    paths = []
    for k, (what, (data, _)) in enumerate(cases.items()):
        p = tmp_path / ("refused_%d.png" % k)
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    assert len(recs) == len(cases)
    for (what, (data, word)), r in zip(cases.items(), recs):
        assert "refused" in r, what
        assert word in r["refused"], (what, r["refused"])
        # ... and the restatement refuses it for the same reason
        with pytest.raises(R.Refused) as ei:
            R.parse(data)
        assert str(ei.value) == r["refused"], what


def test_mutated_and_truncated_files_end_in_ok_or_a_refusal(exe):
    """56 files x 60 seeded mutations (a byte of the signature, of a chunk's length, type or CRC, of
    IHDR, PLTE or the zlib header changed, or the file cut short), each parsed from a heap buffer of
    exactly its size and its spans copied out: any read outside it, any overflow is a sanitizer report
    and a non-zero exit"""
    names = PI.fixture_names()
    ok, refused = (int(x) for x in _run(exe, "fuzz", 20261019, 60, *[PI.fixture_path(n) for n in names]).split())
    assert ok + refused == 56 * 60
    # (accepted: a mutation inside an ancillary chunk's header or CRC, or one that left the byte as it was;
    # nearly every other one breaks a CRC or a length)
    assert ok >= 10 and refused > 2500
