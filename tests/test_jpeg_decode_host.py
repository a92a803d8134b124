"""The host-only code of the JPEG decoder (amhip_jpeg_decode_host.h) as a stand-alone program
(tests/cpp/jpeg_decode_host_main.cc) under the address and undefined-behaviour sanitizers, compared
with tests/jpeg_decode_reference.py.  No GPU, nothing loaded into python."""
import os
import subprocess

import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_decode_host") / "jpeg_decode_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "jpeg_decode_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as
    # it is, whatever that preloads)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args[:3], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def _records(text):
    """the program's output -> [{key: [fields]}] per file (keys that repeat get the component in the key)"""
    out = []
    for line in text.strip().split("\n"):
        k, _, rest = line.partition(" ")
        if k == "file":
            out.append({})
            continue
        if k == "refused":
            out[-1][k] = rest
            continue
        v = rest.split()
        if k in ("comp", "quant"):
            k, v = "%s%s" % (k, v[0]), v[1:]
        out[-1][k] = [int(x) for x in v]
    return out


def _check_descriptors(names, recs, bytes_of):
    assert len(recs) == len(names)
    for name, r in zip(names, recs):
        assert "refused" not in r, (name, r)
        h = D.parse_header(bytes_of(name))
        hmax, vmax, mcux, mcuy, samp = D.layout(h)
        assert r["size"] == [h.width, h.height, h.channels], name
        assert r["mcu"] == [hmax, vmax, mcux, mcuy, h.restart], name
        assert r["scan"] == [h.scan_begin, h.scan_end], name
        base = 0
        for ci, (hh, v) in enumerate(samp):
            c = h.comps[ci]
            assert r["comp%d" % ci] == [hh, v, mcux * hh, mcuy * v, base, c["td"], c["ta"]], name
            assert r["quant%d" % ci] == [int(x) for x in h.qtables[c["tq"]]], name
            base += mcux * hh * mcuy * v
            for cls, tid in ((0, c["td"]), (1, c["ta"])):
                t = h.huff[(cls, tid)]
                key = "%s%d" % ("ac" if cls else "dc", tid)
                assert r[key + ".look"] == t.look, (name, key)
                assert r[key + ".maxcode"] == t.maxcode, (name, key)
                assert r[key + ".valoffset"] == t.valoffset, (name, key)
                assert r[key + ".huffval"] == t.huffval, (name, key)
        assert r["blocks"] == [base], name
        # the marks of the scan, counted from its bytes, are those the restatement's walk meets
        c = D.Counters()
        D.entropy_decode(bytes_of(name), h, c)
        assert r["marks"] == [c.restarts, c.stuffed, c.fill_bytes], name


def test_descriptors_and_tables_equal_the_restatement(exe):
    names = DI.fixture_names()
    recs = _records(_run(exe, "desc", *[DI.fixture_path(n) for n in names]))
    _check_descriptors(names, recs, DI.fixture_bytes)


def test_every_stream_is_accepted_and_its_descriptor_equals_the_restatement(exe, tmp_path):
    """the second family: header and scan rewrites, hand-coded scans, flat quantisation tables and
    Pillow's further shapes; scan bounds, tables and marks as the restatement has them"""
    names = DI.stream_names()
    paths = []
    for n in names:
        if n in DI.BUILT_NOT_COMMITTED:
            p = tmp_path / (n + ".jpg")
            p.write_bytes(DI.stream_bytes(n))
            paths.append(str(p))
        else:
            paths.append(DI.stream_path(n))
    extra = {"ff_ff_00_at_619": DI.ff_ff_00_at_619()[0], "run_past_63": DI.run_past_63()}
    for n, data in extra.items():
        p = tmp_path / (n + ".jpg")
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    assert len(recs) == 170 + 2
    _check_descriptors(names, recs[:170], DI.stream_bytes)
    for (n, data), r in zip(extra.items(), recs[170:]):
        h = D.parse_header(data)
        assert r["scan"] == [h.scan_begin, h.scan_end] and r["size"] == [h.width, h.height, h.channels], n
    # fill bytes in front of EOI lie outside the scan: it ends at the first 0xFF of the run
    a = _records(_run(exe, "desc", DI.stream_path("b_fill_before_eoi_420"), DI.fixture_path("noise_33x15_420_q95_rst1")))
    assert a[0]["scan"] == a[1]["scan"]


def test_mutated_headers_of_the_streams_end_in_ok_or_a_refusal(exe):
    """169 files x 10 seeded mutations, as below: rearranged and hand-written headers under the sanitizers"""
    names = [n for n in DI.stream_names() if n not in DI.BUILT_NOT_COMMITTED]
    ok, refused = (int(x) for x in _run(exe, "fuzz", 20261019, 10, *[DI.stream_path(n) for n in names]).split())
    assert ok + refused == 169 * 10
    assert ok > 20 and refused > 400


def test_every_refusal_is_refused_with_a_text(exe, tmp_path):
    cases = DI.refusals()
    paths = []
    for k, (what, (data, _)) in enumerate(cases.items()):
        p = tmp_path / ("refused_%d.jpg" % k)
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    assert len(recs) == len(cases)
    for (what, (data, word)), r in zip(cases.items(), recs):
        assert "refused" in r, what
        assert word in r["refused"], (what, r["refused"])
        # ... and the restatement refuses it for the same reason
        with pytest.raises(D.Refused) as ei:
            D.parse_header(data)
        assert str(ei.value) == r["refused"], what


def test_skipped_segments_leave_the_descriptor_alone(exe, tmp_path):
    for k, (what, (data, same_as)) in enumerate(DI.accepted_extras().items()):
        p = tmp_path / ("extra_%d.jpg" % k)
        p.write_bytes(data)
        a, b = _records(_run(exe, "desc", str(p), DI.fixture_path(same_as)))
        h = D.parse_header(data)
        b.pop("scan")
        assert a.pop("scan") == [h.scan_begin, h.scan_end]
        assert h.scan_end - h.scan_begin == len(DI.split(DI.fixture_bytes(same_as))[1])
        assert a == b, what


def test_mutated_and_truncated_headers_end_in_ok_or_a_refusal(exe):
    """96 files x 40 seeded mutations (one header byte changed, or the file cut short), each parsed
    from a heap buffer of exactly its size: any read outside it, any overflow is a sanitizer report
    and a non-zero exit"""
    ok, refused = (int(x) for x in _run(exe, "fuzz", 20240611, 40, *[DI.fixture_path(n) for n in DI.fixture_names()]).split())
    assert ok + refused == 96 * 40
    assert ok > 50 and refused > 1000
