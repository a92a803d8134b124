"""The host parser of the JPEG decoder (amhip_jpeg_decode_host.h) on progressive files, as a
stand-alone program (tests/cpp/jpeg_progressive_host_main.cc) under the address and
undefined-behaviour sanitizers, compared with tests/jpeg_progressive_reference.py.  No GPU, nothing
loaded into python."""
import os
import subprocess

import pytest

import jpeg_decode_inputs as DI
import jpeg_decode_reference as D
import jpeg_progressive_inputs as PI
import jpeg_progressive_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_progressive_host") / "jpeg_progressive_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "jpeg_progressive_host_main.cc"), "-o", out])
    return out


def _run(exe, *args):
    # (the sanitizer runtimes are linked statically: the program runs in the caller's environment as
    # it is, whatever that preloads)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, (args[:3], r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def _records(text):
    """the program's output -> [{key: fields}] per file"""
    out = []
    for line in text.strip().split("\n"):
        k, _, rest = line.partition(" ")
        if k == "file":
            out.append({"scan": []})
        elif k == "refused":
            out[-1][k] = rest
        elif k == "scan":
            out[-1][k].append([int(x) for x in rest.split()])
        elif k in ("comp", "quant"):
            v = rest.split()
            out[-1]["%s%s" % (k, v[0])] = [int(x) for x in v[1:]]
        else:
            out[-1][k] = [int(x) for x in rest.split()]
    return out


def table_hash(t):
    """FNV-1a over the table's numbers, 32 bits each, as the program's"""
    if t is None:
        return 0
    h = 2166136261
    for v in t.look + t.maxcode + t.valoffset + t.huffval:
        v &= 0xFFFFFFFF
        for k in range(4):
            h = ((h ^ ((v >> (8 * k)) & 255)) * 16777619) & 0xFFFFFFFF
    return h


def _check(name, r, data):
    assert "refused" not in r, (name, r)
    h = P.parse(data)
    hmax, vmax, mcux, mcuy, samp = D.layout(h)
    assert r["size"] == [h.width, h.height, h.channels, 1], name
    assert r["mcu"] == [hmax, vmax, mcux, mcuy], name
    base = 0
    for ci, (hh, v) in enumerate(samp):
        assert r["comp%d" % ci] == [hh, v, mcux * hh, mcuy * v, base], name
        assert r["quant%d" % ci] == [int(x) for x in h.qtables[ci]], name        # (the latched table)
        base += mcux * hh * mcuy * v
    assert r["scans"][0] == len(h.scans) == len(r["scan"]), name
    hashes = set()
    for s, got in zip(h.scans, r["scan"]):
        comps = s.comps + [0] * (3 - len(s.comps))
        dc = [table_hash(t) for t in s.dc] + [0] * (3 - len(s.dc))
        want = [s.index, s.begin, s.end, len(s.comps)] + comps + [s.ss, s.se, s.ah, s.al, s.restart, s.nx, s.ny]
        assert got == want + dc + [table_hash(s.ac)], (name, s.index)
        hashes.update(x for x in dc + [table_hash(s.ac)] if x)
    assert r["scans"][1] == len(hashes), name      # every distinct table once


def test_scan_lists_and_tables_equal_the_restatement(exe):
    """every fixture of A, B and C: the frame, the latched quantisation tables, every scan's range,
    fields, MCU counts and tables; the program itself checks ranges, indices and the script"""
    names = PI.names()
    recs = _records(_run(exe, "desc", *[PI.path(n) for n in names]))
    assert len(recs) == len(names) == 182
    for name, r in zip(names, recs):
        _check(name, r, PI.file_bytes(name))
    assert max(r["scans"][0] for r in recs) == 66      # (every AC position of Y its own scan)


def test_a_script_of_thousands_of_scans(exe, tmp_path):
    """every AC position of every component in its own scan, at every bit from Al = 13 down: 3 + 3 * 63
    * 14 scans and as many tables as differ"""
    w = PI.writer_of(PI.B_BASES["444"] % "17x17")
    script = [PI.scan([c], 0, 0, 0, 0) for c in range(3)]
    for c in range(3):
        for k in range(1, 64):
            script += [PI.scan([c], k, k, 0, 13, ta=k & 3)]
            script += [PI.scan([c], k, k, a + 1, a, ta=a & 3) for a in range(12, -1, -1)]
    data = w.write(script)
    p = tmp_path / "many.jpg"
    p.write_bytes(data)
    r = _records(_run(exe, "desc", str(p)))[0]
    assert r["scans"][0] == 3 + 3 * 63 * 14
    _check("many", r, data)
    # ... and they decode to the baseline fixture's pixels
    import numpy as np
    d = P.decode(data)
    g, b = DI.fixture_pixels(PI.B_BASES["444"] % "17x17")
    assert np.array_equal(d.gray, g) and np.array_equal(d.bgr, b)


def test_every_refusal_is_refused_in_the_restatements_words(exe, tmp_path):
    cases = PI.refusals()
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
        with pytest.raises(P.Refused) as ei:
            P.parse(data)
        assert str(ei.value) == r["refused"], what
        if what not in ("a baseline scan under SOF2", "no EOI", "no EOI, cut inside a scan", "no EOI, cut behind a scan",
                        "SOF2 twice"):
            assert r["refused"].startswith("SOF2 (progressive): "), what


def test_baseline_files_and_their_refusals_are_parsed_as_ever(exe, tmp_path):
    """the six-argument parse on SOF0 files: no scan list, the texts of the baseline restatement"""
    names = DI.fixtures_by_size()[(17, 17)]
    recs = _records(_run(exe, "desc", *[DI.fixture_path(n) for n in names]))
    for n, r in zip(names, recs):
        h = D.parse_header(DI.fixture_bytes(n))
        assert r["size"] == [h.width, h.height, h.channels, 0] and r["scans"] == [0, 0] and not r["scan"], n
    cases = DI.refusals()
    paths = []
    for k, (what, (data, _)) in enumerate(cases.items()):
        p = tmp_path / ("refused_%d.jpg" % k)
        p.write_bytes(data)
        paths.append(str(p))
    recs = _records(_run(exe, "desc", *paths))
    for (what, (data, word)), r in zip(cases.items(), recs):
        with pytest.raises(D.Refused) as ei:
            D.parse_header(data)
        assert r.get("refused") == str(ei.value), what
    # DHT ids 2 and 3 are SOF2's alone, also where the DHT precedes the frame header
    segs, scan, tr = DI.split(DI.fixture_bytes("noise_17x17_444_q95"))
    dht = [s for s in segs if s[0] == 0xC4]
    early = [s for s in segs if s[0] not in (0xC4, 0xC0, 0xDA)] + \
        [(0xC4, bytes([dht[0][1][0] | 2]) + dht[0][1][1:])] + dht + [s for s in segs if s[0] in (0xC0, 0xDA)]
    p = tmp_path / "early_dht.jpg"
    p.write_bytes(DI.join(early, scan, tr))
    assert "DHT" in _records(_run(exe, "desc", str(p)))[0]["refused"]


def test_bytes_behind_eoi_are_ignored(exe, tmp_path):
    for k, (what, (data, same_as)) in enumerate(PI.accepted_extras().items()):
        p = tmp_path / ("extra_%d.jpg" % k)
        p.write_bytes(data)
        a, b = _records(_run(exe, "desc", str(p), PI.path(same_as)))
        assert a == b, what


def test_mutated_and_truncated_files_end_in_ok_or_a_refusal(exe):
    """182 files x 40 seeded mutations (one byte of a header, DHT, DQT, DRI or SOS segment changed, or
    the file cut short), each parsed from a heap buffer of exactly its size: any read outside it, any
    overflow is a sanitizer report and a non-zero exit, and every file still accepted is held to
    what the kernel relies on"""
    names = PI.names()
    ok, refused = (int(x) for x in _run(exe, "fuzz", 20261019, 40, *[PI.path(n) for n in names]).split())
    assert ok + refused == 182 * 40
    assert ok > 500 and refused > 2000
