"""The pure half of a session call (aerial_mapper_amd/csrc/amhip_session_plan.h: the layer states, sync_in, the three
sync_out stages, the window / routing / staging arithmetic) as a stand-alone program (tests/cpp/
session_plan_host_main.cc), built with g++ alone: once plain, once under the address and undefined-behaviour
sanitizers.  No GPU, nothing loaded into python.

tests/golden/session_plan/expected.txt is the program's output for tests/golden/session_plan/cases.txt as the
statements of amhip_session.hip (the window-edge lambda of amhip_session_create, halo_margin_m, the slice bounds, the
counts -> offsets -> totals loops of the routing, the rectangle test and the staging cap of sync_out) and of
amhip_api.hip (amhip_layers_reset, materialize, touch, overwrite, ctx_layer_set_initial, ctx_layer_is_initial, the
fused-fill claim) gave it BEFORE they moved into the header: recorded from a copy of the program in which those
statements stood unchanged.  Every later version of the header has to reproduce it byte for byte.

The protocol model enumerates EVERY sequence of LENGTH events out of: the host edits a matrix (new content, the
constant, the content it held before); a call that reads one layer and writes two (full window or a small rectangle
dirty, the second output changed or not, staging available or not); the same call failing inside and after each
sync_in, behind the kernel, and with downloads pending; amhip_layers_reset on the context; set_always_copy on / off.
What it asserts after every step is spelled out in the program (violations (a) .. (f))."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "session_plan")
CASES = os.path.join(GOLDEN, "cases.txt")
LENGTH = 5          # 26 events: 11 881 376 sequences, half a second plain, a few seconds under the sanitizers


def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp(name) / "session_plan_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "session_plan_host_main.cc"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "session_plan_host", [])


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "session_plan_host_san", [
        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])


def _run(exe, verb, arg):
    r = subprocess.run([exe, verb, arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=300)
    return r.returncode, r.stdout, r.stderr


def _expected():
    with open(os.path.join(GOLDEN, "expected.txt")) as fh:
        return fh.read()


def _assert_same(got, want):
    if got == want:
        return
    for k, (a, b) in enumerate(zip(got.split("\n"), want.split("\n"))):
        assert a == b, "line %d" % (k + 1)
    assert len(got) == len(want)


def _assert_model_holds(rc, out, err):
    """No violation, every action of the plan reached, and the whole enumeration done."""
    assert rc == 0, (out[-4000:], err[-4000:])
    assert "never reached" not in out, out[-2000:]
    last = out.strip().split("\n")[-1].split()
    assert last[:4] == ["0", "violations", "in", str(26 ** LENGTH)] and last[4:7] == ["sequences", "of", str(LENGTH)], \
        out[-500:]


def test_arithmetic_equals_the_recorded_table(exe):
    rc, out, err = _run(exe, "dump", CASES)
    assert rc == 0, err[-2000:]
    _assert_same(out, _expected())


def test_protocol_model_holds_for_every_event_sequence(exe):
    _assert_model_holds(*_run(exe, "model", str(LENGTH)))


def test_under_the_sanitizers(exe_sanitized):
    rc, out, err = _run(exe_sanitized, "dump", CASES)
    assert rc == 0, err[-4000:]
    _assert_same(out, _expected())
    _assert_model_holds(*_run(exe_sanitized, "model", str(LENGTH)))


def test_case_list_holds_what_it_has_to():
    """The arithmetic cases the table must not lose: a single window, the half-way edge (320 rows in 2: 192 + 128,
    llround), tiles equal to rows, the clamp n - (parts - k), 3 x 2 on a map smaller than one alignment unit per tile;
    the margin for radius_sq 1 .. 8 at two resolutions; routing for W = 1, 2, 6 and 9 (kMaxHaloDests = 8 crossed) with
    zero-count slices, a window whose total is zero and a refused total; the rectangle at exactly half the window and
    one cell over."""
    want = _expected()
    for needle in ("edges 128 96 1 1\n", "edges 320 256 2 1\n  edges_i 0 192 320\n", "edges 5 7 5 7\n",
                   "edges 33 33 1 5\n  edges_i 0 33\n  edges_j 0 1 2 31 32 33\n", "edges 100 40 3 2\n",
                   "rect 0 0 3 1 3 2\n  partial 1\n", "rect 0 0 2 2 3 2\n  partial 0\n",
                   "rect 0 0 64 96 128 96\n  partial 1\n", "rect 0 0 65 96 128 96\n  partial 0\n", "(refused)",
                   "staging 268435456 1\n  floats 268435456\n", "staging 268435457 1\n  floats 0\n"):
        assert needle in want, needle
    for r2 in range(1, 9):
        assert "halo %d 0.5\n" % r2 in want and "halo %d 0.25\n" % r2 in want
    routed = [line.split() for line in want.split("\n") if line.startswith("route ")]
    assert sorted(set(int(w[1]) for w in routed)) == [1, 2, 6, 9]
    for W in (6, 9):
        counts = [[int(v) for v in w[2:]] for w in routed if int(w[1]) == W][0]
        assert any(sum(counts[k * W:(k + 1) * W]) == 0 for k in range(W))      # a slice nobody needs
        assert any(sum(counts[d::W]) == 0 for d in range(W))                    # a window without points
