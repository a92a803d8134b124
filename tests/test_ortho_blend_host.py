"""The arithmetic of the blended mosaic (amhip_ortho_blend.h: the functions the kernel calls) as a
stand-alone program (tests/cpp/ortho_blend_host_main.cc) under the address and undefined-behaviour
sanitizers, compared bit for bit with the same steps in numpy float64 (the steps of
tests/ortho_blend_reference.py).  No GPU, nothing loaded into python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ortho_blend_host") / "ortho_blend_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ortho_blend_host_main.cc"), "-o", out])
    return out


def _run(exe, tmp_path, nch, sharpness, points, pixels):
    path = str(tmp_path / "case.txt")
    with open(path, "w") as fh:
        fh.write("%d %d %d\n" % (nch, sharpness, len(points)))
        for c, px in zip(points, pixels):
            fh.write(" ".join(float(v).hex() for v in list(c) + list(px)) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    out = r.stdout.split()
    sums = [float.fromhex(v) for v in out[:1 + nch]]
    return sums, (int(out[1 + nch], 16) if len(out) > 1 + nch else None)


def _numpy(nch, sharpness, points, pixels):
    wsum, acc = np.float64(0.0), [np.float64(0.0)] * nch
    for c, px in zip(np.asarray(points, np.float64), np.asarray(pixels, np.float64)):
        zz = c[2] * c[2]
        n2 = (c[0] * c[0] + c[1] * c[1]) + zz
        w = zz / n2
        for _ in range(sharpness):
            w = w * w
        acc = [acc[ch] + w * px[ch] for ch in range(nch)]
        wsum = wsum + w
    if not wsum > 0.0:
        return [wsum] + acc, None
    q = [np.rint(a / wsum) for a in acc]
    if nch == 3:
        return [wsum] + acc, (int(q[2]) << 16) | (int(q[1]) << 8) | int(q[0])
    return [wsum] + acc, int(np.float32(q[0]).view(np.uint32))


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("sharpness", [0, 1, 2, 3, 4])
def test_sums_and_values_match_numpy(exe, tmp_path, nch, sharpness):
    rng = np.random.Generator(np.random.PCG64(100 * nch + sharpness))
    for n in (1, 2, 7, 40):
        points = np.concatenate([rng.uniform(-40.0, 40.0, size=(n, 2)), rng.uniform(5.0, 70.0, size=(n, 1))], axis=1)
        pixels = rng.integers(0, 256, size=(n, nch))
        got = _run(exe, tmp_path, nch, sharpness, points, pixels)
        want = _numpy(nch, sharpness, points, pixels)
        assert [float(v).hex() for v in got[0]] == [float(v).hex() for v in want[0]]
        assert got[1] == want[1] and got[1] is not None


def test_ties_round_to_even_and_colour_packs_like_the_reference(exe, tmp_path):
    above = [(0.0, 0.0, 8.0)] * 2   # w = 1 exactly
    assert _run(exe, tmp_path, 1, 2, above, [(10,), (11,)]) == ([2.0, 21.0], int(np.float32(10.0).view(np.uint32)))
    assert _run(exe, tmp_path, 1, 2, above, [(11,), (12,)]) == ([2.0, 23.0], int(np.float32(12.0).view(np.uint32)))
    sums, bits = _run(exe, tmp_path, 3, 0, above[:1], [(37, 140, 251)])
    assert sums == [1.0, 37.0, 140.0, 251.0]
    assert bits == int(np.float32(O.color_value_bgr(37, 140, 251)).view(np.uint32))


def test_underflowed_weights_paint_nothing(exe, tmp_path):
    # sin^2 = 1e-24 squared four times: 1e-384, that is 0
    sums, bits = _run(exe, tmp_path, 1, 4, [(1e12, 0.0, 1.0)], [(200,)])
    assert sums == [0.0, 0.0] and bits is None
