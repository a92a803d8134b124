"""GPU: stereo::Stereo::setPairsInFlight of the drop-in C++ class, run by
tests/cpp/shim_stereo_batch.cc: three pairs in flight give the cloud of the default object and of
the CPU chain (tests/stereo_sequence.py), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import stereo_batch_inputs as SB
import stereo_sequence as SS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from aerial_mapper_amd import build
    build.build_all()
    out = str(tmp_path_factory.mktemp("shim") / "shim_stereo_batch")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_stereo_batch.cc"), "-o", out,
                           "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip",
                           "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("use_bm", [True, False])
def test_cpp_set_pairs_in_flight_gives_the_default_objects_cloud(exe, tmp_path, use_bm):
    F, W, H = 6, 160, 120
    seq = SS.Sequence(F, W, H)
    xyz, inten, ns, _ = SB.cpu_chain(seq, SS.pairs_of(F, 1), use_bm)
    assert len(ns) == 5 and min(ns) > 0.25 * W * H
    path = str(tmp_path / "sequence.bin")
    with open(path, "wb") as f:
        f.write(np.array([F, W, H, 1, int(use_bm), xyz.shape[0], ns[-1]], np.int64).tobytes())
        K = seq.K
        f.write(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64).tobytes())
        f.write(seq.T_C_B.astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(seq.T_G_B, np.float64).tobytes())
        f.write(np.ascontiguousarray(seq.frames).tobytes())
        f.write(np.ascontiguousarray(xyz, np.float64).tobytes())
        f.write(np.ascontiguousarray(inten, np.int32).tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()[-2000:]
