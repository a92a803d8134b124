"""GPU: ortho::OrthoBackwardGrid::setBlend of the C++ drop-in (tests/cpp/shim_blend.cc, built like
the programs of test_gpu_cpp_shim.py) on the main scene of tests/ortho_blend_scenes.py: with
setBlend(true, 2) the layers of the rule's numpy statement, after setBlend(false) the plain mosaic's."""
import os
import subprocess

import numpy as np
import pytest

import ortho_blend_reference as B
import ortho_blend_scenes as BS
import ortho_occlusion_reference as R
import ortho_occlusion_scenes as SC
import scenarios as S
from aerial_mapper_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from aerial_mapper_amd import build
    if not (os.path.exists(build.LIB_PATH) and os.path.exists(build.SHIM_PATH)):
        build.build_all()
    out = str(tmp_path_factory.mktemp("shim_blend") / "shim_blend")
    lib = os.path.join(ROOT, "aerial_mapper_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_blend.cc"), "-o", out,
                           "-L" + lib, "-laerial_mapper_shim", "-laerial_mapper_hip", "-Wl,-rpath," + lib])
    return out


@pytest.mark.parametrize("mode", ["on", "off"])
def test_cpp_dropin_set_blend(exe, tmp_path, mode):
    BS.elevation("block").tofile(str(tmp_path / "elevation.f32"))
    BS.main_poses().tofile(str(tmp_path / "poses.f64"))
    np.stack(BS.frames()).tofile(str(tmp_path / "frames.u8"))
    env = dict(os.environ)
    env.pop("AERIAL_MAPPER_HIP_DEVICES", None)
    r = subprocess.run([exe, str(tmp_path), mode, "2"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300, env=env)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    got = {n: np.fromfile(str(tmp_path / ("%s.%s.f32" % (n, mode))), np.float32).reshape(SC.COLS, SC.ROWS)
           for n in B.LAYERS}
    if mode == "on":
        want, _ = BS.expected()
    else:
        want = SC.fresh_layers(BS.elevation("block"))
        R.process(SC.grid(), BS.camera(), BS.main_poses(), synth.IDENTITY_POSE, BS.frames(), want, False, None)
    S.assert_layers_equal(got, want, B.LAYERS)
