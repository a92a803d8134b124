"""The host-side planner of a backward-grid mosaic call (aerial_mapper_amd/csrc/amhip_ortho_plan.h: hpose_*,
camera_view_bounds, side_planes, build_frame_table, plan_ortho_call) as a stand-alone program
(tests/cpp/ortho_plan_host_main.cc), built with g++ alone and -ffp-contract=off like the library: once plain, once
under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into python.

tests/golden/ortho_plan/expected.txt is the program's output for tests/golden/ortho_plan/cases.txt as the arithmetic
of amhip_api.hip (the quaternion rotation and hpose_*, distorted_view_cone, distorted_rectangle_and_inner_cone, the
set-up of OrthoParams with its two plane blocks and two-level camera cache, amhip_camera_view_bounds, the
frame-table loop and the switches of amhip_ortho_backward_process_dev) and of
ortho_run gave it BEFORE the planner was restructured: it was recorded with a header that held those statements
moved unchanged, line range by line range, behind the interface the program drives.  Every later version of the
header has to reproduce it byte for byte.  Doubles are %a; what lies downstream of libm's atan / tan (the bounds and
planes of an equidistant camera, the atan table) is %.13g.

The mosaic has seven tuning knobs (six read on the way through the API call, one by ortho_run), not eight: each
is on alone in one case.

Recorded as it is, not judged here: `if (!(dev <= qdev)) qdev = dev` lets a NaN |q|^2 stick only when it comes from
the LAST frame -- a finite deviation behind it replaces it (case nan_before_the_last_frame: the cull stays on).

Branches no input reaches, so that no tag stands for them:
  * "no cone, but a rectangle": the rectangle is computed only from a usable cone (camera_view_bounds);
  * the final `return false` of distorted_view_cone: a camera with a distortion model is radtan or equidistant;
  * list_grid below 256 * 16 together with the tile list: the list is walked from 16 384 tiles."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ortho_plan")
CASES = os.path.join(GOLDEN, "cases.txt")

ALL_TAGS = {
    # pose chain
    "compose_identity", "compose_general", "pose_identity", "pose_general", "pose_nan", "pose_far", "table_F1",
    "table_F3", "norm_above_keeps_fast", "norm_below_keeps_fast", "norm_above_refuses_fast",
    "norm_below_refuses_fast", "qdev_quarter_cull_off", "qdev_nan_cull_off", "nan_before_the_last_frame_qdev_finite",
    "fast", "exact",
    # cameras
    "bounds_image_box", "cull_view_pyramid", "no_cull_no_focal", "no_cull_distorted_no_focal", "bounds_radtan",
    "bounds_equidistant", "inner_cone", "no_inner_cone", "rectangle_inside_cone", "rectangle_is_cone",
    "cone_beyond_1e3_no_rectangle", "no_bound_half_space", "no_bound_tangential_only", "no_bound_weak_k1_tail",
    "no_bound_weak_k2_tail", "no_bound_dip_beyond_half_the_scan", "colored",
    # knobs
    "knob_no_distorted_cull", "knob_no_distorted_prune", "knob_distorted_square_cull", "knob_ortho_exact_fold",
    "knob_no_coarse_cull", "knob_ortho_no_prune", "knob_ortho_no_tile_list",
    # layer states
    "outputs_all_lazy", "outputs_one_materialized", "nobs_initial", "nobs_lazy", "nobs_written", "prune", "no_prune",
    # launch
    "coarse", "coarse_F64", "no_coarse_F65", "no_coarse_no_zrange", "tile_list", "tile_list_16384", "dense_16383",
    "dense_lazy_outputs", "dense_no_coarse", "partial_tile", "window_offset",
}


def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp(name) / "ortho_plan_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "ortho_plan_host_main.cc"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "ortho_plan_host", [])


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "ortho_plan_host_san", [
        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])


def _run(exe, verb, cases=CASES):
    r = subprocess.run([exe, verb, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120)
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


def test_plan_equals_the_recorded_table(exe):
    rc, out, err = _run(exe, "dump")
    assert rc == 0, err[-2000:]
    _assert_same(out, _expected())


def test_plan_under_the_sanitizers(exe_sanitized):
    rc, out, err = _run(exe_sanitized, "dump")
    assert rc == 0, err[-4000:]
    _assert_same(out, _expected())
    rc, out, err = _run(exe_sanitized, "check")
    assert rc == 0, (out[-2000:], err[-4000:])


def test_case_list_reaches_every_branch():
    seen = set()
    for line in _expected().split("\n"):
        if line.startswith("tags"):
            seen.update(line.split()[1:])
    assert seen == ALL_TAGS, (sorted(seen - ALL_TAGS), sorted(ALL_TAGS - seen))


def test_invariants_of_a_plan(exe):
    """Per call: the side planes are of unit length; prune implies cull and virt_nobs; coarse implies cull; the
    tile list implies coarse and materialized outputs; the list buffer holds its header and every tile
    (>= ntiles + 8); the builder's and the dense grid reach every tile; fast implies an undistorted camera;
    radius_scale == 1 + 2 qdev; no cull with |q|^2 off by a quarter or more; the camera cache is filled exactly
    when the distorted cull is on, and a warm cache plans the same; sizeof(OrthoParams) and
    sizeof(FrameFast) == 2 * sizeof(FramePose) (static_asserts of the program)."""
    rc, out, err = _run(exe, "check")
    assert rc == 0, (out[-4000:], err[-2000:])
    last = out.strip().split("\n")[-1].split()
    assert last[:3] == ["0", "violations", "in"] and int(last[3]) >= 54, out[-500:]


def test_inverse_keeps_the_sign_of_a_zero_translation(exe):
    """hpose_inverse negates the rotated translation without adding a zero to it first: the identity's inverse has
    the translation (-0, -0, -0), as the product always computed it."""
    rc, out, err = _run(exe, "dump")
    assert rc == 0, err[-2000:]
    at = out.index("case call pose_identity")
    pose = [ln for ln in out[at:].split("\n") if ln.startswith("pose[0]")][0].split()
    assert pose[1:] == ["0x1p+0"] + ["-0x0p+0"] * 6 + ["0x0p+0"]
