"""The host-side planner of a DSM call (aerial_mapper_amd/csrc/amhip_dsm_plan.h: plan_dsm, plan_gather_classes,
rough_policy_step) as a stand-alone program (tests/cpp/dsm_plan_host_main.cc), built with g++ alone: once plain,
once under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into python.

tests/golden/dsm_plan/expected.txt is the program's output for tests/golden/dsm_plan/cases.txt as the arithmetic
of make_dsm_params / dsm_run / dsm_rough_policy gave it BEFORE the planner was restructured (the bodies moved
into the header statement for statement); the plan_dsm part of it was also produced by calling that
make_dsm_params itself.  Every later version of the header has to reproduce it byte for byte.

Branches no input reaches, so that no tag stands for them:
  * "image over 150 KB at cap <= 2048": the largest image of a 2048-point launch (w0 = kMaxW0 = 16, bins of 8,
    tile height 32) is 90 624 bytes -- test_largest_small_image_is_far_below_the_budget holds the case;
  * rej_own false at cap0 = 4096 / true at 7680: the FP64 image of 4096 points is at most 98 352 + 32 336
    bytes (w0 = 16, tile height 16) against the 153 600 of the budget, the points of a 7680-point image
    alone take 184 368;
  * the n * d >= 2^32 escape of mul_r1: a sort plan has p3_r1 <= 256, so nby <= 32768 (mul_B and mul_w reach
    theirs: cases division_escape, division_escape_column_blocks);
  * "radius ladder too long": radius_sq >= 1 gives at most 22 levels; the case list reaches it with
    radius_sq = 0, which the API refuses before it plans."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dsm_plan")
CASES = os.path.join(GOLDEN, "cases.txt")

ALL_TAGS = {
    # ladder
    "ladder_long", "ladder_two", "pcl_first", "pcl_retry", "err_ladder", "err_bins",
    # main-launch shapes
    "shape_16_1024", "shape_32_2048", "shape_16_2048", "shape_16_4096", "shape_16_7680",
    "shape_fallback_beyond_7680", "nowide_exact", "nowide_exact_now", "nowide_knn",
    # lds_ok off, records that do not fit
    "ldsoff_w0", "ldsoff_pcl_retry", "ldsoff_knn_global", "recfits_rows", "recfits_points", "fx_on",
    # sort plan, multipliers
    "p3_on", "p3_off_points", "p3_off_geometry", "p3_r1_gt1", "p3_cc_cmax", "p3_cc_nbx", "p3_cap_lo", "p3_cap_hi",
    "mul_d1", "mul_escape", "mul_w_escape",
    # class plan
    "cls_tj16", "cls_tj32", "cls_f32", "cls_fp64", "cls_class1_empty", "rej_own_4096_true", "rej_own_7680_false",
    "sparse_on", "sparse_off_8192_tiles", "sparse_off_16_per_cell", "sparse_off_fill",
    "rej_dense_at_a_tenth", "rej_dense_above_a_tenth",
    "skip_classes_on", "skip_off_stale_signature", "skip_off_counters", "skip_off_no_launch_skips",
    # rough-terrain switch
    "policy_hold_and_release", "policy_exactly_half", "policy_smooth", "policy_switch_off", "policy_exact_mode",
    "policy_capped_mode", "policy_no_counters",
}


def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp(name) / "dsm_plan_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "dsm_plan_host_main.cc"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "dsm_plan_host", [])


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "dsm_plan_host_san", [
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


def test_invariants_of_the_lds_image_and_the_class_caps(exe):
    """Per case: lds_bytes / lds_bytes_f32 are lds_image_bytes of the plan's shape; what the kernels carve ends
    inside the image; class caps even and ordered; no image a launch can ask for above 160 KB; fx_ok implies
    lds_ok, mode 0, none of exact / exact-now / cap; lds_cells + 1 a multiple of four."""
    rc, out, err = _run(exe, "check")
    assert rc == 0, (out[-4000:], err[-2000:])
    last = out.strip().split("\n")[-1].split()
    assert last[:3] == ["0", "violations", "in"] and int(last[3]) >= 70, out[-500:]


def test_largest_small_image_is_far_below_the_budget(exe, tmp_path):
    """The widest window the LDS gather takes (w0 = 16) at both tile heights: the 2048-point image stays below
    150 KB, so `lds_bytes > 150 KB && cap <= 2048` turns lds_ok off for no input."""
    cases = tmp_path / "cases.txt"
    cases.write_text("plan name=a res=0.0625 n=2048\nplan name=b res=0.0625 n=2867\n")
    rc, out, err = _run(exe, "dump", str(cases))
    assert rc == 0, err[-2000:]
    sizes = [int(tok.split("=")[1]) for tok in out.split() if tok.startswith("lds_bytes=")]
    assert sizes == [90624, 81536] and max(sizes) < 150 * 1024
    assert out.count("lds_ok=1") == 2 and "shape_32_2048" in out and "shape_16_2048" in out
