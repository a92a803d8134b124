"""The host-side planner of a dsm_sort call (aerial_mapper_amd/csrc/amhip_sort_plan.h: plan_sort_call) as a
stand-alone program (tests/cpp/sort_plan_host_main.cc), built with g++ alone: once plain, once under the address
and undefined-behaviour sanitizers.  No GPU, nothing loaded into python.

tests/golden/sort_plan/expected.txt is the program's output for tests/golden/sort_plan/cases.txt as the arithmetic
of dsm_sort_impl / dsm_sort_runs gave it BEFORE the planner was restructured (their statements moved into the
header one by one, in their order).  Every later version of the header has to reproduce it byte for byte.

Branches no input reaches, so that no tag stands for them:
  * the run pipeline refused for n1 > kP3MaxKeys or n2 > kP3MaxKeys: plan_sort cuts the bin rows into
    p3_r1 = ceil(nby / 128) rows per partition, so p3_n1 <= 128, and takes at most 256 / p3_r1 column blocks,
    so p3_n2 = p3_r1 * p3_c <= 256;
  * the scan-2 grid cut BELOW what it asks for: a sort plan has at most 32768 sub-partitions, which ask for
    exactly the ceiling of 2048 workgroups (case scan2_grid_ceiling);
  * the rounds knob "at or above the default" when the default is not kP3BigCap is reached (case
    rounds_default_cut_by_tables), as is the knob on records.

Not in the case list, because `check` reports it (a limit of the driver this planner restates, not of the
planner): a column block of more than 3360 bins on records, or more than 3936 on doubles (plan_sort allows
4096), makes the big placement's image of kP3BigCap points larger than kLdsMaxBytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sort_plan")
CASES = os.path.join(GOLDEN, "cases.txt")

ALL_TAGS = {
    # outcomes
    "one_level", "halo_only", "count_doubles", "count_records", "runs",
    "one_level_by_size", "one_level_by_knob", "one_level_records", "one_level_doubles",
    # why the run pipeline was refused
    "refused_records", "refused_split", "refused_windowed", "refused_points", "refused_width", "refused_knob",
    # tiled calls, values
    "split_phase1", "split_phase2_no_second_part", "split_phase2_second_part", "split_dropped_one_level",
    "with_values",
    # the big placement launch
    "want_big_false", "want_big_stale_signature", "want_big_no_host_word", "want_big_count",
    "want_big_no_launch_skips", "want_big_records",
    # the rounds knob
    "rounds_knob_applied", "rounds_knob_below_16", "rounds_knob_at_default", "rounds_reread",
    # grids at their ends
    "count_grid_floor", "count_grid_ceiling", "scan2_grid_ceiling",
}


def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp(name) / "sort_plan_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "sort_plan_host_main.cc"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "sort_plan_host", [])


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "sort_plan_host_san", [
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


def _assert_no_violations(rc, out, err):
    assert rc == 0, (out[-4000:], err[-4000:])
    last = out.strip().split("\n")[-1].split()
    assert last[:3] == ["0", "violations", "in"] and int(last[3]) >= 50, out[-500:]


def test_plan_equals_the_recorded_table(exe):
    rc, out, err = _run(exe, "dump")
    assert rc == 0, err[-2000:]
    _assert_same(out, _expected())


def test_plan_under_the_sanitizers(exe_sanitized):
    rc, out, err = _run(exe_sanitized, "dump")
    assert rc == 0, err[-4000:]
    _assert_same(out, _expected())
    _assert_no_violations(*_run(exe_sanitized, "check"))


def test_case_list_reaches_every_branch():
    seen = set()
    for line in _expected().split("\n"):
        if line.startswith("tags"):
            seen.update(line.split()[1:])
    assert seen == ALL_TAGS, (sorted(seen - ALL_TAGS), sorted(ALL_TAGS - seen))


def test_invariants_of_workspace_images_and_placement_policy(exe):
    """Per case: the stripe_ws regions are disjoint, in order, in whole quads behind the plan block, and end inside
    ws_words; every LDS image is at most kLdsMaxBytes, holds what its kernel carves (spelled out in the program
    from the kernels' lines, and equal to the header's list), and the big placement's is the larger of its two
    users'; the run table fits the points' image; cap_rounds >= 16; the skip words send every sub-partition size to
    exactly one placement launch, with and without the big one; range_parts is the first scatter's grid times its
    waves."""
    _assert_no_violations(*_run(exe, "check"))


def test_widest_column_blocks_exceed_the_big_placement_image(exe, tmp_path):
    """What the docstring says of column blocks beyond 3360 / 3936 bins: the limit is where it is said to be."""
    cases = tmp_path / "cases.txt"
    cases.write_text("sort name=rec_3360 p3min=0 rows=3354 cols=8 res=1 n=1000\n"
                     "sort name=rec_3361 p3min=0 rows=3355 cols=8 res=1 n=1000\n"
                     "sort name=dbl_3936 exact=1 p3min=0 rows=3930 cols=8 res=1 n=1000\n"
                     "sort name=dbl_3937 exact=1 p3min=0 rows=3931 cols=8 res=1 n=1000\n")
    rc, out, err = _run(exe, "check", str(cases))
    assert rc == 1, (out, err)
    lines = out.strip().split("\n")
    assert lines[-1] == "2 violations in 4 plans", out
    assert lines[0].startswith("rec_3361: big record placement: image above") and \
        lines[1].startswith("dbl_3937: big placement: image above"), out
