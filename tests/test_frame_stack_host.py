"""The group planner of the image decoders (amhip_frame_plan.h: which frames of a call share one
scratch buffer) as a stand-alone program (tests/cpp/frame_stack_host_main.cc) under the address and
undefined-behaviour sanitizers, compared with a restatement of the rule.  No GPU, nothing loaded into
python.  The decoders' count cap (32768 frames per group) is reached by no GPU test: here the cap is
a parameter."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frame_stack_host") / "frame_stack_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "frame_stack_host_main.cc"), "-o", out])
    return out


def _run(exe, cases):
    """cases: (costs, budget, max_frames) -> per case (group_begin, bases, max)"""
    args = ["%d:%d:%s" % (budget, max_frames, ",".join(str(c) for c in costs)) for costs, budget, max_frames in cases]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3 * len(cases)
    out = []
    for k in range(len(cases)):
        g, b, m = (line.split() for line in lines[3 * k:3 * k + 3])
        assert (g[0], b[0], m[0]) == ("groups", "bases", "max") and len(m) == 2
        out.append(([int(x) for x in g[1:]], [int(x) for x in b[1:]], int(m[1])))
    return out


def _rule(costs, budget, max_frames):
    """A new group starts at i == 0, when running + cost[i] > budget, or when count == max_frames;
    base[i] is the running total before frame i; group_begin ends with F."""
    groups, bases, running, count, biggest = [], [], 0, 0, 0
    for i, c in enumerate(costs):
        if i == 0 or running + c > budget or count == max_frames:
            groups.append(i)
            running = count = 0
        bases.append(running)
        running += c
        count += 1
        biggest = max(biggest, running)
    return groups + [len(costs)], bases, biggest


def _properties(case, got):
    costs, budget, max_frames = case
    groups, bases, biggest = got
    F = len(costs)
    # contiguous, covering 0..F-1, no group empty
    assert groups[0] == 0 and groups[-1] == F and all(a < b for a, b in zip(groups, groups[1:])), (case, got)
    assert len(bases) == F
    totals = []
    for a, b in zip(groups, groups[1:]):
        assert b - a <= max_frames, (case, got)
        total = sum(costs[a:b])
        assert total <= budget or b - a == 1, (case, got)
        assert bases[a:b] == [sum(costs[a:i]) for i in range(a, b)], (case, got)
        totals.append(total)
    assert biggest == max(totals), (case, got)


AMPLE = 1 << 40

# (what, costs, budget, max_frames, group_begin, bases, max)
NAMED = [
    ("one frame", [700], 1000, 4, [0, 1], [0], 700),
    ("one frame dearer than the budget", [700], 10, 4, [0, 1], [0], 700),
    ("budget 0: one frame per group", [5, 1, 9, 2], 0, 4, [0, 1, 2, 3, 4], [0, 0, 0, 0], 9),
    ("budget = the exact sum: one group", [5, 1, 9, 2], 17, 8, [0, 4], [0, 5, 6, 15], 17),
    ("budget = the sum - 1: the last frame splits off", [5, 1, 9, 2], 16, 8, [0, 3, 4], [0, 5, 6, 0], 15),
    ("a dear frame first", [50, 3, 4], 10, 8, [0, 1, 3], [0, 0, 3], 50),
    ("a dear frame in the middle", [3, 50, 4], 10, 8, [0, 1, 2, 3], [0, 0, 0], 50),
    ("a dear frame last", [3, 4, 50], 10, 8, [0, 2, 3], [0, 3, 0], 50),
    ("the count cap alone", [1] * 7, AMPLE, 3, [0, 3, 6, 7], [0, 1, 2, 0, 1, 2, 0], 3),
    ("budget and count cap trip on the same frame", [2, 2, 2, 2], 6, 3, [0, 3, 4], [0, 2, 4, 0], 6),
    ("the count cap trips one frame before the budget", [2, 2, 2, 2, 2], 8, 3, [0, 3, 5], [0, 2, 4, 0, 2], 6),
    ("the budget trips one frame before the count cap", [2, 2, 2, 2, 2], 5, 3, [0, 2, 4, 5], [0, 2, 0, 2, 0], 4),
    ("frames that cost nothing", [0, 0, 0], 0, 2, [0, 2, 3], [0, 0, 0], 0),
    ("costs near 2^63 do not wrap", [1 << 62, 1 << 62, 1], (1 << 63) - 1, 8, [0, 1, 3], [0, 0, 1 << 62], (1 << 62) + 1),
]


def test_named_cases(exe):
    cases = [(c, b, m) for _, c, b, m, _, _, _ in NAMED]
    for (what, costs, budget, max_frames, groups, bases, biggest), got in zip(NAMED, _run(exe, cases)):
        assert got == (groups, bases, biggest), what
        assert got == _rule(costs, budget, max_frames), what
        _properties((costs, budget, max_frames), got)


def test_seeded_random_cases_equal_the_rule(exe):
    rng = random.Random(20261019)
    cases = []
    for _ in range(400):
        F = rng.randint(1, 12)
        cases.append(([rng.randint(0, 2000) for _ in range(F)], rng.randint(0, 5000), rng.randint(1, 5)))
    got = _run(exe, cases)
    for case, g in zip(cases, got):
        assert g == _rule(*case), case
        _properties(case, g)
    # both reasons for a new group, and groups of several frames, occur
    assert any(len(g[0]) == 2 for g in got) and any(len(g[0]) > 4 for g in got)
    assert any(max(b - a for a, b in zip(g[0], g[0][1:])) == c[2] for c, g in zip(cases, got))
