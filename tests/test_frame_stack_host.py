"""The group planner of the image decoders and encoders (amhip_frame_plan.h: which frames of a call share
one scratch buffer), the cut of a group's files into download slices and the files' offsets, as a
stand-alone program (tests/cpp/frame_stack_host_main.cc) under the address and
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


# ---- the writers' download slices and the encoders' offsets ------------------------------------------
LIMIT = 1000


def _run_slices(exe, cases):
    """cases: (sizes, limit) -> per case (ends, bytes, offsets)"""
    args = ["%d:%s" % (limit, ",".join(str(c) for c in sizes)) for sizes, limit in cases]
    r = subprocess.run([exe, "slices"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3 * len(cases)
    out = []
    for k in range(len(cases)):
        e, b, o = (line.split() for line in lines[3 * k:3 * k + 3])
        assert (e[0], b[0], o[0]) == ("ends", "bytes", "offsets")
        out.append(([int(x) for x in e[1:]], [int(x) for x in b[1:]], [int(x) for x in o[1:]]))
    return out


def _slice_rule(sizes, limit):
    """A slice starts at a file and takes the following files while the sum stays <= limit; offsets are
    the exclusive prefix sums."""
    ends, sums, f = [], [], 0
    while f < len(sizes):
        total, end = sizes[f], f + 1
        while end < len(sizes) and total + sizes[end] <= limit:
            total += sizes[end]
            end += 1
        ends.append(end)
        sums.append(total)
        f = end
    return ends, sums, [sum(sizes[:i]) for i in range(len(sizes) + 1)]


def _slice_properties(case, got):
    sizes, limit = case
    ends, sums, offsets = got
    # contiguous, every file in exactly one slice, none empty
    starts = [0] + ends[:-1]
    assert ends[-1] == len(sizes) and all(a < b for a, b in zip(starts, ends)), (case, got)
    for a, b, total in zip(starts, ends, sums):
        assert total == sum(sizes[a:b]), (case, got)
        assert total <= limit or b - a == 1, (case, got)
    assert offsets == [sum(sizes[:i]) for i in range(len(sizes) + 1)], (case, got)


# (what, sizes, ends, bytes)
NAMED_SLICES = [
    ("one file exactly at the limit", [LIMIT], [1], [LIMIT]),
    ("one file over the limit, alone", [LIMIT + 1], [1], [LIMIT + 1]),
    ("[1, limit]: the second file does not fit behind the first", [1, LIMIT], [1, 2], [1, LIMIT]),
    ("[limit/2, limit/2, 1]: two fill the slice exactly", [LIMIT // 2, LIMIT // 2, 1], [2, 3], [LIMIT, 1]),
    ("a zero-length file rides along", [LIMIT, 0, 5], [2, 3], [LIMIT, 5]),
    ("a zero-length file first and alone", [0], [1], [0]),
    ("an oversized file in the middle", [3, 5 * LIMIT, 4], [1, 2, 3], [3, 5 * LIMIT, 4]),
]


def test_named_slice_cases(exe):
    cases = [(s, LIMIT) for _, s, _, _ in NAMED_SLICES]
    for (what, sizes, ends, sums), got in zip(NAMED_SLICES, _run_slices(exe, cases)):
        assert got[:2] == (ends, sums), what
        assert got == _slice_rule(sizes, LIMIT), what
        _slice_properties((sizes, LIMIT), got)


def test_seeded_random_slice_cases_equal_the_rule(exe):
    rng = random.Random(20261020)
    cases = []
    for _ in range(200):
        F = rng.randint(1, 14)
        cases.append(([rng.choice([0, 1, LIMIT // 2, LIMIT, LIMIT + 1, rng.randint(0, 1500)]) for _ in range(F)], LIMIT))
    got = _run_slices(exe, cases)
    for case, g in zip(cases, got):
        assert g == _slice_rule(*case), case
        _slice_properties(case, g)
    # slices of one oversized file and slices of several files both occur
    assert any(b > LIMIT for g in got for b in g[1])
    assert any(e - s > 2 for g in got for s, e in zip([0] + g[0][:-1], g[0]))
