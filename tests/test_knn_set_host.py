"""CPU: the sorted set of the DSM's capped mode (aerial_mapper_amd/csrc/amhip_knn_set.h: KnnSetT,
knn_add, knn_init -- the functions k_dsm_gather_tiled_knn and k_dsm_gather_knn compile), emulated
on the host by tests/cpp/knn_set_emul.cc, against what oracle/amo_dsm.cc does: a stable sort of the
sequence by d2, cut to k.  Exact equality, including WHICH of two equal distances stays (a later
arrival never displaces an equal distance), the count n and the cached `worst`."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = list(range(1, 9))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("knn") / "libknn_set_emul.so")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
        "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "knn_set_emul.cc"), "-o", out])
    lib = C.CDLL(out)
    lib.emul_knn_set.restype = C.c_int
    lib.emul_knn_set_batch.restype = C.c_int
    return lib


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _run_batch(emul, k, seqs):
    """seqs: list of (d2 list, z list) -> list of (n, d2[8], z[8], worst)"""
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s[0]) for s in seqs])
    d2 = np.array([v for s in seqs for v in s[0]] + [0.0], np.float64)   # (+ one: never an empty buffer)
    z = np.array([v for s in seqs for v in s[1]] + [0.0], np.float64)
    od = np.full((len(seqs), 8), -1.0)
    oz = np.full((len(seqs), 8), -1.0)
    ow = np.full(len(seqs), -1.0)
    on = np.full(len(seqs), -1, np.int32)
    rc = emul.emul_knn_set_batch(C.c_int(k), C.c_int(len(seqs)), _p(off, C.c_int32), _p(d2), _p(z),
                                 _p(od), _p(oz), _p(ow), _p(on, C.c_int32))
    assert rc == 0
    return [(int(on[t]), od[t], oz[t], float(ow[t])) for t in range(len(seqs))]


def _stand_in(k, d2, z):
    """std::stable_sort by d2, cut to k (sorted() is stable)"""
    order = sorted(range(len(d2)), key=lambda q: d2[q])[:k]
    return [d2[q] for q in order], [z[q] for q in order]


def _assert_all(emul, k, seqs, what):
    bad = []
    for (d2, z), (n, gd, gz, worst) in zip(seqs, _run_batch(emul, k, seqs)):
        wd, wz = _stand_in(k, d2, z)
        want_worst = wd[k - 1] if len(wd) == k else float("inf")
        if not (n == len(wd) and list(gd[:n]) == wd and list(gz[:n]) == wz and worst == want_worst):
            bad.append((d2, z, n, list(gd), list(gz), worst))
    assert not bad, "%s, k = %d: %d of %d sequences differ, first: %r" % (what, k, len(bad), len(seqs), bad[0])


@pytest.mark.parametrize("k", KS)
def test_every_sequence_up_to_six_over_four_values_with_a_duplicate(emul, k):
    """Exhaustive: 5461 sequences.  Two of the four symbols share d2 = 0.5, so ties fall inside the
    set, at the k-th place, and among more candidates than slots; z tells the arrivals apart."""
    values = [0.25, 0.5, 0.5, 1.0]
    seqs = []
    for length in range(0, 7):
        for sym in itertools.product(range(4), repeat=length):
            seqs.append(([values[s] for s in sym], [100.0 + 10.0 * q + s for q, s in enumerate(sym)]))
    assert len(seqs) == sum(4 ** n for n in range(7))
    _assert_all(emul, k, seqs, "exhaustive")


@pytest.mark.parametrize("k", KS)
def test_ascending_and_descending_runs_of_twenty(emul, k):
    up = [0.125 * (q + 1) for q in range(20)]
    z = [300.0 + q for q in range(20)]
    _assert_all(emul, k, [(up, z)], "ascending")
    _assert_all(emul, k, [(up[::-1], z)], "descending")


@pytest.mark.parametrize("k", KS)
def test_two_thousand_random_sequences_with_frequent_duplicates(emul, k):
    rng = np.random.default_rng(8800 + k)
    values = np.array([0.0625 * v for v in (1, 2, 3, 5, 7, 8, 11, 12, 13, 14, 15, 16)])
    assert len(values) == 12
    seqs = []
    for _ in range(2000):
        n = int(rng.integers(1, 41))
        seqs.append((list(values[rng.integers(0, 12, n)]), list(400.0 + rng.permutation(n).astype(np.float64))))
    _assert_all(emul, k, seqs, "random")


@pytest.mark.parametrize("k", KS)
def test_fewer_entries_than_k_leave_worst_infinite(emul, k):
    for n in range(0, k):
        d2 = [0.5, 0.25, 0.5, 1.0, 0.125, 0.25, 2.0][:n]
        z = [500.0 + q for q in range(n)]
        (got_n, gd, gz, worst), = _run_batch(emul, k, [(d2, z)])
        assert got_n == n and worst == float("inf"), (k, n, got_n, worst)
        wd, wz = _stand_in(k, d2, z)
        assert list(gd[:n]) == wd and list(gz[:n]) == wz
        # (the unused slots stay as knn_init left them)
        assert (gd[n:] == 0.0).all() and (gz[n:] == 0.0).all()
