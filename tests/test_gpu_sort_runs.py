"""The three-pass sort without its count pass (tuning key sort_runs): local sorts,
runs gathered on the read side.  Every case runs in a child process whose knobs come from
conftest.tuning_env (p3_min_points=0: clouds of 1e4..1e5 points take the three-pass path) and is
checked three ways: against the CPU oracle (1e-6 m, the FP64 mode's bar), bit for bit against the
counting pipeline (sort_runs=0; the reproducible-floats guard of DESIGN.md 4.2 makes the FP64 mode's
heights a function of the point SET), and on the number of points binned.  The accessor
dsm_stats()["sort_pipeline"] proves which pipeline a call took.

The child is this file run as a script: python test_gpu_sort_runs.py <case>.

Not reachable, and therefore not a case: n1 = 1.  A map has at least three bin rows (the margin
on both sides is at least one bin) and up to 128 bin rows form a partition each, so n1 >= 3; the
smallest map stands in for it ("tiny-map").  n2 = 1 is forced with a large p3_target.

Sizes at which the code changes path: kP3Chunk = 2560 points (chunk and segment edges), 2048
covering chunks of a pass-2 segment and 512 segments of a k1 partition (the run tables are searched
in memory instead of LDS: "sparse", 5.3 M points, and "long-partition", 1.3 M -- the smallest that
get there; about 4 s each on an MI355X box), sub-partitions beyond p3_cap / p3_rounds_cap (the
skew cases under the forcing knobs).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

CHUNK = 2560


# ---------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------
def _terrain(xy, rng, noise=0.3):
    from aerial_mapper_amd import synth
    return synth.terrain_height(xy[:, 0], xy[:, 1]) + rng.uniform(-noise, noise, xy.shape[0])


def _cloud(xy, rng):
    pts = np.empty((xy.shape[0], 3))
    pts[:, :2] = xy
    pts[:, 2] = _terrain(xy, rng)
    return np.ascontiguousarray(pts)


def _uniform(n, lx, ly, rng, margin=2.0):
    return np.c_[rng.uniform(-lx / 2 - margin, lx / 2 + margin, n),
                 rng.uniform(-ly / 2 - margin, ly / 2 + margin, n)]


def _band(n, y, lx, rng):
    """n points on ONE northing (one cell row, so one bin row, so one k1 partition), inside the map"""
    return np.c_[rng.uniform(-lx / 2 + 1.0, lx / 2 - 1.0, n), np.full(n, y)]


class _Child(object):
    def __init__(self):
        import aerial_mapper_amd as A
        import oracle_ffi as O
        import scenarios as S
        from aerial_mapper_amd import hip_lib
        self.A, self.O, self.S, self.L = A, O, S, hip_lib

    def dsm(self, g, clouds, runs, exact=True, window=None):
        """the clouds one after the other on one context; elevation and stats of the last"""
        A = self.A
        if runs is not None:
            self.L.set_tuning("sort_runs", 1 if runs else 0)
        st = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)
        with A.AerialGridMap(st, window=window) as m:
            m.set_dsm_precision(exact)
            d = A.Dsm(A.DsmSettings(), m)
            for pts in clouds:
                m.reset()
                d.process(pts, m)
            return m.get("elevation"), m.dsm_stats()

    def check(self, g, pts, expect="runs", warm=(), binned=None):
        """the three checks of the module's docstring on `pts` (after the clouds `warm`)"""
        rc, want, _ = self.O.dsm_process(pts, g)
        assert rc == self.O.OK
        clouds = list(warm) + [pts]
        e1, s1 = self.dsm(g, clouds, True)
        e0, s0 = self.dsm(g, clouds, False)
        assert s1["sort_pipeline"] == expect, s1
        assert s0["sort_pipeline"] == "count", s0
        self.S.assert_dsm_close(e1, want, tol=1e-6)
        self.S.assert_dsm_close(e0, want, tol=1e-6)
        same = (e1.view(np.uint32) == e0.view(np.uint32)) | (np.isnan(e1) & np.isnan(e0))
        assert same.all(), "%d cells differ between the pipelines" % int((~same).sum())
        assert s1["points_binned"] == s0["points_binned"], (s1, s0)
        if binned is not None:
            assert s1["points_binned"] == binned, (s1, binned)
        return e1

    # ---- cases ----
    def chunk_edges(self):
        O = self.O
        g = O.make_grid(120.0, 80.0, 0.5)
        rng = np.random.default_rng(11)
        for n in (4 * CHUNK - 1, 4 * CHUNK, 4 * CHUNK + 1):
            self.check(g, _cloud(_uniform(n, 120.0, 80.0, rng), rng))
        # a third outside the map: chunks compact to fewer than 2560 points ...
        n = 6 * CHUNK + 5
        xy = _uniform(n, 120.0, 80.0, rng)
        out = rng.permutation(n)[:n // 3]
        xy[out, 0] += 1000.0
        self.check(g, _cloud(xy, rng))
        # ... and the last chunk bins nothing
        xy = _uniform(n, 120.0, 80.0, rng)
        xy[5 * CHUNK:, 1] -= 1000.0
        self.check(g, _cloud(xy, rng))

    def segment_edges(self):
        # k1 partitions of exactly 2560 m, 2560 m + 1 and 1 points, the cloud shuffled: every chunk
        # holds a run of each of the two large partitions, the segments' edges fall inside runs
        O = self.O
        lx, ly = 120.0, 60.0
        g = O.make_grid(lx, ly, 0.5)
        rng = np.random.default_rng(12)
        m = 2
        xy = np.concatenate([_band(CHUNK * m, -20.0, lx, rng), _band(CHUNK * m + 1, 0.0, lx, rng),
                             _band(1, 20.0, lx, rng)])
        xy = xy[rng.permutation(xy.shape[0])]
        self.check(g, _cloud(xy, rng), binned=xy.shape[0])

    def _sparse_cloud(self, rng, lx, ly, chunks):
        n = CHUNK * chunks
        xy = _uniform(n, lx, ly - 20.0, rng, margin=0.0)      # (nothing within 10 m of the band below)
        xy[:, 1] -= 10.0
        xy[::50 * CHUNK, 1] = ly / 2 - 3.0                    # one point of every 50th chunk
        return xy

    def sorted_input(self):
        # sorted by coordinate: a chunk is one long run of one key (or two), most keys are absent
        # from most chunks; and the reverse order
        O = self.O
        lx, ly = 160.0, 120.0
        g = O.make_grid(lx, ly, 0.5)
        rng = np.random.default_rng(13)
        pts = _cloud(self._sparse_cloud(rng, lx, ly, 30), rng)
        order = np.lexsort((pts[:, 0], pts[:, 1]))
        a = self.check(g, np.ascontiguousarray(pts[order]))
        b = self.check(g, np.ascontiguousarray(pts[order[::-1]]))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))

    def sparse(self):
        # a partition that gets one point from every 50th chunk of 2060: its one segment spans
        # thousands of chunks with empty runs -- more than the 2048 whose table LDS holds
        O = self.O
        lx, ly = 800.0, 600.0
        g = O.make_grid(lx, ly, 0.5)
        rng = np.random.default_rng(14)
        self.check(g, _cloud(self._sparse_cloud(rng, lx, ly, 2060), rng))

    def long_partition(self):
        # one k1 partition of 520 segments and a bit: the placement searches its run lists in memory
        O = self.O
        lx, ly = 2400.0, 12.0
        g = O.make_grid(lx, ly, 0.5)
        rng = np.random.default_rng(15)
        n = CHUNK * 520 + 7
        self.check(g, _cloud(_band(n, 1.0, lx, rng), rng), binned=n)

    def skew(self):
        # all points in one k1 partition / one sub-partition / one bin; under the forcing knobs of the
        # parent process the big and the rounds placement read through the run lists.  Each also
        # after a uniform cloud of the same size on the same context: the big launch is then
        # skipped and the main placement kernel takes the over-full sub-partitions itself.
        O = self.O
        lx, ly = 120.0, 60.0
        g = O.make_grid(lx, ly, 0.5)
        rng = np.random.default_rng(16)
        n = 20000
        uni = _cloud(_uniform(n, lx, ly, rng), rng)
        one_partition = _band(n, 0.0, lx, rng)
        one_sub = np.c_[rng.uniform(10.0, 11.4, n), np.full(n, 0.0)]
        one_bin = np.c_[np.full(n, 10.1), np.full(n, 0.1)]
        for xy in (one_partition, one_sub, one_bin):
            pts = _cloud(xy, rng)
            self.check(g, pts, binned=n)
            self.check(g, pts, warm=[uni, uni], binned=n)

    def tiny_map(self):
        O = self.O
        rng = np.random.default_rng(17)
        g = O.make_grid(1.0, 1.0, 0.5)
        self.check(g, _cloud(_uniform(3 * CHUNK + 3, 1.0, 1.0, rng, margin=1.0), rng))

    def one_column_block(self):
        # (the parent sets p3_target so that a bin row is one column block: n2 = 1)
        O = self.O
        rng = np.random.default_rng(18)
        g = O.make_grid(40.0, 30.0, 0.5)
        self.check(g, _cloud(_uniform(3 * CHUNK + 3, 40.0, 30.0, rng), rng))

    def values(self):
        A, O, S = self.A, self.O, self.S
        rng = np.random.default_rng(19)
        uni = S.Scene(150.0, 110.0, 0.5, 70000, seed=82)
        clu = S.Scene(60.0, 40.0, 0.25, 20000, seed=81)
        dense = np.empty((40000, 3))
        dense[:, 0] = rng.uniform(10.0, 20.0, 40000)
        dense[:, 1] = rng.uniform(5.0, 15.0, 40000)
        dense[:, 2] = 400.0 + rng.uniform(-0.5, 0.5, 40000)
        clu.points = np.ascontiguousarray(np.concatenate([clu.points, dense]))
        for sc in (uni, clu):
            g = sc.grid
            inten = (np.arange(sc.points.shape[0]) % 251).astype(np.int32)
            rc, want = O.ortho_from_pcl(sc.points, inten, g)
            for runs in (True, False):
                self.L.set_tuning("sort_runs", 1 if runs else 0)
                st = A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)
                with A.AerialGridMap(st) as m:
                    A.OrthoFromPcl(A.OrthoFromPclSettings()).process(sc.points, inten, m)
                    got = m.get("ortho")
                    assert m.dsm_stats()["sort_pipeline"] == ("runs" if runs else "count")
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-3)

    def _not_eligible(self, exact=True, window=None):
        O, S = self.O, self.S
        sc = S.Scene(150.0, 110.0, 0.5, 70000, seed=82)
        g = sc.grid
        rc, want, _ = O.dsm_process(sc.points, g)
        assert rc == O.OK
        got, st = self.dsm(g, [sc.points], None, exact=exact, window=window)
        assert st["sort_pipeline"] == "count", st
        if window is not None:
            i0, j0, r, c = window
            want = want[j0:j0 + c, i0:i0 + r]
        S.assert_dsm_close(got, want, tol=1e-6 if exact else 1e-4)

    def single_precision(self):
        self._not_eligible(exact=False)

    def windowed(self):
        g = self.O.make_grid(150.0, 110.0, 0.5)
        self._not_eligible(window=(0, 0, g.rows // 2, g.cols))

    def switched_off(self):
        # (the parent sets sort_runs=0 in AMHIP_TUNING; nothing here touches the key)
        self._not_eligible()

    def determinism(self):
        O = self.O
        sc = self.S.Scene(150.0, 110.0, 0.5, 70000, seed=85)
        rng = np.random.default_rng(20)
        maps = []
        for _ in range(2):
            pts = np.ascontiguousarray(sc.points[rng.permutation(sc.points.shape[0])])
            e, st = self.dsm(sc.grid, [pts], True)
            assert st["sort_pipeline"] == "runs"
            maps.append(e)
        same = (maps[0].view(np.uint32) == maps[1].view(np.uint32)) | (np.isnan(maps[0]) & np.isnan(maps[1]))
        assert same.all()
        rc, want, _ = O.dsm_process(sc.points, sc.grid)
        self.S.assert_dsm_close(maps[0], want, tol=1e-6)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    getattr(_Child(), sys.argv[1])()
    print("SORT_RUNS_OK")
    sys.exit(0)


# ---------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu

_ROUNDS = {"p3_target": "4000", "p3_cap": "64", "p3_rounds_cap": "96"}

CASES = [
    ("chunk_edges", {}),
    ("segment_edges", {}),
    ("sorted_input", {}),
    ("sparse", {}),
    ("long_partition", {}),
    ("skew", {}),
    ("skew", {"p3_target": "48"}),
    ("skew", _ROUNDS),
    ("skew", dict(_ROUNDS, p3_rounds_reread="1")),
    ("tiny_map", {}),
    ("one_column_block", {"p3_target": "1000000"}),
    ("values", {}),
    ("single_precision", {}),
    ("windowed", {}),
    ("switched_off", {"sort_runs": "0"}),
    ("determinism", {}),
]


@pytest.mark.parametrize("case,knobs", CASES,
                         ids=["%s%s" % (c, "".join("-%s=%s" % kv for kv in sorted(k.items()))) for c, k in CASES])
def test_sort_runs(case, knobs):
    from conftest import tuning_env
    env = tuning_env(p3_min_points="0", **knobs)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"SORT_RUNS_OK" in r.stdout, r.stdout.decode()[-3000:]
