"""An exact restatement of ortho::OrthoFromPcl (ortho-from-pcl.cc:20-113; oracle/amo_dsm.cc
amo_ortho_from_pcl_process), for the tests of its edges: numpy and Python integers / fractions, every
cell against the points of a band around it -- no kd-tree, no bins, no GPU.

Per cell:
  * the centre is oracle_ffi.cell_position; d2 = dx*dx; d2 = d2 + dy*dy in doubles, unfused, against the
    points as they are (no centre offsets in this class);
  * the search keeps d2 < T, strictly, T = radius (the int the settings hold: a SQUARED radius);
  * adaptive mode: a cell whose search is empty repeats it with T = lambda * radius for lambda = 10, 100,
    ... -- an int product.  The restatement stops where that product would pass 2^31 - 1 (the
    reference's int overflows there: undefined; the product's contract is that such a cell is left
    alone).  `level` says which search filled a cell: 0 the first, k the retry with lambda = 10^k;
  * a kept point with d2 == 0 makes the cell that point's value: the answer is the SET of the values of
    the coincident points (which of several the reference takes is its tree order's choice);
  * otherwise the answer is the exact rational h = sum(z / d2) / sum(1 / d2) over the double d2's.

What a stored float may be (assert_obeys), from the product's own bound (amhip_dsm.hip, "Run-to-run
reproducibility"): a double evaluation of h whose terms pass n + 1 roundings lies within (2 n + 3) 2^-53
max|z| of h; the kernels store (float)h only where every value within (4 n + 8) 2^-53 max|z| rounds to one
float, and recompute the cell in double-double otherwise.  With n <= N, the points of the call:

    delta = (4 N + 8) 2^-53 max|z|                        (max|z| over the call's points)
    RN32(h - delta) == RN32(h + delta)   ->  the cell holds exactly that float
    otherwise ("in the band")            ->  any float from RN32(h - delta) to RN32(h + delta): the two
                                             adjacent floats around the rounding boundary
    exact hit                            ->  a member of the set, as a float
    no sample                            ->  the bits the layer had before the call

How the exact answer is reached without a rational per cell: h~, the same sums in numpy doubles, lies
within (2 n + 3) 2^-53 max|z| <= delta / 2 of h (each term one division, at most n - 1 additions, one
final division; positive weights).  So [h - delta, h + delta] lies inside [h~ - 3 delta, h~ + 3 delta]
(the outer ends computed in doubles: one more rounding each, below delta / 8), and where the two outer
ends round to one float, so do the inner ones, rounding being monotone.  Every other cell -- a few per
ten thousand -- is decided with fractions.Fraction: h exactly, h -+ delta exactly, rounded to float32
by rn32().  exact_cell() is the Fraction evaluation on its own; tests/test_ortho_from_pcl_reference.py
holds the shortcut to it."""
import math
from fractions import Fraction

import numpy as np

import oracle_ffi as O

INT_MAX = 2 ** 31 - 1
INIT_VALUE = np.float32(255.0)      # the ortho layer's initial value (aerial-mapper-grid-map.cc:40-48)


def thresholds(radius, adaptive):
    """T of every search in order; the ladder ends before the int product passes 2^31 - 1"""
    T = [int(radius)]
    lam = 10
    while adaptive and lam * int(radius) <= INT_MAX:
        T.append(lam * int(radius))
        lam *= 10
    return T


def rn32(x):
    """the float32 nearest to the rational x, ties to even"""
    x = Fraction(x)
    c = np.float32(float(x))        # (a double rounding: at most one float off)
    assert np.isfinite(c)
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        key = (abs(Fraction(float(cand)) - x), int(np.float32(cand).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(cand))
    return best[1]


class Search(object):
    """Which points every cell's search keeps, independent of the values.  level, count: (cols, rows)
    (level -1: no search found anything, count 0).  The kept points as one list per cell in cell order
    lin = i + j * rows: cell c owns idx[ptr[c] : ptr[c + 1]] (rows of the cloud) and their d2."""

    def __init__(self, g, n_points):
        self.grid, self.n_points = g, n_points
        self.level = np.full((g.cols, g.rows), -1, np.int64)
        self.count = np.zeros((g.cols, g.rows), np.int64)
        self._parts = []

    def _finish(self):
        g = self.grid
        if self._parts:
            lin = np.concatenate([p[0] for p in self._parts])
            idx = np.concatenate([p[1] for p in self._parts])
            d2 = np.concatenate([p[2] for p in self._parts])
            order = np.argsort(lin, kind="stable")
            lin, self.idx, self.d2 = lin[order], idx[order], d2[order]
        else:
            lin, self.idx, self.d2 = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
        self.ptr = np.searchsorted(lin, np.arange(g.rows * g.cols + 1), side="left")
        assert np.array_equal(np.diff(self.ptr), self.count.reshape(-1))
        del self._parts
        return self

    @property
    def touched(self):
        return self.count > 0


def search(points, g, radius, adaptive):
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    order = np.argsort(pts[:, 0], kind="stable")
    px, py = pts[order, 0], pts[order, 1]
    qx = np.array([O.cell_position(g, i, 0)[0] for i in range(g.rows)])
    qy = np.array([O.cell_position(g, 0, j)[1] for j in range(g.cols)])
    s = Search(g, pts.shape[0])
    big = max(np.abs(qx).max(), np.abs(qy).max(), np.abs(px).max(), np.abs(py).max())
    for level, T in enumerate(thresholds(radius, adaptive)):
        T = float(T)
        # (a kept point has fl(dx * dx) <= d2 < T: |dx| < sqrt(T) (1 + 2^-52); the reach is a superset)
        reach = math.sqrt(T) * 1.001 + big * 1e-12
        left = 0
        for j in range(g.cols):
            rows = np.nonzero(s.count[j] == 0)[0]
            if rows.size == 0:
                continue
            dy = qy[j] - py
            dy2 = dy * dy
            sel = np.nonzero(dy2 < T)[0]            # (d2 >= dy * dy: rounding is monotone)
            if sel.size:
                xs = px[sel]
                lo = np.searchsorted(xs, qx[rows] - reach, side="left")
                hi = np.searchsorted(xs, qx[rows] + reach, side="right")
                cnt = hi - lo
                total = int(cnt.sum())
            else:
                total = 0
            if total:
                cell = np.repeat(np.arange(rows.size), cnt)
                at = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
                pidx = sel[at]
                dx = qx[rows][cell] - px[pidx]
                d2 = dx * dx
                d2 = d2 + dy2[pidx]
                keep = d2 < T
                cell, pidx, d2 = cell[keep], pidx[keep], d2[keep]
                found = np.bincount(cell, minlength=rows.size)
                s.count[j, rows] = found
                s.level[j, rows[found > 0]] = level
                s._parts.append((rows[cell] + j * g.rows, order[pidx], d2))
                left += int((found == 0).sum())
            else:
                left += rows.size
        if left == 0:
            break
    return s._finish()


def delta_of(n_points, values):
    """(4 N + 8) 2^-53 max|z|, exactly (an integer times 2^-53)"""
    zmax = max(abs(int(np.min(values))), abs(int(np.max(values))))
    return Fraction((4 * n_points + 8) * zmax, 2 ** 53)


def exact_cell(d2, z):
    """h = sum(z / d2) / sum(1 / d2) as a Fraction; d2: doubles > 0, z: ints"""
    num = den = Fraction(0)
    for d, v in zip(d2, z):
        w = 1 / Fraction(float(d))
        num += int(v) * w
        den += w
    return num / den


class Expect(object):
    """What a call may leave.  kind: (cols, rows) 0 untouched, 1 interpolated, 2 exact hit.  lo, hi:
    the floats an interpolated cell may hold (equal outside the band).  hits: {(j, i): set of float32
    bit patterns}."""

    def __init__(self, s, values):
        g = s.grid
        z = np.ascontiguousarray(values, np.int64).reshape(-1)
        assert z.shape[0] == s.n_points
        self.search, self.grid = s, g
        self.delta = delta_of(s.n_points, z)
        cells = np.nonzero(np.diff(s.ptr) > 0)[0]
        starts = s.ptr[cells]
        zz = z[s.idx].astype(np.float64)            # (|z| <= 2^31: exact)
        zero = s.d2 == 0.0
        hit = np.add.reduceat(zero.astype(np.int64), starts) > 0 if cells.size else np.zeros(0, bool)
        d2 = np.where(zero, 1.0, s.d2)
        num = np.add.reduceat(zz / d2, starts) if cells.size else np.zeros(0)
        den = np.add.reduceat(1.0 / d2, starts) if cells.size else np.zeros(0)
        ht = num / den
        d3 = 3.0 * float(self.delta)                # (delta is an integer of < 53 bits times 2^-53: exact)
        lo = (ht - d3).astype(np.float32)
        hi = (ht + d3).astype(np.float32)
        self.decided_exactly = 0
        for k in np.nonzero((lo != hi) & ~hit)[0]:
            a, b = s.ptr[cells[k]], s.ptr[cells[k] + 1]
            h = exact_cell(s.d2[a:b], z[s.idx[a:b]])
            lo[k], hi[k] = rn32(h - self.delta), rn32(h + self.delta)
            self.decided_exactly += 1
        assert (lo <= hi).all()
        shape = (g.cols, g.rows)
        self.kind = np.zeros(g.rows * g.cols, np.int8)
        self.kind[cells] = np.where(hit, 2, 1)
        self.lo = np.zeros(g.rows * g.cols, np.float32)
        self.hi = np.zeros(g.rows * g.cols, np.float32)
        self.lo[cells], self.hi[cells] = lo, hi
        self.hits = {}
        for k in np.nonzero(hit)[0]:
            a, b = s.ptr[cells[k]], s.ptr[cells[k] + 1]
            vals = z[s.idx[a:b]][s.d2[a:b] == 0.0]
            # (float)double(int): one rounding, ties to even
            self.hits[divmod(int(cells[k]), g.rows)] = set(
                int(np.float32(np.float64(v)).view(np.uint32)) for v in vals)
        self.kind, self.lo, self.hi = (a.reshape(shape) for a in (self.kind, self.lo, self.hi))
        self.band = (self.kind == 1) & (self.lo.view(np.uint32) != self.hi.view(np.uint32))

    @property
    def interpolated(self):
        return self.kind == 1

    @property
    def band_share(self):
        return float(self.band.sum()) / max(int(self.interpolated.sum()), 1)

    @property
    def several_valued(self):
        """exact-hit cells whose coincident points differ in value: order dependent by design"""
        out = np.zeros(self.kind.shape, bool)
        for at, members in self.hits.items():
            out[at] = len(members) > 1
        return out


def new_layer(g):
    return np.full((g.cols, g.rows), INIT_VALUE, np.float32)


def assert_obeys(got, before, e, what=""):
    """THE rule of comparison (see the head of the file).  Returns the share of band cells."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == e.kind.shape == before.shape, (what, got.shape)
    gb = got.view(np.uint32)
    un = e.kind == 0
    bad = un & (gb != before.view(np.uint32))
    assert not bad.any(), "%s: %d cells without a sample changed, first (j, i) %s: %r" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])])
    it = e.kind == 1
    sure = it & ~e.band
    bad = sure & (gb != e.lo.view(np.uint32))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d interpolated cells hold another float than the exact answer's; "
                             "first (j, i) %s: got %r, exact %r (level %d, %d points)" % (
                                 what, int(bad.sum()), int(it.sum()), at, got[at], e.lo[at],
                                 e.search.level[at], e.search.count[at]))
    # (a comparison of floats: the band is an interval, -0.0 == 0.0 inside one that holds 0)
    bad = e.band & ~((got >= e.lo) & (got <= e.hi))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: band cell %s holds %r outside [%r, %r]" % (what, at, got[at], e.lo[at], e.hi[at]))
    for at, members in e.hits.items():
        assert int(gb[at]) in members, "%s: exact-hit cell %s holds %r, not one of %s" % (
            what, at, got[at], sorted(np.array(sorted(members), np.uint32).view(np.float32).tolist()))
    return e.band_share


def assert_same_decisions(got, want, e, what=""):
    """Two results that both obey the rule agree in bits wherever the rule leaves no choice: outside
    the band and outside exact hits with several different values."""
    free = e.band | e.several_valued
    bad = ~free & (np.asarray(got).view(np.uint32) != np.asarray(want).view(np.uint32))
    assert not bad.any(), "%s: %d cells differ, first (j, i) %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
