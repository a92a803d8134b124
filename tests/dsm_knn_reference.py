"""A plain restatement of the DSM's OPTIONAL capped mode (amhip_ctx_set_dsm_knn), for the tests of
its edges: numpy / Python floats (float64), brute force over cells x points -- no kd-tree, no bins
(search_plain; search() looks only at the points in a square around the cell, for the scenes all
pairs cannot afford, and is held to search_plain by tests/test_dsm_knn_reference.py).

Per cell (oracle/amo_dsm.cc DsmOracle::cell, dsm.cc:119-174):
  * the centre is oracle_ffi.cell_position; d2 = dx*dx; d2 = d2 + dy*dy against every point, unfused,
    the points shifted by the centre offsets the way dsm.cc:36-52 does (x - center_NORTHING,
    y - center_EASTING);
  * the first search takes d2 < R; an empty one climbs the ladder of dsm.cc:133-144 (T = R, 1.1 R,
    1.1^2 R, ... while lambda R <= 7) and stops at the first level that finds something;
  * a stable ascending sort of the result, cut to k, then num += z / d2, den += 1 / d2 in that
    order, num / den rounded to float32.  A kept d2 that is not > 0 is the CHECK of dsm.cc:165.

Besides the value it says what the cell exercised: the size of the search result, the ladder level,
the exact-hit flag, and `ambiguous` -- two kept distances equal, or the k-th equal to the (k+1)-th:
the one case in which the ARRIVAL order of the points (kd-tree, bins, LDS image: all different) shows
in the result.  For such a cell `admissible` holds every value an arrival order can give.

The second half of the file builds the input families of tests/test_gpu_dsm_knn_edges.py; the CPU
tests of tests/test_dsm_knn_reference.py hold the oracle to this restatement on each of them and
assert what each family is there to cover."""
import functools
import itertools
import math

import numpy as np

import oracle_ffi as O

KEEP = 9          # nearest entries a cap needs per cell: every k <= 8 and its (k+1)-th
STORE = 16        # nearest entries stored per cell (whatever ties with the KEEP-th must fit: asserted)
MAX_COMBINATIONS = 70


def ladder(radius_sq):
    """T[0]: the first search; T[1:]: the retries of dsm.cc:133-144 in order (T[1] == T[0])."""
    T = [float(radius_sq)]
    lam = 1.0
    while True:
        T.append(lam * radius_sq)
        lam *= 1.1
        if lam * radius_sq > 7.0:
            break
    return T


class Search(object):
    """What every cell's search found, independent of k.  size, level: (cols, rows) arrays (level
    -1: nothing at any level; cells outside `window`: size -1).  d2, z: the nearest STORE entries
    of every cell of the window in ascending d2, padded with +inf / 0 -- (j1 - j0, i1 - i0, STORE)."""

    def __init__(self, g, window):
        i0, i1, j0, j1 = window
        self.grid, self.window = g, window
        self.size = np.full((g.cols, g.rows), -1, np.int64)
        self.level = np.full((g.cols, g.rows), -1, np.int64)
        self.d2 = np.full((j1 - j0, i1 - i0, STORE), np.inf)
        self.z = np.zeros((j1 - j0, i1 - i0, STORE))

    @property
    def inside(self):
        return self.size >= 0

    def _store(self, j, rows, level, d2, z, hit):
        """rows: cell rows (i) of column j; d2, z: (len(rows), L) candidates; hit: the search's take"""
        i0, _, j0, _ = self.window
        d2 = np.where(hit, d2, np.inf)
        # (equal distances stay in candidate order, which is nobody's arrival order: a cell where
        # that could show is flagged ambiguous by cap() and held to its admissible set instead)
        order = np.argsort(d2, axis=1, kind="stable")[:, :STORE + 1]
        sd, sz = np.take_along_axis(d2, order, 1), np.take_along_axis(z, order, 1)
        if sd.shape[1] > STORE:
            assert not (np.isfinite(sd[:, STORE]) & (sd[:, STORE] == sd[:, KEEP - 1])).any(), \
                "a tie group around the %d-th nearest does not fit the %d stored entries" % (KEEP, STORE)
            sd, sz = sd[:, :STORE], sz[:, :STORE]
        n = sd.shape[1]
        self.size[j, rows] = hit.sum(1)
        self.level[j, rows] = level
        self.d2[j - j0, rows - i0, :n] = sd
        self.z[j - j0, rows - i0, :n] = np.where(np.isfinite(sd), sz, 0.0)


def _setup(points, g, radius_sq, center_easting, center_northing, window):
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    # dsm.cc:36-52: x - center_NORTHING, y - center_EASTING
    px, py, pz = pts[:, 0] - center_northing, pts[:, 1] - center_easting, pts[:, 2].copy()
    i0, i1, j0, j1 = window if window is not None else (0, g.rows, 0, g.cols)
    window = (max(i0, 0), min(i1, g.rows), max(j0, 0), min(j1, g.cols))
    qx = np.array([O.cell_position(g, i, 0)[0] for i in range(g.rows)])
    qy = np.array([O.cell_position(g, 0, j)[1] for j in range(g.cols)])
    return px, py, pz, window, qx, qy, np.array(ladder(radius_sq))


def _take(s, j, rows, T, d2, z, first):
    """first: the first search (T[0]) of these cells -> the rows it left empty; else the ladder"""
    if first:
        hit = d2 < T[0]
        some = hit.any(1)
        if some.any():
            s._store(j, rows[some], 0, d2[some], z[some], hit[some])
        return rows[~some]
    # the first level whose threshold exceeds the nearest d2 is the first search that returns something
    dmin = d2.min(1)
    level = 1 + np.searchsorted(T[1:], dmin, side="right")
    some = level < len(T)
    if some.any():
        level, d2, z = level[some], d2[some], z[some]
        s._store(j, rows[some], level, d2, z, d2 < T[level][:, None])
    return rows[~some]


def search_plain(points, g, radius_sq=1, center_easting=0.0, center_northing=0.0, window=None):
    """THE restatement: every cell against every point.  window: (i0, i1, j0, j1), half-open cell
    ranges to restate (default: the whole map)."""
    px, py, pz, window, qx, qy, T = _setup(points, g, radius_sq, center_easting, center_northing, window)
    i0, i1, j0, j1 = window
    s = Search(g, window)
    rows = np.arange(i0, i1)
    z = np.broadcast_to(pz, (rows.size, pz.size))
    for j in range(j0, j1):
        s.size[j, rows] = 0
        dx = qx[rows][:, None] - px[None, :]
        dy = qy[j] - py
        d2 = dx * dx
        d2 = d2 + (dy * dy)[None, :]
        empty = _take(s, j, rows, T, d2, z, True)
        if empty.size:
            _take(s, j, empty, T, d2[empty - i0], z[empty - i0], False)
    return s


def _box(qx, qy, px_sorted, py_sorted, pz_sorted, reach):
    """Candidates of the cells (qx[r], qy): the points inside the square of half-width `reach`
    around each, as (len(qx), L) arrays d2 (+inf beyond a cell's own candidates) and z; None:
    no candidate at all.  The points come sorted by x."""
    lo = np.searchsorted(px_sorted, qx - reach, side="left")
    hi = np.searchsorted(px_sorted, qx + reach, side="right")
    L = int((hi - lo).max()) if lo.size else 0
    if L == 0:
        return None
    idx = lo[:, None] + np.arange(L)[None, :]
    valid = idx < hi[:, None]
    idx = np.minimum(idx, px_sorted.size - 1)
    dx = qx[:, None] - px_sorted[idx]
    dy = qy - py_sorted[idx]
    d2 = dx * dx
    d2 = d2 + dy * dy
    d2[~valid | (np.abs(dy) >= reach)] = np.inf
    return d2, pz_sorted[idx]


def search(points, g, radius_sq=1, center_easting=0.0, center_northing=0.0, window=None):
    """search_plain's result (tests/test_dsm_knn_reference.py holds it to that) at a cost the
    larger scenes can afford: the same arithmetic and the same decisions per (cell, point), but
    only for the points inside a square around the cell that is wider than the search's disc
    (first radius; the last one for the cells the first search left empty) -- nothing a search
    could take lies outside it."""
    px, py, pz, window, qx, qy, T = _setup(points, g, radius_sq, center_easting, center_northing, window)
    i0, i1, j0, j1 = window
    s = Search(g, window)
    rows = np.arange(i0, i1)
    order = np.argsort(px, kind="stable")
    px, py, pz = px[order], py[order], pz[order]
    reach = [math.sqrt(t) * 1.000001 + 1e-6 for t in (T[0], T[-1])]
    for j in range(j0, j1):
        s.size[j, rows] = 0
        empty = rows
        for first in (True, False):
            if not empty.size:
                break
            band = np.abs(qy[j] - py) < reach[0 if first else 1]
            c = _box(qx[empty], qy[j], px[band], py[band], pz[band], reach[0 if first else 1])
            if c is None:
                continue
            empty =_take(s, j, empty, T, c[0], c[1], first)
    return s


def _idw(d2s, zs):
    num = den = 0.0
    for d2, z in zip(d2s, zs):
        num += z / d2
        den += 1.0 / d2
    return np.float32(num / den)


def _arrangements(d2s, zs, k):
    """Every (order of) kept heights an arrival order can leave: groups of equal d2 in any order,
    the group at the k-th place filled in every way.  -> (kind, number of combinations, list of z
    tuples) with kind: set of 'inside' (a tied group wholly kept), 'one_open' (a tied group at
    the k-th place, one slot open), 'more_than_slots' (... two or more slots open, fewer than
    the group has)."""
    kinds, combos, per_group = set(), 1, []
    left = k
    for d2, grp in itertools.groupby(zip(d2s, zs), key=lambda e: e[0]):
        zg = [e[1] for e in grp]
        if left == 0:
            break
        if len(zg) <= left:
            if len(zg) > 1:
                kinds.add("inside")
            per_group.append(list(itertools.permutations(zg)))
            left -= len(zg)
        else:
            kinds.add("one_open" if left == 1 else "more_than_slots")
            combos *= math.comb(len(zg), left)
            per_group.append(list(itertools.permutations(zg, left)))
            left = 0
    return kinds, combos, [sum(c, ()) for c in itertools.product(*per_group)]


class Capped(object):
    """The capped result of one Search: value (float32, (cols, rows); untouched cells keep
    `elevation`, NaN by default), exact, ambiguous as arrays; admissible: {(j, i): set of float32};
    kinds: {(j, i): set of tie kinds}; size / level / inside: the Search's."""


def cap(s, k, elevation=None):
    assert 1 <= k < KEEP
    g = s.grid
    i0, i1, j0, j1 = s.window
    r = Capped()
    r.k, r.size, r.level, r.inside = k, s.size, s.level, s.inside
    r.value = (np.full((g.cols, g.rows), np.nan, np.float32) if elevation is None
               else np.array(elevation, np.float32, copy=True))
    r.exact = np.zeros((g.cols, g.rows), bool)
    r.ambiguous = np.zeros((g.cols, g.rows), bool)
    r.admissible, r.kinds = {}, {}
    n = np.maximum(s.size[j0:j1, i0:i1], 0)
    kept = np.arange(k)[None, None, :] < np.minimum(n, k)[:, :, None]
    d, z = s.d2[:, :, :k], s.z[:, :, :k]
    exact = (kept & ~(d > 0.0)).any(2)          # the CHECK of dsm.cc:165: the cell is left as it was
    tie = (kept[:, :, 1:] & (d[:, :, 1:] == d[:, :, :-1])).any(2) | ((n > k) & (s.d2[:, :, k - 1] == s.d2[:, :, k]))
    tie &= ~exact
    # the oracle's arithmetic: true divisions, ascending distance, one term after the other
    num, den = np.zeros(n.shape), np.zeros(n.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for q in range(k):
            num = np.where(kept[:, :, q], num + z[:, :, q] / d[:, :, q], num)
            den = np.where(kept[:, :, q], den + 1.0 / d[:, :, q], den)
        value = (num / den).astype(np.float32)
    write = (n > 0) & ~exact
    r.value[j0:j1, i0:i1][write] = value[write]
    r.exact[j0:j1, i0:i1] = exact
    r.ambiguous[j0:j1, i0:i1] = tie
    for jj, ii in np.argwhere(tie):
        fin = np.isfinite(s.d2[jj, ii])
        d2s, zs = s.d2[jj, ii][fin].tolist(), s.z[jj, ii][fin].tolist()
        kinds, combos, arr = _arrangements(d2s, zs, k)
        assert combos <= MAX_COMBINATIONS, (jj, ii, combos)
        key = (int(jj) + j0, int(ii) + i0)
        r.kinds[key] = kinds
        # (d2 of slot q is the same in every arrangement: only the heights move)
        r.admissible[key] = set(_idw(d2s[:len(a)], a) for a in arr)
        assert r.value[key] in r.admissible[key]
    return r


def spacing(v):
    """spacing of the float32 grid at |v|"""
    return float(np.spacing(np.abs(np.float32(v))))


def assert_capped_equal(got, want, r, what="", exact_membership=False):
    """The rule of comparison of the capped mode's tests.  got: the layer under test; want: the
    oracle's; r: the restatement (Capped) of the same call.
      * the NaN pattern equals the oracle's;
      * every cell that is not ambiguous equals the oracle's float bit for bit -- all of them;
      * every ambiguous cell lies within one float32 spacing of an admissible value (reordering
        equal-d2 terms moves the double sums by ulps of double: that is the whole allowance);
        exact_membership (CPU: oracle against restatement): it IS an admissible value."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN pattern differs in %d cells" % (what, int((gn != wn).sum()))
    plain = ~r.ambiguous
    diff = plain & (got.view(np.uint32) != want.view(np.uint32))
    assert not diff.any(), "%s: %d non-ambiguous cells differ in bits, first (j, i) = %s: %r != %r" % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[diff][0], want[diff][0])
    for (j, i), adm in r.admissible.items():
        v = got[j, i]
        if exact_membership:
            assert v in adm, "%s: cell (%d, %d) = %r not in %r" % (what, j, i, v, sorted(adm))
        else:
            assert any(abs(float(v) - float(a)) <= spacing(a) for a in adm), \
                "%s: cell (%d, %d) = %r not within one spacing of %r" % (what, j, i, v, sorted(adm))


# ---------------------------------------------------------------------------------------------
# The input families (tests/test_gpu_dsm_knn_edges.py, section letters as in its docstring)
# ---------------------------------------------------------------------------------------------
class Family(object):
    def __init__(self, name, grid, points, radius_sq=1, center_easting=0.0, center_northing=0.0, window=None):
        self.name, self.grid, self.points = name, grid, np.ascontiguousarray(points, np.float64)
        self.radius_sq, self.center_easting, self.center_northing = radius_sq, center_easting, center_northing
        self.window = window
        self._search, self._oracle = None, {}

    def search(self):
        if self._search is None:
            self._search = search(self.points, self.grid, self.radius_sq, self.center_easting,
                                  self.center_northing, self.window)
        return self._search

    def cap(self, k, elevation=None):
        return cap(self.search(), k, elevation)

    def oracle(self, k, which=None, elevation=None):
        """(rc, layer) of the oracle's capped mode; cached (and never modified) for elevation=None"""
        which = which or ("ref" if O.have_ref() else "port")
        if elevation is not None:
            return O.dsm_process_knn(self.points, self.grid, k, self.radius_sq, self.center_easting,
                                     self.center_northing, elevation=np.array(elevation, np.float32, copy=True),
                                     which=which)
        if (k, which) not in self._oracle:
            rc, e = O.dsm_process_knn(self.points, self.grid, k, self.radius_sq, self.center_easting,
                                      self.center_northing, which=which)
            e.setflags(write=False)
            self._oracle[(k, which)] = (rc, e)
        return self._oracle[(k, which)]


def _heights(rng, x, y, noise=0.3):
    return 420.0 + 3.0 * np.sin(0.11 * x) + 2.0 * np.cos(0.07 * y) + rng.uniform(-noise, noise, x.shape[0])


@functools.lru_cache(maxsize=None)
def family_a():
    """Every k, every set size: 100 x 40 cells at 0.5 m (one and a half gather tiles long, two
    and a half high at tile_j = 16), a density ramp along x, a hole, a far strip left empty."""
    g = O.make_grid(50.0, 20.0, 0.5)
    rng = np.random.default_rng(9101)
    n = 2600
    x = -26.0 + 40.0 * rng.uniform(0.0, 1.0, n) ** 2.2          # dense at x = -26, thin towards +14
    y = rng.uniform(-11.0, 11.0, n)
    keep = ~((np.abs(x + 12.0) < 2.5) & (np.abs(y - 2.0) < 3.0))   # the hole (ladder inside it)
    x, y = x[keep], y[keep]                                        # x > 14: the empty strip
    return Family("a", g, np.c_[x, y, _heights(rng, x, y)])


TIE_KINDS = ("inside", "one_open", "more_than_slots")


@functools.lru_cache(maxsize=None)
def family_b():
    """Ties.  Resolution 0.5 at origin (0, 0): dyadic cell centres.  Around 40 centres: `a` points
    at distinct distances (a = 0 .. 6), then a group at one exact d2 -- a pair, a quadruple or two
    points at the same (x, y) --, offsets in multiples of 1/64 m, heights metres apart; so that for
    k = a + 1 the tie is at the k-th place with one slot open, for a quadruple and k = a + 2, a + 3
    with more tied points than slots, and for larger k inside the set.  Plus a thin background."""
    g = O.make_grid(40.0, 30.0, 0.5)
    rng = np.random.default_rng(9102)
    pts = []
    z = [100.0]

    def put(cx, cy, ox, oy):
        pts.append((cx + ox / 64.0, cy + oy / 64.0, z[0]))
        z[0] += 3.0

    groups = {"pair": [(24, 16), (-24, -16)],
              "pair_swapped": [(24, 16), (16, 24)],
              "quad": [(24, 16), (-16, 24), (-24, -16), (16, -24)],
              "same_xy": [(20, 12), (20, 12)],
              "triple_same_xy": [(-20, 12), (-20, 12), (-20, 12)]}
    names = sorted(groups)
    centres = [(4 + 9 * (c % 8), 5 + 10 * (c // 8)) for c in range(40)]      # cells (i, j), >= 4.5 m apart
    for c, (i, j) in enumerate(centres):
        cx, cy = O.cell_position(g, i, j)
        a = c % 7
        for m in range(a):                                   # d2 = ((3 + 2m)^2 + (1 + m)^2) / 4096, ascending
            sx, sy = (1, 1) if m % 2 == 0 else (-1, 1)
            put(cx, cy, sx * (3 + 2 * m), sy * (1 + m))
        for ox, oy in groups[names[(c // 7 + c) % len(names)]]:
            put(cx, cy, ox, oy)
        if c % 3 == 0:                                       # something beyond the group, still inside the radius
            put(cx, cy, 40, -36)
    n = 260
    x, y = rng.uniform(-21.0, 21.0, n), rng.uniform(-16.0, 16.0, n)
    pts = np.r_[np.array(pts), np.c_[x, y, 400.0 + rng.uniform(-5.0, 5.0, n)]]
    return Family("b", g, pts[rng.permutation(pts.shape[0])])


@functools.lru_cache(maxsize=None)
def family_c(radius_sq):
    """The ladder under a cap: one blob in a corner of a 96 x 48-cell map at 0.5 m."""
    g = O.make_grid(48.0, 24.0, 0.5)
    rng = np.random.default_rng(9103)
    n = 700         # (dense: a ladder step widens the disc by 5 %, and that ring has to hold more than k points)
    x = 21.0 + rng.uniform(-1.2, 1.2, n)
    y = 9.5 + rng.uniform(-1.0, 1.0, n)
    return Family("c%d" % radius_sq, g, np.c_[x, y, 430.0 + rng.uniform(-4.0, 4.0, n)], radius_sq=radius_sq)


WINDOW_SHAPES = [(1, 1.0), (2, 0.3), (3, 0.25), (9, 0.25)]     # (radius^2, resolution): w0 = 1 .. 12


@functools.lru_cache(maxsize=None)
def family_d(radius_sq, res, offsets):
    """Window shapes: 40 x 30 m at UTM magnitudes, a non-dyadic resolution among them; offsets:
    non-zero center_easting / center_northing (dsm.cc:36-52 swaps them)."""
    cx, cy = 464980.3, 5272690.7
    g = O.make_grid(40.0, 30.0, res, cx, cy)
    rng = np.random.default_rng(9104 + radius_sq)
    n = 2400
    x, y = cx + rng.uniform(-23.0, 23.0, n), cy + rng.uniform(-18.0, 18.0, n)
    keep = ~((np.abs(x - cx - 6.0) < 4.5) & (np.abs(y - cy + 3.0) < 4.0))     # a hole wider than any first radius
    x, y = x[keep], y[keep]
    zz = _heights(rng, x - cx, y - cy, 1.0)
    ce, cn = (1250.25, -830.5) if offsets else (0.0, 0.0)
    return Family("d%d/%g/%d" % (radius_sq, res, offsets), g, np.c_[x + cn, y + ce, zz], radius_sq=radius_sq,
                  center_easting=ce, center_northing=cn)


@functools.lru_cache(maxsize=None)
def family_e():
    """Wider than the LDS gather handles: radius^2 1 at 0.05 m, w0 = 20."""
    g = O.make_grid(5.0, 3.0, 0.05)
    rng = np.random.default_rng(9105)
    n = 600
    x, y = rng.uniform(-3.5, 3.5, n), rng.uniform(-2.5, 2.5, n)
    return Family("e", g, np.c_[x, y, _heights(rng, x, y)])


F_TILE = (64, 32)            # the gather tile make_dsm_params picks at this density (asserted on the GPU)
F_PATCH_CELL = (96, 48)      # (i, j): the centre of gather tile (1, 1)


@functools.lru_cache(maxsize=None)
def family_f():
    """A tile beyond the image: 256 x 64 cells at 0.5 m, ~0.5 points per cell, and 2500 points inside
    a 4 m x 4 m patch in the interior of one 64 x 32-cell tile (12 cells from its nearest edge)."""
    g = O.make_grid(128.0, 32.0, 0.5)
    rng = np.random.default_rng(9106)
    n = 9500
    x, y = rng.uniform(-66.0, 66.0, n), rng.uniform(-18.0, 18.0, n)
    cx, cy = O.cell_position(g, *F_PATCH_CELL)
    bx, by = cx + rng.uniform(-2.0, 2.0, 2500), cy + rng.uniform(-2.0, 2.0, 2500)
    x, y = np.r_[x, bx], np.r_[y, by]
    pts = np.c_[x, y, _heights(rng, x, y)]
    return Family("f", g, pts[rng.permutation(pts.shape[0])])


@functools.lru_cache(maxsize=None)
def family_g(with_hit):
    """Exact hit: one point on a cell centre (with_hit), and the same cloud without it."""
    g = O.make_grid(40.0, 30.0, 1.0)
    rng = np.random.default_rng(9107)
    n = 3000
    x, y = rng.uniform(-24.0, 24.0, n), rng.uniform(-19.0, 19.0, n)
    pts = np.c_[x, y, _heights(rng, x, y)]
    if with_hit:
        hx, hy = O.cell_position(g, 7, 11)
        pts = np.r_[pts[:1500], [[hx, hy, 400.0]], pts[1500:]]
    return Family("g%d" % with_hit, g, pts)


H_GRID = (60.0, 40.0, 0.5)


@functools.lru_cache(maxsize=None)
def family_h(call):
    """Earlier content and mode switches: call 0 .. 4 of five partly overlapping clouds on a
    120 x 80-cell map (call 2: rough heights, +-30 m)."""
    g = O.make_grid(*H_GRID)
    rng = np.random.default_rng(9110 + call)
    x0, x1, y0, y1 = [(-32.0, 2.0, -22.0, 6.0), (-12.0, 20.0, -10.0, 22.0), (-5.0, 32.0, -22.0, 4.0),
                      (-32.0, -4.0, -4.0, 22.0), (-18.0, 14.0, -14.0, 12.0)][call]
    n = int(2.2 * (x1 - x0) * (y1 - y0))
    x, y = rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)
    zz = _heights(rng, x, y) + 2.0 * call
    if call == 2:
        zz = zz + rng.uniform(-30.0, 30.0, n)
    return Family("h%d" % call, g, np.c_[x, y, zz])


def h_base():
    return np.random.default_rng(9109).uniform(300.0, 310.0, (80, 120)).astype(np.float32)


J_MAP = (2304, 2048, 0.5, 100.0, -50.0)      # rows, cols, resolution, position


@functools.lru_cache(maxsize=None)
def family_j():
    """Sub-window: one 60 000-point cloud across a corner of a 2304 x 2048-cell map; restated on
    the cloud's bounding box plus sqrt(7) m only."""
    rows, cols, res, px, py = J_MAP
    lx, ly = rows * res, cols * res
    g = O.make_grid(lx, ly, res, px, py)
    rng = np.random.default_rng(9111)
    cx, cy = px + lx / 2 - 10.0, py - ly / 2 + 12.0
    n = 60000
    x, y = rng.uniform(cx - 40.0, cx + 40.0, n), rng.uniform(cy - 25.0, cy + 25.0, n)
    reach = math.sqrt(7.0) + res
    # cell index of a position: x = base_x - res * i
    bx, by = O.cell_position(g, 0, 0)
    i0, i1 = int(math.floor((bx - (x.max() + reach)) / res)), int(math.ceil((bx - (x.min() - reach)) / res)) + 1
    j0, j1 = int(math.floor((by - (y.max() + reach)) / res)), int(math.ceil((by - (y.min() - reach)) / res)) + 1
    return Family("j", g, np.c_[x, y, 400.0 + rng.uniform(-1.0, 1.0, n)], window=(i0, i1, j0, j1))
