"""The input families of tests/test_gpu_ortho_from_pcl_edges.py (values mode of the DSM machinery at its
edges), shared with tests/test_ortho_from_pcl_reference.py, which holds the exact reference
(ortho_from_pcl_reference.py) to the compiled oracle on each of them and asserts what each family is
there to cover.  Seeded, small, built once per process (functools.lru_cache): a Scene is a cloud's
geometry with its search (which points every cell keeps), a Case a scene with values -- the value
families of one scene share its search.

Sizes follow what the planner distinguishes (amhip_dsm_plan.h): a gather tile is 64 cells along i and
16 or 32 along j, so 130 x 70 cells hold interior, edge and partial tiles; the capacity classes are cut
at 2048 / ~2752 / ~5600 points per tile region; the LDS gather ends at a first window of 16 cells."""
import functools

import numpy as np

import oracle_ffi as O
import ortho_from_pcl_reference as R

UTM = (465120.0, 5247300.0)         # magnitudes of UTM 32T coordinates (doubles: 2^-34 / 2^-30 m apart)


class Scene(object):
    def __init__(self, name, grid, points, radius, adaptive=False, marks=None, oracle=True):
        self.name, self.grid, self.radius, self.adaptive = name, grid, int(radius), bool(adaptive)
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self.marks = marks or {}    # what the scene planted, for the tests that assert its coverage
        self.oracle_defined = oracle
        self._search = None

    @property
    def n(self):
        return self.points.shape[0]

    def search(self):
        if self._search is None:
            self._search = R.search(self.points, self.grid, self.radius, self.adaptive)
        return self._search

    def fills_before_overflow(self):
        """adaptive: every cell found something at a threshold an int holds (else the reference's loop
        is undefined: such a scene must never reach the oracle)"""
        return bool((self.search().level >= 0).all())


class Case(object):
    def __init__(self, scene, values, name=None):
        self.scene = scene
        self.values = np.ascontiguousarray(values, np.int32).reshape(-1)
        assert self.values.shape[0] == scene.n
        self.name = name or scene.name
        self._expect = None

    grid = property(lambda self: self.scene.grid)
    points = property(lambda self: self.scene.points)
    radius = property(lambda self: self.scene.radius)
    adaptive = property(lambda self: self.scene.adaptive)

    def expect(self):
        if self._expect is None:
            self._expect = R.Expect(self.scene.search(), self.values)
        return self._expect

    def oracle(self, which="port", before=None):
        assert self.scene.oracle_defined and (not self.adaptive or self.scene.fills_before_overflow())
        layer = R.new_layer(self.grid) if before is None else before.copy()
        rc, out = O.ortho_from_pcl(self.points, self.values, self.grid, self.radius, self.adaptive,
                                   ortho=layer, which=which)
        assert rc == O.OK
        return out


def _cloud(xy):
    pts = np.zeros((xy.shape[0], 3))
    pts[:, :2] = xy
    pts[:, 2] = 100.0 + 0.01 * np.arange(xy.shape[0])      # (heights: not read in values mode)
    return pts


def _extent(g, margin):
    """(x0, x1, y0, y1) of the map grown by `margin` metres"""
    return (g.pos_x - g.length_x / 2 - margin, g.pos_x + g.length_x / 2 + margin,
            g.pos_y - g.length_y / 2 - margin, g.pos_y + g.length_y / 2 + margin)


def _uniform(rng, g, n, margin):
    x0, x1, y0, y1 = _extent(g, margin)
    return np.c_[rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)]


def _centre(g, i, j):
    return np.array(O.cell_position(g, i, j))


# ---- the value families (a) ---------------------------------------------------------------------
VALUE_KINDS = ("u8", "negative", "mixed", "int32_ends", "above_2p24", "constant")
ENDS = (2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31)


def draw_values(kind, points, seed):
    """int32 values for the rows of `points`"""
    n = points.shape[0]
    rng = np.random.default_rng(seed)
    if kind == "u8":
        v = rng.integers(0, 256, n)
    elif kind == "negative":
        v = rng.integers(-70000, 0, n)
    elif kind == "mixed":                       # |h| << max|z| in most cells
        v = rng.integers(-1000, 1001, n)
    elif kind == "int32_ends":
        # within 5000 of either end of the range, the sign in a chequerboard of 6 x 5 fields over the cloud
        # (so that cells of one sign, and cells that mix the two, both exist), the three ends themselves planted
        u = (points[:, :2] - points[:, :2].min(0)) / np.ptp(points[:, :2], axis=0)
        side = (np.floor(5.5 * u[:, 0]) + np.floor(4.5 * u[:, 1])) % 2 == 0
        off = rng.integers(0, 5001, n)
        v = np.where(side, (2 ** 31 - 1) - off, -2 ** 31 + off)
        v[rng.permutation(n)[:3 * (n // 40 + 1)].reshape(3, -1)] = np.array(ENDS)[:, None]
    elif kind == "above_2p24":
        # 2^25 + 4 k + {1, 3}: no float32 holds one (floats are 4 apart there), and none is a tie between
        # two floats.  (An odd integer below 2^25 is such a tie: a cell with ONE sample then lies exactly
        # on a rounding boundary, where the rule admits both floats -- a tenth of these scenes' cells.)
        v = 2 ** 25 + 4 * rng.integers(0, 2000, n) + rng.choice([1, 3], n)
    elif kind == "constant":                    # (a float32: the cell's answer is exactly it)
        v = np.full(n, 12345677)
    else:
        raise KeyError(kind)
    return v.astype(np.int32)


# ---- the scenes of a: one per gather path -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_lds():
    """the LDS-tiled gather, every tile class 0: 3 x 5 tiles of 64 x 16 (interior, edge, partial)"""
    g = O.make_grid(130.0, 70.0, 1.0, 4.0, -3.0)
    rng = np.random.default_rng(9101)
    return Scene("lds", g, _cloud(_uniform(rng, g, 6000, 3.0)), 2)


CLASS_BANDS = ((0, 18, 2.02), (30, 50, 3.5), (62, 80, 7.0))     # (j0, j1, points per cell)


@functools.lru_cache(maxsize=None)
def scene_classes():
    """Bands of graded density across a 130 x 80 map: tile rows 0, 2 and 4 (tiles of 64 x 16; a tile's
    region is 66 x 18 cells at this radius) hold ~2400, ~4150 and ~8300 points -- the capacity classes
    1 and 2 and the wave-per-cell kernel beyond the largest LDS image; the rest stays in class 0."""
    g = O.make_grid(130.0, 80.0, 1.0, 4.0, -3.0)
    rng = np.random.default_rng(9102)
    parts = [_uniform(rng, g, 1600, 3.0)]
    x0, x1, y0, y1 = _extent(g, 3.0)
    top = g.pos_y + g.length_y / 2                    # (y of the upper edge of cell row j = 0)
    for j0, j1, rho in CLASS_BANDS:
        n = int(rho * 136 * (j1 - j0))
        parts.append(np.c_[rng.uniform(x0, x1, n), rng.uniform(top - j1, top - j0, n)])
    return Scene("classes", g, _cloud(np.concatenate(parts)), 2)


@functools.lru_cache(maxsize=None)
def scene_global():
    """a first window of 20 cells (radius 4 on a 0.1 m grid): beyond the LDS gather, k_dsm_gather"""
    g = O.make_grid(13.0, 7.0, 0.1, 4.0, -3.0)
    rng = np.random.default_rng(9103)
    return Scene("global", g, _cloud(_uniform(rng, g, 1500, 2.0)), 4)


PATH_SCENES = {"lds": scene_lds, "classes": scene_classes, "global": scene_global}

SPARSE_TILES = ((3934 + 63) // 64) * (2128 // 16)


@functools.lru_cache(maxsize=None)
def case_sparse():
    """A small cloud on a materialized map of more than 8192 tiles (3934 x 2128 cells: the smallest
    such map is 8.4 M cells): the gather visits the occupied tiles only, from a list the pre-pass
    writes.  A patch of ~2400 points over the region of tile (10, 20) puts one tile on the class-1 list.
    3934 + 2 bin columns in one column block: the widest the three-pass sort takes on doubles
    (amhip_sort.hip: dsm_sort) -- beyond the run pipeline's 2048, so it is the counting one."""
    g = O.make_grid(3934.0, 2128.0, 1.0, UTM[0], UTM[1])
    rng = np.random.default_rng(9104)
    xy = np.c_[rng.uniform(g.pos_x - 300.0, g.pos_x + 200.0, 4000), rng.uniform(g.pos_y - 100.0, g.pos_y + 150.0, 4000)]
    top_x, top_y = g.pos_x + g.length_x / 2, g.pos_y + g.length_y / 2
    n = int(2.02 * 68 * 20)
    patch = np.c_[rng.uniform(top_x - 706.0, top_x - 638.0, n), rng.uniform(top_y - 338.0, top_y - 318.0, n)]
    sc = Scene("sparse", g, _cloud(np.concatenate([xy, patch])), 2, marks={"patch_region": (639, 705, 319, 337)})
    return Case(sc, draw_values("mixed", sc.points, 9105))


@functools.lru_cache(maxsize=None)
def case_values(path, kind):
    sc = PATH_SCENES[path]()
    return Case(sc, draw_values(kind, sc.points, 9200 + VALUE_KINDS.index(kind)), "%s/%s" % (path, kind))


@functools.lru_cache(maxsize=None)
def case_wide_strip():
    """4094 x 16 cells: 4096 bin columns, one column block -- wider than the three-pass sort's big placement
    holds next to its points (3936 on doubles).  Such a call keeps the one-level sort however many points
    it has; it used to fail in hipFuncSetAttribute."""
    g = O.make_grid(4094.0, 16.0, 1.0, UTM[0], UTM[1])
    rng = np.random.default_rng(9106)
    sc = Scene("wide strip", g, _cloud(_uniform(rng, g, 3000, 2.0)), 2)
    return Case(sc, draw_values("int32_ends", sc.points, 9107))


# ---- b: the strict radius -----------------------------------------------------------------------
STRICT_RADII = (1, 2, 4, 5, 8, 9, 10)


def lattice_offsets(T):
    """every (a, b) of integers with a^2 + b^2 == T"""
    r = int(np.sqrt(T)) + 1
    return [(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1) if a * a + b * b == T]


def _inward(centre, p):
    """p moved one double spacing toward the centre, in the first coordinate that differs"""
    p = p.copy()
    k = 0 if p[0] != centre[0] else 1
    p[k] = np.nextafter(p[k], centre[k])
    return p


def _strict_grid():
    # 1 m cells whose centres are integers + 0.5: exact in binary, like every lattice point around them
    return O.make_grid(130.0, 70.0, 1.0, 1000.0, -2000.0)


@functools.lru_cache(maxsize=None)
def case_strict(radius, inside):
    """First search.  A background of 8-bit values and, around target cells spread over the tiles, one
    probe per lattice offset at d2 == radius exactly (inside: one double spacing nearer), valued 3000 and
    up: a probe counted wrongly moves its cell by thousands of float spacings.  (Not farther: delta
    grows with max|z| while the cells stay near 128 -- at 10^6 a third of them would lie in the band.)"""
    g = _strict_grid()
    rng = np.random.default_rng(9300 + radius)
    xy = [_uniform(rng, g, 3000, 3.0)]
    vals = [rng.integers(0, 256, 3000)]
    offs = lattice_offsets(radius)
    targets = []
    for k, (a, b) in enumerate(offs):
        i, j = 7 + (k * 37) % 117, 5 + (k * 23) % 60
        c = _centre(g, i, j)
        p = c + np.array([a, b], np.float64)
        assert ((p - c)[0] ** 2 + (p - c)[1] ** 2) == radius
        xy.append((_inward(c, p) if inside else p)[None, :])
        vals.append([3000 + 10 * k])
        targets.append((j, i))
    sc = Scene("strict r=%d %s" % (radius, "inside" if inside else "at"), g, _cloud(np.concatenate(xy)),
               radius, marks={"targets": targets})
    return Case(sc, np.concatenate(vals))


@functools.lru_cache(maxsize=None)
def case_strict_adaptive(radius, k, which, inside):
    """Retry k (T = 10^k radius): the cloud is one probe at d2 == T exactly from the centre of cell
    (65, 35) and a companion of another value at d2 ~ 3.5 T.  At: the probe misses retry k and the cell
    takes both at retry k + 1.  Inside: the probe alone at retry k."""
    g = _strict_grid()
    T = 10 ** k * radius
    offs = [o for o in lattice_offsets(T) if o[0] >= abs(o[1])]
    a, b = offs[which % len(offs)]
    c = _centre(g, 65, 35)
    p = c + np.array([a, b], np.float64)
    assert ((p - c)[0] ** 2 + (p - c)[1] ** 2) == T
    q = c + np.array([-0.37, 1.0]) * np.sqrt(3.1 * T)
    xy = np.stack([_inward(c, p) if inside else p, q])
    sc = Scene("strict r=%d T=%d (%d,%d) %s" % (radius, T, a, b, "inside" if inside else "at"), g, _cloud(xy),
               radius, adaptive=True, marks={"targets": [(35, 65)], "retry": k})
    return Case(sc, [1000000, -77])


# ---- c: exact hits ------------------------------------------------------------------------------
HIT_KINDS = ("single", "equal", "different")
HIT_CELLS = {   # (i, j): edge, interior and partial tiles; for `classes` one per band and the background
    "lds": ((5, 3), (70, 20), (64, 16), (129, 69)),
    "classes": ((10, 8), (100, 40), (129, 70), (40, 24), (64, 79)),
    "global": ((5, 3), (70, 20), (129, 69)),
}


@functools.lru_cache(maxsize=None)
def case_hits(path, kind):
    """`single`: one point on the cell centre, two more within 2 % of a cell of it (and the scene's own
    cloud around them).  `equal` / `different`: three points on the centre."""
    base = PATH_SCENES[path]()
    g = base.grid
    rng = np.random.default_rng(9400 + HIT_KINDS.index(kind))
    vals = draw_values("above_2p24" if path == "lds" else "int32_ends" if path == "classes" else "mixed",
                       base.points, 9410)
    xy, extra, cells = [base.points[:, :2]], [], []
    for n, (i, j) in enumerate(HIT_CELLS[path]):
        c = _centre(g, i, j)
        if kind == "single":
            near = c + g.resolution * rng.uniform(-0.02, 0.02, (2, 2))
            assert (near != c).any(1).all()
            xy.append(np.vstack([c, near]))
        else:
            xy.append(np.vstack([c, c, c]))
        v = int(vals[17 * n + 5])
        toward0 = 1 if v > 0 else -1            # (the other values: nearer zero, inside the int32 range)
        extra += [v, v, v] if kind == "equal" else [v, v - toward0 * (4001 + 2 * n), v - toward0 * 9001]
        cells.append((j, i))
    sc = Scene("hits %s %s" % (path, kind), g, _cloud(np.concatenate(xy)), base.radius, marks={"hit_cells": cells})
    return Case(sc, np.concatenate([vals, np.array(extra, np.int32)]))


# ---- d: the adaptive ladder ---------------------------------------------------------------------
LADDER_RADII = (1, 2)
LADDER_PLACES = ("corner", "b6", "b7", "b8", "b9", "far")


@functools.lru_cache(maxsize=None)
def case_ladder(radius, place):
    """A cluster of five points, 66 x 40 cells with a UTM origin.  corner: inside the map -- the cells
    stop at lambda = 1 .. 10^5 by their distance.  bK: at sqrt(10^(K-1) radius) metres from the map's
    centre -- the circle on which retry K - 1 ends passes through the map.  far: 25 km (radius 1) /
    39 km (radius 2) away: every cell stops at the last threshold an int holds."""
    g = O.make_grid(66.0, 40.0, 1.0, UTM[0], UTM[1])
    rng = np.random.default_rng(9500 + 10 * radius + LADDER_PLACES.index(place))
    if place == "corner":
        at = np.array([g.pos_x + 29.3, g.pos_y - 17.1])
    else:
        dist = {1: 25000.0, 2: 39000.0}[radius] if place == "far" else np.sqrt(10.0 ** (int(place[1]) - 1) * radius)
        phi = 0.3 + 0.9 * LADDER_PLACES.index(place)
        at = np.array([g.pos_x, g.pos_y]) + dist * np.array([np.cos(phi), np.sin(phi)])
    xy = at + rng.uniform(-4.0, 4.0, (5, 2)) * (0.05 if place != "corner" else 1.0)
    sc = Scene("ladder r=%d %s" % (radius, place), g, _cloud(xy), radius, adaptive=True)
    return Case(sc, np.array([40, 90, 140, 190, 240]) * (1 if radius == 1 else -1000003))


DEGENERATE = ((1, 1), (1, 90), (90, 1), (1, 3), (2, 1))


@functools.lru_cache(maxsize=None)
def case_degenerate(rows, cols, adaptive):
    """1 x 1, 1 x N, N x 1 grids: a few points around one end, the rest of the strip reached by retries"""
    g = O.make_grid(float(rows), float(cols), 1.0, UTM[0], UTM[1])
    assert (g.rows, g.cols) == (rows, cols)
    rng = np.random.default_rng(9600 + rows + 7 * cols)
    c = _centre(g, 0, 0)
    xy = c + rng.uniform(-2.5, 2.5, (12, 2))
    sc = Scene("grid %dx%d%s" % (rows, cols, " adaptive" if adaptive else ""), g, _cloud(xy), 2, adaptive=adaptive)
    return Case(sc, rng.integers(-500, 500, 12))


@functools.lru_cache(maxsize=None)
def case_first_pass_fills(adaptive):
    """dense enough for the first search to fill every cell: the adaptive call has nothing to retry"""
    base = scene_lds()
    sc = Scene("full%s" % (" adaptive" if adaptive else ""), base.grid, base.points, 9, adaptive=adaptive)
    return Case(sc, draw_values("negative", base.points, 9701))


@functools.lru_cache(maxsize=None)
def case_beyond_the_ladder():
    """radius 3: the last threshold an int holds is 3e8; the nearest point lies beyond it (20 km).  The
    reference's int product overflows on its way to this cloud -- never sent to the oracle."""
    g = O.make_grid(66.0, 40.0, 1.0, UTM[0], UTM[1])
    rng = np.random.default_rng(9702)
    xy = np.array([g.pos_x, g.pos_y]) + 20000.0 * np.array([0.6, 0.8]) + rng.uniform(0.0, 50.0, (30, 2))
    sc = Scene("beyond the ladder", g, _cloud(xy), 3, adaptive=True, oracle=False)
    return Case(sc, rng.integers(0, 256, 30))


# ---- e: layer state -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_second_cloud():
    """a cloud over the middle of scene_lds's map only: a second call that leaves most cells alone"""
    g = scene_lds().grid
    rng = np.random.default_rng(9801)
    xy = np.c_[rng.uniform(g.pos_x - 30.0, g.pos_x + 25.0, 1500), rng.uniform(g.pos_y - 12.0, g.pos_y + 20.0, 1500)]
    sc = Scene("second cloud", g, _cloud(xy), 2)
    return Case(sc, draw_values("negative", sc.points, 9802))


def arbitrary_layer(g):
    """a caller's layer: NaN (several payloads), -0.0, infinities, denormals, ordinary floats"""
    rng = np.random.default_rng(9803)
    bits = rng.integers(0, 2 ** 32, (g.cols, g.rows), dtype=np.uint64).astype(np.uint32)
    bits[::3, ::5] = 0x80000000         # -0.0
    bits[1::3, ::7] = 0x7FC00001        # a quiet NaN with a payload
    bits[2::3, ::11] = 0xFF800000       # -inf
    return bits.view(np.float32)


# ---- f: geometry --------------------------------------------------------------------------------
GEOMETRIES = ((0.1, 131, 71, 1), (0.3, 131, 71, 1), (0.7, 131, 71, 2), (0.3, 37, 11, 2), (0.7, 63, 15, 4))


@functools.lru_cache(maxsize=None)
def case_geometry(res, rows, cols, radius):
    """non-dyadic resolutions at UTM magnitudes, odd cell counts, maps smaller than one tile"""
    g = O.make_grid(rows * res, cols * res, res, UTM[0] + 0.37, UTM[1] - 0.21)
    assert (g.rows, g.cols) == (rows, cols)
    rng = np.random.default_rng(9900 + rows + int(100 * res))
    n = int(min(6000, max(200, 0.8 * rows * cols)))
    sc = Scene("geometry res=%g %dx%d r=%d" % (res, rows, cols, radius), g,
               _cloud(_uniform(rng, g, n, 1.5 * np.sqrt(radius))), radius)
    return Case(sc, draw_values("above_2p24", sc.points, 9950))
