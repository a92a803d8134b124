"""CPU: the exact restatement of ortho::OrthoFromPcl (tests/ortho_from_pcl_reference.py) against the
compiled oracle -- O.ortho_from_pcl in the port build and in the vendored-nanoflann build -- on every input
family of tests/test_gpu_ortho_from_pcl_edges.py (tests/ortho_from_pcl_inputs.py), before a GPU is involved:

  * the same cells touched and left alone;
  * the oracle's floats obey the rule of comparison (ortho_from_pcl_reference.assert_obeys);
  * at most 1 % of a case's interpolated cells lie in the band where the rule admits two floats -- a
    condition of the inputs, asserted with the reference alone;
  * every adaptive family fills all its cells before the reference's int product would overflow (the one
    family that does not is never sent to the oracle);
  * each family plants what it is there to cover."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_ffi as O
import ortho_from_pcl_inputs as I
import ortho_from_pcl_reference as R

BAND_CAP = 0.01


def builds():
    return ["port"] + (["ref"] if O.have_ref() else [])


def hold_oracle(case, before=None):
    e = case.expect()
    if case.adaptive:
        assert case.scene.fills_before_overflow(), case.name
    assert e.band_share <= BAND_CAP, (case.name, e.band_share, int(e.band.sum()))
    start = R.new_layer(case.grid) if before is None else before
    outs = []
    for which in builds():
        got = case.oracle(which, before=start)
        R.assert_obeys(got, start, e, "%s (%s oracle)" % (case.name, which))
        outs.append(got)
    for got in outs[1:]:
        R.assert_same_decisions(got, outs[0], e, case.name)
    return e, outs[0]


# ---- the reference's own pieces -----------------------------------------------------------------
def test_rn32_rounds_to_nearest_even():
    f = lambda x: float(R.rn32(Fraction(x)))
    assert f(2 ** 24 + 1) == 2.0 ** 24 and f(2 ** 24 + 3) == 2.0 ** 24 + 4       # ties to even
    assert f(Fraction(2 ** 24 + 1) + Fraction(1, 10 ** 30)) == 2.0 ** 24 + 2     # just above a tie
    assert f(Fraction(2 ** 24 + 1) - Fraction(1, 10 ** 30)) == 2.0 ** 24
    assert f(-2 ** 31) == -2.0 ** 31 and f(2 ** 31 - 1) == 2.0 ** 31 and f(-(2 ** 31 - 1)) == -2.0 ** 31
    assert f(Fraction(1, 3)) == float(np.float32(1.0) / np.float32(3.0))
    # a double rounding would go wrong here: 1 + 2^-24 + 2^-60 is above the tie, its double is the tie
    assert f(1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == 1.0 + 2.0 ** -23
    assert f(0) == 0.0 and f(Fraction(-1, 10 ** 9)) == float(np.float32(-1e-9))


def test_thresholds_stop_where_the_int_product_would_overflow():
    assert R.thresholds(2, False) == [2]
    assert R.thresholds(1, True) == [10 ** k for k in range(10)]
    assert R.thresholds(2, True)[-1] == 2 * 10 ** 9 and len(R.thresholds(2, True)) == 10
    assert R.thresholds(3, True)[-1] == 3 * 10 ** 8                # 3e9 > 2^31 - 1
    assert R.thresholds(214, True)[-1] == 214 * 10 ** 7 and R.thresholds(215, True)[-1] == 215 * 10 ** 6


@pytest.mark.parametrize("case", [lambda: I.case_geometry(0.3, 37, 11, 2), lambda: I.case_degenerate(1, 90, True),
                                  lambda: I.case_strict_adaptive(5, 1, 0, False), lambda: I.case_ladder(2, "b7"),
                                  lambda: I.case_hits("global", "different")])
def test_the_shortcut_is_the_fraction_evaluation(case):
    """Expect decides most cells from a double evaluation and its error bound; here every interpolated
    cell is decided with fractions alone, against every point of the cloud (no band search either)."""
    case = case()
    e, s, g = case.expect(), case.scene.search(), case.grid
    T = R.thresholds(case.radius, case.adaptive)
    cells = np.argwhere(e.kind >= 0)
    if len(cells) > 700:
        cells = cells[np.random.default_rng(5).permutation(len(cells))[:700]]
    for j, i in cells:
        qx, qy = O.cell_position(g, int(i), int(j))
        dx, dy = qx - case.points[:, 0], qy - case.points[:, 1]
        d2 = dx * dx
        d2 = d2 + dy * dy
        keep, level = np.zeros(d2.shape, bool), -1
        for level_k, t in enumerate(T):
            if (d2 < t).any():
                keep, level = d2 < t, level_k
                break
        assert level == s.level[j, i] and keep.sum() == s.count[j, i]
        if not keep.any():
            assert e.kind[j, i] == 0
        elif (d2[keep] == 0.0).any():
            assert e.kind[j, i] == 2
            assert e.hits[(j, i)] == set(int(np.float32(np.float64(v)).view(np.uint32))
                                         for v in case.values[keep & (d2 == 0.0)])
        else:
            h = R.exact_cell(d2[keep], case.values[keep])
            assert e.kind[j, i] == 1
            assert (e.lo[j, i], e.hi[j, i]) == (R.rn32(h - e.delta), R.rn32(h + e.delta)), (j, i)


# ---- a ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.VALUE_KINDS)
@pytest.mark.parametrize("path", sorted(I.PATH_SCENES))
def test_a_value_families(path, kind):
    case = I.case_values(path, kind)
    e, want = hold_oracle(case)
    v = case.values.astype(np.int64)
    assert e.interpolated.mean() > 0.9 and not e.hits
    if kind == "int32_ends":
        assert set(I.ENDS) <= set(v.tolist())
        mixed = (want > -2.0 ** 30) & (want < 2.0 ** 30) & e.interpolated        # cells that mix the signs
        assert mixed.any()
        if path != "global":        # (there every window spans several fields of the chequerboard)
            assert want.max() > 2.0 ** 31 - 5200 and want[e.interpolated].min() < -2.0 ** 31 + 5200
    if kind == "above_2p24":
        assert (np.float32(v).astype(np.int64) != v).all()
    if kind == "mixed":     # |h| << max|z|: where an absolute bar says nothing
        assert np.median(np.abs(want[e.interpolated])) < 0.3 * np.abs(v).max()
    if kind == "constant":
        assert (want[e.interpolated] == np.float32(v[0])).all() and np.float32(v[0]) == v[0]


def test_a_scene_shapes():
    """what the planner's thresholds (amhip_dsm_plan.h) will see: points per tile region"""
    sc = I.scene_classes()
    g = sc.grid
    top = g.pos_y + g.length_y / 2
    row = np.floor(top - sc.points[:, 1])              # cell row j of every point
    inside_i = np.abs(sc.points[:, 0] - g.pos_x) < 33.0     # a 66-cell wide region
    per_region = [int(((row >= 16 * t - 1) & (row <= 16 * t + 16) & inside_i).sum()) for t in range(5)]
    assert 2048 < per_region[0] <= 2752 and 2752 < per_region[2] <= 5200 and per_region[4] > 5600, per_region
    assert I.scene_lds().n / (130 * 70) * 66 * 18 < 900         # class 0 throughout, 64 x 16 tiles of 1024
    s = I.scene_global()
    assert np.floor(np.sqrt(s.radius) / s.grid.resolution + 0.5) > 16


def test_a_sparse_call():
    case = I.case_sparse()
    g = case.grid
    e, _ = hold_oracle(case, before=I.arbitrary_layer(g))
    assert I.SPARSE_TILES == ((g.rows + 63) // 64) * ((g.cols + 15) // 16) > 8192 and case.scene.n * 16 < g.rows * g.cols
    assert 0.001 < e.interpolated.mean() < 0.01
    i0, i1, j0, j1 = case.scene.marks["patch_region"]       # the region of tile (10, 20), cells
    assert (i0, j0) == (64 * 10 - 1, 16 * 20 - 1)
    x, y = O.cell_position(g, i0, j0)
    inside = ((case.points[:, 0] < x + 0.5) & (case.points[:, 0] > x + 0.5 - (i1 - i0)) &
              (case.points[:, 1] < y + 0.5) & (case.points[:, 1] > y + 0.5 - (j1 - j0)))
    assert 2048 < inside.sum() <= 2752, inside.sum()


def test_a_wide_strip():
    case = I.case_wide_strip()
    e, _ = hold_oracle(case)
    assert case.grid.rows + 2 > 3936 and case.scene.n >= 1000 and 0.05 < e.interpolated.mean() < 0.5


# ---- what the rule notices -----------------------------------------------------------------------
def _first_failure(fn):
    with pytest.raises(AssertionError) as ei:
        fn()
    return str(ei.value)


def test_the_rule_notices_subtle_mistakes():
    """Mistakes a kernel could make, made on purpose on the oracle's result: each must fail the rule."""
    case = I.case_values("lds", "above_2p24")
    e, want = hold_oracle(case)
    start = R.new_layer(case.grid)
    sure = np.argwhere(e.interpolated & ~e.band)
    for up in (np.inf, -np.inf):            # one float off in one cell
        got = want.copy()
        at = tuple(sure[len(sure) // 2])
        got[at] = np.nextafter(got[at], np.float32(up))
        assert "hold another float" in _first_failure(lambda: R.assert_obeys(got, start, e))
    # values rounded to float32 before they are averaged
    as_floats = R.Expect(case.scene.search(), np.float32(case.values).astype(np.int64))
    got = np.where(e.kind == 0, start, as_floats.lo)
    assert "hold another float" in _first_failure(lambda: R.assert_obeys(got, start, e))
    # a neighbour's value: the payload of the sorted points shifted by one
    shifted = I.Case(case.scene, np.roll(case.values, 1)).oracle()
    assert "hold another float" in _first_failure(lambda: R.assert_obeys(shifted, start, e))
    # an untouched cell written, a touched cell left
    got = want.copy()
    got[tuple(np.argwhere(e.kind == 0)[0])] = 0.0
    assert "without a sample" in _first_failure(lambda: R.assert_obeys(got, start, e))
    got = want.copy()
    got[tuple(sure[0])] = R.INIT_VALUE
    _first_failure(lambda: R.assert_obeys(got, start, e))
    # a decision at the radius taken the other way; a hit cell holding a neighbour's value
    at, inside = I.case_strict(5, False), I.case_strict(5, True)
    _first_failure(lambda: R.assert_obeys(inside.oracle(), start_of(at), at.expect()))
    _first_failure(lambda: R.assert_obeys(at.oracle(), start_of(at), inside.expect()))
    hits = I.case_hits("lds", "equal")
    got = hits.oracle()
    cell = hits.scene.marks["hit_cells"][1]
    got[cell] = got[cell[0], cell[1] + 1]
    assert "exact-hit cell" in _first_failure(lambda: R.assert_obeys(got, start_of(hits), hits.expect()))


def start_of(case):
    return R.new_layer(case.grid)


# ---- b ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", I.STRICT_RADII)
def test_b_strict_radius(radius):
    at, inside = I.case_strict(radius, False), I.case_strict(radius, True)
    ea, _ = hold_oracle(at)
    ei, _ = hold_oracle(inside)
    targets = at.scene.marks["targets"]
    assert len(targets) == len(I.lattice_offsets(radius)) >= 4
    for t in targets:
        # the probe at d2 == T does not count; one double spacing nearer it does -- and moves the cell far
        assert ei.search.count[t] == ea.search.count[t] + 1, t
        assert ei.kind[t] == 1 and ei.lo[t] > ea.hi[t] + 1.0 if ea.kind[t] else ei.kind[t] == 1
        assert ea.kind[t] == 0 or ea.hi[t] < 256.0
    assert any(ea.kind[t] == 1 for t in targets)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("radius", I.STRICT_RADII)
def test_b_strict_retry_threshold(radius, k):
    for which in (0, 1):
        at, inside = (I.case_strict_adaptive(radius, k, which, ins) for ins in (False, True))
        ea, _ = hold_oracle(at)
        ei, _ = hold_oracle(inside)
        t = (35, 65)
        assert ei.search.level[t] == k and ei.search.count[t] == 1 and ei.lo[t] == ei.hi[t] == 1000000.0
        assert ea.search.level[t] == k + 1 and ea.search.count[t] == 2 and ea.hi[t] < 999000.0


# ---- c ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.HIT_KINDS)
@pytest.mark.parametrize("path", sorted(I.PATH_SCENES))
def test_c_exact_hits(path, kind):
    case = I.case_hits(path, kind)
    e, want = hold_oracle(case)
    cells = case.scene.marks["hit_cells"]
    assert sorted(e.hits) == sorted(cells)
    assert int(e.several_valued.sum()) == (len(cells) if kind == "different" else 0)
    for (j, i) in cells:
        assert e.search.count[j, i] >= (3 if kind != "single" else 4)      # the hit is not alone
        for dj, di in ((0, 1), (1, 0), (0, -1), (-1, 0)):                   # and its neighbours interpolate
            if 0 <= j + dj < case.grid.cols and 0 <= i + di < case.grid.rows:
                assert e.kind[j + dj, i + di] == 1


# ---- d ------------------------------------------------------------------------------------------
def test_d_ladder_reaches_every_retry():
    seen = {}
    for radius in I.LADDER_RADII:
        for place in I.LADDER_PLACES:
            case = I.case_ladder(radius, place)
            e, _ = hold_oracle(case)
            levels = set(np.unique(e.search.level).tolist())
            seen.setdefault(radius, set()).update(levels)
            if place == "far":
                assert levels == {9}
                d = np.hypot(case.points[:, 0] - case.grid.pos_x, case.points[:, 1] - case.grid.pos_y)
                assert d.min() > 24000.0
            elif place != "corner":
                assert levels == {int(place[1]) - 1, int(place[1])}, (place, levels)
    assert seen == {1: set(range(10)), 2: set(range(10))}, seen


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("rows,cols", I.DEGENERATE)
def test_d_degenerate_grids(rows, cols, adaptive):
    e, _ = hold_oracle(I.case_degenerate(rows, cols, adaptive))
    assert e.kind[0, 0] == 1
    if max(rows, cols) > 3:
        assert (e.search.level.max() >= 3) if adaptive else (e.kind == 0).any()


def test_d_first_pass_fills_everything():
    plain, adaptive = I.case_first_pass_fills(False), I.case_first_pass_fills(True)
    ep, wp = hold_oracle(plain)
    ea, wa = hold_oracle(adaptive)
    assert (ea.search.level == 0).all() and (ep.kind == 1).all()
    assert np.array_equal(wp.view(np.uint32), wa.view(np.uint32))


def test_d_beyond_the_ladder_is_not_the_oracles():
    case = I.case_beyond_the_ladder()
    assert not case.scene.oracle_defined and not case.scene.fills_before_overflow()
    assert (case.expect().kind == 0).all()
    with pytest.raises(AssertionError):
        case.oracle()


# ---- e ------------------------------------------------------------------------------------------
def test_e_layer_state():
    first, second = I.case_values("lds", "u8"), I.case_second_cloud()
    _, after_first = hold_oracle(first)
    e, _ = hold_oracle(second, before=after_first)
    assert 0.1 < e.interpolated.mean() < 0.5
    e2, got = hold_oracle(second, before=I.arbitrary_layer(second.grid))
    assert np.isnan(got[e2.kind == 0]).any() and (got[e2.kind == 0].view(np.uint32) == 0x80000000).any()


# ---- f ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,rows,cols,radius", I.GEOMETRIES)
def test_f_geometry(res, rows, cols, radius):
    e, _ = hold_oracle(I.case_geometry(res, rows, cols, radius))
    assert e.interpolated.mean() > 0.5
