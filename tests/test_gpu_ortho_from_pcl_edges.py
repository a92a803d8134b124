"""GPU: ortho::OrthoFromPcl -- the values mode of the DSM machinery (pcl_mode = 1: the sort carries an int32
per point, the gathers write the ortho layer, use_adaptive_interpolation adds the host loop of retries)
-- at its edges.

The rule of comparison, everywhere (ortho_from_pcl_reference.assert_obeys): against the EXACT rational
inverse-distance average of the points with d2 < T, with delta = (4 N + 8) 2^-53 max|z| from the kernels'
own bound (amhip_dsm.hip: idw_err_bound): a cell whose answer rounds to one float over [h - delta,
h + delta] holds exactly that float; a cell in the band holds one of the two floats; an exact-hit cell a
member of the coincident points' values; a cell without a sample the bits it had.  And against the
oracle where the reference is defined: the same bits wherever the rule leaves no choice.
tests/test_ortho_from_pcl_reference.py holds the oracle to the same rule on the same inputs without a GPU
and asserts what each family covers (band cells <= 1 % everywhere).  No tolerance but delta, bit equality
and set membership.

Which path a call took is read back, not assumed: m.dsm_gather_stats() (tiles: the LDS-tiled gather ran;
class1 / class2: tiles on the list launches with larger images; beyond_lds: tiles of the wave-per-cell
kernel; sparse_list: occupied tiles walked from the pre-pass's list) and m.dsm_stats()["sort_pipeline"]
describe a from-pcl call like a DSM call (the retries of an adaptive call run the global gather:
tiles == 0 after them).

  a  value ranges (8 bit, negative, mixed sign, the ends of int32, non-floats above 2^24, constant) on the
     LDS-tiled gather, the capacity classes with the wave-per-cell kernel, the global gather; the one-level
     sort and both three-pass pipelines; a sparse call on a large materialized map (the tile lists)
  b  d2 == T exactly does not count, one double spacing nearer does: the first search and retries 1, 2
  c  exact hits: one among near neighbours, coincident with equal / different values, on every gather
  d  the ladder up to lambda = 10^9 with points 25 / 39 km outside the map; 1 x 1, 1 x N, N x 1 grids; a
     first pass that fills everything; the end of the ladder (radius 3: nothing within 3e8)
  e  layer state: a second call, a call after reset(), a caller's layer of arbitrary bits, device == host,
     run-to-run and under a permutation of the cloud
  f  resolutions 0.1 / 0.3 / 0.7 at UTM magnitudes, odd cell counts, maps smaller than a tile"""
import numpy as np
import pytest

import ortho_from_pcl_inputs as I
import ortho_from_pcl_reference as R

pytestmark = pytest.mark.gpu

SORTS = {"one-level": dict(p3_min_points=None, sort_runs=None),
         "runs": dict(p3_min_points=1000, sort_runs=None),      # the three-pass sort, run pipeline
         "count": dict(p3_min_points=1000, sort_runs=0)}        # the three-pass sort, counting pipeline


def _A():
    import aerial_mapper_amd as A
    return A


def _map(g):
    A = _A()
    return A.AerialGridMap(A.GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution))


def _process(m, case, device=False, order=None):
    A = _A()
    pts, vals = case.points, case.values
    if order is not None:
        pts, vals = np.ascontiguousarray(pts[order]), np.ascontiguousarray(vals[order])
    mosaic = A.OrthoFromPcl(A.OrthoFromPclSettings(interpolation_radius=case.radius,
                                                   use_adaptive_interpolation=case.adaptive))
    if device:
        import torch
        mosaic.process(torch.from_numpy(pts).cuda(), torch.from_numpy(vals).cuda(), m)
    else:
        mosaic.process(pts, vals, m)


def _run(tuning, case, sort="one-level", device=False, order=None):
    """one call on a fresh map -> (the ortho layer, where the call went)"""
    tuning(**SORTS[sort])
    with _map(case.grid) as m:
        _process(m, case, device, order)
        got = m.get("ortho")
        st = m.dsm_gather_stats()
        st["sort_pipeline"] = m.dsm_stats()["sort_pipeline"]
    if case.scene.n >= 1000:
        assert st["sort_pipeline"] == sort, (case.name, st)
    return got, st


def _hold(got, case, before=None, what=""):
    before = R.new_layer(case.grid) if before is None else before
    e = case.expect()
    share = R.assert_obeys(got, before, e, "%s %s" % (case.name, what))
    assert share <= 0.01
    if case.scene.oracle_defined:
        R.assert_same_decisions(got, case.oracle("port", before=before), e, "%s %s vs oracle" % (case.name, what))


def _assert_path(path, st, name):
    if path == "lds":          # 3 x 5 tiles of 64 x 16, all in the main launch
        assert st["tiles"] == 15 and st["class1"] == st["class2"] == st["beyond_lds"] == 0, (name, st)
    elif path == "classes":    # 3 x 5 tiles, every capacity class taken
        assert st["tiles"] == 15 and st["class1"] > 0 and st["class2"] > 0 and st["beyond_lds"] > 0, (name, st)
    else:                      # the window is wider than the LDS gather handles
        assert st["tiles"] == 0, (name, st)


# ---- a ----------------------------------------------------------------------------------------
PATH_SORTS = [("lds", "one-level"), ("lds", "runs"), ("lds", "count"), ("classes", "one-level"),
              ("classes", "runs"), ("classes", "count"), ("global", "one-level"), ("global", "runs")]


@pytest.mark.parametrize("kind", I.VALUE_KINDS)
@pytest.mark.parametrize("path,sort", PATH_SORTS)
def test_a_value_ranges(tuning, path, sort, kind):
    case = I.case_values(path, kind)
    got, st = _run(tuning, case, sort)
    _assert_path(path, st, case.name)
    _hold(got, case, what=sort)


@pytest.mark.parametrize("sort", ["one-level", "count"])
def test_a_sparse_call_walks_the_tile_lists(tuning, sort):
    """a small cloud on a materialized map of > 8192 tiles: only the occupied tiles are visited (sparse_list),
    the class lists behind them; 8.6 M cells of arbitrary bits stay as they are"""
    case = I.case_sparse()
    before = I.arbitrary_layer(case.grid)
    tuning(**SORTS[sort])
    with _map(case.grid) as m:
        m.set("ortho", before)
        _process(m, case, device=True)
        got = m.get("ortho")
        st = m.dsm_gather_stats()
        assert m.dsm_stats()["sort_pipeline"] == sort
    assert st["tiles"] == I.SPARSE_TILES and 0 < st["sparse_list"] < 200 and st["class1"] >= 1, st
    _hold(got, case, before=before, what=sort)


@pytest.mark.parametrize("device", [False, True])
def test_a_column_block_too_wide_for_the_three_pass_sort_keeps_the_one_level_sort(tuning, device):
    """4096 bin columns in one column block: the big placement's LDS image of the three-pass sort cannot hold
    them next to its points (amhip_sort.hip: dsm_sort).  The call used to fail with a HIP error."""
    case = I.case_wide_strip()
    tuning(p3_min_points=1000)
    with _map(case.grid) as m:
        _process(m, case, device)
        got = m.get("ortho")
        assert m.dsm_stats()["sort_pipeline"] == "one-level"
    _hold(got, case)


# ---- b ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", ["one-level", "runs"])
@pytest.mark.parametrize("radius", I.STRICT_RADII)
def test_b_decisions_at_the_search_radius_are_the_references(tuning, radius, sort):
    for inside in (False, True):
        case = I.case_strict(radius, inside)
        got, st = _run(tuning, case, sort)
        assert st["tiles"] > 0
        _hold(got, case, what=sort)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("radius", I.STRICT_RADII)
def test_b_decisions_at_a_retry_threshold_are_the_references(tuning, radius, k):
    for which in (0, 1):
        for inside in (False, True):
            case = I.case_strict_adaptive(radius, k, which, inside)
            got, _ = _run(tuning, case)
            _hold(got, case)
            # (what the reference test asserts of the expectation, of the result: the probe alone, or
            # probe and companion one retry later)
            assert (got[35, 65] == 1000000.0) == inside, (case.name, got[35, 65])


# ---- c ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.HIT_KINDS)
@pytest.mark.parametrize("path,sort", [("lds", "one-level"), ("lds", "runs"), ("classes", "one-level"),
                                       ("classes", "count"), ("global", "one-level")])
def test_c_exact_hits(tuning, path, sort, kind):
    case = I.case_hits(path, kind)
    got, st = _run(tuning, case, sort)
    _assert_path(path, st, case.name)
    _hold(got, case, what=sort)
    e = case.expect()
    for at in case.scene.marks["hit_cells"]:
        assert int(got.view(np.uint32)[at]) in e.hits[at]


# ---- d ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", I.LADDER_PLACES)
@pytest.mark.parametrize("radius", I.LADDER_RADII)
def test_d_the_ladder(tuning, radius, place):
    case = I.case_ladder(radius, place)
    got, st = _run(tuning, case)
    _hold(got, case)
    assert (got != R.INIT_VALUE).all() and st["tiles"] == 0      # every cell filled; the last pass was a retry
    dev, _ = _run(tuning, case, device=True)
    assert np.array_equal(dev.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("rows,cols", I.DEGENERATE)
def test_d_degenerate_grids(tuning, rows, cols, adaptive):
    case = I.case_degenerate(rows, cols, adaptive)
    got, _ = _run(tuning, case)
    assert got.shape == (cols, rows)
    _hold(got, case)
    dev, _ = _run(tuning, case, device=True)
    assert np.array_equal(dev.view(np.uint32), got.view(np.uint32))


def _gather_launches(case):
    with _map(case.grid) as m:
        m.enable_timing()
        m.timing_reset()
        _process(m, case)
        got = m.get("ortho")
        return got, m.kernel_times()["k_dsm_gather"][1]


def test_d_a_first_pass_that_fills_everything_launches_no_retry(tuning):
    tuning(**SORTS["one-level"])
    plain, n_plain = _gather_launches(I.case_first_pass_fills(False))
    adaptive, n_adaptive = _gather_launches(I.case_first_pass_fills(True))
    _hold(adaptive, I.case_first_pass_fills(True))
    assert np.array_equal(plain.view(np.uint32), adaptive.view(np.uint32))
    assert n_plain == n_adaptive == 1
    _, n_ladder = _gather_launches(I.case_ladder(1, "corner"))      # (the counter does count retries)
    assert n_ladder == 1 + int(I.case_ladder(1, "corner").expect().search.level.max())


@pytest.mark.parametrize("device", [False, True])
def test_d_beyond_the_ladder_every_cell_keeps_its_bits(tuning, device):
    """radius 3: the retries end at T = 3e8 (the next int product would overflow); the nearest point is
    20 km away.  The call returns OK and writes nothing.  (The reference is undefined here: no oracle.)"""
    case = I.case_beyond_the_ladder()
    assert (case.expect().kind == 0).all()
    before = I.arbitrary_layer(case.grid)
    tuning(**SORTS["one-level"])
    with _map(case.grid) as m:
        m.set("ortho", before)
        _process(m, case, device)
        got = m.get("ortho")
    assert np.array_equal(got.view(np.uint32), before.view(np.uint32))
    got, _ = _run(tuning, case, device=device)                       # ... and on a map never written
    assert np.array_equal(got.view(np.uint32), R.new_layer(case.grid).view(np.uint32))


# ---- e ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_e_a_second_call_and_a_call_after_reset(tuning, device):
    first, second = I.case_values("lds", "u8"), I.case_second_cloud()
    tuning(**SORTS["one-level"])
    with _map(first.grid) as m:
        _process(m, first, device)
        after_first = m.get("ortho")
        _hold(after_first, first, what="first call")
        _process(m, second, device)
        after_second = m.get("ortho")
        _hold(after_second, second, before=after_first, what="second call")
        assert (second.expect().kind == 0).mean() > 0.5
        m.reset()                       # lazy: nothing is filled until a call needs the layer
        _process(m, second, device)
        _hold(m.get("ortho"), second, what="after reset()")
    adaptive = I.case_ladder(1, "corner")
    with _map(adaptive.grid) as m:      # ... and an adaptive call (it materializes the layer first)
        _process(m, I.case_ladder(2, "b6"), device)
        m.reset()
        _process(m, adaptive, device)
        _hold(m.get("ortho"), adaptive, what="adaptive after reset()")


@pytest.mark.parametrize("case", [lambda: I.case_second_cloud(), lambda: I.case_hits("lds", "single"),
                                  lambda: I.case_strict_adaptive(4, 1, 0, True)])
def test_e_a_callers_layer_of_arbitrary_bits(tuning, case):
    """the host entry point with a caller-provided layer: NaN payloads, -0.0, infinities stay as they are
    wherever the call has no sample"""
    from aerial_mapper_amd import hip_lib as L
    case = case()
    before = I.arbitrary_layer(case.grid)
    layer = before.copy()
    tuning(**SORTS["one-level"])
    with _map(case.grid) as m:
        L.check(L.load().amhip_ortho_from_pcl_process(m.handle, case.points.ctypes.data, case.values.ctypes.data,
                                                      case.scene.n, case.radius, int(case.adaptive),
                                                      layer.ctypes.data))
        on_device = m.get("ortho")
    _hold(layer, case, before=before)
    assert np.array_equal(on_device.view(np.uint32), layer.view(np.uint32))
    if not case.adaptive:
        assert (case.expect().kind == 0).sum() > 100


E_CASES = [("lds", "int32_ends", "one-level"), ("lds", "mixed", "runs"), ("classes", "above_2p24", "count"),
           ("classes", "mixed", "one-level"), ("global", "negative", "one-level")]


@pytest.mark.parametrize("path,kind,sort", E_CASES)
def test_e_device_path_second_run_and_permuted_cloud_give_the_same_bits(tuning, path, kind, sort):
    case = I.case_values(path, kind)
    host, _ = _run(tuning, case, sort)
    _hold(host, case, what=sort)
    again, _ = _run(tuning, case, sort)
    dev, _ = _run(tuning, case, sort, device=True)
    perm, _ = _run(tuning, case, sort, order=np.random.default_rng(31).permutation(case.scene.n))
    for other, what in ((again, "second run"), (dev, "device path"), (perm, "permuted cloud")):
        assert np.array_equal(other.view(np.uint32), host.view(np.uint32)), (case.name, what)


@pytest.mark.parametrize("sort", ["one-level", "runs", "count"])
def test_e_the_value_range_of_an_earlier_call_does_not_linger(tuning, sort):
    """max|z| of the rounding bound is the CALL's (the sort leaves it): after a call with other values, on
    the same context, a call stores the floats it stores on a fresh one -- small after large and large
    after small"""
    small, large = I.case_values("lds", "u8"), I.case_values("lds", "int32_ends")
    fresh = {c.name: _run(tuning, c, sort)[0] for c in (small, large)}
    with _map(small.grid) as m:
        for c in (small, large, small, large):
            m.reset()
            _process(m, c, device=True)
            got = m.get("ortho")
            assert np.array_equal(got.view(np.uint32), fresh[c.name].view(np.uint32)), c.name
            assert m.dsm_stats()["sort_pipeline"] == sort


@pytest.mark.parametrize("kind", ["single", "equal"])
@pytest.mark.parametrize("path", ["lds", "classes", "global"])
def test_e_exact_hits_under_a_permutation(tuning, path, kind):
    # (coincident hits with DIFFERENT values are order dependent by design: docs/HISTORY.md)
    case = I.case_hits(path, kind)
    host, _ = _run(tuning, case)
    perm, _ = _run(tuning, case, order=np.random.default_rng(32).permutation(case.scene.n), device=True)
    assert np.array_equal(perm.view(np.uint32), host.view(np.uint32))


# ---- f ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,rows,cols,radius", I.GEOMETRIES)
def test_f_geometry(tuning, res, rows, cols, radius):
    case = I.case_geometry(res, rows, cols, radius)
    got, st = _run(tuning, case)
    assert st["tiles"] == ((rows + 63) // 64) * ((cols + 15) // 16) or st["tiles"] == ((rows + 63) // 64) * ((cols + 31) // 32)
    _hold(got, case)
    dev, _ = _run(tuning, case, device=True)
    assert np.array_equal(dev.view(np.uint32), got.view(np.uint32))
