"""CPU: the oracle's capped mode (oracle/amo_dsm.cc amo_dsm_process_knn: own kd-tree and stable sort;
the vendored nanoflann's KNNResultSet where oracle/_ref is built) against the plain restatement of
tests/dsm_knn_reference.py, on every input family of tests/test_gpu_dsm_knn_edges.py: bit for bit on
every cell that is not ambiguous, inside the admissible set on every cell that is, same NaN pattern.
And what each family is there to cover is asserted here, on the restatement alone, so that a changed
seed cannot quietly empty a GPU test of its subject."""
import numpy as np
import pytest

import dsm_knn_reference as R
import oracle_ffi as O

ALL_K = list(range(1, 9))


def _whiches():
    return ["port"] + (["ref"] if O.have_ref() else [])


def _hold_oracle_to_restatement(fam, ks, expect_ambiguous=False):
    for k in ks:
        r = fam.cap(k)
        if not expect_ambiguous:
            assert not r.ambiguous.any(), (fam.name, k, int(r.ambiguous.sum()))
        assert not r.exact.any()
        for which in _whiches():
            rc, e = fam.oracle(k, which)
            assert rc == O.OK
            R.assert_capped_equal(e, r.value, r, "%s k=%d %s" % (fam.name, k, which), exact_membership=True)
    return r


def test_ladder_thresholds():
    T = R.ladder(1)
    assert T[0] == T[1] == 1.0 and T[2] == 1.1 and T[3] == 1.1 * 1.1
    assert T[-1] <= 7.0 < T[-1] * 1.1 and len(T) == 22
    assert R.ladder(9) == [9.0, 9.0]          # the first level exceeds 7: one retry only
    assert R.ladder(2)[-1] <= 7.0 < R.ladder(2)[-1] * 1.1


@pytest.mark.parametrize("fam", [R.family_a, R.family_b, lambda: R.family_c(1), lambda: R.family_c(9),
                                 lambda: R.family_d(2, 0.3, 1), R.family_e], ids=["a", "b", "c1", "c9", "d", "e"])
def test_the_affordable_search_is_the_plain_one(fam):
    """search() looks at the points inside a square around the cell only; search_plain() at every
    (cell, point) pair.  Same sizes, levels and stored distances and heights, to the bit -- except the
    ORDER of the heights of equal distances, which is the candidates' (cap() flags those cells)."""
    fam = fam()
    fast = fam.search()
    plain = R.search_plain(fam.points, fam.grid, fam.radius_sq, fam.center_easting, fam.center_northing)
    assert np.array_equal(fast.size, plain.size) and np.array_equal(fast.level, plain.level)
    assert np.array_equal(fast.d2, plain.d2)
    tied = np.zeros(fast.d2.shape, bool)
    tied[:, :, 1:] = fast.d2[:, :, 1:] == fast.d2[:, :, :-1]
    tied[:, :, :-1] |= tied[:, :, 1:]
    assert np.array_equal(fast.z[~tied], plain.z[~tied]) and (fam.name != "b" or tied.any())
    assert np.array_equal(np.sort(np.where(tied, fast.z, 0.0), axis=2), np.sort(np.where(tied, plain.z, 0.0), axis=2))


def test_a_every_k_and_every_set_size():
    fam = R.family_a()
    s = fam.search()
    assert s.grid.rows == 100 and s.grid.cols == 40
    sizes = set(np.unique(s.size).tolist())
    assert set(range(0, 10)) <= sizes and max(sizes) > 16, sorted(sizes)
    assert (s.level > 1).any() and (s.size == 0).mean() > 0.05        # the hole's ladder, the empty strip
    r = _hold_oracle_to_restatement(fam, ALL_K)
    assert np.isnan(r.value).any() and (~np.isnan(r.value)).any()


def test_b_ties_of_every_kind():
    fam = R.family_b()
    seen = {kind: set() for kind in R.TIE_KINDS}
    for k in ALL_K:
        r = fam.cap(k)
        assert r.ambiguous.any()
        for kinds in r.kinds.values():
            for kind in kinds:
                seen[kind].add(k)
    for kind in R.TIE_KINDS:
        assert len(seen[kind]) >= 3, (kind, sorted(seen[kind]))
    # (an admissible set with more than one value: the choice at the k-th place shows in the height)
    assert any(len(a) > 1 and max(a) - min(a) > 0.5 for a in fam.cap(3).admissible.values())
    _hold_oracle_to_restatement(fam, ALL_K, expect_ambiguous=True)


@pytest.mark.parametrize("radius_sq", [1, 2, 9])
def test_c_the_ladder_under_a_cap(radius_sq):
    fam = R.family_c(radius_sq)
    s = fam.search()
    assert s.grid.rows == 96 and s.grid.cols == 48
    levels = set(np.unique(s.level[s.level > 0]).tolist())
    if radius_sq == 9:
        assert not levels                   # T = 9, then 9 once more: nothing new, the rest stays NaN
    else:
        assert len(levels) >= 3, sorted(levels)
        for k in (1, 4, 8):
            assert ((s.level > 0) & (s.size > k)).any(), k      # a ladder cell the cap cuts
    assert (s.size == 0).mean() > 0.5
    _hold_oracle_to_restatement(fam, (1, 4, 8))


@pytest.mark.parametrize("offsets", [0, 1])
@pytest.mark.parametrize("radius_sq,res", R.WINDOW_SHAPES)
def test_d_window_shapes(radius_sq, res, offsets):
    fam = R.family_d(radius_sq, res, offsets)
    s = fam.search()
    assert (s.size > 8).any() and (s.size == 0).any() and (s.level > 1).any() == (radius_sq < 9)
    _hold_oracle_to_restatement(fam, (3, 8))
    if offsets:         # the swap of dsm.cc:36-52 matters: the same call with the offsets exchanged differs
        rc, swapped = O.dsm_process_knn(fam.points, fam.grid, 3, radius_sq, fam.center_northing, fam.center_easting)
        assert rc == O.OK and np.isnan(swapped).all()


def test_e_wider_than_the_lds_gather():
    fam = R.family_e()
    assert fam.grid.rows == 100 and fam.grid.cols == 60 and fam.points.shape[0] == 600
    _hold_oracle_to_restatement(fam, (2, 8))


def points_in_tile(fam, ti, tj):
    """points whose nearest cell lies in gather tile (ti, tj)"""
    g = fam.grid
    bx, by = O.cell_position(g, 0, 0)
    i = np.floor((bx - fam.points[:, 0]) / g.resolution + 0.5).astype(np.int64)
    j = np.floor((by - fam.points[:, 1]) / g.resolution + 0.5).astype(np.int64)
    return int(((i // R.F_TILE[0] == ti) & (j // R.F_TILE[1] == tj) & (i >= 0) & (j >= 0)).sum())


def test_f_a_tile_beyond_the_image():
    fam = R.family_f()
    assert fam.grid.rows == 256 and fam.grid.cols == 64
    ti, tj = R.F_PATCH_CELL[0] // R.F_TILE[0], R.F_PATCH_CELL[1] // R.F_TILE[1]
    assert points_in_tile(fam, ti, tj) > 2048 + 1024            # the largest capped image, and the rest of the tile
    for di, dj in ((-1, 0), (1, 0), (0, -1)):
        assert 700 < points_in_tile(fam, ti + di, tj + dj) < 1400       # ~0.5 points per cell
    _hold_oracle_to_restatement(fam, (1, 8))


def test_g_exact_hit():
    hit, clean = R.family_g(1), R.family_g(0)
    for k in (1, 8):
        r = hit.cap(k)
        assert r.exact[11, 7] and r.exact.sum() == 1
        for which in _whiches():
            rc, _ = hit.oracle(k, which)
            assert rc == O.ERR_EXACT_HIT
    _hold_oracle_to_restatement(clean, (1, 8))


def test_h_capped_calls_of_the_chain_have_no_ambiguous_cell():
    for call, k in ((1, 4), (2, 8), (4, 2)):
        fam = R.family_h(call)
        assert fam.points.shape[0] > 1000            # (the three-pass sort at p3_min_points = 1000)
        _hold_oracle_to_restatement(fam, (k,))
    # the five clouds overlap pairwise and leave part of the map to the base layer
    reached = [R.family_h(c).search().size > 0 for c in range(5)]
    assert sum(r.astype(int) for r in reached).max() >= 3 and (~np.any(reached, axis=0)).mean() > 0.02


def test_j_sub_window_restated_on_the_bounding_box():
    fam = R.family_j()
    r = fam.cap(4)
    assert not r.ambiguous.any() and 0.001 < r.inside.mean() < 0.05
    # the box is wide enough: no value on its rim
    i0, i1, j0, j1 = fam.search().window
    v = ~np.isnan(r.value)
    assert v.any() and not v[j0, :].any() and not v[:, i1 - 1].any()
    rc, e = fam.oracle(4, "port")
    assert rc == O.OK
    R.assert_capped_equal(e, r.value, r, "j", exact_membership=True)
