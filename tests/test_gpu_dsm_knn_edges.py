"""GPU: the DSM's OPTIONAL capped mode (amhip_ctx_set_dsm_knn, AerialGridMap.set_dsm_knn) at its edges.
Two kernels carry it -- k_dsm_gather_tiled_knn (gather_tile with kKnn > 0, on the LDS image) and
k_dsm_gather_knn (cell_global_knn, one lane per cell on the global bins; tuning knob knn_global_bins) --
around one sorted set in registers (amhip_knn_set.h; tests/test_knn_set_host.py holds it on the host).

The rule of comparison, everywhere (dsm_knn_reference.assert_capped_equal): the oracle's NaN pattern;
EVERY cell that is not ambiguous equals the oracle's float bit for bit; every ambiguous cell (an exact
distance tie among the kept points or at the k-th place: the restatement of tests/dsm_knn_reference.py
says which) lies within one float32 spacing of an admissible value.  Random families have no ambiguous
cell -- asserted, so that no cell is left out; only the tie family (b) has them, and there they are the
subject.  tests/test_dsm_knn_reference.py holds the oracle to the restatement on the same inputs and
asserts what each family covers.

  a  every k = 1 .. 8 against every size of the search result (0, 1 .. 9, > 16), partial tiles
  b  exact ties: inside the set, at the k-th place with one slot open, more tied points than slots
  c  the radius ladder with a capped set (cell_global_knn; the `again` branch of the tiled kernel)
  d  window shapes w0 = 1 .. 12, a non-dyadic resolution, UTM magnitudes, the centre-offset swap
  e  a window wider than the LDS gather handles: k_dsm_gather_knn without the knob
  f  a tile whose region exceeds the LDS image (use_lds false: cell_global_knn per cell)
  g  an exact hit found in the tiled loop and handed to cell_global_knn
  h  earlier content and mode switches on one context, the three-pass sort taking part
  i  AMHIP_DSM_FAST under the cap: the FP64 pipeline all the same
  j  the sub-window path (dsm_subwindow)
  k  a device-resident cloud; the cap is dsm::Dsm's only"""
import numpy as np
import pytest

import dsm_knn_reference as R
import oracle_ffi as O
import scenarios as S

pytestmark = pytest.mark.gpu

KERNELS = ("tiled", "global")


def _A():
    import aerial_mapper_amd as A
    return A


def _settings(g):
    return _A().GridMapSettings(g.pos_x, g.pos_y, g.length_x, g.length_y, g.resolution)


def _dsm(fam, m):
    A = _A()
    return A.Dsm(A.DsmSettings(fam.radius_sq, False, fam.center_easting, fam.center_northing), m)


def _select(tuning, kernel):
    tuning(knn_global_bins=None if kernel == "tiled" else 1)


def _run(tuning, fam, k, kernel, exact=True, device=False, want_tiles=None):
    """one capped call on a fresh map -> the elevation layer"""
    A = _A()
    _select(tuning, kernel)
    with A.AerialGridMap(_settings(fam.grid)) as m:
        m.set_dsm_precision(exact)
        m.set_dsm_knn(k)
        pts = fam.points
        if device:
            import torch
            pts = torch.from_numpy(fam.points).cuda()
        _dsm(fam, m).process(pts, m)
        got = m.get("elevation")
        st = m.dsm_gather_stats()
    if want_tiles is None:
        want_tiles = kernel == "tiled"
    assert (st["tiles"] > 0) == want_tiles, (kernel, st)
    return got


def _check(tuning, fam, k, kernels=KERNELS, ambiguous=False, **kw):
    r = fam.cap(k)
    assert r.ambiguous.any() == ambiguous, (fam.name, k, int(r.ambiguous.sum()))
    rc, want = fam.oracle(k)
    assert rc == O.OK
    out = {}
    for kernel in kernels:
        out[kernel] = _run(tuning, fam, k, kernel, **kw)
        R.assert_capped_equal(out[kernel], want, r, "%s k=%d %s" % (fam.name, k, kernel))
    return out


# ---- a ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_a_every_k_against_every_set_size(tuning, k):
    out = _check(tuning, R.family_a(), k)
    assert np.array_equal(out["tiled"].view(np.uint32), out["global"].view(np.uint32))


# ---- b ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_b_exact_distance_ties(tuning, k):
    """Which of two equal distances stays is the arrival order's choice -- the kd-tree's, the bins',
    the LDS image's --, never a third value: every ambiguous cell is held to its admissible set."""
    fam = R.family_b()
    _check(tuning, fam, k, ambiguous=True)
    assert len(fam.cap(k).admissible) >= 20


# ---- c ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius_sq", [1, 2, 9])
def test_c_the_ladder_under_a_cap(tuning, radius_sq):
    fam = R.family_c(radius_sq)
    for k in (1, 4, 8):
        out = _check(tuning, fam, k)
        filled = ~np.isnan(out["tiled"])
        assert filled.any() and (~filled).mean() > 0.5
        assert np.array_equal(filled, fam.search().size > 0)


# ---- d ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [0, 1])
@pytest.mark.parametrize("radius_sq,res", R.WINDOW_SHAPES)
def test_d_window_shapes(tuning, radius_sq, res, offsets):
    fam = R.family_d(radius_sq, res, offsets)
    for k in (3, 8):
        _check(tuning, fam, k)


# ---- e ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 8])
def test_e_window_wider_than_the_lds_gather_handles(tuning, k):
    # (no knob: lds_ok = 0 by the window alone, asserted through tiles == 0)
    _check(tuning, R.family_e(), k, kernels=("tiled",), want_tiles=False)


# ---- f ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
def test_f_a_tile_beyond_the_image(tuning, k):
    A = _A()
    fam = R.family_f()
    r = fam.cap(k)
    assert not r.ambiguous.any()
    rc, want = fam.oracle(k)
    assert rc == O.OK
    _select(tuning, "tiled")
    with A.AerialGridMap(_settings(fam.grid)) as m:
        m.set_dsm_knn(k)
        _dsm(fam, m).process(fam.points, m)
        got = m.get("elevation")
        st = m.dsm_gather_stats()
    # the counters describe THIS call: 4 x 2 tiles of 64 x 32 cells (dsm_knn_reference.F_TILE), one of them
    # denser than the main launch's image of 2048 points (a capacity class of the pre-pass; the capped
    # launch takes every class, and that tile walks the global bins)
    assert st["tiles"] == (256 // R.F_TILE[0]) * (64 // R.F_TILE[1]), st
    assert st["class1"] + st["class2"] + st["beyond_lds"] == 1, st
    R.assert_capped_equal(got, want, r, "f k=%d" % k)


# ---- g ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", [1, 8])
def test_g_exact_hit_is_reported_and_the_context_goes_on(tuning, k, kernel):
    A = _A()
    hit, clean = R.family_g(1), R.family_g(0)
    rc, _ = hit.oracle(k)
    assert rc == O.ERR_EXACT_HIT
    r = clean.cap(k)
    assert not r.ambiguous.any()
    rc, want = clean.oracle(k)
    assert rc == O.OK
    _select(tuning, kernel)
    with A.AerialGridMap(_settings(hit.grid)) as m:
        m.set_dsm_knn(k)
        with pytest.raises(A.AmhipError) as ei:
            _dsm(hit, m).process(hit.points, m)
        assert ei.value.status == 2  # AMHIP_ERR_EXACT_HIT
        m.synchronize()              # the sticky status is cleared by the failing call
        m.reset()
        _dsm(clean, m).process(clean.points, m)
        got = m.get("elevation")
    R.assert_capped_equal(got, want, r, "g k=%d %s" % (k, kernel))


# ---- h ----------------------------------------------------------------------------------------
H_CALLS = [(True, 0), (True, 4), (False, 8), (False, 0), (True, 2)]      # (exact mode, k)


@pytest.mark.parametrize("kernel", KERNELS)
def test_h_earlier_content_and_mode_switches_on_one_context(tuning, kernel):
    from test_gpu_dsm_fast import _check as fast_check
    A = _A()
    tuning(p3_min_points=1000)
    _select(tuning, kernel)
    base = R.h_base()
    want = base.copy()
    reached = np.zeros(base.shape, bool)
    with A.AerialGridMap(_settings(R.family_h(0).grid)) as m:
        m.set("elevation", base)
        prev = base
        for call, (exact, k) in enumerate(H_CALLS):
            fam = R.family_h(call)
            touched = fam.search().size > 0
            reached |= touched
            if k:
                r = fam.cap(k)
                assert not r.ambiguous.any()
                rc, want = fam.oracle(k, elevation=want)
            else:
                rc, want, _ = O.dsm_process(fam.points, fam.grid, fam.radius_sq, 0.0, 0.0, elevation=want.copy())
            assert rc == O.OK
            m.set_dsm_precision(exact)
            m.set_dsm_knn(k)
            _dsm(fam, m).process(fam.points, m)
            got = m.get("elevation")
            if call == 0:
                assert m.dsm_stats()["sort_pipeline"] in ("count", "runs")      # the three-pass sort
            what = "call %d (%s, k=%d, %s)" % (call + 1, "exact" if exact else "fast", k, kernel)
            # what the call does not reach stays as it was, in bits
            assert np.array_equal(got[~touched].view(np.uint32), prev[~touched].view(np.uint32)), what
            assert not np.isnan(got).any()
            if k:       # capped: held to bits
                assert np.array_equal(got[touched].view(np.uint32), want[touched].view(np.uint32)), what
            else:
                comp = np.where(touched, got, want)
                if exact:
                    S.assert_dsm_close(comp, want, tol=1e-6)
                else:
                    fast_check(comp, want)
            prev = got
    assert (~reached).any() and np.array_equal(prev[~reached].view(np.uint32), base[~reached].view(np.uint32))


# ---- i ----------------------------------------------------------------------------------------
def _timed_capped_call(fam, k, exact):
    A = _A()
    with A.AerialGridMap(_settings(fam.grid)) as m:
        m.enable_timing()
        m.set_dsm_precision(exact)
        m.set_dsm_knn(k)
        m.timing_reset()
        _dsm(fam, m).process(fam.points, m)
        got = m.get("elevation")
        launches = {name: n for name, (ms, n) in m.kernel_times().items() if n}
        st = m.dsm_gather_stats()
        st["sort_pipeline"] = m.dsm_stats()["sort_pipeline"]      # ("count": the record sort's; "runs": doubles)
    return got, launches, st


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene,k", [("a", 1), ("a", 4), ("a", 8), ("rough", 8)])
def test_i_fast_mode_under_the_cap_is_the_fp64_pipeline(tuning, scene, k, kernel):
    """set_dsm_precision(False) with a cap: the capped gathers read sorted doubles and nothing else,
    so the call sorts doubles (no 16-byte records, no bin ranges) -- the same launches and the same
    bits as in exact mode."""
    fam = R.family_a() if scene == "a" else R.family_h(2)
    if scene == "rough":
        tuning(p3_min_points=1000)
    _select(tuning, kernel)
    r = fam.cap(k)
    assert not r.ambiguous.any()
    rc, want = fam.oracle(k)
    assert rc == O.OK
    fast, launches_fast, st_fast = _timed_capped_call(fam, k, False)
    exact, launches_exact, st_exact = _timed_capped_call(fam, k, True)
    R.assert_capped_equal(fast, want, r, "fast %s k=%d %s" % (scene, k, kernel))
    assert np.array_equal(fast.view(np.uint32), exact.view(np.uint32))
    assert launches_fast == launches_exact and "k_dsm_gather" in launches_fast, (launches_fast, launches_exact)
    assert st_fast == st_exact
    assert (st_fast["sort_pipeline"] == "one-level") == (scene == "a"), st_fast


# ---- j ----------------------------------------------------------------------------------------
def test_j_sub_window_under_the_cap(tuning):
    A = _A()
    fam = R.family_j()
    g = fam.grid
    base = np.random.default_rng(78).uniform(300.0, 310.0, (g.cols, g.rows)).astype(np.float32)
    r = fam.cap(4)
    assert not r.ambiguous.any()
    rc, want = fam.oracle(4, elevation=base)
    assert rc == O.OK
    outs = {}
    for sub in (True, False):
        tuning(dsm_no_subwindow=None if sub else 1)
        with A.AerialGridMap(_settings(g)) as m:
            m.set("elevation", base)               # a materialized layer with earlier content
            m.set_dsm_knn(4)
            _dsm(fam, m).process(fam.points, m)
            outs[sub] = m.get("elevation")
    assert np.array_equal(outs[True].view(np.uint32), outs[False].view(np.uint32))
    R.assert_capped_equal(outs[True], want, r, "j")
    changed = outs[True] != base
    assert 0.0005 < changed.mean() < 0.05 and not changed[~r.inside].any()


# ---- k ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_k_device_cloud_gives_the_bits_of_the_host_path(tuning, kernel):
    fam = R.family_a()
    host = _run(tuning, fam, 4, kernel)
    dev = _run(tuning, fam, 4, kernel, device=True)
    assert np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    R.assert_capped_equal(dev, fam.oracle(4)[1], fam.cap(4), "k device %s" % kernel)


def test_k_the_cap_is_dsm_dsms_only():
    """OrthoFromPcl shares the gather; the cap must not reach it."""
    A = _A()
    fam = R.family_a()
    inten = ((np.arange(fam.points.shape[0]) * 37) % 256).astype(np.int32)
    rc, want = O.ortho_from_pcl(fam.points, inten, fam.grid, 2, False)
    assert rc == O.OK
    outs = {}
    for k in (0, 4):
        with A.AerialGridMap(_settings(fam.grid)) as m:
            m.set_dsm_knn(k)
            A.OrthoFromPcl(A.OrthoFromPclSettings(interpolation_radius=2, use_adaptive_interpolation=False)).process(
                fam.points, inten, m)
            outs[k] = m.get("ortho")
    assert np.array_equal(outs[0].view(np.uint32), outs[4].view(np.uint32))
    assert np.abs(outs[4].astype(np.float64) - want).max() <= 1e-4
