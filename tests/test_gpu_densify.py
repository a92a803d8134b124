"""GPU: the densifier's disparity -> world-point reprojection
against the oracle, and the device-resident chain densify -> DSM -> OrthoFromPcl."""
import numpy as np
import pytest

import oracle_ffi as O
import stereo_front_inputs as FI
import stereo_front_reference as FR

pytestmark = pytest.mark.gpu


def _case(h, w, seed):
    rng = np.random.default_rng(seed)
    disp = rng.uniform(0.0, 80.0, (h, w)).astype(np.float32)
    disp[rng.random((h, w)) < 0.2] = rng.choice(np.array([0.0, 1.0, -1.0, 0.5], np.float32))
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    K = np.array([[520.0, 0, (w - 1) / 2.0], [0, 531.0, (h - 1) / 2.0], [0, 0, 1]])
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    qw, qx, qy, qz = q
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return disp, img, K, 0.83, R, np.array([12.5, -40.0, 430.0])


@pytest.mark.parametrize("h,w,seed", [(48, 64, 1), (480, 752, 2), (333, 1021, 3)])
def test_densify_matches_oracle_bitwise_in_raster_order(h, w, seed):
    import torch
    import aerial_mapper_amd as A
    disp, img, K, b, R, t = _case(h, w, seed)
    # directly against the reference's own densifier.cpp (compiled unchanged over oracle/refkit)
    # where it was built, and against the restatement
    want_p, want_i = O.densify(disp, img, K, b, R, t, which="loops" if O.have_loops() else "port")
    port_p, port_i = O.densify(disp, img, K, b, R, t)
    assert np.array_equal(port_p.view(np.uint64), want_p.view(np.uint64)) and np.array_equal(port_i, want_i)
    with A.AerialGridMap(A.GridMapSettings(0, 0, 8, 8, 1.0)) as m:
        got_p, got_i = A.densify(m, torch.from_numpy(disp).cuda(), torch.from_numpy(img).cuda(),
                                 K, b, R, t)
        got_p, got_i = got_p.cpu().numpy(), got_i.cpu().numpy()
    assert got_p.shape == want_p.shape and want_p.shape[0] > 0.5 * h * w
    assert np.array_equal(got_p.view(np.uint64), want_p.view(np.uint64))
    assert np.array_equal(got_i, want_i)


def test_densify_feeds_dsm_and_from_pcl_without_leaving_hbm():
    import torch
    import aerial_mapper_amd as A
    h, w = 240, 320
    rng = np.random.default_rng(9)
    disp = rng.uniform(30.0, 34.0, (h, w)).astype(np.float32)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    K = np.array([[300.0, 0, (w - 1) / 2.0], [0, 300.0, (h - 1) / 2.0], [0, 0, 1]])
    R = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])  # looking down
    t = np.array([0.0, 0.0, 120.0])
    pts, inten = O.densify(disp, img, K, 10.0, R, t)  # z_r = 300*10/32 ~ 94 m below the camera
    g = O.make_grid(60.0, 44.0, 1.0)
    rc, want_elev, _ = O.dsm_process(pts, g)
    rc2, want_ortho = O.ortho_from_pcl(pts, inten, g, 2, False)
    assert rc == O.OK and rc2 == O.OK and (~np.isnan(want_elev)).mean() > 0.5
    with A.AerialGridMap(A.GridMapSettings(0, 0, 60.0, 44.0, 1.0)) as m:
        dp, di = A.densify(m, torch.from_numpy(disp).cuda(), torch.from_numpy(img).cuda(),
                           K, 10.0, R, t)
        A.Dsm(A.DsmSettings(), m).process(dp.contiguous(), m)
        A.OrthoFromPcl(A.OrthoFromPclSettings()).process(dp.contiguous(), di.contiguous(), m)
        elev, ortho = m.get("elevation"), m.get("ortho")
    ok = ~np.isnan(want_elev)
    assert np.array_equal(np.isnan(elev), ~ok)
    assert np.abs(elev[ok].astype(np.float64) - want_elev[ok]).max() <= 1e-4
    assert np.abs(ortho.astype(np.float64) - want_ortho).max() <= 1e-4


# ---- the edges: tests/stereo_front_inputs.py, against the numpy restatement and the oracle --------
@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0, 0, 8, 8, 1.0)) as m:
        yield m


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_gpu(gmap, args, disp_t=None, img_t=None):
    """A.densify on `args` == densify_ref == the oracle, bit for bit -> the reference's dict."""
    import torch
    import aerial_mapper_amd as A
    disp, img, K, b, R, t = args
    want = FR.densify_full(*args)
    port_p, port_i = O.densify(*args)
    assert np.array_equal(u64(port_p), u64(want["xyz"])) and np.array_equal(port_i, want["intensity"])
    disp_t = torch.from_numpy(disp).cuda() if disp_t is None else disp_t
    img_t = torch.from_numpy(img).cuda() if img_t is None else img_t
    got_p, got_i = A.densify(gmap, disp_t, img_t, K, b, R, t)
    got_p, got_i = got_p.cpu().numpy(), got_i.cpu().numpy()
    assert got_p.shape == want["xyz"].shape and got_i.shape == want["intensity"].shape
    assert np.array_equal(u64(got_p), u64(want["xyz"]))
    assert np.array_equal(got_i, want["intensity"])
    return want


@pytest.mark.parametrize("W,H", FI.SHAPES)
def test_densify_shapes_at_the_thread_block_and_scan_edges(gmap, W, H):
    check_gpu(gmap, FI.shape_case(W, H))


@pytest.mark.parametrize("W,H", FI.PATTERN_SIZES)
@pytest.mark.parametrize("name", FI.PATTERNS)
def test_densify_validity_patterns(gmap, name, W, H):
    *args, valid = FI.pattern_case(name, W, H)
    want = check_gpu(gmap, args)
    assert want["xyz"].shape[0] == valid.sum() and (name == "none") == (want["xyz"].shape[0] == 0)


@pytest.mark.parametrize("kind", FI.SPECIAL_KINDS)
def test_densify_special_values(gmap, kind):
    want = check_gpu(gmap, FI.special_case(kind))
    if kind != "plain":
        assert want["rejected_inf"] > 0
    if kind == "z_nan":
        assert want["nan_kept"] > 0


@pytest.mark.parametrize("baseline", FI.BASELINES)
def test_densify_baselines(gmap, baseline):
    disp, img, K, _, R, t = FI.special_case("plain")
    assert check_gpu(gmap, (disp, img, K, baseline, R, t))["xyz"].shape[0] > 0


def test_densify_refuses_a_zero_baseline(gmap):
    import torch
    import aerial_mapper_amd as A
    disp, img, K, _, R, t = FI.special_case("plain")
    with pytest.raises(A.AmhipError) as ei:
        A.densify(gmap, torch.from_numpy(disp).cuda(), torch.from_numpy(img).cuda(), K, 0.0, R, t)
    assert "CHECK_NE(baseline, 0.0)" in str(ei.value)


def test_densify_reads_padded_rows(gmap):
    """disp_step = 4 (W + 3), img_step = W + 5; the padding holds NaN / 255."""
    import torch
    W, H = 333, 211
    args = FI.pattern_case("random_99", W, H)[:6]
    wide_d = torch.full((H, W + 3), float("nan"), dtype=torch.float32, device="cuda")
    wide_i = torch.full((H, W + 5), 255, dtype=torch.uint8, device="cuda")
    wide_d[:, :W] = torch.from_numpy(args[0]).cuda()
    wide_i[:, :W] = torch.from_numpy(args[1]).cuda()
    d, i = wide_d[:, :W], wide_i[:, :W]
    assert d.stride(0) * 4 == 4 * (W + 3) and i.stride(0) == W + 5
    check_gpu(gmap, args, d, i)


@pytest.mark.parametrize("short_by", [7, None])
def test_densify_capacity_below_the_count(gmap, short_by):
    """capacity = count - 7 and capacity = 0: the count is still the true one, the first `capacity`
    points are the reference's, nothing at or behind `capacity` is written."""
    import ctypes as C
    import torch
    from aerial_mapper_amd import hip_lib as L
    W, H = 333, 211
    disp, img, K, b, R, t = FI.pattern_case("checker", W, H)[:6]
    want = FR.densify_full(disp, img, K, b, R, t)
    n = want["xyz"].shape[0]
    capacity = n - short_by if short_by else 0
    assert 0 <= capacity < n
    d, i = torch.from_numpy(disp).cuda(), torch.from_numpy(img).cuda()
    xyz = torch.full((W * H, 3), -12345.5, dtype=torch.float64, device="cuda")
    inten = torch.full((W * H,), -777, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    f64p = C.POINTER(C.c_double)
    Kc, Rc, tc = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (K, R, t))
    gmap.wait_for_torch(d)
    L.check(L.load().amhip_densify_dev(
        gmap.handle, C.c_void_p(d.data_ptr()), d.stride(0) * 4, C.c_void_p(i.data_ptr()), i.stride(0), W, H,
        Kc.ctypes.data_as(f64p), float(b), Rc.ctypes.data_as(f64p), tc.ctypes.data_as(f64p),
        C.c_void_p(xyz.data_ptr()), C.c_void_p(inten.data_ptr()), capacity, C.c_void_p(count.data_ptr())))
    gmap.synchronize()
    assert int(count.item()) == n
    xyz, inten = xyz.cpu().numpy(), inten.cpu().numpy()
    assert np.array_equal(u64(xyz[:capacity]), u64(want["xyz"][:capacity]))
    assert np.array_equal(inten[:capacity], want["intensity"][:capacity])
    assert (xyz[capacity:] == -12345.5).all() and (inten[capacity:] == -777).all()
