"""The occlusion march of the true-ortho mosaic (amhip_ortho_occl.h: the function the kernel
calls) as a stand-alone program (tests/cpp/ortho_occl_host_main.cc) under the address and
undefined-behaviour sanitizers, compared query by query with the numpy statement of the rule
(tests/ortho_occlusion_reference.py).  No GPU, nothing loaded into python under a sanitizer.

Also here, without a GPU: the new entry points exist and refuse null arguments and bad margins."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as O
import ortho_occlusion_reference as R
import ortho_occlusion_scenes as S
from aerial_mapper_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ortho_occl_host") / "ortho_occl_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "aerial_mapper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ortho_occl_host_main.cc"), "-o", out])
    return out


def _hex(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == INF else "-inf" if v == -INF else v.hex())


def _run(exe, tmp_path, g, elevation, queries):
    """queries: (i, j, (tx, ty, tz), margin, zcut) -> list of bool"""
    path = str(tmp_path / "case.txt")
    with open(path, "w") as fh:
        fh.write("%d %d %s %d\n" % (g.rows, g.cols, _hex(g.resolution), len(queries)))
        fh.write(" ".join(_hex(v) for v in elevation.reshape(-1)) + "\n")   # (cols, rows) C order = i + j * rows
        for i, j, t, margin, zcut in queries:
            x, y = O.cell_position(g, i, j)
            fh.write(" ".join([str(i), str(j)] + [_hex(v) for v in (x, y, t[0], t[1], t[2], margin, zcut)]) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    out = r.stdout.split()
    assert len(out) == len(queries)
    return [v == "1" for v in out]


def _zmax(elevation):
    ok = ~np.isnan(elevation)
    return float(elevation[ok].max()) if ok.any() else -INF


def _check(exe, tmp_path, g, elevation, cells_cams_margins):
    """Every query twice: without the height cut-off and with the map's largest elevation as the
    cut-off -- the same answers, the rule's."""
    zmax = _zmax(elevation)
    queries, want, why = [], [], []
    for i, j, t, margin in cells_cams_margins:
        w = []
        want.append(R.occluded(elevation, g, i, j, t, margin, w))
        why.append(w)
        queries.append((i, j, t, margin, INF))
        queries.append((i, j, t, margin, zmax))
    got = _run(exe, tmp_path, g, elevation, queries)
    for k, (q, w) in enumerate(zip(cells_cams_margins, want)):
        assert got[2 * k] == w, ("no cut-off", q, why[k])
        assert got[2 * k + 1] == w, ("cut-off at %r" % zmax, q, why[k])
    return want, why


def _rough_map(rows, cols, seed, nan_frac=0.08):
    g = O.make_grid(rows * 0.5, cols * 0.5, 0.5, 100.25, -40.5)
    assert (g.rows, g.cols) == (rows, cols)
    rng = np.random.Generator(np.random.PCG64(seed))
    z = rng.uniform(0.0, 1.5, size=(cols, rows)).astype(np.float32)
    for _ in range(4):   # a few buildings
        i0, j0 = int(rng.integers(0, rows - 3)), int(rng.integers(0, cols - 3))
        z[j0:j0 + 3, i0:i0 + 3] = np.float32(rng.uniform(4.0, 15.0))
    z[rng.uniform(size=z.shape) < nan_frac] = np.nan
    return g, z, rng


def test_march_matches_the_rule_on_rough_terrain(exe, tmp_path):
    rows, cols = 23, 17
    g, z, rng = _rough_map(rows, cols, 3)
    x_lo, y_lo = O.cell_position(g, rows - 1, cols - 1)
    x_hi, y_hi = O.cell_position(g, 0, 0)
    cx, cy = 0.5 * (x_lo + x_hi), 0.5 * (y_lo + y_hi)
    cams = [(cx + 0.3, cy - 0.2, 30.0),                       # above the map
            (x_hi + 40.0, cy + 1.0, 6.0), (x_lo - 40.0, cy - 1.0, 6.0),    # outside the footprint, low: the
            (cx + 1.0, y_hi + 40.0, 6.0), (cx - 1.0, y_lo - 40.0, 6.0),    # rays leave through all four edges
            (x_hi + 15.0, y_lo - 22.0, 25.0),                  # beyond a corner
            (cx, cy, 0.75),                                    # below most of the surface: dz <= 0
            (cx + 2.0, cy + 2.0, -5.0)]
    todo = []
    for t in cams:
        for j in range(cols):
            for i in range(rows):
                todo.append((i, j, t, 0.0 if (i + j) % 3 else 0.1))
    want, why = _check(exe, tmp_path, g, z, todo)
    reasons = set(w[0] for w in why)
    assert {"nan", "below", "hit", "end", "i<0", "i>=rows", "j<0", "j>=cols"} <= reasons, reasons
    assert 50 < sum(want) < len(want) - 50
    # NaN samples were stepped over by marches that went on
    stepped = 0
    for (i, j, t, margin), w in zip(todo[:rows * cols], why[:rows * cols]):
        stepped += w[1] > 3
    assert stepped > 50 and np.isnan(z).sum() > 10


def test_cameras_next_to_the_cell_margins_and_degenerate_maps(exe, tmp_path):
    rows, cols = 9, 7
    g, z, rng = _rough_map(rows, cols, 8, nan_frac=0.0)
    z[3, 4] = 0.5
    z[3, 5] = 40.0     # a wall next to cell (4, 3)
    z[2, 4] = np.nan
    x, y = O.cell_position(g, 4, 3)
    res = g.resolution
    todo = []
    # m <= 1: the camera's centre within one cell of the cell's -- no step, whatever stands next to it
    for dx, dy in [(0.0, 0.0), (res, 0.0), (-res, res), (0.999 * res, -0.5 * res), (-res, -res)]:
        todo.append((4, 3, (x + dx, y + dy, 50.0), 0.0))
    # just beyond one cell: one step, one sample (the camera stands over it: nothing reaches the ray)
    todo.append((4, 3, (x - 1.001 * res, y, 50.0), 0.0))
    todo.append((4, 3, (x + 1.001 * res, y, 50.0), 0.0))
    # margins: +inf never occludes, a large one does not either, 0 does
    for margin in (INF, 1e3, 39.0, 0.0):
        todo.append((4, 3, (x - 6.0, y, 3.0), margin))
    # dz == 0 exactly, dz < 0, a camera at the cell's own height plus one ulp
    todo.append((4, 3, (x - 6.0, y, 0.5), 0.0))
    todo.append((4, 3, (x - 6.0, y, 0.25), 0.0))
    todo.append((4, 3, (x - 6.0, y, float(np.nextafter(0.5, 1.0))), 0.0))
    # the NaN cell itself; cameras that are not finite make no step
    todo.append((4, 2, (x - 6.0, y, 30.0), 0.0))
    want, why = _check(exe, tmp_path, g, z, todo)
    assert want[:5] == [False] * 5 and all(w == ["end", 0] for w in why[:5])
    assert want[5:7] == [False, False] and why[5] == ["end", 1] and why[6] == ["end", 1]
    assert want[7:11] == [False, False, True, True]
    assert want[11:13] == [False, False] and why[11][0] == why[12][0] == "below"
    assert why[14][0] == "nan"
    # (not in the rule's numpy statement: int(rint(nan)) has no value there)
    bad = [(4, 3, (INF, y, 30.0), 0.0, INF), (4, 3, (x, float("nan"), 30.0), 0.0, INF),
           (4, 3, (-INF, INF, 30.0), 0.0, INF)]
    assert _run(exe, tmp_path, g, z, bad) == [False, False, False]
    # an infinitely high camera is the rule's: z = h + s * inf lies above every sample
    want, why = _check(exe, tmp_path, g, z, [(4, 3, (x - 6.0, y, INF), 0.0)])
    assert want == [False] and why[0] == ["i>=rows", 4]
    # a 1 x 1 map: the first step leaves it
    g1 = O.make_grid(0.5, 0.5, 0.5)
    assert (g1.rows, g1.cols) == (1, 1)
    z1 = np.array([[2.0]], np.float32)
    x1, y1 = O.cell_position(g1, 0, 0)
    todo = [(0, 0, (x1 + 30.0, y1 - 20.0, 10.0), 0.0), (0, 0, (x1, y1, 10.0), 0.0), (0, 0, (x1, y1 + 0.7, 1.0), 0.0)]
    want, why = _check(exe, tmp_path, g1, z1, todo)
    assert want == [False, False, False] and why[0][0] in ("i<0", "j>=cols") and why[0][1] == 0
    # all NaN: nothing to march from
    zn = np.full((cols, rows), np.nan, np.float32)
    want, why = _check(exe, tmp_path, g, zn, [(i, 3, (x - 6.0, y, 3.0), 0.0) for i in range(rows)])
    assert not any(want)


def test_half_way_steps_round_to_even_and_the_comparison_is_strict(exe, tmp_path):
    """The numbers of tests/ortho_occlusion_scenes.py: s * dj = k / 2, z = k, all exact."""
    g = S.grid()
    t = S.exact_pose()[0, 0:3]
    above = float(np.nextafter(np.float32(3.25), np.float32(10.0)))
    cases = [(3, 2, 3.25, False), (3, 2, above, True),            # == z + margin: not occluded
             (5, 2, 6.0, True), (5, 3, 6.0, False),               # 2.5 -> 2
             (1, 0, 2.0, True), (1, 1, 2.0, False),               # 0.5 -> 0
             (7, 4, 8.0, True), (7, 3, 8.0, False)]               # 3.5 -> 4
    for k, dj, height, occl in cases:
        z = S.exact_elevation(k, dj, height)
        want, why = _check(exe, tmp_path, g, z, [(S.I0, S.J0, t, S.EXACT_MARGIN)])
        assert want == [occl], (k, dj, height, why)


# ---- the block scene of the GPU tests, on the reference alone ---------------------------------
def test_block_scene_reference_is_not_vacuous():
    """On the reference alone: the occlusion term changes the mosaic where it should."""
    want, plain = S.expected("block"), S.expected("block", margin=None)
    a, b = want["observation_index"], plain["observation_index"]
    differs = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert differs.sum() >= 50
    assert not differs[S.BLOCK_J, S.BLOCK_I].any()
    one, one_plain = S.expected("oblique"), S.expected("oblique", margin=None)
    stay = np.isnan(one["observation_index"]) & ~np.isnan(one_plain["observation_index"])
    assert stay.sum() >= 10
    for n in R.LAYERS:   # ... in their initial state, all layers
        init = O.new_layers(S.grid())[n]
        assert np.array_equal(one[n][stay], init[stay], equal_nan=True), n
    T = O.compose_T_G_C(S.block_poses(), synth.IDENTITY_POSE)
    for f in range(2):
        mask = R.occlusion_mask(S.block_elevation(), S.grid(), T[f, 0:3], S.MARGIN)
        assert mask.sum() >= 50 and not mask[S.BLOCK_J, S.BLOCK_I].any()     # no roof cell
        # flat terrain with +-0.05 m of noise occludes nothing at margin 0
        assert not R.occlusion_mask(S.flat_noisy(), S.grid(), T[f, 0:3], 0.0).any()


# ---- the C ABI, without a GPU ----------------------------------------------------------------
def test_new_exports_exist_and_refuse_bad_arguments(hip_built):
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    names = ["amhip_ortho_backward_process_occl_dev", "amhip_ortho_backward_process_occl",
             "amhip_session_ortho_backward_process_occl"]
    for n in names:
        assert n in L.EXPORTS and hasattr(lib, n)
    assert lib.amhip_abi_version() == 2
    cam = L.Camera()
    cam.fu = cam.fv = 70.0
    cam.cu, cam.cv, cam.width, cam.height = 47.5, 26.5, 96, 54
    T = np.array([0.0, 0.0, 60.0, 0.0, 1.0, 0.0, 0.0])
    f64p = C.POINTER(C.c_double)
    Tp = T.ctypes.data_as(f64p)
    ptrs = (C.c_void_p * 1)()
    steps = (C.c_size_t * 1)(96)
    for margin in (0.0, -1.0, float("nan"), INF):
        assert lib.amhip_ortho_backward_process_occl_dev(None, C.byref(cam), Tp, 1, None, 96 * 54, 96, 1, 0,
                                                         margin) == L.ERR_ARG
        assert L.last_error()
        assert lib.amhip_ortho_backward_process_occl(None, C.byref(cam), Tp, 1, ptrs, steps, 1, 0, None, None,
                                                     None, None, None, None, margin) == L.ERR_ARG
        assert lib.amhip_session_ortho_backward_process_occl(None, C.byref(cam), Tp, 1, ptrs, steps, 1, 0, None,
                                                             None, None, None, None, None, margin) == L.ERR_ARG
    # the Python switch: off by default, last in the signature
    import aerial_mapper_amd as A
    s = A.OrthoSettings()
    assert s.occlusion_test is False and s.occlusion_margin_m == 0.0
    s = A.OrthoSettings(True, True, "", 0.0, True, False, True, True, 0.25)
    assert s.occlusion_test is True and s.occlusion_margin_m == 0.25
