"""CPU: the numpy restatement of the rectifier and the densifier (tests/stereo_front_reference.py)
against the oracle (oracle/amo_rectify.cc, amo_densify; and the reference's own rectifier.cpp /
densifier.cpp compiled over oracle/refkit where that was built), bit for bit, on the inputs of
tests/stereo_front_inputs.py and on the older ones -- and, from the restatement alone, that every
input reaches the branch it was built for."""
import numpy as np
import pytest

import oracle_ffi as O
import stereo_front_inputs as FI
import stereo_front_reference as FR
from test_gpu_densify import _case
from test_oracle_rectify import rig


def oracles():
    return ["port", "loops"] if O.have_loops() else ["port"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- densify ---------------------------------------------------------------------------------------
def check_densify(args):
    r = FR.densify_full(*args)
    for which in oracles():
        xyz, inten = O.densify(*args, which=which)
        assert xyz.shape == r["xyz"].shape, which
        assert np.array_equal(bits(xyz), bits(r["xyz"])), which
        assert np.array_equal(inten, r["intensity"]), which
    return r


@pytest.mark.parametrize("h,w,seed", [(48, 64, 1), (480, 752, 2), (333, 1021, 3)])
def test_densify_reference_on_the_older_inputs(h, w, seed):
    r = check_densify(_case(h, w, seed))
    assert r["xyz"].shape[0] > 0.5 * h * w


@pytest.mark.parametrize("W,H", FI.SHAPES)
def test_densify_reference_on_the_shapes(W, H):
    r = check_densify(FI.shape_case(W, H))
    assert r["keep"].shape == (H, W)
    if W * H > 4:
        assert 0 < r["xyz"].shape[0] < W * H


@pytest.mark.parametrize("W,H", FI.PATTERN_SIZES)
@pytest.mark.parametrize("name", FI.PATTERNS)
def test_densify_reference_on_the_validity_patterns(name, W, H):
    *args, valid = FI.pattern_case(name, W, H)
    r = check_densify(args)
    assert np.array_equal(r["keep"], valid)          # the pattern is what decides
    assert (name == "none") == (r["xyz"].shape[0] == 0)


@pytest.mark.parametrize("kind", FI.SPECIAL_KINDS)
def test_densify_reference_on_the_special_values(kind):
    args = FI.special_case(kind)
    r = check_densify(args)
    keep, disp = r["keep"], args[0]
    at = FI.SPECIAL_AT
    # which disparities pass `> 1.0f` (:60)
    for name in ("nan", "-inf", "-0", "1", "1-", "1e-30", "denormal"):
        assert not any(keep[v, u] for (v, u) in at[name]), name
    if kind == "plain":
        for name in ("+inf", "1+", "3e38"):
            assert all(keep[v, u] for (v, u) in at[name]), name
        # +inf: w = inf, the point is t itself
        n_before = int(keep.reshape(-1)[:at["+inf"][0][0] * FI.SW + at["+inf"][0][1]].sum())
        assert np.array_equal(r["xyz"][n_before], args[5])
    if kind in ("z_top", "z_bottom"):
        sign = 1.0 if kind == "z_top" else -1.0
        assert r["rejected_inf"] > 0
        assert disp[0, 47] == disp[0, 48] == disp[0, 49] == 2.0
        assert keep[0, 47] and keep[0, 48] and not keep[0, 49] and not keep[0, 50]
        z = r["xyz"][:, 2]
        assert (z == sign * FI.Z_BELOW).sum() > 0            # the largest double that rounds to FLT_MAX
        assert not (np.abs(z) >= FI.Z_TIE).any()             # the tie, the smallest that rounds to inf
        assert np.float32(sign * FI.Z_BELOW) == sign * np.finfo(np.float32).max
    if kind == "z_nan":
        assert r["nan_kept"] > 0 and r["rejected_inf"] > 0
        assert keep[0, 48] and not keep[0, 47] and not keep[0, 49]


@pytest.mark.parametrize("baseline", FI.BASELINES)
def test_densify_reference_on_the_baselines(baseline):
    disp, img, K, _, R, t = FI.special_case("plain")
    r = check_densify((disp, img, K, baseline, R, t))
    assert r["xyz"].shape[0] > 0


def test_point_cloud2_payload_of_the_reference():
    """densifier.cpp:53-106: pixel k in slot k + 1, slot 0 zero, the last pixel dropped."""
    disp, img, K, b, R, t = FI.special_case("plain")
    r = FR.densify_full(disp, img, K, b, R, t)
    pc2, keep = r["pc2"], r["keep"].reshape(-1)
    assert pc2.shape == (FI.SW * FI.SH, 4) and not pc2[0].any()
    assert keep[-1] and 0 < keep.sum() < keep.size
    body, k = pc2[1:], keep[:-1]
    assert (body[~k] == FR.INVALID).all()
    n = int(k.sum())
    assert n == r["xyz"].shape[0] - 1                        # the last pixel's point is not in the payload
    assert np.array_equal(body[k][:, :3], bits(r["xyz"][:n].astype(np.float32)))
    g = r["intensity"][:n].astype(np.uint32)
    assert np.array_equal(body[k][:, 3], (g << 16) | (g << 8) | g)


# ---- rectify ---------------------------------------------------------------------------------------
def check_rectify(args, want_rc=O.OK):
    r = FR.rectify_ref(*args)
    for which in oracles():
        rc, o = O.rectify_stereo_pair(*args, which=which)
        if which == "port":
            assert rc == want_rc
        assert o["baseline"] == r["baseline"], which
        assert np.array_equal(bits(o["R_G_C"]), bits(r["R_G_C"])), which
        if which == "loops" and want_rc != O.OK:
            continue          # (the reference's own loop stops at its CHECK)
        assert np.array_equal(bits(o["maps"]), bits(r["maps"])), which
        for n in ("left", "right", "mask"):
            assert np.array_equal(o[n], r[n]), (which, n)
    return r


@pytest.mark.parametrize("seed,W,H", [(11, 160, 120), (12, 752, 480), (13, 333, 211), (1, 208, 131), (7, 160, 120)])
def test_rectify_reference_on_the_older_rigs(seed, W, H):
    r = check_rectify(rig(seed, W=W, H=H))
    assert not r["zero_w"] and r["neg_decided"] == 0 and r["clamp_2_31"] == 0


_rigs = FI.rectify_rigs()


@pytest.mark.parametrize("name", sorted(_rigs))
def test_rectify_reference_on_the_new_rigs(name):
    args = _rigs[name]
    r = check_rectify(args)
    assert not r["zero_w"]
    H, W = args[5].shape
    if name == "identity":
        v, u = np.mgrid[0:H, 0:W].astype(np.float32)
        for k in (0, 2):
            assert np.array_equal(bits(r["maps"][k]), bits(u)) and np.array_equal(bits(r["maps"][k + 1]), bits(v))
        assert np.array_equal(r["left"], args[5]) and np.array_equal(r["right"], args[6])
        assert (r["mask"] == 255).all()
    if name.startswith("axis"):
        assert r["neg_decided"] > 0 and r["neg_decided"] == (r["mask"] == 255).sum()
    else:
        assert r["neg_decided"] == 0     # (a rotation about the centre keeps the corners' winding)
    if name == "axis far":
        assert r["wide_edges"] > 0 and max(abs(x) for (x, y) in r["corners"]) > 2 ** 20
    if name.startswith("base"):
        assert (r["left"] == 0).sum() > 0.05 * W * H      # the maps leave the image (inputs are >= 1)
        assert 0 < (r["mask"] == 255).sum() < W * H
    if name.startswith("yaw"):
        assert r["tap_left"] > 0 and r["tap_right"] > 0 and 0 < (r["mask"] == 255).sum() < W * H
        assert any(x < 0 or y < 0 or x >= W or y >= H for (x, y) in r["corners"])
    if name == "2^26":
        assert r["clamp_2_31"] > 0 and r["clamp_short"] > 0
        assert np.abs(r["maps"][2:]).max() > 2.0 ** 26


def test_every_reach_count_is_reached_by_some_rig():
    tot = {}
    for name, args in _rigs.items():
        r = FR.rectify_ref(*args)
        for k in ("neg_decided", "wide_edges", "tap_left", "tap_right", "clamp_short", "clamp_2_31"):
            tot[k] = tot.get(k, 0) + r[k]
    assert all(v > 0 for v in tot.values()), tot


def test_the_zero_w_rig():
    args = FI.zero_w_rig()
    assert set(np.unique(args[1])) <= {-1.0, 0.0, 1.0} and set(np.unique(args[2])) <= {-1.0, 0.0, 1.0}
    r = check_rectify(args, want_rc=O.ERR_EXACT_HIT)
    assert r["zero_w"] and r["zero_w_pixels"] == 160        # w2 == 0.0f along row 60
    w2_zero = ~np.isfinite(r["maps"][2]) | ~np.isfinite(r["maps"][3])
    assert w2_zero[60].all() and not w2_zero[:60].any() and not w2_zero[61:].any()


def test_the_zero_w_sequence_has_exact_poses_and_one_zero_w_pair():
    seq = FI.ZeroWSequence()
    Rs, ts = seq.camera_poses()
    assert np.array_equal(ts, seq.T_G_B[:, :3])
    for k in (0, 1, 2):
        assert np.array_equal(Rs[k], FI.NADIR)
    for k in (3, 4):
        assert np.array_equal(Rs[k], [[0, 1, 0], [0, 0, 1], [1, 0, 0]])
    # exactly the third pair: the pair behind it is a good one (w = 1 everywhere)
    zero = []
    for (i, j) in [(0, 1), (1, 2), (2, 3), (3, 4)]:
        args = (seq.K, Rs[i], Rs[j], ts[i], ts[j], seq.frames[i], seq.frames[j])
        z = (i, j) == (2, 3)
        r = check_rectify(args, want_rc=O.ERR_EXACT_HIT if z else O.OK)
        zero.append(r["zero_w"])
        if (i, j) == (3, 4):
            assert r["zero_w_pixels"] == 0 and np.isfinite(r["maps"]).all()
    assert zero == [False, False, True, False]
    good = FI.ZeroWSequence(turned=False)
    assert np.array_equal(good.frames, seq.frames)
    assert all(np.array_equal(R, FI.NADIR) for R in good.camera_poses()[0])
