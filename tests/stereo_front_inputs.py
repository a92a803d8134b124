"""Inputs for the rectifier and the densifier at their edges (tests/test_stereo_front_reference.py
shows on the CPU that each one reaches what it is for; tests/test_gpu_densify.py,
tests/test_gpu_rectify.py and tests/test_gpu_stereo_sequence.py hold the GPU to the same bits)."""
import numpy as np

import stereo_sequence as SS
from test_oracle_rectify import rig

F32 = np.float32

# ================================ densify ==========================================================
INVALID_CYCLE = np.array([0.0, 1.0, -1.0, 0.5], F32)


def pose(seed, t=(12.5, -40.0, 430.0)):
    q = np.random.default_rng(seed).normal(size=4)
    qw, qx, qy, qz = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return R, np.array(t, np.float64)


def intrinsics(W, H):
    return np.array([[520.0, 0, (W - 1) / 2.0], [0, 531.0, (H - 1) / 2.0], [0, 0, 1]])


def ramp(W, H):
    """The intensity image lin % 251: a point in the wrong slot shows in the intensity too."""
    return (np.arange(W * H) % 251).astype(np.uint8).reshape(H, W)


# W x H: fewer than one thread's four pixels; the edges of one 1024-pixel block; 256, 257 and 513
# blocks (the chunk edges of the one-block scan of the block counts and its carry)
SHAPES = [(1, 1), (1, 5), (5, 1), (4, 1), (1023, 1), (1024, 1), (1025, 1), (64, 16), (257, 4),
          (512, 512), (5, 52429), (1024, 513)]


def shape_case(W, H):
    """About 80 % valid pixels, uniform disparities (the family of tests/test_gpu_densify.py)."""
    rng = np.random.default_rng(1000 * W + H)
    disp = rng.uniform(1.5, 80.0, (H, W)).astype(F32)
    bad = rng.random((H, W)) < 0.2
    disp[bad] = INVALID_CYCLE[rng.integers(0, 4, int(bad.sum()))]
    R, t = pose(W + H)
    return disp, ramp(W, H), intrinsics(W, H), 0.83, R, t


PATTERNS = ["all", "none", "last", "first", "one_per_block", "mod4_3", "mod4_0", "waves",
            "checker", "random_1", "random_99"]
PATTERN_SIZES = [(5, 52429), (333, 211), (1025, 1)]


def pattern_valid(name, W, H):
    n = W * H
    lin = np.arange(n)
    if name == "all":
        v = np.ones(n, bool)
    elif name == "none":
        v = np.zeros(n, bool)
    elif name == "last":
        v = lin == n - 1
    elif name == "first":
        v = lin == 0
    elif name == "one_per_block":        # block b's only point at offset b % 1024
        v = (lin % 1024) == ((lin // 1024) % 1024)
    elif name == "mod4_3":               # the last / the first of a thread's four pixels
        v = lin % 4 == 3
    elif name == "mod4_0":
        v = lin % 4 == 0
    elif name == "waves":                # 256 pixels = one 64-lane wave's share of a block
        v = (lin // 256) % 2 == 1
    elif name == "checker":
        v = ((lin // W) + (lin % W)) % 2 == 0
    elif name == "random_1":
        v = np.random.default_rng(7).random(n) < 0.01
    elif name == "random_99":
        v = np.random.default_rng(8).random(n) < 0.99
    else:
        raise KeyError(name)
    return v.reshape(H, W)


def pattern_case(name, W, H):
    valid = pattern_valid(name, W, H)
    lin = np.arange(W * H).reshape(H, W)
    disp = np.where(valid, F32(2.0) + (lin % 61).astype(F32) * F32(0.25), INVALID_CYCLE[lin % 4]).astype(F32)
    R, t = pose(11)
    return disp, ramp(W, H), intrinsics(W, H), 0.83, R, t, valid


# ---- special values, 96 x 80 ----------------------------------------------------------------------
SW, SH = 96, 80
ONE = F32(1.0)
SPECIALS = [("nan", F32(np.nan)), ("+inf", F32(np.inf)), ("-inf", F32(-np.inf)), ("-0", F32(-0.0)),
            ("1", ONE), ("1+", np.nextafter(ONE, F32(2.0))), ("1-", np.nextafter(ONE, F32(0.0))),
            ("1e-30", F32(1e-30)), ("3e38", F32(3e38)), ("denormal", F32(1e-41))]
SPECIAL_AT = {}
for _i, (_n, _) in enumerate(SPECIALS):
    SPECIAL_AT[_n] = [(5 + 7 * _i, 3 + 9 * _i), (70 - 6 * _i, 90 - 8 * _i)]

# float32 rounding at the top: FLT_MAX = (2 - 2^-23) 2^127; the tie (2 - 2^-24) 2^127 goes to the
# even neighbour, which is +inf; one double below it still rounds to FLT_MAX
Z_TIE = (2.0 - 2.0 ** -24) * 2.0 ** 127
Z_BELOW = float(np.nextafter(Z_TIE, 0.0))
with np.errstate(over="ignore"):
    assert np.isinf(F32(Z_TIE)) and F32(Z_BELOW) == np.finfo(F32).max and Z_TIE - Z_BELOW == 2.0 ** 75


def special_map():
    """Rows 0 .. 39 hold disparity 2 (w = 2 with baseline 1: exact quotients), rows 40 .. 79 uniform
    ones; the special values sit at SPECIAL_AT."""
    rng = np.random.default_rng(5)
    disp = np.full((SH, SW), 2.0, F32)
    disp[40:] = rng.uniform(0.0, 80.0, (40, SW)).astype(F32)
    for name, val in SPECIALS:
        for (v, u) in SPECIAL_AT[name]:
            disp[v, u] = val
    return disp


SPECIAL_KINDS = ["plain", "z_top", "z_bottom", "z_nan"]


def special_case(kind):
    """K has an integer principal point (48, 40) and fx = fy = 512, baseline 1.
    z_top:    R's third row (2^76, 0, 0), t_z = Z_BELOW: where d = 2, z = Z_BELOW + (u - 48) 2^75 -- the
              largest double that rounds to FLT_MAX at u = 48, the smallest that rounds to +inf at 49;
    z_bottom: the mirror image;
    z_nan:    R's third row (inf, 0, 0): z = inf * 0 = NaN in column 48 (kept), +-inf beside it."""
    K = np.array([[512.0, 0, 48.0], [0, 512.0, 40.0], [0, 0, 1]])
    R, t = pose(21)
    if kind == "z_top":
        R[2], t[2] = (2.0 ** 76, 0.0, 0.0), Z_BELOW
    elif kind == "z_bottom":
        R[2], t[2] = (-2.0 ** 76, 0.0, 0.0), -Z_BELOW
    elif kind == "z_nan":
        R[2] = (np.inf, 0.0, 0.0)
    else:
        assert kind == "plain"
    return special_map(), ramp(SW, SH), K, 1.0, R, t


BASELINES = [-0.83, 1e-300, 1e300]


# ================================ rectify ==========================================================
NADIR = np.diag([1.0, -1.0, -1.0])
K_EXACT = np.array([[128.0, 0.0, 80.0], [0.0, 128.0, 60.0], [0.0, 0.0, 1.0]])   # dyadic f, integer principal point
T_LEFT = np.array([10.0, -4.0, 80.0])
# the second camera turned by 90 degrees about the rectified x axis: its z axis is the rectified y
# axis, w2 is a multiple of (v - 60) and exactly 0.0f along row 60
R_TURNED = NADIR @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
# the same from a unit quaternion whose rotation matrix is exact: (w, x, y, z) = (-1/2, 1/2, 1/2, 1/2)
Q_TURNED = np.array([-0.5, 0.5, 0.5, 0.5])
Q_NADIR = np.array([0.0, 1.0, 0.0, 0.0])

# the pitch of camera 2 of rig(36) at which one pixel's w2 is so small (3e-7) that its map passes
# 2^26 (5.3e8) while no w is zero: found by scanning pi / 2 - 0.35 .. pi / 2 + 0.35 in steps of 1e-4
# with stereo_front_reference.rectify_plan on the CPU
PITCH_2_26 = 1.9095963267948206


def images(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    left = ((np.sin(xx * 0.21) + np.cos(yy * 0.17)) * 60 + 128 + rng.integers(-9, 9, (H, W))).clip(1, 255)
    right = ((np.sin(xx * 0.19 + 1.0) + np.cos(yy * 0.23)) * 60 + 128 + rng.integers(-9, 9, (H, W))).clip(1, 255)
    return left.astype(np.uint8), right.astype(np.uint8)


def exact_rig(R2=NADIR, base=(6.0, 0.0, 0.0), W=160, H=120):
    left, right = images(W, H, 3)
    return K_EXACT.copy(), NADIR.copy(), np.array(R2, np.float64), T_LEFT.copy(), T_LEFT + np.array(base), left, right


SIZES = [(1, 1), (3, 2), (63, 3), (64, 4), (65, 5), (129, 7)]


def rectify_rigs():
    """name -> (K, R1, R2, t1, t2, left, right)."""
    rigs = {
        "identity": exact_rig(),
        "base -x": rig(31, base=(-6.0, 0.7, -0.4)),
        "base +y": rig(32, base=(0.5, 6.0, 0.3)),
        "base -y": rig(33, base=(-0.4, -6.0, 0.2)),
        "yaw +0.6": rig(34, yaw=0.6, noise=0.3),
        "yaw -0.6": rig(35, yaw=-0.6, noise=0.3),
        "2^26": rig(36, pitch2=PITCH_2_26),
        # A rectification turns the camera about its centre, so the projected corners keep the winding
        # of the image corners -- whichever way the baseline points ACROSS the optical axis -- unless
        # the vanishing line of the rectified plane cuts the image: a baseline mostly ALONG the
        # optical axis.  These two are wound the other way (the mask's all-non-positive branch); in
        # the second the line passes 1e-5 of the image beside a corner, which lands 3e7 pixels away
        # (edge functions of 1e10: the 64-bit arithmetic)
        "axis": rig(37, base=(2.0, 1.0, 6.0)),
        "axis far": rig(37, base=(3.550391, 1.0, 6.0)),
    }
    for (W, H) in SIZES:
        rigs["%dx%d" % (W, H)] = rig(40 + W, W=W, H=H, yaw=0.1, noise=0.05)
    return rigs


def zero_w_rig():
    return exact_rig(R2=R_TURNED)


# ================================ the zero-w sequence ==============================================
class ZeroWSequence(object):
    """Five 160 x 120 frames along +x over the scene of tests/stereo_sequence.py, T_C_B the identity,
    every pose exact: frames 0, 1, 2 look straight down (Q_NADIR), frames 3 and 4 carry Q_TURNED.
    Pairs (0, 1) and (1, 2) are ordinary pairs with the identity rectification; pair (2, 3) is the
    zero-w pair, and the only one: pair (3, 4) has two parallel turned cameras, its rectification is
    a quarter turn of the image with w = 1 everywhere -- a good pair BEHIND the failing one, which
    only the stickiness of the error word keeps out of the cloud.  turned=False: all five look down.
    The interface tests/stereo_sequence.py's cpu_pair / cpu_chain expect."""

    def __init__(self, turned=True):
        F, W, H = 5, 160, 120
        self.F, self.W, self.H = F, W, H
        self.K = K_EXACT.copy()
        self.T_C_B = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        rng = np.random.default_rng(17)
        f = self.K[0, 0]
        span = 80.0 * max(W, H) / f + 40.0
        x0, y0 = 10.0 - span, -4.0 - span
        lattice = rng.uniform(-70.0, 70.0, (int(2 * span) + 4, int(2 * span + 6 * F) + 4))
        vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
        rays = np.stack([(uu - self.K[0, 2]) / f, (vv - self.K[1, 2]) / f, np.ones_like(uu)], -1) @ NADIR.T
        frames, T = [], []
        for i in range(F):
            t = np.array([10.0 + 6.0 * i, -4.0, 80.0])
            z = np.zeros((H, W))
            for _ in range(4):
                s = (z - t[2]) / rays[..., 2]
                z = SS.ground(t[0] + s * rays[..., 0], t[1] + s * rays[..., 1])
            s = (z - t[2]) / rays[..., 2]
            img = SS.texture(t[0] + s * rays[..., 0], t[1] + s * rays[..., 1], lattice, x0, y0)
            img = img + rng.integers(-3, 4, (H, W))
            frames.append(np.clip(np.rint(img), 1, 255).astype(np.uint8))
            q = Q_TURNED if (turned and i >= 3) else Q_NADIR
            T.append(np.concatenate([t, q]))
        self.frames = np.stack(frames)
        self.T_G_B = np.stack(T)

    def camera_poses(self):
        import oracle_ffi as O
        T_G_C = O.compose_T_G_C(self.T_G_B, self.T_C_B)
        return np.stack([SS.quat_to_matrix(p[3:]) for p in T_G_C]), T_G_C[:, :3].copy()
