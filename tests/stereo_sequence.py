"""Input of the stereo::Stereo sequence tests: F nadir frames along a track over a textured height
field, with body poses and a NON-identity T_C_B, and the expected result from the CPU chain
(oracle rectifier -> bm_reference / sgbm_reference -> oracle densifier, concatenated).

The scene: ground z = 3 sin(0.05 x) cos(0.04 y); its gray value is bilinear value noise on a 1 m
lattice (+-70) + 25 sin(0.13 x) cos(0.11 y) + 128, plus integer sensor noise in [-3, 3] per frame.
Camera i sits at (10 + 6 i, -4 + N(0, 0.3), 80 + N(0, 0.3)) and looks down with small random tilts
and yaws (as rig() of tests/test_oracle_rectify.py builds its two cameras); every pixel's ray is
intersected with the ground by four fixed-point steps."""
import numpy as np

import bm_reference as B
import oracle_ffi as O
import sgbm_reference as R

T_C_B = np.array([0.12, -0.07, 0.05, 0.9987, 0.03, -0.025, 0.03])
T_C_B[3:] /= np.linalg.norm(T_C_B[3:])


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def quat_to_matrix(q):
    """Eigen::Quaterniond::toRotationMatrix for q = (w, x, y, z), operation for operation."""
    w, x, y, z = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def _matrix_to_quat(M):
    w = np.sqrt(max(0.0, 1.0 + M[0, 0] + M[1, 1] + M[2, 2])) / 2.0
    if w > 0.1:   # (a nadir camera is a half turn about x: w is near 0, the x branch is taken)
        q = np.array([w, (M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w),
                      (M[1, 0] - M[0, 1]) / (4 * w)])
    else:
        x = np.sqrt(max(0.0, 1.0 + M[0, 0] - M[1, 1] - M[2, 2])) / 2.0
        q = np.array([(M[2, 1] - M[1, 2]) / (4 * x), x, (M[0, 1] + M[1, 0]) / (4 * x),
                      (M[0, 2] + M[2, 0]) / (4 * x)])
    return q / np.linalg.norm(q)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def ground(x, y):
    return 3.0 * np.sin(0.05 * x) * np.cos(0.04 * y)


def _texture(x, y, lattice, x0, y0):
    fx, fy = x - x0, y - y0
    ix = np.clip(np.floor(fx).astype(np.int64), 0, lattice.shape[1] - 2)
    iy = np.clip(np.floor(fy).astype(np.int64), 0, lattice.shape[0] - 2)
    ax, ay = np.clip(fx - ix, 0.0, 1.0), np.clip(fy - iy, 0.0, 1.0)
    v = (lattice[iy, ix] * (1 - ax) * (1 - ay) + lattice[iy, ix + 1] * ax * (1 - ay) +
         lattice[iy + 1, ix] * (1 - ax) * ay + lattice[iy + 1, ix + 1] * ax * ay)
    return v + 25.0 * np.sin(0.13 * x) * np.cos(0.11 * y) + 128.0


texture = _texture       # (the scene's gray value, for other renderers of the same scene)


def distort(kind, d, x, y):
    """aslam's radtan (kind 1) / equidistant (kind 2) distortion of normalised coordinates."""
    if kind == 1:
        k1, k2, p1, p2 = d
        r2 = x * x + y * y
        rad = k1 * r2 + k2 * r2 * r2
        return (x + (x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)),
                y + (y * rad + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)))
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    th2 = th * th
    thd = th * (1.0 + d[0] * th2 + d[1] * th2 ** 2 + d[2] * th2 ** 3 + d[3] * th2 ** 4)
    sc = np.where(r > 1e-8, thd / np.maximum(r, 1e-300), 1.0)
    return x * sc, y * sc


class Sequence(object):
    """frames (F, H, W) uint8, T_G_B (F, 7), the camera matrix K, T_C_B.  distortion = (kind,
    (4 parameters)): the frames are rendered THROUGH that lens (every raw pixel's ray is the
    undistorted one, found by fixed-point iteration), so undistorting them gives pinhole images."""

    def __init__(self, F, W, H, seed=1, f=150.0, distortion=None):
        rng = np.random.default_rng(seed)
        self.F, self.W, self.H = F, W, H
        self.K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
        self.T_C_B = T_C_B.copy()
        span = 80.0 * max(W, H) / f + 40.0
        x0, y0 = 10.0 - span, -4.0 - span
        lattice = rng.uniform(-70.0, 70.0, (int(2 * span) + 4, int(2 * span + 6 * F) + 4))
        down = _rot(np.pi, 0.0, 0.0)
        vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
        xd, yd = (uu - self.K[0, 2]) / f, (vv - self.K[1, 2]) / f
        xn, yn = xd, yd
        if distortion is not None:
            for _ in range(60):                      # y <- y + (y_d - distort(y)): a contraction here
                ex, ey = distort(distortion[0], distortion[1], xn, yn)
                xn, yn = xn + (xd - ex), yn + (yd - ey)
            ex, ey = distort(distortion[0], distortion[1], xn, yn)
            assert max(np.abs(ex - xd).max(), np.abs(ey - yd).max()) < 1e-9
        rays_c = np.stack([xn, yn, np.ones_like(uu)], -1)
        frames, T_G_B = [], []
        # T_G_B = T_G_C * T_C_B
        q_cb = self.T_C_B[3:]
        for i in range(F):
            t = np.array([10.0 + 6.0 * i, -4.0 + rng.normal(0, 0.3), 80.0 + rng.normal(0, 0.3)])
            Rm = _rot(*rng.normal(0, 0.02, 3)) @ down @ _rot(0.0, 0.0, rng.normal(0, 0.03))
            rays = rays_c @ Rm.T
            z = np.zeros((H, W))
            for _ in range(4):
                s = (z - t[2]) / rays[..., 2]
                z = ground(t[0] + s * rays[..., 0], t[1] + s * rays[..., 1])
            s = (z - t[2]) / rays[..., 2]
            gx, gy = t[0] + s * rays[..., 0], t[1] + s * rays[..., 1]
            img = _texture(gx, gy, lattice, x0, y0) + rng.integers(-3, 4, (H, W))
            frames.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
            q_gc = _matrix_to_quat(Rm)
            q_gb = _qmul(q_gc, q_cb)
            t_gb = t + quat_to_matrix(q_gc) @ self.T_C_B[:3]
            T_G_B.append(np.concatenate([t_gb, q_gb / np.linalg.norm(q_gb)]))
        self.frames = np.stack(frames)
        self.T_G_B = np.stack(T_G_B)

    def camera_poses(self):
        """(R_G_C (F, 3, 3), t_G_C (F, 3)) as stereo.cpp:129-137 derives them from the body poses."""
        T_G_C = O.compose_T_G_C(self.T_G_B, self.T_C_B)
        return np.stack([quat_to_matrix(p[3:]) for p in T_G_C]), T_G_C[:, :3].copy()


def selected(F, nth):
    """stereo.cpp:91-93: frame i is used iff (i + 1) % nth == 0."""
    return [i for i in range(F) if (i + 1) % nth == 0]


def pairs_of(F, nth):
    used = selected(F, nth)
    return list(zip(used[:-1], used[1:]))


def cpu_pair(seq, i, j, use_bm, params=None, frames=None):
    """One pair through the CPU chain -> (xyz, intensities, dict of the intermediate results)."""
    frames = seq.frames if frames is None else frames
    Rs, ts = seq.camera_poses()
    rc, r = O.rectify_stereo_pair(seq.K, Rs[i], Rs[j], ts[i], ts[j], frames[i], frames[j])
    assert rc == O.OK
    if use_bm:
        disp, _ = B.restate(r["left"], r["right"], params or B.Params(), r["mask"])
    else:
        disp, _ = R.restate(r["left"], r["right"], params or R.Params(), r["mask"])
    xyz, inten = O.densify(disp, r["left"], seq.K, r["baseline"], r["R_G_C"], ts[i])
    r["disparity"] = disp
    r["t_G_C1"] = ts[i]
    return xyz, inten, r


_cache = {}


def cpu_chain(seq, pairs, use_bm, frames=None, key=None):
    """The expected sequence cloud: the pairs' clouds concatenated -> (xyz, intensities, [n per
    pair], last pair's intermediates).  Every pair must give more than 40 % of W * H points (the
    comparisons are never of empty clouds)."""
    if key is not None and key in _cache:
        return _cache[key]
    xs, is_, ns, last = [], [], [], None
    for (i, j) in pairs:
        x, it, last = cpu_pair(seq, i, j, use_bm, frames=frames)
        assert x.shape[0] > 0.4 * seq.W * seq.H, (i, j, x.shape[0] / float(seq.W * seq.H))
        xs.append(x)
        is_.append(it)
        ns.append(x.shape[0])
    if xs:
        out = (np.concatenate(xs), np.concatenate(is_), ns, last)
    else:
        out = (np.zeros((0, 3)), np.zeros(0, np.int32), ns, last)
    if key is not None:
        _cache[key] = out
    return out
