"""The occlusion-tested backward-grid mosaic ("true ortho") in plain
numpy and Python: the expected result of tests/test_gpu_ortho_occlusion.py.

Per (cell, frame) pair the keypoint, the view angle and the projection status come from the CPU
oracle (oracle_ffi.project_probe: bit for bit the reference's arithmetic); the march and the fold
are written out here.  Loops over cells x frames: for maps of a few thousand cells.

Layers as everywhere in the tests: float32 arrays of shape (cols, rows), a[j, i] = layer(i, j).
"""
import math

import numpy as np

import oracle_ffi as O

LAYERS = ["elevation_angle", "observation_index", "num_observations", "ortho", "colored_ortho"]
POINT_BEHIND_CAMERA, PROJECTION_INVALID = 2, 3


def occluded(elevation, g, i, j, centre, margin, why=None):
    """The rule: FP64, every operation rounded on its own (Python floats), in this order.
    why: a list that receives how the march ended ("nan", "below", "hit", "end", or the edge the
    ray left the map through: "i<0", "i>=rows", "j<0", "j>=cols") and the number of samples read."""
    def done(result, reason, samples):
        if why is not None:
            why[:] = [reason, samples]
        return result
    rows, cols = g.rows, g.cols
    h = float(elevation[j, i])
    if h != h:
        return done(False, "nan", 0)
    x_c, y_c = O.cell_position(g, i, j)
    tx, ty, tz = float(centre[0]), float(centre[1]), float(centre[2])
    res = float(g.resolution)
    di = (x_c - tx) / res
    dj = (y_c - ty) / res
    m = max(abs(di), abs(dj))
    dz = tz - h
    if not dz > 0.0:
        return done(False, "below", 0)
    k = 1
    while float(k) < m:
        s = float(k) / m
        ii = i + int(np.rint(s * di))
        jj = j + int(np.rint(s * dj))
        if not (0 <= ii < rows and 0 <= jj < cols):
            return done(False, "i<0" if ii < 0 else "i>=rows" if ii >= rows else "j<0" if jj < 0 else "j>=cols",
                        k - 1)
        z = h + s * dz
        if float(elevation[jj, ii]) > z + margin:
            return done(True, "hit", k)
        k += 1
    return done(False, "end", k - 1)


def occlusion_mask(elevation, g, centre, margin):
    """(cols, rows) bool: occluded(i, j) for one camera."""
    out = np.zeros((g.cols, g.rows), bool)
    for j in range(g.cols):
        for i in range(g.rows):
            out[j, i] = occluded(elevation, g, i, j, centre, margin)
    return out


def _round_half_away(x):
    """std::round for x >= 0 (a visible keypoint): x - floor(x) is exact."""
    fl = math.floor(x)
    return int(fl) + (1 if x - fl >= 0.5 else 0)


def _pixel(cam, image, u, v, colored):
    kp_y = min(_round_half_away(v), cam.height - 1)
    kp_x = min(_round_half_away(u), cam.width - 1)
    if colored:
        b, gr, r = (int(c) for c in image[kp_y, kp_x])
        return O.color_value_bgr(b, gr, r)
    return np.float32(image[kp_y, kp_x])


def process(g, cam, T_G_B, T_C_B, images, layers, colored=False, margin=None):
    """ortho::OrthoBackwardGrid::process with visible = in_box and z > 1e-10 and not occluded.
    margin None: the reference's rule (no occlusion term).  `layers` is updated in place.
    Returns the number of marches a lazy evaluation makes (pairs otherwise visible whose angle
    would be accepted)."""
    T_G_C = O.compose_T_G_C(T_G_B, T_C_B)
    elev = layers["elevation"]
    angle, index, nobs = layers["elevation_angle"], layers["observation_index"], layers["num_observations"]
    out = layers["colored_ortho" if colored else "ortho"]
    marches = 0
    for j in range(g.cols):
        for i in range(g.rows):
            x, y = O.cell_position(g, i, j)
            landmark = (x, y, float(elev[j, i]))
            for f in range(T_G_C.shape[0]):
                pr = O.project_probe(cam, T_G_C[f], landmark)
                u, v = pr["u"], pr["v"]
                visible = u >= 0.0 and v >= 0.0 and u < float(cam.width) and v < float(cam.height) and \
                    pr["status"] not in (POINT_BEHIND_CAMERA, PROJECTION_INVALID)
                if not visible:
                    continue
                alpha = pr["alpha"]
                assert alpha > 0.0  # CHECK(alpha > 0.0)
                # (occluded pairs and losing pairs leave the fold alone: asked in this order the
                # result is the same as with the march in front)
                if not abs(alpha) > float(angle[j, i]):
                    continue
                if margin is not None:
                    marches += 1
                    if occluded(elev, g, i, j, T_G_C[f, 0:3], margin):
                        continue
                angle[j, i] = np.float32(abs(alpha))
                index[j, i] = np.float32(f)
                nobs[j, i] = nobs[j, i] + nobs[j, i]
                out[j, i] = _pixel(cam, images[f], u, v, colored)
    return marches


def look_at_pose(eye, target, yaw=0.0):
    """T_G_C (tx, ty, tz, qw, qx, qy, qz) of a pinhole camera (z forward) at `eye` whose optical
    axis passes through `target`; `yaw` turns it about that axis."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    a = np.array([math.cos(yaw), math.sin(yaw), 0.0])
    x = a - z * np.dot(a, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)  # columns: the camera's axes in the map frame
    # rotation matrix -> quaternion (Shepperd)
    t = np.trace(R)
    if t > 0.0:
        s = math.sqrt(t + 1.0) * 2.0
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        k = int(np.argmax(np.diag(R)))
        a, b = (k + 1) % 3, (k + 2) % 3
        s = math.sqrt(1.0 + R[k, k] - R[a, a] - R[b, b]) * 2.0
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (R[b, a] - R[a, b]) / s
        q[1 + k] = 0.25 * s
        q[1 + a] = (R[a, k] + R[k, a]) / s
        q[1 + b] = (R[b, k] + R[k, b]) / s
    return np.array(list(eye) + q, np.float64)
