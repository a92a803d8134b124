"""The blended backward-grid mosaic in plain numpy and Python: the expected
result of tests/test_gpu_ortho_blend.py.

Per (cell, frame) pair the keypoint (u, v), the projection status, the view angle alpha and the
landmark in the camera frame C come from the CPU oracle (oracle_ffi.project_probe: bit for bit the
reference's arithmetic), the occlusion term from ortho_occlusion_reference.occluded; the weights,
the sums and the fold are written out here.  The pairs are probed once per scene (probe(), a Python
loop over cells x frames: maps of a few thousand cells); process() then runs over whole layers,
frame after frame -- numpy's elementwise float64 operations round every operation on its own, like
the rule.

Layers as everywhere in the tests: float32 arrays of shape (cols, rows), a[j, i] = layer(i, j).
"""
import numpy as np

import oracle_ffi as O
import ortho_occlusion_reference as R

LAYERS = R.LAYERS


def probe(g, cam, T_G_C, elevation, cells=None):
    """The pairs of a call: arrays of shape (F, cols, rows) -- u, v, alpha (float64), status (int),
    C (F, cols, rows, 3) -- and `visible`, the reference's rule.  cells: a (cols, rows) bool mask of
    the cells to evaluate (the others are never visible); None: all."""
    F = T_G_C.shape[0]
    shape = (F, g.cols, g.rows)
    out = dict(u=np.full(shape, np.nan), v=np.full(shape, np.nan), alpha=np.full(shape, np.nan),
               status=np.full(shape, R.PROJECTION_INVALID, np.int64), C=np.full(shape + (3,), np.nan))
    for j in range(g.cols):
        for i in range(g.rows):
            if cells is not None and not cells[j, i]:
                continue
            x, y = O.cell_position(g, i, j)
            landmark = (x, y, float(elevation[j, i]))
            for f in range(F):
                pr = O.project_probe(cam, T_G_C[f], landmark)
                out["u"][f, j, i], out["v"][f, j, i] = pr["u"], pr["v"]
                out["alpha"][f, j, i], out["status"][f, j, i] = pr["alpha"], pr["status"]
                out["C"][f, j, i] = pr["C"]
    u, v = out["u"], out["v"]
    with np.errstate(invalid="ignore"):
        out["visible"] = (u >= 0.0) & (v >= 0.0) & (u < float(cam.width)) & (v < float(cam.height)) & \
            (out["status"] != R.POINT_BEHIND_CAMERA) & (out["status"] != R.PROJECTION_INVALID)
    return out


def occlusion(g, T_G_C, elevation, margin, pairs):
    """(F, cols, rows) bool: occluded(cell, frame), asked of the visible pairs only."""
    occ = np.zeros(pairs["visible"].shape, bool)
    for f, j, i in zip(*np.nonzero(pairs["visible"])):
        occ[f, j, i] = R.occluded(elevation, g, int(i), int(j), T_G_C[f, 0:3], margin)
    return occ


def new_sums(g, colored):
    """The accumulators of a fresh context: wsum (cols, rows) and acc (channels, cols, rows)."""
    return dict(wsum=np.zeros((g.cols, g.rows)), acc=np.zeros((3 if colored else 1, g.cols, g.rows)))


def _round_half_away(x):
    """std::round for x >= 0 (a visible keypoint): x - floor(x) is exact."""
    fl = np.floor(x)
    return (fl + (x - fl >= 0.5)).astype(np.int64)


def process(cam, pairs, images, layers, sums, colored=False, sharpness=2, occluded=None, frames=None):
    """One blended call over the frames `frames` (indices into pairs / images, ascending; None: all)
    onto `layers` and `sums`, both updated in place.  occluded: occlusion()'s array, or None (no
    occlusion test).  observation_index counts within the call, like the library's.
    Returns the per-cell count of contributing views, (cols, rows) int."""
    frames = list(range(pairs["visible"].shape[0])) if frames is None else list(frames)
    angle, index, nobs = layers["elevation_angle"], layers["observation_index"], layers["num_observations"]
    out = layers["colored_ortho" if colored else "ortho"]
    wsum, acc = sums["wsum"], sums["acc"]
    assert acc.shape[0] == (3 if colored else 1) and 0 <= sharpness <= 4
    # a cell no view was ever accepted for starts from zero
    restart = np.isnan(index)
    wsum[restart] = 0.0
    acc[:, restart] = 0.0
    count = np.zeros(index.shape, np.int64)
    for n, f in enumerate(frames):
        contributes = pairs["visible"][f].copy()
        if occluded is not None:
            contributes &= ~occluded[f]
        cx, cy, cz = pairs["C"][f, ..., 0], pairs["C"][f, ..., 1], pairs["C"][f, ..., 2]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            zz = cz * cz
            n2 = (cx * cx + cy * cy) + zz
            w = zz / n2
            for _ in range(sharpness):
                w = w * w
        kp_y = np.minimum(_round_half_away(np.where(contributes, pairs["v"][f], 0.0)), cam.height - 1)
        kp_x = np.minimum(_round_half_away(np.where(contributes, pairs["u"][f], 0.0)), cam.width - 1)
        px = np.asarray(images[f])[kp_y, kp_x].astype(np.float64)   # (cols, rows[, 3]); colour: B, G, R
        px = px[..., None] if px.ndim == 2 else px
        with np.errstate(invalid="ignore"):
            for ch in range(acc.shape[0]):
                acc[ch] = np.where(contributes, acc[ch] + w * px[..., ch], acc[ch])
            wsum[...] = np.where(contributes, wsum + w, wsum)
        count += contributes
        # the fold beside the sums: strict `>` against the float-rounded running maximum
        alpha = pairs["alpha"][f]
        assert np.all(alpha[contributes] > 0.0)   # CHECK(alpha > 0.0)
        with np.errstate(invalid="ignore"):
            accept = contributes & (np.abs(alpha) > angle.astype(np.float64))
        angle[accept] = np.abs(alpha[accept]).astype(np.float32)
        index[accept] = np.float32(n)
        nobs[accept] = nobs[accept] + nobs[accept]
    paint = (count > 0) & (wsum > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.rint(acc / wsum)          # half to even
    if colored:
        b, gr, r = (np.where(paint, q[ch], 0.0).astype(np.uint32) for ch in range(3))
        out[paint] = ((r << 16) | (gr << 8) | b).view(np.float32)[paint]
    else:
        out[paint] = q[0][paint].astype(np.float32)
    return count
