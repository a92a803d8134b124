"""Scenes of the occlusion-tested mosaic's tests, with their expected layers (computed once per
process by tests/ortho_occlusion_reference.py and handed out as copies).

The map: 80 x 72 cells at 0.5 m -- two tiles of 64 x 64 cells in both directions, the second ones
partial -- under the 96 x 54 camera of test_abi.py (fu = fv = 70), about 60 m above the ground.
"""
import functools

import numpy as np

import oracle_ffi as O
import ortho_occlusion_reference as R
from aerial_mapper_amd import synth

RES = 0.5
ROWS, COLS = 80, 72
MARGIN = 0.1
BLOCK_I, BLOCK_J = slice(60, 68), slice(58, 66)   # 8 x 8 cells across both tile borders (64)
BLOCK_HEIGHT = 12.0


def grid():
    g = O.make_grid(ROWS * RES, COLS * RES, RES)
    assert (g.rows, g.cols) == (ROWS, COLS)
    return g


def camera(distortion=O.DIST_NONE, dist=(0.0, 0.0, 0.0, 0.0)):
    cam = O.Camera()
    cam.fu = cam.fv = 70.0
    cam.cu, cam.cv, cam.width, cam.height = 47.5, 26.5, 96, 54
    cam.distortion = distortion
    for k in range(4):
        cam.dist[k] = float(dist[k])
    return cam


def frames(F, colored=False, salt=2):
    fr = synth.make_frames(F, 54, 96, 3 if colored else 1, salt=salt)
    return [np.ascontiguousarray(fr[k]) for k in range(F)]


def flat_noisy(seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-0.05, 0.05, size=(COLS, ROWS)).astype(np.float32)


def block_elevation():
    z = flat_noisy()
    z[BLOCK_J, BLOCK_I] = np.float32(BLOCK_HEIGHT)
    return z


def cell_xy(i, j):
    return O.cell_position(grid(), i, j)


def block_poses():
    """Frame 0: an oblique camera beyond the map's corner, behind the block as seen from the map's
    centre, its optical axis on the ground the block hides from it: without the occlusion term it
    wins there (the view angle is measured against the image plane) and paints the ground with the
    roof.  Frame 1: a camera over the centre, a few degrees off nadir, that does see that ground."""
    bx, by = cell_xy(64, 62)        # the block's centre
    oblique = R.look_at_pose((bx - 18.0, by - 19.0, 60.0), (bx + 4.5, by + 4.75, 0.0), yaw=0.3)
    nadirish = R.look_at_pose((1.3, -0.8, 61.0), (4.0, 2.5, 0.0), yaw=1.7)
    return np.stack([oblique, nadirish])


def fresh_layers(elevation):
    lay = O.new_layers(grid())
    lay["elevation"][...] = elevation
    return lay


def _copy(layers):
    return {k: v.copy() for k, v in layers.items()}


@functools.lru_cache(maxsize=None)
def _expected(scene, colored, margin):
    g, cam = grid(), camera()
    fr = frames(2, colored)
    poses = block_poses()
    z = block_elevation()
    if scene == "block":          # both frames, one call
        lay = fresh_layers(z)
        R.process(g, cam, poses, synth.IDENTITY_POSE, fr, lay, colored, margin)
    elif scene == "oblique":      # the oblique frame alone
        lay = fresh_layers(z)
        R.process(g, cam, poses[0:1], synth.IDENTITY_POSE, fr[0:1], lay, colored, margin)
    elif scene == "incremental":  # the nadir-ish frame, then the oblique one onto its layers
        lay = fresh_layers(z)
        R.process(g, cam, poses[1:2], synth.IDENTITY_POSE, fr[1:2], lay, colored, margin)
        R.process(g, cam, poses[0:1], synth.IDENTITY_POSE, fr[0:1], lay, colored, margin)
    elif scene == "nan":          # holes on the rays and under the block's shadow
        z = nan_elevation()
        lay = fresh_layers(z)
        R.process(g, cam, poses, synth.IDENTITY_POSE, fr, lay, colored, margin)
    else:
        raise KeyError(scene)
    return lay


def expected(scene, colored=False, margin=MARGIN):
    """margin None: the reference's rule (the plain mosaic)."""
    return _copy(_expected(scene, bool(colored), margin))


def nan_elevation():
    z = block_elevation()
    rng = np.random.Generator(np.random.PCG64(5))
    holes = rng.uniform(size=z.shape) < 0.15
    holes[BLOCK_J, BLOCK_I] = False   # the block keeps casting its shadow
    z[holes] = np.nan
    return z


# ---- the strict comparison and the rounding rule: exactly representable numbers ---------------
# h = 0 everywhere; the camera is 8 cells from cell (I0, J0) along i, 4 along j, and 8 m up:
# di = 8, dj = 4, m = 8, dz = 8, so s = k / 8, s * di = k, z = k are exact and s * dj = k / 2 is
# half-way for every odd k.
I0, J0 = 20, 30
EXACT_MARGIN = 0.25


def exact_pose():
    x, y = cell_xy(I0, J0)
    # level camera looking straight down (R_G_C = Rx(pi)): the cell projects 35 / 17.5 pixels off
    # the principal point
    return np.array([[x - 8 * RES, y - 4 * RES, 8.0, 0.0, 1.0, 0.0, 0.0]])


def exact_elevation(k, dj_cells, height):
    """flat 0 with one sample `height` at the cell the march visits at step k -- if it rounds
    k / 2 to dj_cells."""
    z = np.zeros((COLS, ROWS), np.float32)
    z[J0 + dj_cells, I0 + k] = height
    return z
