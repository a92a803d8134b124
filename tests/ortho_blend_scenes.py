"""Scenes of the blended mosaic's tests on the map and camera of tests/ortho_occlusion_scenes.py,
with their expected layers (tests/ortho_blend_reference.py).  The pairs of a scene are probed once
per process, every expected result is computed once and handed out as copies."""
import functools

import numpy as np

import oracle_ffi as O
import ortho_blend_reference as B
import ortho_occlusion_reference as R
import ortho_occlusion_scenes as SC
from aerial_mapper_amd import synth

# (the coefficients of test_gpu_ortho_occlusion.py's CAMERAS)
CAMERAS = {"none": (O.DIST_NONE, (0.0, 0.0, 0.0, 0.0)),
           "radtan": (O.DIST_RADTAN, (-0.25, 0.06, 3e-4, -2e-4)),
           "equidistant": (O.DIST_EQUIDISTANT, (-0.02, 0.004, -0.001, 0.0002))}
F_MAIN = 5


def camera(kind="none"):
    return SC.camera(*CAMERAS[kind])


def main_poses():
    """The oblique and the nadir-ish frame of the block scene, then three near-nadir frames: within
    5 m of the map's centre, 55 - 61 m up, tilted by less than 3 degrees, each with a yaw of its
    own.  At 60 m the camera's footprint is about 82 m x 46 m over the 40 m x 36 m map: most cells
    are seen by four frames."""
    near = [R.look_at_pose((1.0, -2.0, 58.0), (2.5, -0.5, 0.0), yaw=0.4),
            R.look_at_pose((-3.0, 2.0, 55.0), (-1.0, 3.0, 0.0), yaw=2.0),
            R.look_at_pose((2.0, 3.0, 61.0), (0.0, 1.5, 0.0), yaw=-1.1)]
    return np.concatenate([SC.block_poses(), np.stack(near)])


def elevation(name):
    if name == "block":
        return SC.block_elevation()
    if name == "nan":
        return SC.nan_elevation()
    if name == "zero":
        return np.zeros((SC.COLS, SC.ROWS), np.float32)
    raise KeyError(name)


def frames(colored=False):
    return SC.frames(F_MAIN, colored)


def T_G_C():
    return O.compose_T_G_C(main_poses(), synth.IDENTITY_POSE)


@functools.lru_cache(maxsize=None)
def pairs(elev="block", kind="none", nframes=F_MAIN):
    return B.probe(SC.grid(), camera(kind), T_G_C()[:nframes], elevation(elev))


@functools.lru_cache(maxsize=None)
def occluded(elev="block", kind="none", nframes=F_MAIN):
    return B.occlusion(SC.grid(), T_G_C()[:nframes], elevation(elev), SC.MARGIN, pairs(elev, kind, nframes))


@functools.lru_cache(maxsize=None)
def _expected(elev, kind, colored, sharpness, occl, calls, nframes):
    lay = SC.fresh_layers(elevation(elev))
    sums = B.new_sums(SC.grid(), colored)
    count = None
    for call in calls:
        count = B.process(camera(kind), pairs(elev, kind, nframes), frames(colored), lay, sums, colored,
                          sharpness, occluded(elev, kind, nframes) if occl else None, call)
    return lay, count


def expected(elev="block", kind="none", colored=False, sharpness=2, occl=False, calls=None, nframes=F_MAIN):
    """(layers, the last call's per-cell count of contributing views) of the calls `calls` (tuples
    of ascending frame indices; None: one call of all nframes frames) onto a fresh map."""
    calls = (tuple(range(nframes)),) if calls is None else tuple(tuple(c) for c in calls)
    lay, count = _expected(elev, kind, bool(colored), int(sharpness), bool(occl), calls, nframes)
    return {k: v.copy() for k, v in lay.items()}, count.copy()
