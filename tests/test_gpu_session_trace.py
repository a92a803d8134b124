"""What a session transfers, call by call, is decided by content alone: the same script of calls and host-side
edits moves the same bytes and leaves the same matrices, whatever the driver behind it looks like.

The script below runs on a 128 x 96 map (the smallest that gives tiles = (2, 2) four non-trivial windows under the
64 x 32 alignment) in the exact DSM mode, which is deterministic (tests/test_gpu_determinism.py).  After every call
the trace takes transfer_stats() and the CRC32 of each host matrix; the whole trace is compared, for equality, with
tests/golden/session_plan/trace.txt.

trace.txt was recorded by running THIS file (python tests/test_gpu_session_trace.py) at the commit before the session
driver was rebuilt around amhip_session_plan.h, twice, with equal output; it uses only HostSession methods that
existed then."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "session_plan", "trace.txt")
TILES = [(1, 1), (2, 2)]
LAYERS = ["ortho", "elevation", "elevation_angle", "num_observations", "observation_index", "colored_ortho"]


def trace(tiles):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import synth
    lx, ly, res = 64.0, 48.0, 0.5
    points = synth.make_points(12000, 36.0, 1201)
    # a small cloud over one corner of the map, three metres above the terrain
    corner = synth.make_points(400, 4.0, 1202, center=(-26.0, -18.0))
    corner[:, 2] += 3.0
    width, height = 96, 64
    ncam = A.NCamera(140.0, 140.0, (width - 1) / 2.0, (height - 1) / 2.0, width, height)
    poses = synth.make_lawnmower_poses(6, 0.45 * ly, 700.0, 1203)
    frames = [np.ascontiguousarray(f) for f in synth.make_frames(6, height, width, 1, salt=3)]
    inten = (np.arange(points.shape[0]) * 7 % 251).astype(np.int32)
    dsm, ortho = A.DsmSettings(1), A.OrthoSettings()
    lines = []
    with A.HostSession(A.GridMapSettings(0.0, 0.0, lx, ly, res), tiles=tiles) as hs:
        assert (hs.grid.rows, hs.grid.cols) == (128, 96)
        lines.append("tiles %d %d windows %s" % (tiles[0], tiles[1], " ".join(
            "%d,%d,%d,%d" % hs.window(k) for k in range(hs.num_windows))))

        def note(what):
            up, down = hs.transfer_stats()
            lines.append("%-22s up %9d down %9d %s" % (what, up, down, " ".join(
                "%08x" % (zlib.crc32(hs.layers[n].tobytes()) & 0xFFFFFFFF) for n in LAYERS)))

        hs.set_dsm_precision(True)
        hs.dsm_process(dsm, points)
        note("1 dsm")
        hs.ortho_process(ncam, ortho, poses, frames)
        note("2 mosaic")
        hs.ortho_process(ncam, ortho, poses, frames)
        note("3 mosaic again")
        hs.layers["elevation"][40, 50] = 123.25
        hs.dsm_process(dsm, corner)
        note("4 edit + corner dsm")
        hs.ortho_process(ncam, ortho, poses, frames)
        note("5 mosaic")
        for name, v in A.mapper.LAYER_INIT.items():
            hs.layers[name].fill(v)
        hs.dsm_process(dsm, points)
        note("6 refill + dsm")
        hs.ortho_process(ncam, ortho, poses, frames)
        note("6 mosaic")
        hs.set_always_copy(True)
        hs.dsm_process(dsm, points)
        note("7 always_copy dsm")
        hs.set_always_copy(False)
        hs.dsm_process(dsm, points)
        note("7 content dsm")
        hs.ortho_from_pcl_process(A.OrthoFromPclSettings(interpolation_radius=2), points, inten)
        note("8 ortho_from_pcl")
    return lines


def _golden():
    out = {}
    with open(GOLDEN) as fh:
        for line in fh.read().split("\n"):
            if line.startswith("tiles"):
                out[line] = cur = [line]
            elif line:
                cur.append(line)
    return {tuple(int(v) for v in k.split()[1:3]): v for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", TILES)
def test_session_trace_equals_the_recorded_one(tiles):
    got, want = trace(tiles), _golden()[tiles]
    for a, b in zip(got, want):
        assert a == b
    assert len(got) == len(want)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    for t in TILES:
        print("\n".join(trace(t)))
