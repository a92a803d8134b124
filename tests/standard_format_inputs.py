"""A small simulated dataset in the layout io::AerialMapperIO::toStandardFormat reads, built from the
committed PNG fixtures (tests/golden/png_decode/): <dir>/cam0/<integer name>.png, blender_id_time.csv
(`id name` pairs; an image's timestamp is its name - 1) and vi_imu_poses.csv (`time x y z qx qy qz qw`).
The poses stand in another order than the images, one timestamp is there twice (the later pose must
win) and some poses belong to no image.  Shared by tests/test_gpu_standard_format.py and
tests/test_gpu_cpp_write_images.py."""
import os

import numpy as np

import jpeg_reference as J
import png_decode_inputs as PI

SIZE = (129, 47)
_jpg = {}


def fixtures():
    return PI.fixtures_by_size()[SIZE]


def image_name(i):
    return 1000 + 7 * i


def pose_of(i, salt=0):
    """x y z qw qx qy qz; values that %g shortens and values it does not"""
    q = np.array([0.5 + 0.01 * i, 0.5, -0.5 + 0.003 * salt, 0.5 - 0.01 * i])
    q = q / np.sqrt((q * q).sum())
    return [464499.25 + 1.5 * i + 100.0 * salt, 5272700.0 - 0.125 * i, 100.0 + i / 3.0] + q.tolist()


def build(directory, missing_pose_for=None):
    """-> (names of the fixtures in image order, the poses toStandardFormat must associate (n, 7))"""
    names = fixtures()
    os.makedirs(os.path.join(directory, "cam0"))
    for i, n in enumerate(names):
        with open(os.path.join(directory, "cam0", "%d.png" % image_name(i)), "wb") as f:
            f.write(PI.fixture_bytes(n))
    with open(os.path.join(directory, "blender_id_time.csv"), "w") as f:
        for i in range(len(names)):
            f.write("%d %d\n" % (i, image_name(i)))
    lines = []

    def line(stamp, pose, form="%d"):
        x, y, z, qw, qx, qy, qz = pose
        lines.append((form + " %.17g %.17g %.17g %.17g %.17g %.17g %.17g") % (stamp, x, y, z, qx, qy, qz, qw))

    line(image_name(0) - 1, pose_of(0, salt=1))               # the first of two poses at image 0's timestamp
    line(5, pose_of(40))                                      # poses without an image
    for i in reversed(range(len(names))):                     # another order than the images
        if i != missing_pose_for:
            line(image_name(i) - 1, pose_of(i), "%.3f" if i % 2 else "%d")
        line(image_name(i) + 2, pose_of(50 + i))
    with open(os.path.join(directory, "vi_imu_poses.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return names, np.array([pose_of(i) for i in range(len(names))])


def expected_jpg(name):
    """what cv::imwrite writes for the fixture's gray pixels: libjpeg at quality 95, through the restatement"""
    if name not in _jpg:
        _jpg[name] = J.encode(PI.fixture_pixels(name)[0], 95)
    return _jpg[name]


def expected_poses_text(poses):
    return "".join(" ".join("%g" % v for v in p) + "\n" for p in poses)


def expected_geofile(poses):
    return "".join("image_%010d.jpeg %.15g %.15g %.15g\n" % (i + 1, p[0], p[1], p[2]) for i, p in enumerate(poses))
