"""GPU: the Python mirrors of io::AerialMapperIO's format converters (aerial_mapper_amd.io):
to_standard_format turns a simulated dataset (tests/standard_format_inputs.py) into opt_poses.txt and
image_<i>.jpg, the PNG frames decoded into HBM and encoded from there in one batch; export_pix4d_geofile
writes image_%010d.jpeg and geofile.txt.  The files are libjpeg's at quality 95 (tests/jpeg_reference.py)."""
import os

import numpy as np
import pytest

import png_decode_inputs as PI
import standard_format_inputs as SF

pytestmark = pytest.mark.gpu


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


def test_load_poses_ros_reads_time_then_xyz_then_xyzw(tmp_path):
    src = str(tmp_path / "in") + os.sep
    names, _ = SF.build(src)
    poses, stamps = _io().load_poses_ros(src + "vi_imu_poses.csv")
    assert poses.shape == (2 * len(names) + 2, 7) and stamps.dtype == np.int64 and len(stamps) == len(poses)
    assert stamps[0] == SF.image_name(0) - 1 and stamps[1] == 5
    assert np.array_equal(poses[0], SF.pose_of(0, salt=1)) and np.array_equal(poses[1], SF.pose_of(40))
    assert stamps[-2] == SF.image_name(0) - 1 and np.array_equal(poses[-2], SF.pose_of(0))


def test_to_standard_format_writes_the_poses_and_libjpegs_files(tmp_path):
    src, dst = str(tmp_path / "in") + os.sep, str(tmp_path / "out") + os.sep
    names, poses = SF.build(src)
    assert len(names) >= 15
    os.makedirs(dst)
    got = _io().to_standard_format(src, "vi_imu_poses.csv", "blender_id_time.csv", dst)
    assert np.array_equal(got, poses)                    # the later of the two poses at image 0's timestamp
    assert open(dst + "opt_poses.txt").read() == SF.expected_poses_text(poses)
    assert sorted(os.listdir(dst)) == sorted(["opt_poses.txt"] + ["image_%d.jpg" % i for i in range(len(names))])
    for i, n in enumerate(names):
        assert open("%simage_%d.jpg" % (dst, i), "rb").read() == SF.expected_jpg(n), n


def test_an_image_without_a_pose_raises_and_names_it(tmp_path):
    from aerial_mapper_amd import hip_lib as L
    src, dst = str(tmp_path / "in") + os.sep, str(tmp_path / "out") + os.sep
    SF.build(src, missing_pose_for=3)
    os.makedirs(dst)
    with pytest.raises(L.AmhipError) as err:
        _io().to_standard_format(src, "vi_imu_poses.csv", "blender_id_time.csv", dst)
    assert "found_pose_for_image" in str(err.value) and "%d.png" % SF.image_name(3) in str(err.value)
    assert not [f for f in os.listdir(dst) if f.endswith(".jpg")]


@pytest.mark.parametrize("ch", [1, 3])
def test_export_pix4d_geofile_numbers_from_one_and_writes_15_digits(ch, tmp_path):
    names = SF.fixtures()[:6]
    stack = np.stack([PI.fixture_pixels(n)[1 if ch == 3 else 0] for n in names])
    poses = np.array([SF.pose_of(i, salt=2) for i in range(len(names))])
    poses[:, 0] += 1.0 / 3.0                                    # (more than 15 digits to cut)
    out = str(tmp_path / "pix4d")
    os.makedirs(out)
    _io().export_pix4d_geofile(poses, stack, out)
    files = _io().encode_jpeg_frames(stack, 95)
    assert sorted(os.listdir(out)) == ["geofile.txt"] + ["image_%010d.jpeg" % (i + 1) for i in range(len(names))]
    for i in range(len(names)):
        assert open(os.path.join(out, "image_%010d.jpeg" % (i + 1)), "rb").read() == files[i]
        if ch == 1:
            assert files[i] == SF.expected_jpg(names[i])
    text = open(os.path.join(out, "geofile.txt")).read()
    assert text == SF.expected_geofile(poses)
    assert text.splitlines()[0].startswith("image_0000000001.jpeg 464699.583333333 ")


def test_export_pix4d_geofile_refuses_a_pose_count_that_differs(tmp_path):
    from aerial_mapper_amd import hip_lib as L
    stack = np.zeros((3, 16, 16), np.uint8)
    with pytest.raises(L.AmhipError):
        _io().export_pix4d_geofile(np.zeros((2, 7)), stack, str(tmp_path))
    assert os.listdir(str(tmp_path)) == []
