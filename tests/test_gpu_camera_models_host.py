"""FiducialsNode under the camera models of CameraInfo.distortion_model (host/include/fiducials_host.hpp) through
host/test/camera_models_test.cpp, on a written-out 640 x 480 frame rendered with the plain pinhole: rational_polynomial with zero
coefficients gives the plumb-bob node's transforms; equidistant with zero coefficients and a depth camera's rational coefficients
give fid_pose_cam's for that camera, which differ from the plumb-bob node's; a tilted 14-coefficient model publishes vertices and
no transforms; and the catkin nodes' syntax check."""
import os
import subprocess

import pytest

import aruco_map_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "camera_models_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_camera_models_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_nodes_hand_the_distortion_model_over():
    for node in ("aruco_detect_amd", "stag_detect_amd"):
        src = open(os.path.join(ROOT, "ros", node, "src", node + "_node.cpp")).read()
        assert "ci.distortion_model = msg->distortion_model" in src and "ci.D = msg->D" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("syntax ok") == 2


@pytest.mark.gpu
def test_node_poses_under_the_model_of_its_camera_info(tmp_path):
    from fiducials_amd.dictionary import get_predefined_dictionary
    from fiducials_amd.synth import make_frame

    W, H = 640, 480
    fr = make_frame(get_predefined_dictionary(mc.DICT), seed=7, width=W, height=H, n_markers=4, side_range=(60, 110))
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (W, H))
        fh.write(fr.image.tobytes())
    f = 1400.0 * W / 1920.0
    (tmp_path / "camera.txt").write_text("%r %r %r %r\n" % (f, f, W / 2.0, H / 2.0))
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "camera.txt"), os.path.join(ROOT, "fiducials_amd", "data"), str(mc.DICT), "0.14"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
