"""FiducialsNode and StagNode with ~pose_covariance (host/include/fiducials_host.hpp, stag_host.hpp) through
host/test/pose_cov_test.cpp, on a written-out 640 x 480 scene of a map's fiducials and a written-out STag frame: off, the outputs
are the default node's; on, the vision_msgs hypotheses carry fid_pose_last_cov_cam's cov_pose, map_pose_cov carries
fid_map_pose_last_cov_cam's cov_cam_pose beside an unchanged map_pose, and StagNode's Detection2DArray carries
fid_stag_pose_last_cov_cam's; and the catkin nodes read the two parameters and pass the syntax check."""
import os
import subprocess

import numpy as np
import pytest

import aruco_map_cases as mc
import pose_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "pose_cov_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_pose_cov_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_nodes_read_the_covariance_parameters():
    for node in ("aruco_detect_amd", "stag_detect_amd"):
        src = open(os.path.join(ROOT, "ros", node, "src", node + "_node.cpp")).read()
        assert '"pose_covariance"' in src and '"pose_covariance_sigma_px"' in src and "covariance[k] = h.covariance[k]" in src, node
    src = open(os.path.join(ROOT, "ros", "aruco_detect_amd", "src", "aruco_detect_amd_node.cpp")).read()
    assert '"fiducial_map_pose_cov"' in src and "map_pose_cov_pub_" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("syntax ok") == 2


def _rpy_deg(R):
    """roll, pitch, yaw (degrees) of R = Rz(yaw) Ry(pitch) Rx(roll)."""
    p = -np.arcsin(R[2, 0])
    return np.degrees([np.arctan2(R[2, 1], R[2, 2]), p, np.arctan2(R[1, 0], R[0, 0])])


def _write_pgm(path, image):
    h, w = image.shape
    with open(path, "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (w, h))
        fh.write(np.ascontiguousarray(image).tobytes())


@pytest.mark.gpu
def test_nodes_publish_the_covariance(tmp_path):
    fr = mc.scene("2x2", 1)
    _write_pgm(tmp_path / "frame.pgm", fr.image)
    lines = []
    for e in mc.scene_map("2x2"):
        r, p, y = _rpy_deg(e["R"])
        lines.append("%d %.17g %.17g %.17g %.17g %.17g %.17g 0.01 5" % (e["id"], e["t"][0], e["t"][1], e["t"][2], r, p, y))
    (tmp_path / "map.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "camera.txt").write_text("%r %r %r %r\n" % (float(mc.K[0, 0]), float(mc.K[1, 1]), float(mc.K[0, 2]), float(mc.K[1, 2])))
    n_markers, stag_image = pc.stag_frames()[1]
    _write_pgm(tmp_path / "stag.pgm", stag_image)
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "map.txt"), str(tmp_path / "camera.txt"),
                        os.path.join(ROOT, "fiducials_amd", "data"), str(mc.DICT), repr(mc.SCENE_LEN), str(tmp_path / "stag.pgm"), "21"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
