"""FiducialsNode with ~map_file (host/include/fiducials_host.hpp) through host/test/aruco_map_test.cpp, on a written-out scene and map
file: the PoseStamped of the camera in the map equals fid_map_pose_last's record, nothing extra without a map; and the catkin node's
syntax check with `~map_file`."""
import os
import subprocess

import pytest

import aruco_map_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "aruco_map_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_aruco_map_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_node_reads_map_file():
    src = open(os.path.join(ROOT, "ros", "aruco_detect_amd", "src", "aruco_detect_amd_node.cpp")).read()
    assert '"map_file"' in src and '"fiducial_map_pose"' in src and "map_pose_pub" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("syntax ok") == 2


def _rpy_deg(R):
    """roll, pitch, yaw (degrees) of R = Rz(yaw) Ry(pitch) Rx(roll)."""
    import numpy as np
    p = -np.arcsin(R[2, 0])
    return np.degrees([np.arctan2(R[2, 1], R[2, 2]), p, np.arctan2(R[1, 0], R[0, 0])])


@pytest.mark.gpu
def test_node_publishes_the_camera_in_the_map(tmp_path):
    """The two-wall corner scene; the map file as fiducial_slam writes it, with links, an entry out of sight and an invalid line."""
    fr = mc.scene("corner", 1)
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (mc.W, mc.H))
        fh.write(fr.image.tobytes())
    lines = []
    for e in mc.scene_map("corner"):
        r, p, y = _rpy_deg(e["R"])
        lines.append("%d %.17g %.17g %.17g %.17g %.17g %.17g 0.01 5 30 31" % (e["id"], e["t"][0], e["t"][1], e["t"][2], r, p, y))
    lines.insert(2, "this line is not an entry")
    lines.append("77 3.0 0.0 0.0 0 0 0 0.5 1")
    (tmp_path / "map.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "camera.txt").write_text("%r %r %r %r\n4\n" % (float(mc.K[0, 0]), float(mc.K[1, 1]), float(mc.K[0, 2]), float(mc.K[1, 2])))
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "map.txt"), str(tmp_path / "camera.txt"),
                        os.path.join(ROOT, "fiducials_amd", "data"), str(mc.DICT), repr(mc.SCENE_LEN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
