"""FiducialsNode with ~map_outlier_px (host/include/fiducials_host.hpp) through host/test/aruco_map_robust_test.cpp, on a
written-out scene and two map files -- one in which two entries have exchanged places, one in which every entry is wrong: off, the
node's serialised outputs are those of a node that never heard of the parameter; on, map_outliers names the two ids, map_pose is
fid_map_pose_robust_last_cam's, map_pose_cov is fid_map_pose_cov_cam's over the inliers, and the all-wrong map gives no pose; and the
catkin node's syntax check with the two parameters."""
import os
import subprocess

import numpy as np
import pytest

import aruco_map_cases as mc
import map_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "aruco_map_robust_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_aruco_map_robust_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_node_reads_the_two_parameters():
    src = open(os.path.join(ROOT, "ros", "aruco_detect_amd", "src", "aruco_detect_amd_node.cpp")).read()
    assert '"map_outlier_px"' in src and '"map_min_markers"' in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("syntax ok") == 2


def _rpy_deg(R):
    """roll, pitch, yaw (degrees) of R = Rz(yaw) Ry(pitch) Rx(roll)."""
    p = -np.arcsin(R[2, 0])
    return np.degrees([np.arctan2(R[2, 1], R[2, 2]), p, np.arctan2(R[1, 0], R[0, 0])])


def _write_map(path, entries):
    lines = []
    for e in entries:
        r, p, y = _rpy_deg(e["R"])
        lines.append("%d %.17g %.17g %.17g %.17g %.17g %.17g 0.01 5" % (e["id"], e["t"][0], e["t"][1], e["t"][2], r, p, y))
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_node_leaves_the_lying_entries_out(tmp_path):
    fr = mc.scene("3x2", 1)
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (mc.W, mc.H))
        fh.write(fr.image.tobytes())
    truthful = mc.scene_map("3x2")
    lying = truthful.copy()
    lying["R"][[1, 4]], lying["t"][[1, 4]] = truthful["R"][[4, 1]], truthful["t"][[4, 1]]
    wrong = truthful.copy()  # no two entries keep their distance: pitch 0.13 m, every entry moved by its own 3 .. 9 cm
    for k, d in enumerate(([0.05, 0.0, 0.0], [0.0, 0.06, 0.0], [-0.07, 0.03, 0.0], [0.04, -0.08, 0.0], [-0.03, -0.05, 0.02], [0.09, 0.04, -0.03])):
        wrong["t"][k] += d
    _write_map(tmp_path / "lying.txt", lying)
    _write_map(tmp_path / "wrong.txt", wrong)
    (tmp_path / "camera.txt").write_text("%r %r %r %r\n%r\n21 24\n" % (float(mc.K[0, 0]), float(mc.K[1, 1]), float(mc.K[0, 2]), float(mc.K[1, 2]), rc.INLIER_PX))
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "lying.txt"), str(tmp_path / "wrong.txt"), str(tmp_path / "camera.txt"),
                        os.path.join(ROOT, "fiducials_amd", "data"), str(mc.DICT), repr(mc.SCENE_LEN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
