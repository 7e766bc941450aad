"""CharucoCalibrator (host/include/camera_calibrator.hpp) through host/test/charuco_calibrate_test.cpp: the views of a
charuco_calib_cases case written out, calibrated through the class, handed on as CameraInfo fields and as the camera_info YAML file,
read back, and through fid_camera_from_info the same camera again.  The calibrated values are held to the NumPy restatement's on the
same views at the parameter bar of tests/test_gpu_charuco_calibrate.py."""
import os
import subprocess

import numpy as np
import pytest

import charuco_calib_cases as ccc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "charuco_calibrate_test")
FREE = 0x000F | 1 << 4  # fx fy cx cy k1


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_charuco_calibrate_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_views_to_yaml_and_back(tmp_path):
    base = ccc.case("plumb_bob", "12x72")
    k16 = np.zeros(16)
    k16[:5] = base["k16"][:5]  # (the fixed slots of this run are zero: p1 p2 k2 k3 are not estimated)
    c = dict(base, k16=k16, free=FREE, poses=None)
    ref = ccc.reference_of(c)
    assert ref["kept"], ref["gap"]
    best = ref["best"]
    t = max(10.0 * ref["gap"], 1e-9)
    bar = 2.0 * np.sqrt(2.0 * t * (2 * best["n_points"] - len(best["x"]))) * best["std_dev"]
    lines = ["%d %d %d %d %d" % (ccc.W, ccc.H, 0, 5, ccc.DICT), "%d %d %.17g %.17g %d" % ccc.BOARDS[c["board"]], str(len(c["views"]))]
    for ids, xy in c["views"]:
        lines.append(str(len(ids)))
        for i, p in zip(ids, xy):
            lines.append("%d %.9g %.9g" % (i, p[0], p[1]))
    lines.append(" ".join("%.17g" % v for v in best["k16"][:5]))
    lines.append("%.17g %.17g" % (bar[:4].min(), bar[4]))
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build(), str(tmp_path / "views.txt"), os.path.join(ROOT, "fiducials_amd", "data"), str(tmp_path / "camera.yaml")],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    text = (tmp_path / "camera.yaml").read_text()
    assert text.startswith("image_width: 1280\nimage_height: 720\ncamera_name: calibrated\ncamera_matrix:\n  rows: 3\n  cols: 3\n  data: [")
    assert "distortion_model: plumb_bob\ndistortion_coefficients:\n  rows: 1\n  cols: 5\n" in text
    assert "rectification_matrix:\n  rows: 3\n  cols: 3\n  data: [1, 0, 0, 0, 1, 0, 0, 0, 1]\n" in text and "projection_matrix:\n  rows: 3\n  cols: 4\n" in text
