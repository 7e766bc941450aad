"""CharucoBoard (host/include/charuco_board.hpp) through host/test/charuco_test.cpp on a written-out frame: the C++ side finds the corners
and the board pose the Python side found for the same frame, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import charuco_cases as cc
from aruco_map_cases import D_NONZERO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "charuco_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_charuco_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_the_host_wrapper_finds_what_the_python_side_finds(tmp_path):
    from fiducials_amd.detector import ArucoDetector
    fr, b = cc.view("tilted"), cc.board("5x4")
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (cc.W, cc.H))
        fh.write(fr.image.tobytes())
    det = ArucoDetector(cc.DICT, max_width=cc.W, max_height=cc.H)
    try:
        det.set_charuco_board(b)
        det.detect_markers(fr.image)
        rec = det.charuco_last(K=cc.K, D=D_NONZERO)[0]
        pose = det.charuco_pose_last(cc.K, D_NONZERO)[0]
    finally:
        det.close()
    assert len(rec) >= 4 and pose["status"] == 0
    lines = ["%d %d %d %r %r %d" % (cc.DICT, b.squares_x, b.squares_y, b.square_len, b.marker_len, b.first_id),
             " ".join(repr(float(v)) for v in (cc.K[0, 0], cc.K[1, 1], cc.K[0, 2], cc.K[1, 2], *D_NONZERO)), str(len(rec))]
    lines += ["%d %.9g %.9g" % (r["id"], r["x"], r["y"]) for r in rec]
    lines.append(" ".join(repr(float(v)) for v in pose["tvec"]))
    (tmp_path / "case.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "case.txt"), os.path.join(ROOT, "fiducials_amd", "data")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
