"""DiamondDetector (host/include/diamond_detector.hpp) through host/test/diamond_test.cpp on a written-out frame: the C++ side finds the
diamonds and the poses the Python side found for the same frame, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import diamond_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "diamond_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_diamond_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_the_host_wrapper_finds_what_the_python_side_finds(tmp_path):
    from fiducials_amd.detector import ArucoDetector
    fr = dc.two_frame()
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (dc.W, dc.H))
        fh.write(fr.image.tobytes())
    det = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H)
    try:
        det.detect_markers(fr.image)
        rec = det.diamonds_last(dc.RATE)[0]
        poses = det.diamond_pose(rec, dc.SQUARE, dc.K, dc.Z5)
    finally:
        det.close()
    assert len(rec) == 2
    lines = ["%d %r %r" % (dc.DICT, dc.RATE, dc.SQUARE), " ".join(repr(float(v)) for v in (dc.K[0, 0], dc.K[1, 1], dc.K[0, 2], dc.K[1, 2], *dc.Z5)), str(len(rec))]
    for r, t in zip(rec, np.asarray(poses.tvecs)):
        lines.append(" ".join(str(int(i)) for i in r["ids"]) + " " + " ".join("%.9g" % v for v in r["corners"].reshape(-1)) + " " +
                     " ".join(repr(float(v)) for v in t))
    (tmp_path / "case.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "case.txt"), os.path.join(ROOT, "fiducials_amd", "data")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
