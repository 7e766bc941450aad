"""StagNode with a layout (host/include/stag_host.hpp) through host/test/stag_bundles_test.cpp, on a written-out scene and YAML file:
the bundle PoseStamped, frame names and TF, members of a multi-tag bundle absent from the per-marker outputs, a standalone tag under
its own frame, outputs without a layout unchanged; and the catkin node's syntax check with `~tags` / `~bundles`."""
import os
import subprocess

import numpy as np
import pytest

import stag_bundle_cases as bc
from fiducials_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "stag_bundles_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_stag_bundles_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_node_reads_tags_and_bundles():
    src = open(os.path.join(ROOT, "ros", "stag_detect_amd", "src", "stag_detect_amd_node.cpp")).read()
    assert 'getParam("bundles"' in src and 'getParam("tags"' in src and "bundles_pub_.publish(" in src
    assert '"stag_ros/bundles"' in open(os.path.join(ROOT, "host", "include", "stag_host.hpp")).read()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("syntax ok") == 2


def _corners_yaml(c, indent):
    return "\n".join(f"{indent}- [{p[0]:.17g}, {p[1]:.17g}, {p[2]:.17g}]" for p in c[:3])


@pytest.mark.gpu
def test_node_publishes_bundles_standalone_tags_and_loose_markers(tmp_path):
    """One frame with a 2 x 2 board (a bundle), a standalone 0.05 m tag and a marker the layout does not name."""
    Rb, tb = bc.pose_of(0.3, 0.55)
    tb = tb + np.array([-0.10, -0.03, 0.0])
    Rs, ts = bc.pose_of(-0.25, 0.40)
    ts = ts + np.array([0.13, -0.06, 0.0])
    Rl, tl = bc.pose_of(0.2, 0.45)
    tl = tl + np.array([0.12, 0.09, 0.0])
    board = synth.make_stag_board_frame(21, [0, 1, 2, 3], 2, 2, bc.K, Rb, tb, 1, bc.W, bc.H, 96, 0.08, 40, noise_sigma=0.0)
    alone = synth.make_stag_board_frame(21, [9], 1, 1, bc.K, Rs, ts, 2, bc.W, bc.H, 96, 0.05, 40, noise_sigma=0.0)
    loose = synth.make_stag_board_frame(21, [7], 1, 1, bc.K, Rl, tl, 3, bc.W, bc.H, 96, 0.08, 40, noise_sigma=0.0)
    img = board.image
    for fr in (alone, loose):
        img = np.where(fr.image != 150, fr.image, img)
    img = np.clip(np.rint(img.astype(np.float32) + np.random.default_rng(4).normal(0, 2.0, img.shape)), 0, 255).astype(np.uint8)
    with open(tmp_path / "frame.pgm", "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (bc.W, bc.H))
        fh.write(img.tobytes())
    yaml = "tags:\n  - id: 9\n    frame: small_tag\n    corners:\n" + _corners_yaml(alone.corners_board[0], "      ") + "\n"
    yaml += "bundles:\n  - frame: plate\n    tags:\n"
    for i, c in zip(board.ids, board.corners_board):
        yaml += f"      - id: {int(i)}\n        corners:\n" + _corners_yaml(c, "          ") + "\n"
    (tmp_path / "layout.yaml").write_text(yaml)
    with open(tmp_path / "expected.txt", "w") as fh:
        fh.write("%r %r %r %r\n2\n" % (float(bc.K[0, 0]), float(bc.K[1, 1]), float(bc.K[0, 2]), float(bc.K[1, 2])))
        fh.write("plate 0 %r %r %r\n" % tuple(float(v) for v in tb))
        fh.write("small_tag 1 %r %r %r\n" % tuple(float(v) for v in ts))
        fh.write("1\n7\n")
    r = subprocess.run([_build(), str(tmp_path / "frame.pgm"), str(tmp_path / "layout.yaml"), str(tmp_path / "expected.txt"),
                        os.path.join(ROOT, "fiducials_amd", "data"), "21", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
