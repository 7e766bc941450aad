"""StagNode::compressedImageCallback (host/include/stag_host.hpp) through host/test/stag_compressed_test.cpp: one rendered STag
frame as JPEG (decoded on the device, then fid_stag_detect_markers_device) and as PNG (decoded on the host) must publish exactly
what imageCallback publishes for the mono8 frame each file decodes to; damaged files publish nothing."""
import io
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "stag_compressed_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_stag_compressed_test_builds_without_a_gpu():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_the_ros_node_subscribes_to_compressed_frames_when_asked():
    """is_compressed: the catkin node takes the CompressedImage messages itself (<raw_image_topic>/compressed) and hands them to
    StagNode::compressedImageCallback, as the aruco node does; `make -C ros syntax` type-checks it against the ROS stand-ins."""
    src = open(os.path.join(ROOT, "ros", "stag_detect_amd", "src", "stag_detect_amd_node.cpp")).read()
    assert 'p.raw_image_topic + "/compressed"' in src and "compressedImageCallback(" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ros"), "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_compressed_frames_publish_what_the_decoded_frame_publishes(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image

    import sys
    sys.path.insert(0, ROOT)
    from fiducials_amd import synth
    from fiducials_amd.stag import load_library
    exe = _build()
    gray = synth.make_stag_frame(load_library(15), 21, 1280, 720, 8).image
    rng = np.random.default_rng(5)
    g = gray.astype(np.int64)
    rgb = np.stack([np.clip(g * 1.08 - 6 + rng.integers(-4, 5, g.shape), 0, 255), g,
                    np.clip(g * 0.9 + 15 + rng.integers(-4, 5, g.shape), 0, 255)], axis=-1).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=90)
    (tmp_path / "frame.jpg").write_bytes(b.getvalue())
    Image.fromarray(rgb).save(tmp_path / "frame.png")
    r = subprocess.run([exe, str(tmp_path / "frame.jpg"), str(tmp_path / "frame.png"), os.path.join(ROOT, "fiducials_amd", "data"), "15", "7"],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
