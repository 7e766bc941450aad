"""What the two C++ nodes publish on <marker image topic>/compressed for COMPRESSED frames (host/test/compressed_out_test.cpp):
FiducialsNode's /fiducial_images/compressed and StagNode's stag_ros/image_markers/compressed, made on the device
(fid_jpeg_marker_jpeg; a PNG frame's image through fid_jpeg_encode), each against the device encoder's file of the raw marker image
the Image overload publishes -- on the reference's tag_01 image as colour JPEG and PNG, a frame without markers, and an HD21 STag
frame."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "bin", "compressed_out_test")


def test_compressed_out_test_builds_without_a_gpu():
    r = subprocess.run([_exe()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_compressed_frames_publish_compressed_marker_images(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from fiducials_amd import synth
    from fiducials_amd.stag import load_library
    from test_gpu_marker_jpeg import tinted

    exe = _exe()
    color = tinted(np.load(os.path.join(GOLD, "tag_01.npz"))["gray"], 1)
    Image.fromarray(color).save(tmp_path / "tag_01_color.jpg", "JPEG", quality=90, subsampling=2)  # 4:2:0
    Image.fromarray(color).save(tmp_path / "tag_01_color.png")
    yy, xx = np.mgrid[0:480, 0:640]
    blank = np.stack([(xx // 3) % 256, (yy // 2) % 256, np.full_like(xx, 128)], axis=-1).astype(np.uint8)  # smooth: no markers
    Image.fromarray(blank).save(tmp_path / "blank.jpg", "JPEG", quality=90)
    fr = synth.make_stag_frame(load_library(21), 8, 1280, 720, 8)
    Image.fromarray(fr.image).save(tmp_path / "stag.jpg", "JPEG", quality=95)
    Image.fromarray(fr.image).save(tmp_path / "stag.png")
    r = subprocess.run([exe, str(tmp_path), os.path.join(ROOT, "fiducials_amd", "data")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
