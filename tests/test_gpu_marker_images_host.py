"""The marker images of the two C++ nodes for COMPRESSED frames (host/test/marker_images_test.cpp): FiducialsNode's
/fiducial_images (the decoded BGR8 frame with the outlines; a JPEG is decoded, detected and drawn on the device) and StagNode's
stag_ros/image_markers (the detector's gray image as BGR with the outlines), each against the library's host decode and host
drawer, on the reference's tag_01 image as one-component and colour 4:2:0 JPEG and as PNG, a frame without markers, and an HD21
STag frame."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "bin", "marker_images_test")


def test_marker_images_test_builds_without_a_gpu():
    r = subprocess.run([_exe()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _tinted(gray, seed):
    rng = np.random.default_rng(seed)
    g = gray.astype(np.int64)
    b = np.clip(g * 0.85 + 20 + rng.integers(-4, 5, g.shape), 0, 255)
    r = np.clip(g * 1.1 - 8 + rng.integers(-4, 5, g.shape), 0, 255)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)  # (RGB, as Pillow takes it)


@pytest.mark.gpu
def test_compressed_frames_publish_marker_images(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from fiducials_amd import synth
    from fiducials_amd.stag import load_library

    exe = _exe()
    gray = np.load(os.path.join(GOLD, "tag_01.npz"))["gray"]
    with open(tmp_path / "tag_01.pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (gray.shape[1], gray.shape[0]) + np.ascontiguousarray(gray).tobytes())
    color = _tinted(gray, 1)
    Image.fromarray(gray).save(tmp_path / "tag_01_gray.jpg", "JPEG", quality=90)           # one component
    Image.fromarray(color).save(tmp_path / "tag_01_color.jpg", "JPEG", quality=90, subsampling=2)  # 4:2:0
    Image.fromarray(gray).save(tmp_path / "tag_01_gray.png")
    Image.fromarray(color).save(tmp_path / "tag_01_color.png")
    yy, xx = np.mgrid[0:480, 0:640]
    blank = np.stack([(xx // 3) % 256, (yy // 2) % 256, np.full_like(xx, 128)], axis=-1).astype(np.uint8)  # smooth: no markers
    Image.fromarray(blank).save(tmp_path / "blank.jpg", "JPEG", quality=90)
    Image.fromarray(blank).save(tmp_path / "blank.png")
    fr = synth.make_stag_frame(load_library(21), 8, 1280, 720, 8)
    Image.fromarray(fr.image).save(tmp_path / "stag.jpg", "JPEG", quality=95)
    Image.fromarray(fr.image).save(tmp_path / "stag.png")
    r = subprocess.run([exe, str(tmp_path), os.path.join(ROOT, "fiducials_amd", "data")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
