"""The work order of k_subpix, k_pose and k_pose_cov in a batch (slot-major: every frame's slot 0, then every frame's slot 1 ...)
changes which wave works on which marker and nothing else: every marker, pose and covariance record of a batch call is the record
the same frame gives alone on a context of one frame, byte for byte, and what lies at and beyond a frame's count in the caller's
arrays is what the library has always left there.  Run on the MI355X: -m gpu."""
import ctypes as C

import numpy as np
import pytest

from fiducials_amd import camera as _camera
from fiducials_amd.detector import POSE_COV_DTYPE, ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from tail_frames import grid_frame, paste_frame

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = np.array([[233.3, 0.0, 160.0], [0.0, 233.3, 120.0], [0.0, 0.0, 1.0]])
D = np.array([0.05, -0.02, 0.001, -0.001, 0.0])
LEN = 0.14
FILL = 0xA5  # what the caller's arrays hold before a call
# markers per frame, in the order of the batch (a batch of F frames takes the first F): none, one, nine, seventeen, and for the two
# smaller contexts a frame that fills max_markers exactly (a frame with more than max_markers is refused: FID_E_CAPACITY)
COUNTS = {8: [8, 0, 1, 8, 1, 0, 8, 1, 8], 20: [17, 0, 9, 1, 20, 9, 0, 17, 1], 64: [17, 0, 9, 1, 17, 9, 0, 17, 1]}
BATCHES = (1, 3, 8, 9)


def _dict():
    return get_predefined_dictionary("DICT_4X4_50")


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _call(det, frames, batch=True):
    """One detect call on frames (F, H, W) and the three pose calls behind it, the caller's arrays filled with FILL beforehand.
    Returns counts and per frame the max_markers records of each array as bytes: markers (behind k_subpix), poses from
    fid_pose_last (k_pose alone), poses and covariances from fid_pose_last_cov_cam (k_pose + k_pose_cov)."""
    F, mm = len(frames), det.max_markers
    cam = _camera.resolve(K, D, None)
    C.memset(det._out, FILL, C.sizeof(det._out))
    if not batch:
        det.detect_markers(frames[0])
    else:
        det.detect_markers_batch(frames)
    n = [int(det._n[f]) for f in range(F)]
    out = {"n": n, "markers": _bytes(det._out_np[:F * mm]).reshape(F, mm, -1).copy()}
    C.memset(det._poses, FILL, C.sizeof(det._poses))
    det.pose_last(LEN, K, D, unpack=False)
    out["poses"] = _bytes(det._poses_np[:F * mm]).reshape(F, mm, -1).copy()
    C.memset(det._poses, FILL, C.sizeof(det._poses))
    cov = np.zeros(F * mm, POSE_COV_DTYPE)
    cov.view(np.uint8)[:] = FILL
    det._check(det._L.fid_pose_last_cov_cam(det._ctx, C.byref(cam.c), LEN, det._poses, mm, 1.0, cov.ctypes.data))
    out["cov_poses"] = _bytes(det._poses_np[:F * mm]).reshape(F, mm, -1).copy()
    out["cov"] = _bytes(cov).reshape(F, mm, -1).copy()
    return out


@pytest.fixture(scope="module", params=sorted(COUNTS))
def alone(request):
    """max_markers, the nine frames and what each gives alone on a context of one frame (computed once, read by every batch size)."""
    mm = request.param
    d = _dict()
    frames = np.stack([grid_frame(d, n, W, H, 10 * mm + i) for i, n in enumerate(COUNTS[mm])])
    det = ArucoDetector(d, max_width=W, max_height=H, max_batch=1, max_markers=mm)
    try:
        ref = [_call(det, frames[f:f + 1], batch=False) for f in range(len(frames))]
    finally:
        det.close()
    assert [r["n"][0] for r in ref] == COUNTS[mm]
    return mm, frames, ref


@pytest.mark.parametrize("F", BATCHES)
def test_batch_records_equal_the_frames_alone(alone, F):
    mm, frames, ref = alone
    det = ArucoDetector(_dict(), max_width=W, max_height=H, max_batch=F, max_markers=mm)
    try:
        first = _call(det, frames[:F])   # (the pose calls run k_pose / k_pose_cov on the context's stream)
        second = _call(det, frames[:F])  # (the covariance request is remembered: the detect call runs both behind k_subpix)
    finally:
        det.close()
    for got in (first, second):
        assert got["n"] == COUNTS[mm][:F]
        nmax = max(got["n"])
        for f in range(F):
            n = got["n"][f]
            for key in ("markers", "poses", "cov_poses", "cov"):
                assert np.array_equal(got[key][f, :n], ref[f][key][0, :n]), (key, f)
            # at and beyond the frame's count: the caller's markers and poses are not touched; the covariances come up to the
            # call's largest count in one strided copy, from device records that no kernel has written (zero since fid_create)
            for key in ("markers", "poses", "cov_poses"):
                assert (got[key][f, n:] == FILL).all(), (key, f)
            assert (got["cov"][f, n:nmax] == 0).all() and (got["cov"][f, nmax:] == FILL).all(), f
    for key in ("markers", "poses", "cov_poses", "cov"):
        assert np.array_equal(first[key], second[key]), key
    assert np.array_equal(first["poses"], first["cov_poses"])


def test_more_waves_than_the_grid_cap():
    """129 frames of 128 x 96 with one marker each on a max_markers 256 context: 33 024 pose items are 4 128 workgroups against
    a cap of 4 096, and 132 096 corner items against 16 384, so the stride loops take further turns."""
    d = _dict()
    w, h, mm, F = 128, 96, 256, 129
    base = np.stack([paste_frame(d, [(3 * i, 36 + 2 * i, 26 + i, 32 + i)], w, h, 70 + i) for i in range(5)])
    one = ArucoDetector(d, max_width=w, max_height=h, max_batch=1, max_markers=mm)
    try:
        ref = [_call(one, base[i:i + 1], batch=False) for i in range(5)]
    finally:
        one.close()
    assert [r["n"] for r in ref] == [[1]] * 5
    frames = np.ascontiguousarray(base[np.arange(F) % 5])
    det = ArucoDetector(d, max_width=w, max_height=h, max_batch=F, max_markers=mm)
    try:
        got = _call(det, frames)
    finally:
        det.close()
    assert got["n"] == [1] * F
    for f in range(F):
        for key in ("markers", "poses", "cov_poses", "cov"):
            assert np.array_equal(got[key][f, :1], ref[f % 5][key][0, :1]), (key, f)
            assert (got[key][f, 1:] == FILL).all(), (key, f)


def test_pose_of_caller_markers_with_their_own_lengths():
    """fid_pose on 19 markers handed in with a length each: every record is the record of that marker handed in alone."""
    d = _dict()
    img = grid_frame(d, 19, W, H, 300)
    det = ArucoDetector(d, max_width=W, max_height=H, max_batch=1, max_markers=64)
    try:
        corners, ids = det.detect_markers(img)
        assert len(ids) == 19
        lens = {int(i): 0.05 + 0.01 * k for k, i in enumerate(ids)}
        both = det.estimate_pose_single_markers(corners, ids, LEN, K, D, fiducial_len_override=lens)
        for k in range(19):
            solo = det.estimate_pose_single_markers(corners[k:k + 1], ids[k:k + 1], LEN, K, D, fiducial_len_override=lens)
            for field in ("rvecs", "tvecs", "image_error", "object_error", "fiducial_area"):
                assert np.asarray(getattr(both, field))[k].tobytes() == np.asarray(getattr(solo, field))[0].tobytes(), (field, k)
    finally:
        det.close()
